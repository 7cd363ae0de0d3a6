"""Hand-built degenerate problems for the brute-force matcher (lorb_bf.hip): distance 256, ties on
every train, ties across chunk and lane-tile boundaries, both branches of the chunk choice, tiles
without uniform items.  Pure numpy, seeded; shared by test_oracle_bf_cases.py (CPU),
test_gpu_bf_edges.py and bf_child.py (GPU).

A case is a dict: q / t / lev = one array per problem (lev: the trains' pyramid levels, top-2 only),
ops = the entry points it is meant for ("match" = lorb_bf_match, "top2" = lorb_bf_top2).

The chunk counts in the comments are derived from grid1_of (one-problem crossCheck) and build_tiles
(top-2 and the batched crossCheck) in lorb_bf.hip with 2 lane descriptors per thread (lane tile =
512); chunk_plan() below restates the two functions so test_oracle_bf_cases.py can check the
comments.  If a constant of those functions changes, re-derive the shapes: each case has to keep
hitting its branch."""
import functools

import numpy as np

from lorb_slam_amd import synth

N_BASE = 9  # the pool every tie-heavy case draws from


def _base(rng):
    return synth.random_desc(rng, N_BASE)


def _tied(rng, base, nq, nt, max_flips=3):
    """queries = copies of base rows, trains = base rows with at most max_flips flipped bits: the
    nearest queries of a train are all the copies of its base row (its first copy has to win)"""
    q = base[rng.integers(0, N_BASE, nq)]
    t = synth.flip_bits(rng, base[rng.integers(0, N_BASE, nt)], max_flips)
    return np.ascontiguousarray(q), np.ascontiguousarray(t)


def _case(q, t, lev=None, ops=("match", "top2")):
    return dict(q=list(q), t=list(t), lev=None if lev is None else list(lev), ops=tuple(ops))


def _complement(nq, nt):
    return np.zeros((nq, 32), np.uint8), np.full((nt, 32), 255, np.uint8)


def _complement_1x1():
    # every pair at distance 256: OpenCV's crossCheck takes the arg-min whatever its value, so query
    # 0 gets train 0 at 256 (minDist 256, threshold 512, one match); top-2 never lets 256 enter
    q, t = _complement(1, 1)
    return _case([q], [t])


def _complement_40x9():
    # match: 1 lane tile, 1 chunk (40 / 32); all 9 trains tie on query 0, train 0 wins it
    q, t = _complement(40, 9)
    return _case([q], [t])


def _complement_batch():
    # the batched crossCheck (np > 1 goes through build_tiles / k_cc_scatter): 2 lane tiles, 1 chunk
    a, b = _complement(1, 1), _complement(40, 9)
    return _case([a[0], b[0]], [a[1], b[1]])


def _identical():
    # match: lanes = 13 trains (1 tile), 70 queries in 2 chunks of 35 -> every train's tie between
    # the 70 queries crosses the chunk boundary (query 0 has to win all 13, train 0 wins query 0)
    # top-2: 1 tile, 1 chunk (13 / 32 = 0)
    rng = np.random.default_rng(41)
    d = synth.random_desc(rng, 1)
    return _case([np.repeat(d, 70, 0)], [np.repeat(d, 13, 0)], [rng.integers(0, 8, 13).astype(np.int32)])


def _duplicates():
    # match: lanes = 700 trains -> 2 lane tiles (512 + 188), 600 queries in 18 chunks of 33 - 34;
    # every train's nearest query is tied (700 of 700)
    # top-2: lanes = 600 queries -> 2 tiles, 700 trains in 20 chunks of 35 (the < 256 branch)
    rng = np.random.default_rng(42)
    q, t = _tied(rng, _base(rng), 600, 700)
    return _case([q], [t], [rng.integers(0, 8, 700).astype(np.int32)])


def _tiles_ge256_top2(nt):
    rng = np.random.default_rng(43 + nt)
    base = _base(rng)
    qs, ts, ls = [], [], []
    for _ in range(260):
        q, t = _tied(rng, base, 3, nt)
        qs.append(q); ts.append(t); ls.append(rng.integers(0, 8, nt).astype(np.int32))
    return _case(qs, ts, ls, ops=("top2",))


def _tiles_ge256_top2_2chunks():
    # top-2: 260 problems x 3 queries -> 260 lane tiles (>= 256 branch); 300 trains per problem:
    # want = ceil(2048 / 260) = 8, cap = 300 / 128 = 2 -> 2 chunks of 150 + k_bf_merge<true>
    return _tiles_ge256_top2(300)


def _tiles_ge256_top2_1chunk():
    # the same branch with 100 trains per problem: cap = max(1, 100 / 128) = 1 chunk, no merge
    return _tiles_ge256_top2(100)


def _tiles_ge256_match():
    # batched crossCheck, lanes = trains: 260 problems x 2 trains -> 260 lane tiles (>= 256 branch),
    # 300 queries per problem in 2 chunks of 150; k_bf_merge<false> runs on a grid sized by the
    # 78,000 query keys it initialises (n_init), far more than its 520 lanes
    rng = np.random.default_rng(44)
    base = _base(rng)
    qs, ts = [], []
    for _ in range(260):
        q, t = _tied(rng, base, 300, 2)
        qs.append(q); ts.append(t)
    return _case(qs, ts, ops=("match",))


def _sparse_chunks():
    # top-2, 2 lane tiles (< 256 branch), max_u = 2100: the cost ceil(2 nc / 256) ceil(2100 / nc) + nc
    # is least (92) first at nc = 42 chunks of 50; the 1-train problem's chunk c is [c / 42, (c + 1) / 42):
    # 41 of its 42 tiles have uni_count == 0
    rng = np.random.default_rng(45)
    base = _base(rng)
    q0, t0 = _tied(rng, base, 5, 2100)
    q1, t1 = _tied(rng, base, 5, 1)
    return _case([q0, q1], [t0, t1], [rng.integers(0, 8, 2100).astype(np.int32), rng.integers(0, 8, 1).astype(np.int32)],
                 ops=("top2",))


_BUILDERS = {
    "complement_1x1": _complement_1x1,
    "complement_40x9": _complement_40x9,
    "complement_batch": _complement_batch,
    "identical": _identical,
    "duplicates": _duplicates,
    "tiles_ge256_top2": _tiles_ge256_top2_2chunks,
    "tiles_ge256_top2_1chunk": _tiles_ge256_top2_1chunk,
    "tiles_ge256_match": _tiles_ge256_match,
    "sparse_chunks": _sparse_chunks,
}
NAMES = tuple(_BUILDERS)
COMPLEMENT = ("complement_1x1", "complement_40x9", "complement_batch")


@functools.lru_cache(maxsize=None)
def case(name):
    """the case's arrays, built once per process; callers must not modify them"""
    c = _BUILDERS[name]()
    for k in ("q", "t", "lev"):
        for a in c[k] or ():
            a.setflags(write=False)
    return c


def empty_batch():
    """4 crossCheck problems: tie-heavy, no trains, no queries, random with planted matches"""
    rng = np.random.default_rng(46)
    q0, t0 = _tied(rng, _base(rng), 90, 140)
    q1 = synth.random_desc(rng, 17)
    t2 = synth.random_desc(rng, 23)
    q3, t3, _ = synth.bf_problem(seed=47, nq=130, nt=75, n_planted=40)
    e = np.zeros((0, 32), np.uint8)
    return [q0, q1, e, q3], [t0, e, t2, t3]


# ---- the chunk choice of lorb_bf.hip restated (what the comments above are derived from) -------
def chunk_plan(c, op, qpl=2):
    """(branch, lane tiles, chunks) the library picks for case c under entry point op: "grid1" for
    the one-problem crossCheck (grid1_of), else build_tiles' branch ">=256" or "<256"."""
    lt = 256 * qpl
    if op == "match":  # reverse pass: lanes = trains, uniform = queries
        lanes, uni = [len(t) for t in c["t"]], [len(q) for q in c["q"]]
        if len(lanes) == 1:
            tiles = -(-lanes[0] // lt)
            return "grid1", tiles, max(1, min(-(-1536 // tiles), uni[0] // 32))
    else:
        lanes, uni = [len(q) for q in c["q"]], [len(t) for t in c["t"]]
    tiles = sum(-(-nl // lt) for nl, nu in zip(lanes, uni) if nu > 0)
    max_u = max(uni)
    if tiles >= 256:
        return ">=256", tiles, max(1, min(-(-2048 // tiles), max(1, max_u // 128), 64))
    cap = max(1, min(64, max_u // 32))
    cost = [-(-tiles * nc // 256) * -(-max_u // nc) + nc for nc in range(1, cap + 1)]
    return "<256", tiles, 1 + int(np.argmin(cost))
