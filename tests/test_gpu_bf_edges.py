"""GPU: the brute-force matcher (lorb_bf.hip) on hand-built degenerate inputs, bit-exact against the
oracle: distance 256 in crossCheck, ties on every train and across chunk / lane-tile boundaries, both
branches of build_tiles' chunk choice, tiles without uniform items (tests/bf_cases.py); the sharded
path against the oracle itself; the state a context carries from call to call (the all-ones train
keys in a growing buffer, the last-workgroup counter, the scratch slots the paths share); argument
errors; the LORB_BF_QPL = 1 / 4 instantiations of the scan kernels in fresh child processes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import bf_cases
import bf_child
from lorb_slam_amd import _abi as A
from lorb_slam_amd import synth

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LORB_E_INVALID = -1


# ---- 1. the case table ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", bf_cases.NAMES)
def test_case_table(ctx, name):
    assert bf_child.check_case(ctx, name) is None


# ---- 2. the sharded path at world 1, against the oracle ------------------------------------------
def _sharded_diff(ctx, comm, qs, ts, ref=None):
    got = ctx.bf_match_sharded(comm, list(qs), [0] * len(qs), list(ts))
    return bf_child.match_diff(got, ref if ref is not None else bf_child.oracle_match(qs, ts))


def test_sharded_world1_vs_oracle(ctx):
    from lorb_slam_amd.runtime import Comm, unique_id
    comm = Comm.rccl(ctx, 1, 0, unique_id())
    try:
        for name in bf_cases.COMPLEMENT + ("identical", "duplicates"):
            c = bf_cases.case(name)
            assert _sharded_diff(ctx, comm, c["q"], c["t"], bf_child.case_reference(name)["match"]) is None, name
        qs, ts = bf_cases.empty_batch()  # one problem without trains, one without queries
        assert _sharded_diff(ctx, comm, qs, ts) is None, "empty_batch"
    finally:
        comm.close()


# ---- 3. call order on a fresh context -------------------------------------------------------------
def test_call_order_fresh_context():
    """Every step against the oracle, on a context of its own so the first call meets fresh buffers:
    the train keys must be all-ones between calls in a buffer that grows (70 x 300 -> 70 x 5000) and
    in entries a shorter call never touched (600 x 13, then 70 x 5000 again); the last workgroup's
    counter must be back at 0; the query-key and output slots are shared by the one-problem path,
    the batched path, top-2 and the sharded path."""
    from lorb_slam_amd.runtime import Comm, Context, unique_id
    small = synth.bf_problem(seed=301, nq=70, nt=300, n_planted=35, random_levels=True)
    wide = synth.bf_problem(seed=302, nq=70, nt=5000, n_planted=35)
    tall = synth.bf_problem(seed=303, nq=600, nt=13, n_planted=6)
    ident, dup = bf_cases.case("identical"), bf_cases.case("duplicates")
    bq, bt = bf_cases.empty_batch()
    ref = {k: bf_child.oracle_match([v[0]], [v[1]]) for k, v in (("small", small), ("wide", wide), ("tall", tall))}
    ref_b3 = bf_child.oracle_match(bq[1:], bt[1:])
    ref_top2 = bf_child.oracle_top2([small[0]], [small[1]], [small[2]])
    e = np.zeros((0, 32), np.uint8)
    c = Context(0)
    comm = None
    try:
        def match1(p, key):
            return bf_child.check_match(c, [p[0]], [p[1]], ref[key])
        assert match1(small, "small") is None, "match 70x300"
        assert match1(wide, "wide") is None, "match 70x5000 (the train-key buffer grows)"
        assert match1(tall, "tall") is None, "match 600x13"
        assert match1(wide, "wide") is None, "match 70x5000 again (entries the short call left alone)"
        assert bf_child.check_match(c, ident["q"], ident["t"], bf_child.case_reference("identical")["match"]) is None
        assert bf_child.check_match(c, bq[1:], bt[1:], ref_b3) is None, "batched, np = 3"
        assert bf_child.check_match(c, [small[0]], [e]) is None, "np = 1, no trains"
        assert bf_child.check_match(c, [e], [small[1]]) is None, "np = 1, no queries"
        assert bf_child.check_top2(c, [small[0]], [small[1]], [small[2]], ref_top2) is None, "top-2"
        comm = Comm.rccl(c, 1, 0, unique_id())
        assert _sharded_diff(c, comm, dup["q"], dup["t"], bf_child.case_reference("duplicates")["match"]) is None
        assert bf_child.check_top2(c, [small[0]], [small[1]], [small[2]], ref_top2) is None, "top-2 again"
        assert match1(small, "small") is None, "match 70x300 again"
    finally:
        if comm is not None:
            comm.close()
        c.close()


# ---- 4. argument errors ----------------------------------------------------------------------------
def _raw_match(ctx, q, q_off, t, t_off):
    from lorb_slam_amd.runtime import lib
    n_p, nq = len(q_off) - 1, len(q)
    o = [np.zeros(nq, np.int32) for _ in range(3)] + [np.zeros(n_p, np.int32)]
    return lib().lorb_bf_match(ctx.handle, C.c_int32(n_p), A.ptr(q, C.c_uint8), A.ptr(q_off, C.c_int32),
                               A.ptr(t, C.c_uint8), A.ptr(t_off, C.c_int32), *[A.ptr(a, C.c_int32) for a in o])


def _raw_top2(ctx, q, q_off, t, t_off):
    from lorb_slam_amd.runtime import lib
    n_p, nq = len(q_off) - 1, len(q)
    o = [np.zeros(nq, np.int32) for _ in range(5)]
    acc = np.zeros(nq, np.uint8)
    return lib().lorb_bf_top2(ctx.handle, C.c_int32(n_p), A.ptr(q, C.c_uint8), A.ptr(q_off, C.c_int32),
                              A.ptr(t, C.c_uint8), A.ptr(t_off, C.c_int32), A.ptr(None, C.c_int32),
                              *[A.ptr(a, C.c_int32) for a in o], A.ptr(acc, C.c_uint8))


GOOD = [0, 30, 50, 80]
BAD_OFFSETS = {  # 3 problems over 80 queries and 80 trains; the bad entry is the middle problem's
    "q_off_start": ([1, 30, 50, 80], GOOD),
    "t_off_start": (GOOD, [1, 30, 50, 80]),
    "q_off_not_monotone": ([0, 50, 30, 80], GOOD),
    "t_off_not_monotone": (GOOD, [0, 50, 30, 80]),
}


@pytest.mark.parametrize("call", ["bf_match", "bf_top2"])
@pytest.mark.parametrize("bad", list(BAD_OFFSETS))
def test_bad_offsets_are_refused(ctx, call, bad):
    """refused on the host (check_offsets / build_tiles, before any matcher kernel is launched) with
    LORB_E_INVALID and a message; the next valid call on the context equals the oracle"""
    from lorb_slam_amd.runtime import lib
    q, t, _ = synth.bf_problem(seed=311, nq=80, nt=80, n_planted=40)
    q_off, t_off = (np.array(o, np.int32) for o in BAD_OFFSETS[bad])
    rc = (_raw_match if call == "bf_match" else _raw_top2)(ctx, q, q_off, t, t_off)
    assert rc == LORB_E_INVALID
    assert lib().lorb_last_error(ctx.handle)
    qs = [q[a:b] for a, b in zip(GOOD[:-1], GOOD[1:])]
    ts = [t[a:b] for a, b in zip(GOOD[:-1], GOOD[1:])]
    if call == "bf_match":
        assert bf_child.check_match(ctx, qs, ts) is None
    else:
        assert bf_child.check_top2(ctx, qs, ts, None) is None


# ---- 5. LORB_BF_QPL = 1 and 4 -----------------------------------------------------------------------
def test_qpl_instantiations():
    """the case table with 1 and with 4 lane descriptors per thread: one fresh child process per value
    (read once per process), one after the other, the second only if the first passed"""
    for qpl in ("1", "4"):
        p = subprocess.Popen([sys.executable, os.path.join(HERE, "bf_child.py")], env=dict(os.environ, LORB_BF_QPL=qpl),
                             stderr=subprocess.PIPE, text=True)
        try:
            _, err = p.communicate(timeout=60)
        except subprocess.TimeoutExpired:
            p.kill()
            p.communicate()
            pytest.fail(f"LORB_BF_QPL={qpl}: the child did not finish in 60 s")
        assert p.returncode == 0, (qpl, p.returncode, err[-2000:])
