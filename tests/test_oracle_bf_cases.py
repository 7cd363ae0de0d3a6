"""CPU: the oracle's matcher restatement against the independent numpy statements of
test_oracle_match.py on the degenerate cases of bf_cases.py (the inputs the GPU edge tests run), and
the properties that make each case what it claims to be."""
import numpy as np
import pytest

import bf_cases
import oracle as O
from test_oracle_match import np_crosscheck, np_dist, np_top2

TOP2_KEYS = ("best_idx", "best_dist", "best_level", "second_dist", "second_level", "accepted")


@pytest.mark.parametrize("name", bf_cases.NAMES)
def test_oracle_vs_numpy(name):
    c = bf_cases.case(name)
    for p, (q, t) in enumerate(zip(c["q"], c["t"])):
        D = np_dist(q, t)
        if "match" in c["ops"]:
            r = O.bf_match(q, t)
            cc, dd, mt = np_crosscheck(D)
            assert (r["cc_train"] == cc).all() and (r["cc_dist"] == dd).all() and (r["match_train"] == mt).all(), p
            assert r["n_matches"] == (mt >= 0).sum(), p
        if "top2" in c["ops"]:
            lev = c["lev"][p] if c["lev"] is not None else np.zeros(len(t), np.int32)
            r = O.bf_top2(q, t, lev)
            got = np.stack([r[k] for k in TOP2_KEYS], 1)
            assert (got == np_top2(D, lev)).all(), p


def test_empty_batch_oracle_vs_numpy():
    for q, t in zip(*bf_cases.empty_batch()):
        r = O.bf_match(q, t)
        if len(q) and len(t):
            cc, dd, mt = np_crosscheck(np_dist(q, t))
            assert (r["cc_train"] == cc).all() and (r["cc_dist"] == dd).all() and (r["match_train"] == mt).all()
        else:
            assert r["n_matches"] == 0 and (r["cc_train"] == -1).all() and (r["match_train"] == -1).all()


@pytest.mark.parametrize("name", bf_cases.COMPLEMENT)
def test_complement_reference_semantics(name):
    """OpenCV's crossCheck takes each train's arg-min whatever its value: with every pair at distance
    256, query 0 gets train 0 at 256; minDist is 256, the filter's threshold 512, so it is a match.
    Pinned with numpy alone, then with the C oracle."""
    c = bf_cases.case(name)
    for q, t in zip(c["q"], c["t"]):
        D = np_dist(q, t)
        assert (D == 256).all()
        cc, dd, mt = np_crosscheck(D)
        r = O.bf_match(q, t)
        for cc_train, cc_dist, match_train, n in ((cc, dd, mt, (mt >= 0).sum()),
                                                  (r["cc_train"], r["cc_dist"], r["match_train"], r["n_matches"])):
            assert cc_train[0] == 0 and cc_dist[0] == 256 and match_train[0] == 0 and n == 1
            assert (cc_train[1:] == -1).all() and (match_train[1:] == -1).all()
        # top-2 is the other way round (bestDist = 256, strict <): 256 never enters
        r = O.bf_top2(q, t)
        assert (r["best_idx"] == -1).all() and (r["best_dist"] == 256).all() and not r["accepted"].any()


def _tied_fraction(q, t):
    D = np_dist(q, t)
    return ((D == D.min(0)).sum(0) > 1).mean()


def test_duplicates_stays_tie_heavy():
    """at least 90 % of the trains have a tied nearest query (a random problem has about 14 %)"""
    c = bf_cases.case("duplicates")
    assert len(c["q"][0]) == 600 and len(c["t"][0]) == 700
    assert _tied_fraction(c["q"][0], c["t"][0]) >= 0.9


def test_identical_ties_everywhere():
    c = bf_cases.case("identical")
    assert (np_dist(c["q"][0], c["t"][0]) == 0).all()


@pytest.mark.parametrize("name,op,plan", [
    ("complement_40x9", "match", ("grid1", 1, 1)),
    ("complement_batch", "match", ("<256", 2, 1)),
    ("identical", "match", ("grid1", 1, 2)),
    ("identical", "top2", ("<256", 1, 1)),
    ("duplicates", "match", ("grid1", 2, 18)),
    ("duplicates", "top2", ("<256", 2, 20)),
    ("tiles_ge256_top2", "top2", (">=256", 260, 2)),
    ("tiles_ge256_top2_1chunk", "top2", (">=256", 260, 1)),
    ("tiles_ge256_match", "match", (">=256", 260, 2)),
    ("sparse_chunks", "top2", ("<256", 2, 42)),
])
def test_chunk_plans_as_commented(name, op, plan):
    """the shapes still give the tile and chunk counts their comments in bf_cases.py state (from the
    restatement of grid1_of / build_tiles there)"""
    assert bf_cases.chunk_plan(bf_cases.case(name), op) == plan


def test_sparse_chunks_has_empty_tiles():
    c = bf_cases.case("sparse_chunks")
    _, _, nc = bf_cases.chunk_plan(c, "top2")
    nu = len(c["t"][1])
    empty = sum(nu * (k + 1) // nc == nu * k // nc for k in range(nc))
    assert (nc, empty) == (42, 41)
