"""The brute-force matcher's case table (tests/bf_cases.py) against the oracle, on a context of its own.

    python tests/bf_child.py

tests/test_gpu_bf_edges.py imports the checks below for the session's context and starts this file
as a fresh process per value of LORB_BF_QPL (the library reads the variable once per process), so
the 1- and 4-descriptor instantiations of every scan kernel run the same table.  Exit status 0: every
case equals the oracle; 1: a mismatch, the case's name and the differing output on stderr."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "oracle"), ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import bf_cases  # noqa: E402
import oracle as O  # noqa: E402

TOP2_KEYS = ("best_idx", "best_dist", "best_level", "second_dist", "second_level", "accepted")


def oracle_match(qs, ts):
    """the oracle's crossCheck per problem, concatenated as lorb_bf_match lays its outputs out"""
    r = [O.bf_match(q, t) for q, t in zip(qs, ts)]
    out = {k: np.concatenate([x[k] for x in r]) for k in ("cc_train", "cc_dist", "match_train")}
    out["n_matches"] = np.array([x["n_matches"] for x in r], np.int32)
    return out


def oracle_top2(qs, ts, levs):
    levs = levs if levs is not None else [None] * len(qs)
    r = [O.bf_top2(q, t, lev) for q, t, lev in zip(qs, ts, levs)]
    return {k: np.concatenate([x[k] for x in r]) for k in TOP2_KEYS}


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """the oracle's outputs for a case of bf_cases, computed once per process"""
    c = bf_cases.case(name)
    return dict(match=oracle_match(c["q"], c["t"]) if "match" in c["ops"] else None,
                top2=oracle_top2(c["q"], c["t"], c["lev"]) if "top2" in c["ops"] else None)


def match_diff(got, ref):
    """None, or the first crossCheck output that differs (cc_dist counts where a train was found)"""
    for k in ("cc_train", "match_train", "n_matches"):
        if not np.array_equal(got[k], ref[k]):
            return k
    has = ref["cc_train"] >= 0
    return None if np.array_equal(got["cc_dist"][has], ref["cc_dist"][has]) else "cc_dist"


def top2_diff(got, ref):
    for k in TOP2_KEYS:
        if not np.array_equal(got[k], ref[k]):
            return k
    return None


def check_match(ctx, qs, ts, ref=None):
    got, _ = ctx.bf_match(list(qs), list(ts))
    return match_diff(got, ref if ref is not None else oracle_match(qs, ts))


def check_top2(ctx, qs, ts, levs, ref=None):
    got, _ = ctx.bf_top2(list(qs), list(ts), None if levs is None else list(levs))
    return top2_diff(got, ref if ref is not None else oracle_top2(qs, ts, levs))


def check_case(ctx, name):
    """None, or "entry point: output" of the first mismatch of case `name` on ctx"""
    c, ref = bf_cases.case(name), case_reference(name)
    if "match" in c["ops"]:
        d = check_match(ctx, c["q"], c["t"], ref["match"])
        if d:
            return f"bf_match: {d}"
    if "top2" in c["ops"]:
        d = check_top2(ctx, c["q"], c["t"], c["lev"], ref["top2"])
        if d:
            return f"bf_top2: {d}"
    return None


def main():
    from lorb_slam_amd.runtime import Context
    ctx = Context(0)
    try:
        for name in bf_cases.NAMES:
            d = check_case(ctx, name)
            if d:
                print(f"LORB_BF_QPL={os.environ.get('LORB_BF_QPL', '')} case {name}: {d} differs from the oracle",
                      file=sys.stderr)
                return 1
    finally:
        ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
