"""CPU: synth.flip_bits against its definition, row by row and bit by bit, on the same generator stream
(the seeded inputs of the tests and of bench.py must not depend on how the flips are applied)."""
import numpy as np

from lorb_slam_amd import synth


def flip_bits_by_definition(rng, desc, max_flips):
    out = desc.copy()
    nf = rng.integers(0, max_flips + 1, size=len(desc))
    for i in range(len(desc)):
        if nf[i]:
            for b in rng.choice(256, size=nf[i], replace=False):
                out[i, b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def test_mapping_sequence_keyframes_see_every_live_point():
    """each stream keyframe re-observes exactly the points created before it that are still alive
    and creates n_new, whatever the stream's length (counted here over all points, by definition)"""
    n_kf, n_fixed, n_new, obs_lens = 6, 2, 13, (3, 5, 4)
    for steps in (1, 9):
        seq = synth.mapping_sequence(seed=8, n_kf=n_kf, n_fixed=n_fixed, n_new=n_new, obs_lens=obs_lens, steps=steps,
                                     n_kps=200)
        first, last = -n_fixed - max(obs_lens) + 1, n_kf + steps
        created = np.repeat(np.arange(first, last), n_new)
        length = np.array(obs_lens)[np.arange(len(created)) % len(obs_lens)]
        assert len(seq["steps"]) == steps
        for i, k in enumerate(seq["steps"]):
            t = n_kf + i
            assert k["kf"] == t and k["n_new"] == n_new
            assert k["n_reobs"] == int(((created < t) & (created + length > t)).sum())
            assert int((k["depth"] > 0).sum()) == n_new and len(k["x"]) == 200


def test_flip_bits_matches_its_definition_and_leaves_the_stream_alike():
    for seed, n, max_flips in ((1, 300, 20), (2, 257, 32), (3, 1, 256), (4, 0, 20), (5, 50, 0)):
        desc = synth.random_desc(np.random.default_rng(seed), n)
        r1, r2 = np.random.default_rng(100 + seed), np.random.default_rng(100 + seed)
        got, ref = synth.flip_bits(r1, desc, max_flips), flip_bits_by_definition(r2, desc, max_flips)
        assert got.dtype == np.uint8 and np.array_equal(got, ref)
        assert r1.integers(1 << 62) == r2.integers(1 << 62)  # the same draws were consumed
        flips = np.unpackbits(got ^ desc, axis=1).sum(1) if n else np.zeros(0)
        assert (flips <= max_flips).all()
