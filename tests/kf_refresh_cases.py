"""Stores with geometry and appearance for lorb_kf_store_refresh_dev, built on tests/kf_ba_cases.py: the hand case
with its answer written out (tests/test_kf_refresh_ref.py checks the restatement tests/kf_refresh_ref.py against it on
the CPU) and generated stores at the sizes where the point kernel changes path.  tests/test_gpu_kf_refresh.py checks
the device against the restatement on all of them.

A case is dict(store, geom, app, kf) (+ want for the hand case)."""
import numpy as np

import kf_ba_cases as BC
import oracle as O

F = np.float32


def appearance_for(store, geom, seed=0):
    """Random descriptors and octaves in [0, 8) for every keyframe slot; the centres are the host's
    O.inv4_f32(O.pose_to_Tcw(rvec, tvec)) of the geometry's pose rows."""
    rng = np.random.default_rng(7000 + seed)
    rows = store["kf_slots"]
    centers = np.zeros((len(rows), 3), F)
    for f, p in enumerate(geom["kf_pose"]):
        p = np.asarray(p, F).reshape(6)
        centers[f] = np.asarray(O.inv4_f32(O.pose_to_Tcw(p[:3], p[3:]))[0], F).reshape(16)[[3, 7, 11]]
    return dict(kf_slot_desc=[rng.integers(0, 256, (len(r), 32), dtype=np.uint8) for r in rows],
                kf_slot_octave=[rng.integers(0, 8, len(r)).astype(np.int32) for r in rows], kf_center=centers)


def with_appearance(case, seed=0):
    case["app"] = appearance_for(case["store"], case["geom"], seed)
    return case


def low_bits(k):
    """A descriptor whose first k bits are set: hamming(low_bits(a), low_bits(b)) = |a - b|."""
    bits = np.zeros(256, np.uint8)
    bits[:k] = 1
    return np.packbits(bits)


def hand_case():
    """BC.hand_case() -- window l2g = [7, 4, 2, 0], kf 2 bad -- with positions and centres on a lattice where every
    viewing ray is a coordinate axis and every distance a power of two, so that each term is exact:
      centres  kf0 (2, 4, 0)  kf1 (4, 2, -4)  kf2 (-4, 0, -1)  kf3 (4, 0, 0)  kf4 (4, 0, -3)  kf5 (4, 4, -1)
      p7 (4, 4, 0)   kf0 +x at 2, kf3 +y at 4, kf5 +z at 1            normal (1, 1, 1) * float(1 / 3)
      p4 (4, 0, -1)  kf2 +x at 8, kf3 -z at 1, kf4 +z at 2, kf5 -y at 4  normal (1, -1, 0) / 4: bad kf2 counts
      p2 (4, 2, 0)   kf1 +z at 4, kf3 +y at 2                         normal (0, 1, 1) / 2
      p0 (5, 2, -4)  kf1 +x at 1                                      normal (1, 0, 0)
    The reference keyframe is the first observer: kf0 slot 0 (octave 1), kf2 slot 0 (octave 3: a bad keyframe is
    still mpRefKF), kf1 slot 1 (octave 0), kf1 slot 0 (octave 2); max_dist = distance * scale_factors[octave].
    Descriptors are low_bits(v), distances |v - w|; the store's descriptors are all zero, so a point's changed bits
    are the v it takes:
      p7  kf0 0, kf3 10, kf5 30: medians 10, 10, 20 -> the first of the equals, kf0 (0 bits)
      p4  kf2 45 is bad and skipped (with it: medians 5, 20, 10, 10 -> kf2); kf3 40, kf4 60, kf5 70: medians 20, 10,
          10 -> kf4, position 1 of the usable ones (60 bits)
      p2  kf1 7, kf3 90: n = 2, element 0 of each row is the self-distance -> the first, kf1 (7 bits)
      p0  kf1 3 (3 bits)"""
    c = BC.hand_case()
    s = c["store"]
    for p, xyz in ((7, (4, 4, 0)), (4, (4, 0, -1)), (2, (4, 2, 0)), (0, (5, 2, -4))):
        s["pos"][p] = xyz
    s["desc"][:] = 0
    app = appearance_for(s, c["geom"], seed=1)
    app["kf_center"] = np.array([(2, 4, 0), (4, 2, -4), (-4, 0, -1), (4, 0, 0), (4, 0, -3), (4, 4, -1)], F)
    for (f, j), octave in {(0, 0): 1, (2, 0): 3, (1, 1): 0, (1, 0): 2}.items():
        app["kf_slot_octave"][f][j] = octave
    for (f, j), v in {(0, 0): 0, (3, 2): 10, (5, 0): 30, (2, 0): 45, (3, 0): 40, (4, 0): 60, (5, 2): 70, (1, 1): 7, (3, 1): 90,
                      (1, 0): 3}.items():
        app["kf_slot_desc"][f][j] = low_bits(v)
    third = F(1.0 / 3.0)
    c["app"] = app
    c["want"] = dict(l2g=[7, 4, 2, 0], normal=[(third, third, third), (0.25, -0.25, 0), (0, 0.5, 0.5), (1, 0, 0)],
                     dist=[2, 8, 4, 1], octave=[1, 3, 0, 2], chosen=[0, 1, 0, 0], took=[0, 60, 7, 3],
                     rec=dict(status=0, kf=5, n_points=4, n_refreshed=4, n_bad=0, n_empty=0, n_obs_bad_slot=0, n_desc_changed=70,
                              n_centers=0))
    return c


OBS_OF_P0 = (1, 2, 3, 63, 64, 65, 128, 255)   # the lane-row borders, median index (n - 1) / 2 at 0, odd and even counts
WINDOW_POINTS = (1, 3, 4, 5)                  # the last wavefronts of a workgroup of four


def star_cases():
    out = {f"obs_{n}": with_appearance(BC.star_case(4, 2, seed=100 + n, n_obs_of_p0=n), n) for n in OBS_OF_P0}
    out.update({f"points_{n}": with_appearance(BC.star_case(1, n, seed=200 + n), 200 + n) for n in WINDOW_POINTS})
    return out


def p0_of(case):
    """The point star_case gave its long list."""
    return case["store"]["kf_slots"][case["kf"]][0]


def identical_case():
    """All 65 observers of p0 carry one descriptor: every median is 0, the first wins."""
    c = with_appearance(BC.star_case(4, 2, seed=31, n_obs_of_p0=65), 31)
    p0, d = p0_of(c), np.arange(32, dtype=np.uint8) * 7 + 1
    for f, j in zip(c["store"]["obs"][p0], c["geom"]["obs_slot"][p0]):
        c["app"]["kf_slot_desc"][f][j] = d
    return c


def equal_medians_case():
    """p0 has three observers with low_bits 0, 10, 30: medians 10, 10, 20, the first of the equals wins.  (Two
    observers, where both medians are the self-distance 0, are star_cases()' obs_2.)"""
    c = with_appearance(BC.star_case(4, 2, seed=32, n_obs_of_p0=3), 32)
    p0 = p0_of(c)
    for (f, j), v in zip(zip(c["store"]["obs"][p0], c["geom"]["obs_slot"][p0]), (0, 10, 30)):
        c["app"]["kf_slot_desc"][f][j] = low_bits(v)
    return c


def all_bad_case():
    """K = 1 is bad (local[0] = K, bad or not) and its two own points are seen by K alone: no usable observer, the
    descriptor stays, the normal is computed.  kf0's points keep the window at status 0."""
    c = with_appearance(BC.star_case(2, 2, seed=33), 33)
    c["store"]["kf_bad"][c["kf"]] = 1
    return c


def all_cases():
    c = dict(hand=hand_case(), identical=identical_case(), equal_medians=equal_medians_case(), all_bad=all_bad_case(),
             random_a=with_appearance(BC.random_case(9, 300, seed=1), 41),
             random_mid=with_appearance(BC.random_case(12, 700, seed=3, kf=5), 42))
    c.update(star_cases())
    return c
