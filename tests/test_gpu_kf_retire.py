"""GPU: lorb_kf_store_retire_dev (lorb_slam_amd.frame.keyframe_retire) against the literal, sequential restatement
tests/kf_retire_ref.py on the fabricated stores of tests/kf_retire_cases.py.

After every call: every array of the store, its geometry, its life and its appearance against the restatement --
integers equal, floats as bytes -- the six true counts, the record (fields the call does not write keep the sentinel),
sentinel bytes past every true count, the list, the count word and the protected words unread.  The scratch marks are
not visible from outside; that they are back at rest shows in a second call on the same store, which retires another
keyframe and is checked in the same way.  A true count outside its capacity cannot be produced through the public
interface; the other status-1 paths run against sentinels."""
import copy
import ctypes as C

import numpy as np
import pytest

import kf_ba_ref as B
import kf_retire_cases as RC
import kf_retire_ref as T
import kf_store_ref as R
import test_gpu_kf_ba as KB
import test_gpu_kf_cull as CU
import test_gpu_kf_store as KS
from lorb_slam_amd import _abi as A
from lorb_slam_amd.frame import KeyframeStore, keyframe_retire, keyframe_retire_record
from lorb_slam_amd.runtime import LorbError

pytestmark = pytest.mark.gpu

G, SENT, FILL, SENT_I32 = KS.G, KS.SENT, KS.FILL, KS.SENT_I32
raw, sentinel, h2d, memset = KS.raw, KS.sentinel, CU.h2d, CU.memset
REC = C.sizeof(A.KfRetireResult)
CASES = RC.cases()


def appearance_for(cn, seed=0):
    rng = np.random.default_rng(500 + seed)
    return dict(kf_slot_desc=rng.integers(0, 256, (cn["n_kf_slots"], 32), dtype=np.uint8),
                kf_slot_octave=rng.integers(0, 8, cn["n_kf_slots"]).astype(np.int32),
                kf_center=rng.normal(size=(cn["n_kf"], 3)).astype(np.float32))


class Rig:
    """A store with geometry, life and appearance a few rows larger than its counts, sentinel bytes behind every count;
    the list with a guard band, its count word, the protected words, the source status word and the record."""

    def __init__(self, ctx, case, slack=5, n_max_list=None):
        self.ctx, self.case = ctx, case
        s = case["store"]
        cn = self.cn = R.counts(s)
        self.store = KeyframeStore(ctx, case.get("max_kf", cn["n_kf"] + slack), cn["n_points"] + slack, cn["n_obs"] + slack,
                                   cn["n_kf_slots"] + slack, init=s, geom=case["geom"])
        st = self.store
        st.fill(cn)
        st.fill_geometry(cn)
        st.fill_life(cn)
        st.fill_appearance(cn)
        st.write_life(case["life"])
        st.write_appearance(appearance_for(cn))
        CU.set_frame_word(ctx, st, case["life"]["frame_word"])
        self.n_max = max(len(case["list"]), 1) if n_max_list is None else n_max_list
        self.list = ctx.to_device(np.full(self.n_max + G, FILL, np.int32))
        self.words = ctx.to_device(np.full(2 + T.MAX_PROTECT + G, FILL, np.int32))   # n_list, src_status, protect
        self.rec = keyframe_retire_record(ctx)
        self.hi_cov = cn["n_cov"]
        self.set(case["list"], case["protect"])

    def set(self, lst, protect=(), n_list=None, src_status=0):
        self.lst, self.protect = list(lst), list(protect)
        self.n_list, self.src = len(lst) if n_list is None else n_list, src_status
        host = np.full(self.n_max + G, FILL, np.int32)
        host[:len(lst)] = lst
        h2d(self.ctx, self.list, host)
        w = np.full(2 + T.MAX_PROTECT + G, FILL, np.int32)
        w[:2] = [self.n_list, src_status]
        w[2:2 + len(protect)] = protect
        h2d(self.ctx, self.words, w)

    def run(self, status_word=True):
        memset(self.ctx, self.rec, REC)
        w = self.words.ptr.value
        keyframe_retire(self.ctx, self.store, self.list, w, self.rec, n_max_list=self.n_max,
                        protect=w + 8 if self.protect else None, n_protect=len(self.protect),
                        d_src_status=w + 4 if status_word else None)
        b = self.rec.numpy()
        assert sentinel(b[REC:])
        return A.KfRetireResult.from_buffer_copy(b.tobytes()[:REC])

    def snapshot(self):
        st = self.store
        a = CU.all_arrays(st)
        a.update({"app_" + k: v.numpy() for k, v in st.appearance.items()})
        return dict(arrays=a, list=self.list.numpy(), words=self.words.numpy())

    def free(self):
        for a in (self.store, self.list, self.words, self.rec):
            a.free()


def restate(rig, state):
    return T.retire(state["store"], state["obs_slot"], state["life"], rig.lst, n_list=rig.n_list, n_max_list=rig.n_max,
                    protect=rig.protect, src_status=rig.src)


def check(rig, rec, ref, before, cn_fill):
    """The device after a call against the restatement.  cn_fill: the counts when the sentinel bytes were written."""
    case, s = rig.case, ref["store"]
    CU.same_record(rec, ref["rec"], T.FIELDS)
    cn = R.counts(s)
    assert rig.store.counts() == cn
    KS.same_store(rig.store.read(), s)
    geom = dict(case["geom"], obs_slot=ref["obs_slot"])
    KB.same_geometry(rig.store, geom)
    CU.same_life(rig.store, case["life"], cn)
    after = rig.snapshot()
    A_, B_ = after["arrays"], before["arrays"]
    # rows past the true counts keep the sentinel fill; between the new and the old n_obs / n_cov the old entries stay
    # (n_cov can also GROW: a neighbour's list that held pairs only is rebuilt from all of its map; the rig keeps the
    # largest n_cov its calls reached)
    rig.hi_cov = max(rig.hi_cov, cn["n_cov"])
    past = dict(obs_off=cn["n_points"] + 1, obs_kf=cn_fill["n_obs"], obs_slot=cn_fill["n_obs"], kf_slot_off=cn["n_kf"] + 1,
                kf_slot_point=cn["n_kf_slots"], cov_off=cn["n_kf"] + 1, cov_kf=rig.hi_cov, kf_bad=cn["n_kf"], kf_pose=cn["n_kf"],
                kf_slot_uv=cn["n_kf_slots"], app_kf_slot_desc=cn["n_kf_slots"], app_kf_slot_octave=cn["n_kf_slots"],
                app_kf_center=cn["n_kf"])
    for k, v in A_.items():
        if k.startswith("life_"):
            continue
        tail = v[past.get(k, cn["n_points"]):]
        assert (tail == 1).all() if k in ("is_bad", "kf_bad") else sentinel(tail), k
    # left as they are: the rows of the points, dead or not; what a retired keyframe keeps; the life; the appearance
    for k in ("locked", "pos", "normal", "max_dist", "min_dist", "desc", "kf_slot_off", "kf_pose", "kf_slot_uv", "life_visible",
              "life_found", "life_first_fid", "life_recent", "life_kf_fid", "life_frame_word", "app_kf_slot_desc", "app_kf_slot_octave",
              "app_kf_center"):
        assert np.array_equal(raw(A_[k]), raw(B_[k])), k
    assert np.array_equal(after["list"], before["list"]) and np.array_equal(after["words"], before["words"])   # read only
    if ref["rec"].get("n_obs_bad_slot", 0) == 0 and ref["rec"]["status"] == 0:
        B.check_invariant(s, geom)
    return after


def unchanged(after, before):
    for k in after["arrays"]:
        assert np.array_equal(raw(after["arrays"][k]), raw(before["arrays"][k])), k


def state_of(case):
    return dict(store=case["store"], obs_slot=case["obs_slot"], life=case["life"])


def next_state(case, ref):
    return dict(store=ref["store"], obs_slot=ref["obs_slot"], life=case["life"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_retire(ctx, name):
    case = CASES[name]
    rig = Rig(ctx, case)
    try:
        before = rig.snapshot()
        ref = restate(rig, state_of(case))
        assert ref["rec"]["status"] == 0 and ref["rec"]["n_retired"] >= 1
        mid = check(rig, rig.run(), ref, before, rig.cn)
        if ref["rec"]["n_obs_removed"] == 0:                 # no point affected: not a byte of the CSR moves
            for k in ("obs_off", "obs_kf", "obs_slot"):
                assert np.array_equal(mid["arrays"][k], before["arrays"][k]), k
        # the same list again: every entry is bad now, V is empty, not a byte changes
        again = restate(rig, next_state(case, ref))
        assert again["rec"]["n_retired"] == 0 and again["rec"]["n_skip_bad"] >= ref["rec"]["n_retired"]
        unchanged(check(rig, rig.run(status_word=False), again, mid, rig.cn), mid)
        # another keyframe on the same store: the marks of the first call are back at rest
        s1 = ref["store"]
        live = [f for f in range(len(s1["kf_bad"])) if not s1["kf_bad"][f] and case["life"]["kf_fid"][f] != 0 and f not in rig.protect]
        if live:
            rig.set([live[-1]], rig.protect)
            ref2 = restate(rig, next_state(case, ref))
            assert ref2["rec"]["n_retired"] == 1
            mid = rig.snapshot()
            check(rig, rig.run(), ref2, mid, rig.cn)
    finally:
        rig.free()


@pytest.mark.parametrize("name", ["points_1025", "point_of_300_loses_150", "weight_row_1025"])
def test_the_order_of_the_list_does_not_matter(ctx, name):
    """The same V ascending, descending and shuffled: identical store bytes and the same record."""
    case = CASES[name]
    V = sorted(case["list"])
    rng = np.random.default_rng(3)
    outs = []
    for lst in (V, V[::-1], [V[i] for i in rng.permutation(len(V))]):
        rig = Rig(ctx, dict(case, list=lst))
        try:
            before = rig.snapshot()
            ref = restate(rig, state_of(case))
            outs.append((check(rig, rig.run(), ref, before, rig.cn), ref["rec"]))
        finally:
            rig.free()
    for after, rec in outs[1:]:
        unchanged(after, outs[0][0])
        assert rec == outs[0][1]


@pytest.mark.parametrize("fail", ["src_status", "n_list_negative", "n_list_above"])
def test_refused_call_then_a_good_one(ctx, fail):
    """Status 1 stores the status and nothing else; the good call behind it equals the good call alone."""
    case = CASES["points_1023"]
    rig = Rig(ctx, case, n_max_list=4)
    try:
        kw = dict(src_status=dict(src_status=3), n_list_negative=dict(n_list=-1), n_list_above=dict(n_list=5))[fail]
        rig.set(case["list"], case["protect"], **kw)
        before = rig.snapshot()
        ref = restate(rig, state_of(case))
        assert ref["rec"] == dict(status=1)
        unchanged(check(rig, rig.run(), ref, before, rig.cn), before)
        rig.set(case["list"], case["protect"])
        ref = restate(rig, state_of(case))
        assert ref["rec"]["status"] == 0 and ref["rec"]["n_points_bad"] > 0
        before = rig.snapshot()
        check(rig, rig.run(status_word=fail != "src_status"), ref, before, rig.cn)
    finally:
        rig.free()


def test_a_damaged_obs_slot_is_counted_and_skipped(ctx):
    """Slots damaged behind create's check (the geometry view is device memory): a dying point's observation names a
    slot that holds another point; it is counted, the row keeps its entry."""
    case = copy.deepcopy(RC.build(3, [[0, 1, 2], [1, 2], [0, 1, 2]], lst=[0]))
    rig = Rig(ctx, case)
    try:
        slot = rig.store.geometry["obs_slot"].numpy()
        assert list(slot[:3]) == [0, 0, 0]
        slot[1] = 1                                          # p0's observation in kf1 now names the slot of p1
        h2d(ctx, rig.store.geometry["obs_slot"], slot)
        case["obs_slot"][0] = [0, 1, 0]
        case["geom"] = dict(case["geom"], obs_slot=case["obs_slot"])
        before = rig.snapshot()
        ref = restate(rig, state_of(case))
        assert ref["rec"]["n_obs_bad_slot"] == 1 and ref["rec"]["n_points_bad"] == 2 and ref["store"]["kf_slots"][1][0] == 0
        check(rig, rig.run(), ref, before, rig.cn)
    finally:
        rig.free()


def test_a_fresh_store_retires_nothing(ctx):
    """kf_fid = 0 everywhere, as create leaves it: if(mnId == 0) return; keeps every keyframe."""
    case = copy.deepcopy(CASES["points_1023"])
    case["life"]["kf_fid"][:] = 0
    rig = Rig(ctx, case)
    try:
        before = rig.snapshot()
        ref = restate(rig, state_of(case))
        assert ref["rec"]["n_retired"] == 0 and ref["rec"]["n_skip_first"] == 2
        unchanged(check(rig, rig.run(), ref, before, rig.cn), before)
    finally:
        rig.free()


def test_retire_errors(ctx):
    """LORB_E_INVALID before anything is enqueued; the next call is fine."""
    case = CASES["list_of_1"]
    rig = Rig(ctx, case)
    bare = KeyframeStore(ctx, 8, 8, 8, 8, init=RC.build(2, [[0, 1]])["store"])
    try:
        before = rig.snapshot()
        w = rig.words.ptr.value
        for kw, what in ((dict(n_max_list=0), "list bound"), (dict(n_max_list=1025), "list bound"),
                         (dict(n_protect=5, protect=w + 8), "protected"), (dict(n_protect=-1), "protected"),
                         (dict(n_protect=1), "null protected")):
            with pytest.raises(LorbError, match=what):
                keyframe_retire(ctx, rig.store, rig.list, w, rig.rec, **dict(dict(n_max_list=1), **kw))
        with pytest.raises(LorbError, match="geometry"):
            keyframe_retire(ctx, bare, rig.list, w, rig.rec, n_max_list=1)
        unchanged(rig.snapshot(), before)
        ref = restate(rig, state_of(case))
        check(rig, rig.run(), ref, before, rig.cn)
    finally:
        rig.free()
        bare.free()
