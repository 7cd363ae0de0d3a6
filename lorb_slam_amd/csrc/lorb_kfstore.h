// lorb_kfstore.h -- the keyframe store's object and what its units share.  The units: lorb_kfstore.hip (create /
// read / insertion, and the shared host helpers declared at the end of this file), lorb_kfba.hip (the local bundle
// adjustment fed from the store), lorb_kfcull.hip (the points' life and MapPointsCulling), lorb_kfcompact.hip
// (reclaiming the dead point rows), lorb_kfrefresh.hip (the appearance and the refresh of the window's points) and
// lorb_kfretire.hip (Frame::SetBadFlag: retiring keyframes).
// Shared on the device: clampi, kf_range (a clamped CSR row), tile_base_1024 (the earlier tiles' sum),
// kf_sort_keys_1024 (a weight map's (weight, index) keys sorted in LDS), kKfTile and
// KfPointRows -- THE list of the per-point arrays: a new per-point array of the store is added there.
#pragma once

#include "lorb_ba_slots.h"
#include "lorb_internal.h"

namespace lorb {

// k_kf_head's verdict and the counts an insertion's later kernels read
struct KfCtl {
  int go;                // the insertion runs
  int n, K, P, O, S;     // n_cur and the true counts on entry
  int n_obs_add, n_new;  // observations added to old points; adopted + created points
  int n_touch;           // neighbours whose weight map took K (touch[])
  int fallback;          // the largest-count neighbour when no count reached 3, else -1
  int n_connected;       // length of K's ordered list
  int pad;
};

constexpr int kKfTile = 1024;  // points per scan tile = threads per workgroup of the tiled kernels

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// row i of a CSR (a point's observation list, a keyframe's slot row, a covisibility row) inside the n entries the
// store holds: [lo, hi), empty rather than outside whatever the offsets say
struct KfRange {
  int lo, hi;
};
__device__ __forceinline__ KfRange kf_range(const int* off, int i, int n) {
  const int lo = clampi(off[i], 0, n);
  return {lo, clampi(off[i + 1], lo, n)};
}

// the sum of tile[0 .. n) in every thread of a 1024-thread workgroup: the rows in front of tile n.  Every thread
// calls it; it holds block_excl_scan_1024's two barriers.  wsum: __shared__ int[16]
__device__ __forceinline__ int tile_base_1024(const int* tile, int n, int* wsum) {
  int s = 0, base;
  for (int i = threadIdx.x; i < n; i += kKfTile) s += tile[i];
  block_excl_scan_1024(s, wsum, &base);
  return base;
}

// s_key[0 .. np2), np2 a power of two, sorted ascending in LDS by a 1024-thread workgroup (bitonic): the (weight,
// index) keys of one weight map, padded with ~0.  Every thread calls it; the keys are written and a barrier passed
// before the call, and it ends on a barrier.
__device__ __forceinline__ void kf_sort_keys_1024(unsigned long long* s_key, int np2) {
  const int t = threadIdx.x;
  for (int k = 2; k <= np2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int q = t; q < np2; q += 1024) {
        const int x = q ^ j;
        if (x > q) {
          const unsigned long long u = s_key[q], v = s_key[x];
          if ((u > v) == ((q & k) == 0)) {
            s_key[q] = v;
            s_key[x] = u;
          }
        }
      }
      __syncthreads();
    }
}

// The row of a point: every per-point array of the store, live (lorb_kf_store::point_rows) or a compaction's
// staging (stage_rows).  A new per-point array is added here -- member, copy_row, fresh_row, kStagedBytes -- and
// in the two builders and create_store's allocation below.
struct KfPointRows {
  float *pos, *normal, *max_dist, *min_dist;
  uint4* desc;
  uint8_t *locked, *is_bad, *recent;
  int *obs_off, *visible, *found, *first_fid;
  // bytes of one row without obs_off, whose staging is the insertion's off2: create_store's "79 bytes of rows"
  static constexpr size_t kStagedBytes = 2 * 12 + 2 * 4 + 32 + 3 * 1 + 3 * 4;
  // row dst of this set = row i of src
  __device__ __forceinline__ void copy_row(size_t dst, const KfPointRows& src, size_t i) const {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      pos[3 * dst + k] = src.pos[3 * i + k];
      normal[3 * dst + k] = src.normal[3 * i + k];
    }
    max_dist[dst] = src.max_dist[i]; min_dist[dst] = src.min_dist[i];
    desc[2 * dst] = src.desc[2 * i]; desc[2 * dst + 1] = src.desc[2 * i + 1];
    locked[dst] = src.locked[i]; is_bad[dst] = src.is_bad[i]; recent[dst] = src.recent[i];
    obs_off[dst] = src.obs_off[i];
    visible[dst] = src.visible[i]; found[dst] = src.found[i]; first_fid[dst] = src.first_fid[i];
  }
  // what a fresh store has in row o: zeros, is_bad = 1.  obs_off is the caller's.
  __device__ __forceinline__ void fresh_row(size_t o) const {
    const uint4 z4 = make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      pos[3 * o + k] = 0.f;
      normal[3 * o + k] = 0.f;
    }
    max_dist[o] = 0.f; min_dist[o] = 0.f;
    desc[2 * o] = z4; desc[2 * o + 1] = z4;
    locked[o] = 0; is_bad[o] = 1; recent[o] = 0;
    visible[o] = 0; found[o] = 0; first_fid[o] = 0;
  }
};
static_assert(KfPointRows::kStagedBytes == 79, "create_store's staging comment states the row's bytes");

constexpr int kKfBaMaxLocal = 128;  // the device plans' camera limit
constexpr int kKfBaNoFirst = 0x7f7f7f7f;  // ba_first[] at rest (a memset of 0x7f); above every sequence position

// the header of the last gathered window (device; the host reads it once per call)
struct KfBaHdr {
  int status;            // the record's status
  int go;                // the gather's later kernels run
  int C, F, P, K;        // local frames, fixed frames, window points, observations
  int maxk;              // the most usable observations of one window point
  int T;                 // the local frames' slots, concatenated
  int kf, n_kf, n_pts, n_obs_store, n_slots;  // K and the store's true counts on entry
  int n_cov_bad, n_obs_bad_kf, n_obs_bad_slot;
};

// k_kf_cull_head's verdict and the counts a cull's later kernels read (lorb_kfcull.hip)
struct KfCullCtl {
  int go;           // the cull runs
  int kf, cur;      // K and kf_fid[K]
  int nk, P, O, S;  // the true counts on entry
  int n_culled;     // points culled by this call: 0 makes the kernels after the verdicts return at once
};

// k_kf_retire_head's verdict and the counts a retirement's later kernels read (lorb_kfretire.hip)
struct KfRetireCtl {
  int go;           // the set V is not empty and the call runs
  int nk, P, O, S;  // the true counts on entry
  int n_v;          // keyframes in V (rt_v[0 .. n_v), in list order)
  int n_affected;   // points that lose an observation: 0 makes the scatter return at once
  int first_row;    // the lowest keyframe whose ordered list changes (integer min): the covisibility CSR is rebuilt from it
};

// k_kf_compact_head's verdict and the counts a compaction's later kernels read (lorb_kfcompact.hip)
struct KfCompactCtl {
  int go;       // the compaction runs
  int P, O, S;  // the true counts on entry
  int n_drop;   // rows dropped by this call: 0 makes the kernels after the count return at once
  int pad[3];
};

// what the refresh's point kernel leaves per window point for the record (lorb_kfrefresh.hip): no atomics
struct KfRefreshStat {
  int kind;          // 0 refreshed, 1 bad, 2 no observation inside the store
  int n_bad_slot;    // observations skipped: a keyframe or slot outside the store
  int n_desc_bits;   // bits of desc that changed
  int pad;
};

// the points' life as one block of ints, so that a kernel takes one pointer: visible | found | first_fid | recent
// (bytes) over max_points each, kf_fid over max_kf, the frame word; every part starts on a multiple of 64 ints
struct KfLife {
  int *visible, *found, *first_fid;
  uint8_t* recent;
  int *kf_fid, *frame_word;
  __host__ __device__ static size_t pad(size_t n) { return (n + 63) & ~size_t(63); }
  __host__ __device__ static size_t ints(int max_points, int max_kf) {
    return 3 * pad((size_t)max_points) + pad(((size_t)max_points + 3) / 4) + pad((size_t)max_kf) + 64;
  }
  __host__ __device__ KfLife(int* base, int max_points, int max_kf) {
    const size_t np = pad((size_t)max_points);
    visible = base;
    found = base + np;
    first_fid = base + 2 * np;
    recent = reinterpret_cast<uint8_t*>(base + 3 * np);
    kf_fid = base + 3 * np + pad(((size_t)max_points + 3) / 4);
    frame_word = kf_fid + pad((size_t)max_kf);
  }
};

}  // namespace lorb

struct lorb_kf_store {
  lorb_ctx* ctx = nullptr;
  lorb_kf_store_caps cap{};
  int max_cov = 0;                                          // max_kf * max_kf
  int b_kf = 0, b_points = 0, b_obs = 0, b_slots = 0, b_cov = 0;  // the host's bounds on the true counts
  bool geom_ok = false;  // kf_pose / kf_slot_uv / obs_slot cover every keyframe the store holds
  bool appear_ok = false;  // kf_slot_desc / kf_slot_octave / kf_center cover every keyframe the store holds
  bool window_current = false;  // w_l2g names the points as they are numbered now: a gather sets it, a compaction clears it
  lorb::Arena mem;
  // the lorb_map_store arrays
  float *pos = nullptr, *normal = nullptr, *max_dist = nullptr, *min_dist = nullptr;
  uint8_t *desc = nullptr, *locked = nullptr, *is_bad = nullptr, *kf_bad = nullptr;
  int *obs_off = nullptr, *obs_kf = nullptr, *kf_slot_off = nullptr, *kf_slot_point = nullptr;
  int *cov_off = nullptr, *cov_kf = nullptr;
  // the geometry: mRvec | mTvec per keyframe, GetKp2d per keyframe slot, the slot of every observation
  float *kf_pose = nullptr, *kf_slot_uv = nullptr;
  int* obs_slot = nullptr;
  // weight maps and ordered lists: rows of stride max_kf
  int *conn_n = nullptr, *conn_kf = nullptr, *conn_w = nullptr, *ord_n = nullptr, *ord_kf = nullptr;
  int* cnt = nullptr;  // n_kf, n_points, n_obs, n_kf_slots, n_cov, n_conn
  // scratch of an insertion
  int *owner = nullptr, *off2 = nullptr, *kf2 = nullptr, *slot2 = nullptr, *tile_cnt = nullptr, *touch = nullptr;
  lorb::KfCtl* ctl = nullptr;
  // the local BA's window (lorb_kfba.hip): gathered on the device, read by the plan in place
  lorb::KfBaHdr* ba_hdr = nullptr;
  int *ba_first = nullptr;   // per point: the first sequence position that holds it; at rest between calls
  int *ba_rank = nullptr, *ba_fixed_id = nullptr, *ba_fixed_flag = nullptr;  // per keyframe
  int *ba_seq_off = nullptr;  // kKfBaMaxLocal + 1
  int *ba_tile = nullptr, *ba_ocnt = nullptr, *ba_ooff = nullptr;
  int *w_local = nullptr, *w_fixed = nullptr, *w_l2g = nullptr, *w_obs_point = nullptr, *w_obs_frame = nullptr;
  float *w_pose = nullptr, *w_fixed_pose = nullptr, *w_point = nullptr, *w_uv = nullptr;
  lorb::KfBaHdr* h_hdr = nullptr;  // pinned
  // the points' life (lorb_kfcull.hip): mnVisible, mnFound, mnFirstFId, membership of mvpRecentAddPoints; mnId per
  // keyframe; the id of the frame the tracker last observed
  int* life = nullptr;  // the block lorb::KfLife lays out; the members below point into it
  int *visible = nullptr, *found = nullptr, *first_fid = nullptr, *kf_fid = nullptr, *frame_word = nullptr;
  uint8_t* recent = nullptr;
  uint8_t* cull_mark = nullptr;  // per point: culled by the call in flight; at rest (0) between calls
  lorb::KfCullCtl* cull_ctl = nullptr;
  // a compaction's staging (lorb_kfcompact.hip): the surviving point rows on their way to their new index (the
  // offsets ride in off2, the tile counts in tile_cnt), old -> new per point, and the holds
  float *cp_pos = nullptr, *cp_normal = nullptr, *cp_max_dist = nullptr, *cp_min_dist = nullptr;
  uint8_t *cp_desc = nullptr, *cp_locked = nullptr, *cp_is_bad = nullptr, *cp_recent = nullptr;
  int *cp_visible = nullptr, *cp_found = nullptr, *cp_first_fid = nullptr;
  int* cp_map = nullptr;       // per point: its rank among its tile's kept points, then its new index; -1: dropped
  uint8_t* cp_hold = nullptr;  // per point: bad and named by a keyframe slot or a gid table; at rest (0) between calls
  lorb::KfCompactCtl* cp_ctl = nullptr;
  // the appearance (lorb_kfrefresh.hip): GetDescriptor and mvKeysUn[].octave per keyframe slot, parallel to
  // kf_slot_point; mptCameraCenter per keyframe; the refresh's verdict per window point (lorb::KfRefreshStat)
  uint8_t* kf_slot_desc = nullptr;
  int* kf_slot_octave = nullptr;
  float* kf_center = nullptr;
  lorb::KfRefreshStat* rf_stat = nullptr;
  // a retirement's scratch (lorb_kfretire.hip): membership of V per keyframe, at rest (0) between calls; V itself
  // (LORB_KF_RETIRE_MAX_LIST words).  The points' marks ride in cull_mark, the CSR copy in off2 / kf2 / slot2, the
  // tile counts in tile_cnt.
  uint8_t* rt_mark = nullptr;
  int* rt_v = nullptr;
  lorb::KfRetireCtl* rt_ctl = nullptr;
  lorb::PlanSlots plans;
  // the point rows where they live, and a compaction's staging of them
  lorb::KfPointRows point_rows() const {
    return {pos, normal, max_dist, min_dist, reinterpret_cast<uint4*>(desc), locked, is_bad, recent, obs_off, visible, found,
            first_fid};
  }
  lorb::KfPointRows stage_rows() const {
    return {cp_pos, cp_normal, cp_max_dist, cp_min_dist, reinterpret_cast<uint4*>(cp_desc), cp_locked, cp_is_bad, cp_recent,
            off2, cp_visible, cp_found, cp_first_fid};
  }
};

// the host helpers the units share (lorb_kfstore.hip)
namespace lorb {

// the store's six true counts (n_kf, n_points, n_obs, n_kf_slots, n_cov, n_conn): one copy to the host, one wait
int kf_true_counts(lorb_kf_store* S, int32_t cnt[6]);
// one asynchronous copy to / from the device on the store's stream; a null host pointer or zero bytes is skipped
hipError_t kf_up(const lorb_kf_store* S, void* dst, const void* host, size_t bytes);
hipError_t kf_down(const lorb_kf_store* S, void* host, const void* src, size_t bytes);
// the entry check of the enqueued calls: LORB_E_INVALID for a null ctx or store and for a store of another context;
// with kKfNeedGeom / kKfNeedAppear also for a store whose initial keyframes lack the geometry / the appearance
enum { kKfNeedGeom = 1, kKfNeedAppear = 2 };
int kf_enter(lorb_ctx* ctx, const lorb_kf_store* S, int need = 0);

}  // namespace lorb
