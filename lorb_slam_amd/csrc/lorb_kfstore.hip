// lorb_kfstore.hip -- the map store as a device object that grows in the frame chain: lorb_kf_store_create /
// _destroy / _view / _counts / _read and lorb_kf_store_insert_dev, which is VisualOdometry::AddKeyFrame
// (src/visual_odometry.cpp:356-404) and the map part of Initialize (:86-103), LocalMapping::ProcessNewFrames
// step 1 (src/local_mapping.cpp:57-70) and Frame::UpdateConnections (src/frame.cpp:801-869) with AddConnection
// and UpdateBestCovisibleFrames (:754-788).
//
// Layout.  Every array of a lorb_map_store lives in place in one block (lorb::Arena) and its address never
// changes, so a view stays valid across insertions.  Points, kf_bad and the keyframe-slot CSR only ever grow at
// their ends.  The observation CSR takes K in the middle of its rows: it is rebuilt by count - scan - scatter
// through a scratch copy (rows in front of the first changed point stay where they are).  The weight maps and
// the ordered lists are kept as fixed-stride rows (stride max_kf) with a length per keyframe -- K is the largest
// index, so AddConnection appends -- and the covisibility CSR of the view is compacted from the ordered rows.
// The true counts live in cnt[6] on the device; the host object only carries upper bounds.
// The geometry a bundle adjustment needs rides along: kf_pose (mRvec | mTvec per keyframe), kf_slot_uv (GetKp2d
// per keyframe slot, parallel to kf_slot_point) and obs_slot (parallel to obs_kf: the slot of the point in that
// keyframe, kf_slot_point[kf_slot_off[f] + obs_slot[o]] == p).  lorb_kfba.hip reads them.
//
// An insertion is six launches on the ctx stream:
//   k_kf_head         one workgroup walking the slots: status, gate, the classification of every slot, the
//                     lowest-slot owner of every held point (atomicMin on a per-point word that is at rest
//                     between calls), the counts, the capacity verdict -- all before the first store write --
//                     then the ordered numbering of the new points, their rows, the slots, the gids, K's slot
//                     row with its keypoints, K's pose vector, the counts, the refer words and the record; a new
//                     point's slot is left in owner[] for k_kf_obs_scatter; the points' life (lorb_kfcull.hip):
//                     kf_fid[K], a new point's visible, found, first_fid, recent for created points and for an
//                     old point K holds in two or more slots; K's appearance (lorb_kfrefresh.hip): the descriptor and
//                     octave of every slot, the camera centre
//   k_kf_obs_count    owners per 1024-point tile; the observation CSR (keyframes and slots) copied to scratch
//   k_kf_obs_scatter  the CSR back with K (and its owning slot) appended to the owned points' lists, the new
//                     points' lists {K} with the slot that made them
//   k_kf_connect      one workgroup: UpdateConnections' counter (k_lm_vote's pattern, kCountWin keyframes in LDS
//                     at a time), K's weight map, the pairs, AddConnection's append to each neighbour's map
//   k_kf_order        one workgroup per changed row: the (weight, index) keys sorted in LDS (bitonic)
//   k_kf_cov          the covisibility CSR from the ordered rows
// Every kernel after the first returns on the first one's verdict (Ctl::go).  All index arithmetic is integer:
// the results do not depend on the order the atomics arrive in.
#include <algorithm>

#include "lorb_internal.h"
#include "lorb_kfstore.h"

namespace {

constexpr int kWalk = 1024;      // threads of the one-workgroup walks over the slots
constexpr int kTile = lorb::kKfTile;  // points per scan tile = threads per workgroup
constexpr int kCountWin = 1024;  // keyframes whose counters are held in LDS at a time
constexpr int kSortMax = 4096;   // keys of one row sort in LDS = the largest max_kf
constexpr int kNoOwner = 0x7f7f7f7f;  // owner[] at rest (a memset of 0x7f); above every slot index
static_assert(kCountWin == kWalk && kTile == kWalk, "one counter / one point per thread");

using Ctl = lorb::KfCtl;

}  // namespace

namespace {

struct HeadArgs {
  lorb_frame_params fp;
  const int* count;  // the frame's counts (entry 0)
  int n_max, gate;
  const int* src_status;  // or null
  const lorb_frame_pose* pose;
  // the frame
  const float *x, *y, *depth;
  const int* octave;
  const uint4* fdesc;
  // the slots
  uint8_t* state;
  float* spos;
  uint4* sdesc;
  int* gid;
  // the store
  int max_kf, max_points, max_obs, max_kf_slots;
  float *pos, *normal, *max_dist, *min_dist;
  uint4* desc;
  uint8_t *locked, *is_bad, *kf_bad;
  int *kf_slot_off, *kf_slot_point;
  float *kf_pose, *kf_slot_uv;
  int* life;  // the points' life (lorb_kfcull.hip): one block, lorb::KfLife's layout over max_points / max_kf
  // the appearance (lorb_kfrefresh.hip)
  uint4* kf_slot_desc;
  int* kf_slot_octave;
  float* kf_center;
  int *cnt, *owner;
  Ctl* ctl;
  int* refer_kf;                  // or null
  lorb_local_map_result* update;  // or null
  lorb_kf_insert_result* rec;
};

enum { kStay = 0, kHeldBad, kObserve, kAdopt, kCreate };

// step d's case of slot j; *g: the store point it holds (kHeldBad, kObserve)
__device__ __forceinline__ int slot_kind(const HeadArgs& a, int j, int P, int* g) {
  if (a.state[j] == LORB_SLOT_EMPTY) return a.depth[j] >= 0 ? kCreate : kStay;
  const int id = a.gid[j];
  if ((unsigned)id >= (unsigned)P) return kAdopt;  // -1, or an index outside the store: a point UpdateFrame created
  *g = id;
  return a.is_bad[id] ? kHeldBad : kObserve;
}

// a new store point seen from K alone: MapPoint::UpdateNormalAndDepth over one observation
// (src/map_point.cpp:224-264), OpenCV's arithmetic restated (lorb_c.h): cv::norm accumulates in double
__device__ __forceinline__ void new_point(const HeadArgs& a, int at, const float* p, const uint4& d0, const uint4& d1,
                                          const float* Ow, int octave, const lorb::KfLife& life, int fid, int created) {
#pragma clang fp contract(off)
  const float dx = p[0] - Ow[0], dy = p[1] - Ow[1], dz = p[2] - Ow[2];
  const double nd = sqrt((double)dx * (double)dx + (double)dy * (double)dy + (double)dz * (double)dz);
  const float inv = (float)(1.0 / nd), dist = (float)nd;
  const int lvl = lorb::clampi(octave, 0, LORB_MAX_LEVELS - 1), top = lorb::clampi(a.fp.n_levels - 1, 0, LORB_MAX_LEVELS - 1);
  const float mx = dist * a.fp.scale_factors[lvl];
  const size_t r = (size_t)at;
  a.pos[3 * r] = p[0]; a.pos[3 * r + 1] = p[1]; a.pos[3 * r + 2] = p[2];
  a.normal[3 * r] = dx * inv; a.normal[3 * r + 1] = dy * inv; a.normal[3 * r + 2] = dz * inv;
  a.max_dist[r] = mx;
  a.min_dist[r] = mx / a.fp.scale_factors[top];
  a.desc[2 * r] = d0;
  a.desc[2 * r + 1] = d1;
  a.locked[r] = 1;
  a.is_bad[r] = 0;
  // its life starts with this frame; a created point already has K as an observation, so ProcessNewFrames pushes
  // it to mvpRecentAddPoints (src/local_mapping.cpp:62-69); an adopted one gets AddObservation there
  life.visible[r] = 1;
  life.found[r] = 1;
  life.first_fid[r] = fid;
  life.recent[r] = (uint8_t)created;
}

__global__ __launch_bounds__(kWalk) void k_kf_head(HeadArgs a) {
  __shared__ lorb::I4 wsum4[16];
  __shared__ int wsum[16];
  const int t = threadIdx.x;
  const int n = a.count[0];
  // a. status
  const bool ok = n >= 0 && n <= a.n_max && a.pose->status == 0 && !(a.src_status && *a.src_status != 0);
  if (!ok) {
    if (t == 0) {
      a.rec->status = 1;
      a.ctl->go = 0;
    }
    return;
  }
  const int K = a.cnt[0], P = a.cnt[1], O = a.cnt[2], S = a.cnt[3];
  // b. the gate (:360-372)
  lorb::I4 c = {{0, 0, 0, 0}}, tot;
  for (int j = t; j < n; j += kWalk) c.v[0] += a.state[j] != LORB_SLOT_EMPTY;
  lorb::block_excl_scan4<kWalk>(c, wsum4, &tot);
  const int n_map = tot.v[0];
  const float ratio = (float)n_map / (float)n;  // NaN for an empty frame: not above
  if (a.gate == LORB_KF_GATE_RATIO && ratio > 0.35f) {
    if (t == 0) {
      a.rec->status = 0;
      a.rec->inserted = 0;
      a.rec->n_map = n_map;
      a.ctl->go = 0;
    }
    return;
  }
  // the owner of every held point: its lowest slot.  owner[] is at rest (kNoOwner) between calls.
  c = lorb::I4{{0, 0, 0, 0}};
  for (int j = t; j < n; j += kWalk) {
    int g = -1;
    const int kind = slot_kind(a, j, P, &g);
    if (kind == kObserve) atomicMin(&a.owner[g], j);
    c.v[1] += kind == kAdopt;
    c.v[2] += kind == kCreate;
  }
  __syncthreads();  // the owners are settled
  for (int j = t; j < n; j += kWalk) {
    int g = -1;
    if (slot_kind(a, j, P, &g) == kObserve)
      c.v[0] += __hip_atomic_load(&a.owner[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == j;
  }
  lorb::block_excl_scan4<kWalk>(c, wsum4, &tot);
  const int n_observed = tot.v[0], n_adopted = tot.v[1], n_created = tot.v[2], n_new = n_adopted + n_created;
  // c. capacity, before the first store write
  const bool full = K + 1 > a.max_kf || (long long)P + n_new > a.max_points ||
                    (long long)O + n_observed + n_new > a.max_obs || (long long)S + n > a.max_kf_slots;
  if (full) {
    for (int j = t; j < n; j += kWalk) {
      int g = -1;
      if (slot_kind(a, j, P, &g) == kObserve) a.owner[g] = kNoOwner;
    }
    if (t == 0) {
      *a.rec = lorb_kf_insert_result{2, 0, n, n_map, -1, n_observed, n_adopted, n_created, 0, P, K, O};
      a.ctl->go = 0;
    }
    return;
  }
  // d + e. the slots in ascending order, 1024 at a time: a new point's index is n_points + the new points
  // before it
  lorb::Mat4f twc;
#pragma unroll
  for (int k = 0; k < 16; ++k) twc.v[k] = a.pose->Twc[k];
  const float Ow[3] = {twc.v[3], twc.v[7], twc.v[11]};
  const lorb::KfLife life(a.life, a.max_points, a.max_kf);
  const int fid = life.frame_word[0];  // mCurrFrame->mnId, as lorb_kf_store_observe_dev left it
  int run = 0;
  for (int base = 0; base < n; base += kWalk) {
    const int j = base + t;
    int kind = kStay, g = -1;
    if (j < n) kind = slot_kind(a, j, P, &g);
    const int is_new = kind == kAdopt || kind == kCreate;
    int made;
    const int at = P + run + lorb::block_excl_scan_1024(is_new, wsum, &made);
    run += made;
    if (j >= n) continue;
    int row = -1;
    if (kind == kHeldBad) {
      row = g;  // src/local_mapping.cpp:60-61
    } else if (kind == kObserve) {
      row = g;  // AddObservation: the owner's mark stays for k_kf_obs_scatter
      a.locked[g] = 1;
      a.state[j] = LORB_SLOT_LOCKED;
      // a later slot of a point held twice finds IsInFrame true: pushed (src/local_mapping.cpp:66-69)
      if (__hip_atomic_load(&a.owner[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != j) life.recent[g] = 1;
    } else if (is_new) {
      float p[3];
      uint4 d0, d1;
      if (kind == kAdopt) {
        p[0] = a.spos[3 * (size_t)j]; p[1] = a.spos[3 * (size_t)j + 1]; p[2] = a.spos[3 * (size_t)j + 2];
        d0 = a.sdesc[2 * (size_t)j];
        d1 = a.sdesc[2 * (size_t)j + 1];
      } else {
        lorb::unproject_kp(a.fp, twc, a.x[j], a.y[j], a.depth[j], p);
        d0 = a.fdesc[2 * (size_t)j];
        d1 = a.fdesc[2 * (size_t)j + 1];
        a.spos[3 * (size_t)j] = p[0]; a.spos[3 * (size_t)j + 1] = p[1]; a.spos[3 * (size_t)j + 2] = p[2];
        a.sdesc[2 * (size_t)j] = d0;
        a.sdesc[2 * (size_t)j + 1] = d1;
      }
      a.state[j] = LORB_SLOT_LOCKED;
      new_point(a, at, p, d0, d1, Ow, a.octave[j], life, fid, kind == kCreate);
      a.owner[at] = j;  // the slot that adopted or created it: k_kf_obs_scatter's obs_slot, which puts the word to rest
      row = at;
    }
    if (kind != kHeldBad && kind != kObserve) a.gid[j] = row;  // the new index; -1 for a slot left EMPTY
    a.kf_slot_point[S + j] = row;
    a.kf_slot_uv[2 * ((size_t)S + j)] = a.x[j];  // GetKp2d(j)
    a.kf_slot_uv[2 * ((size_t)S + j) + 1] = a.y[j];
    a.kf_slot_desc[2 * ((size_t)S + j)] = a.fdesc[2 * (size_t)j];  // GetDescriptor(j), mvKeysUn[j].octave: what new_point reads
    a.kf_slot_desc[2 * ((size_t)S + j) + 1] = a.fdesc[2 * (size_t)j + 1];
    a.kf_slot_octave[(size_t)S + j] = a.octave[j];
  }
  if (t < 3) a.kf_center[3 * (size_t)K + t] = Ow[t];  // mptCameraCenter
  if (t < 6) a.kf_pose[6 * (size_t)K + t] = a.pose->pose[t];  // mRvec | mTvec
  if (t == 0) {
    a.kf_bad[K] = 0;
    life.kf_fid[K] = fid;
    a.kf_slot_off[K + 1] = S + n;
    a.cnt[0] = K + 1; a.cnt[1] = P + n_new; a.cnt[2] = O + n_observed + n_new; a.cnt[3] = S + n;
    *a.ctl = Ctl{1, n, K, P, O, S, n_observed, n_new, 0, -1, 0, 0};
    // n_connected is k_kf_connect's
    a.rec->status = 0; a.rec->inserted = 1; a.rec->n_cur = n; a.rec->n_map = n_map; a.rec->kf = K;
    a.rec->n_observed = n_observed; a.rec->n_adopted = n_adopted; a.rec->n_created = n_created;
    a.rec->n_points = P + n_new; a.rec->n_kf = K + 1; a.rec->n_obs = O + n_observed + n_new;
    if (a.refer_kf) *a.refer_kf = K;  // g. mReferFrame = mCurrFrame (:402)
    if (a.update) a.update->refer_kf = K;
  }
}

// owners per tile of the old points; the observation CSR as it stands into scratch
__global__ __launch_bounds__(kTile) void k_kf_obs_count(const Ctl* ctl, const int* owner, const int* obs_off,
                                                        const int* obs_kf, const int* obs_slot, int* off2, int* kf2,
                                                        int* slot2, int* tile_cnt) {
  __shared__ int wsum[16];
  if (!ctl->go) return;
  const int P = ctl->P, O = ctl->O;
  const int p = blockIdx.x * kTile + threadIdx.x;
  if (p <= P) off2[p] = obs_off[p];
  int tot;
  lorb::block_excl_scan_1024(p < P && owner[p] != kNoOwner, wsum, &tot);
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = tot;
  for (long long o = p; o < O; o += (long long)gridDim.x * kTile) {
    kf2[o] = obs_kf[o];
    slot2[o] = obs_slot[o];
  }
}

// the CSR back: point p's list moves right by the owned points before it and takes K when p is owned; the new
// points' lists are {K}.  Launched over the bound on n_points + n_max_cur + 1.
__global__ __launch_bounds__(kTile) void k_kf_obs_scatter(const Ctl* ctl, int* owner, const int* off2, const int* kf2,
                                                          const int* slot2, const int* tile_cnt, int* obs_off, int* obs_kf,
                                                          int* obs_slot) {
  __shared__ int wsum[16];
  if (!ctl->go) return;
  const int t = threadIdx.x, b = blockIdx.x;
  const int P = ctl->P, O = ctl->O, K = ctl->K, n_add = ctl->n_obs_add, n_new = ctl->n_new;
  if ((long long)b * kTile > (long long)P + n_new) return;
  const int n_tiles = (P + kTile - 1) / kTile;
  int tot;
  const int base = lorb::tile_base_1024(tile_cnt, min(b, n_tiles), wsum);
  const int p = b * kTile + t;
  const int f = p < P && owner[p] != kNoOwner;
  const int before = base + lorb::block_excl_scan_1024(f, wsum, &tot);
  if (p < P) {
    const int lo = off2[p], hi = off2[p + 1], at = lo + before;
    if (before) {
      obs_off[p] = at;
      for (int o = lo; o < hi; ++o) {
        obs_kf[at + (o - lo)] = kf2[o];
        obs_slot[at + (o - lo)] = slot2[o];
      }
    }
    if (f) {
      obs_kf[at + (hi - lo)] = K;  // the largest index: last (src/map_point.cpp:133-139)
      obs_slot[at + (hi - lo)] = owner[p];  // mObservations[K]: the lowest slot that holds p
      owner[p] = kNoOwner;
    }
  } else if (p <= P + n_new) {
    const int at = O + n_add + (p - P);
    obs_off[p] = at;
    if (p < P + n_new) {
      obs_kf[at] = K;
      obs_slot[at] = owner[p];  // k_kf_head left the new point's slot here
      owner[p] = kNoOwner;
    }
  }
}

// Frame::UpdateConnections(K)'s counter and step 2 (src/frame.cpp:801-849), one workgroup
__global__ __launch_bounds__(kWalk) void k_kf_connect(Ctl* ctl, const int* kf_slot_point, const uint8_t* is_bad,
                                                      const int* obs_off, const int* obs_kf, int stride, int* conn_n,
                                                      int* conn_kf, int* conn_w, int* touch, int* cnt,
                                                      lorb_kf_insert_result* rec) {
  __shared__ lorb::I4 wsum4[16];
  __shared__ unsigned long long wkey[16];
  __shared__ int s_cnt[kCountWin];
  if (!ctl->go) return;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int n = ctl->n, K = ctl->K, P = ctl->P, S = ctl->S, O1 = ctl->O + ctl->n_obs_add + ctl->n_new;
  const size_t rowK = (size_t)K * stride;
  int n_conn = 0, n_pairs = 0, best_v = 0, best_k = 0;
  for (int w0 = 0; w0 < K; w0 += kCountWin) {
    const int wn = min(kCountWin, K - w0);
    s_cnt[t] = 0;
    __syncthreads();
    // :808-822, per slot: a point held in two slots counts twice.  The new points (>= P) are seen by K alone.
    for (int j = t; j < n; j += kWalk) {
      const int g = kf_slot_point[S + j];
      if ((unsigned)g >= (unsigned)P || is_bad[g]) continue;
      const int lo = min(max(obs_off[g], 0), O1), hi = min(max(obs_off[g + 1], lo), O1);
      for (int o = lo; o < hi; ++o) {
        const int kf = obs_kf[o] - w0;  // K itself lies above every window (:819)
        if ((unsigned)kf < (unsigned)wn) atomicAdd(&s_cnt[kf], 1);
      }
    }
    __syncthreads();
    const int k = w0 + t, v = t < wn ? s_cnt[t] : 0;
    lorb::I4 tot;
    const lorb::I4 at = lorb::block_excl_scan4<kWalk>(lorb::I4{{v > 0, v >= 3, 0, 0}}, wsum4, &tot);
    if (v > 0) {  // mConnectedKeyFrameWeights = frameCounter (:855), in ascending index
      conn_kf[rowK + n_conn + at.v[0]] = k;
      conn_w[rowK + n_conn + at.v[0]] = v;
      if (v > best_v) { best_v = v; best_k = k; }  // ascending k per thread: the first of equals stays
    }
    if (v >= 3) {  // :838-842; f.AddConnection(K, v): K is f's largest key (:777-782)
      touch[n_pairs + at.v[1]] = k;
      const int i = conn_n[k];
      if (i < stride) {
        conn_kf[(size_t)k * stride + i] = K;
        conn_w[(size_t)k * stride + i] = v;
        conn_n[k] = i + 1;
      }
    }
    n_conn += tot.v[0];
    n_pairs += tot.v[1];
  }
  unsigned long long key = best_v > 0 ? ((unsigned long long)best_v << 32) | (unsigned)(0x7fffffff - best_k) : 0ull;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) key = max(key, (unsigned long long)__shfl_xor((long long)key, o, 64));
  if (lane == 0) wkey[wv] = key;
  __syncthreads();
  if (t != 0) return;
  unsigned long long kmax = 0;
  for (int w = 0; w < 16; ++w) kmax = max(kmax, wkey[w]);
  int n_touch = n_pairs, fallback = -1;
  if (n_pairs == 0 && kmax) {  // :845-849 restated: the first keyframe with the strictly largest count
    const int f = 0x7fffffff - (int)(unsigned)(kmax & 0xffffffffull), w = (int)(kmax >> 32), i = conn_n[f];
    if (i < stride) {
      conn_kf[(size_t)f * stride + i] = K;
      conn_w[(size_t)f * stride + i] = w;
      conn_n[f] = i + 1;
    }
    touch[0] = f;
    fallback = f;
    n_touch = 1;
  }
  conn_n[K] = n_conn;
  ctl->n_touch = n_touch;
  ctl->fallback = fallback;
  ctl->n_connected = n_touch;
  rec->n_connected = n_touch;
  cnt[5] += n_conn + n_touch;
}

// UpdateBestCovisibleFrames (:754-774) for every neighbour that took K -- ALL of its weight map, entries below
// 3 included -- and K's own pairs (:851): ascending by (weight, index).  One workgroup per row, keys in LDS.
__global__ __launch_bounds__(1024) void k_kf_order(const Ctl* ctl, const int* touch, int stride, const int* conn_n,
                                                   const int* conn_kf, const int* conn_w, int* ord_n, int* ord_kf) {
  __shared__ unsigned long long s_key[kSortMax];
  if (!ctl->go) return;
  const int t = threadIdx.x, K = ctl->K, n_touch = ctl->n_touch, fb = ctl->fallback;
  for (int i = blockIdx.x; i <= n_touch; i += gridDim.x) {
    const bool own = i == n_touch;
    const int r = own ? K : touch[i];
    const size_t row = (size_t)r * stride;
    const int m = min(conn_n[r], kSortMax);
    int np2 = 1;
    while (np2 < m) np2 <<= 1;
    for (int q = t; q < np2; q += 1024) {
      unsigned long long key = ~0ull;
      if (q < m) {
        const int w = conn_w[row + q], kf = conn_kf[row + q];
        if (!own || w >= 3 || kf == fb) key = ((unsigned long long)(unsigned)w << 32) | (unsigned)kf;
      }
      s_key[q] = key;
    }
    __syncthreads();
    lorb::kf_sort_keys_1024(s_key, np2);
    const int len = own ? ctl->n_connected : m;  // K's keys outside the pairs sorted to the end
    for (int q = t; q < len; q += 1024) ord_kf[row + q] = (int)(unsigned)(s_key[q] & 0xffffffffull);
    if (t == 0) ord_n[r] = len;
    __syncthreads();
  }
}

// mvpOrderedKeyFrames as the view's CSR: every workgroup scans the row lengths (at most kSortMax), then copies
// its share of the rows from the first changed one on
__global__ __launch_bounds__(1024) void k_kf_cov(const Ctl* ctl, const int* touch, int stride, const int* ord_n,
                                                 const int* ord_kf, int* cov_off, int* cov_kf, int* cnt) {
  __shared__ int s_off[kSortMax + 1];
  __shared__ int wsum[16];
  if (!ctl->go) return;
  const int t = threadIdx.x, K = ctl->K, nk = K + 1;
  int run = 0;
  for (int base = 0; base < nk; base += 1024) {
    const int k = base + t;
    int tot;
    const int at = run + lorb::block_excl_scan_1024(k < nk ? ord_n[k] : 0, wsum, &tot);
    if (k < nk) s_off[k] = at;
    run += tot;
  }
  if (t == 0) s_off[nk] = run;
  __syncthreads();
  const int first = ctl->n_touch ? touch[0] : K;  // touch[] ascends
  if (blockIdx.x == 0) {
    for (int k = first + t; k <= nk; k += 1024) cov_off[k] = s_off[k];
    if (t == 0) cnt[4] = run;
  }
  for (int f = first + blockIdx.x; f < nk; f += gridDim.x) {
    const int lo = s_off[f], len = s_off[f + 1] - lo;
    for (int q = t; q < len; q += 1024) cov_kf[lo + q] = ord_kf[(size_t)f * stride + q];
  }
}

// offsets of a CSR over n rows: ascending from 0 to len
bool csr_ok(const int32_t* off, int n, int len) {
  if (!off || off[0] != 0 || off[n] != len) return false;
  for (int i = 0; i < n; ++i)
    if (off[i + 1] < off[i]) return false;
  return true;
}

const char* init_fault(const lorb_kf_store_caps& c, int max_cov, const lorb_kf_store_host& h) {
  if (h.n_kf < 0 || h.n_points < 0 || h.n_obs < 0 || h.n_kf_slots < 0 || h.n_cov < 0 || h.n_conn < 0) return "negative sizes";
  if (h.n_kf > c.max_kf || h.n_points > c.max_points || h.n_obs > c.max_obs || h.n_kf_slots > c.max_kf_slots ||
      h.n_cov > max_cov || h.n_conn > max_cov)
    return "a count exceeds its capacity";
  if (h.n_points > 0 && (!h.pos || !h.normal || !h.max_dist || !h.min_dist || !h.desc || !h.locked)) return "null array";
  if ((h.n_obs > 0 && !h.obs_kf) || (h.n_kf_slots > 0 && !h.kf_slot_point) || (h.n_cov > 0 && !h.cov_kf) ||
      (h.n_conn > 0 && (!h.conn_kf || !h.conn_w)))
    return "null array";
  if (h.n_points > 0 || h.n_obs > 0) {
    if (!csr_ok(h.obs_off, h.n_points, h.n_obs)) return "obs_off is no CSR over the points";
  }
  if (h.n_kf > 0 || h.n_kf_slots > 0 || h.n_cov > 0 || h.n_conn > 0) {
    if (!csr_ok(h.kf_slot_off, h.n_kf, h.n_kf_slots) || !csr_ok(h.cov_off, h.n_kf, h.n_cov) ||
        !csr_ok(h.conn_off, h.n_kf, h.n_conn))
      return "a keyframe table's offsets are no CSR over the keyframes";
  }
  for (int o = 0; o < h.n_obs; ++o)
    if (h.obs_kf[o] < 0 || h.obs_kf[o] >= h.n_kf) return "obs_kf names a keyframe outside the store";
  for (int s = 0; s < h.n_kf_slots; ++s)
    if (h.kf_slot_point[s] < -1 || h.kf_slot_point[s] >= h.n_points) return "kf_slot_point names a point outside the store";
  for (int s = 0; s < h.n_cov; ++s)
    if (h.cov_kf[s] < 0 || h.cov_kf[s] >= h.n_kf) return "cov_kf names a keyframe outside the store";
  for (int k = 0; k < h.n_kf; ++k) {
    if (h.cov_off[k + 1] - h.cov_off[k] > c.max_kf) return "a covisibility list is longer than max_kf";
    for (int s = h.conn_off[k]; s < h.conn_off[k + 1]; ++s) {
      if (h.conn_kf[s] < 0 || h.conn_kf[s] >= h.n_kf || h.conn_w[s] < 0) return "a weight map entry is outside the store";
      if (s > h.conn_off[k] && h.conn_kf[s] <= h.conn_kf[s - 1]) return "a weight map row is not strictly ascending";
    }
  }
  return nullptr;
}

// the geometry of an init that init_fault passed: the counts are init's, and every observation's slot lies in
// its keyframe's row and holds its point.  msg: the offending entry.
bool geom_fault(const lorb_kf_store_host& h, const lorb_kf_store_geom_host& g, char* msg, size_t n) {
  if (g.n_kf != h.n_kf || g.n_kf_slots != h.n_kf_slots || g.n_obs != h.n_obs) {
    snprintf(msg, n, "counts %d / %d / %d differ from init's %d / %d / %d (kf, slots, obs)", g.n_kf, g.n_kf_slots, g.n_obs,
             h.n_kf, h.n_kf_slots, h.n_obs);
    return true;
  }
  if ((g.n_kf > 0 && !g.kf_pose) || (g.n_kf_slots > 0 && !g.kf_slot_uv) || (g.n_obs > 0 && !g.obs_slot)) {
    snprintf(msg, n, "null array");
    return true;
  }
  for (int p = 0; p < h.n_points; ++p)
    for (int o = h.obs_off[p]; o < h.obs_off[p + 1]; ++o) {
      const int f = h.obs_kf[o], s = g.obs_slot[o], len = h.kf_slot_off[f + 1] - h.kf_slot_off[f];
      if (s < 0 || s >= len) {
        snprintf(msg, n, "obs_slot[%d] = %d (point %d in keyframe %d) is outside the keyframe's %d slots", o, s, p, f, len);
        return true;
      }
      if (h.kf_slot_point[h.kf_slot_off[f] + s] != p) {
        snprintf(msg, n, "obs_slot[%d] = %d (point %d in keyframe %d) names a slot that holds %d", o, s, p, f,
                 h.kf_slot_point[h.kf_slot_off[f] + s]);
        return true;
      }
    }
  return false;
}

int create_store(lorb_ctx* ctx, const lorb_kf_store_caps* caps, const lorb_kf_store_host* init,
                 const lorb_kf_store_geom_host* geom, lorb_kf_store** out);

}  // namespace

// the host helpers the store's units share (lorb_kfstore.h)
namespace lorb {

int kf_true_counts(lorb_kf_store* S, int32_t cnt[6]) {
  lorb_ctx* ctx = S->ctx;
  LORB_HIP(ctx, hipMemcpyAsync(cnt, S->cnt, 6 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  LORB_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return LORB_OK;
}

hipError_t kf_up(const lorb_kf_store* S, void* dst, const void* host, size_t bytes) {
  return bytes && host ? hipMemcpyAsync(dst, host, bytes, hipMemcpyHostToDevice, S->ctx->stream) : hipSuccess;
}

hipError_t kf_down(const lorb_kf_store* S, void* host, const void* src, size_t bytes) {
  return bytes && host ? hipMemcpyAsync(host, src, bytes, hipMemcpyDeviceToHost, S->ctx->stream) : hipSuccess;
}

int kf_enter(lorb_ctx* ctx, const lorb_kf_store* S, int need) {
  if (!ctx || !S) return LORB_E_INVALID;
  if (S->ctx != ctx) return set_error(ctx, LORB_E_INVALID, "the keyframe store belongs to another context");
  if ((need & kKfNeedGeom) && !S->geom_ok)
    return set_error(ctx, LORB_E_INVALID, "the keyframe store has no geometry for its initial keyframes "
                                          "(lorb_kf_store_create_geom)");
  if ((need & kKfNeedAppear) && !S->appear_ok)
    return set_error(ctx, LORB_E_INVALID, "the keyframe store has no appearance for its initial keyframes "
                                          "(lorb_kf_store_appear_write)");
  return LORB_OK;
}

}  // namespace lorb

extern "C" {

int lorb_kf_store_destroy(lorb_kf_store* S) {
  if (!S) return LORB_E_INVALID;
  if (S->ctx) (void)hipStreamSynchronize(S->ctx->stream);
  S->plans.release_all();
  if (S->h_hdr) (void)hipHostFree(S->h_hdr);
  S->mem.release();
  delete S;
  return LORB_OK;
}

int lorb_kf_store_create(lorb_ctx* ctx, const lorb_kf_store_caps* caps, const lorb_kf_store_host* init, lorb_kf_store** out) {
  return create_store(ctx, caps, init, nullptr, out);
}

int lorb_kf_store_create_geom(lorb_ctx* ctx, const lorb_kf_store_caps* caps, const lorb_kf_store_host* init,
                              const lorb_kf_store_geom_host* geom, lorb_kf_store** out) {
  if (!ctx) return LORB_E_INVALID;
  if (!out) return lorb::set_error(ctx, LORB_E_INVALID, "null output");
  *out = nullptr;
  if (!geom) return lorb::set_error(ctx, LORB_E_INVALID, "null geometry");
  if (!init && (geom->n_kf || geom->n_kf_slots || geom->n_obs))
    return lorb::set_error(ctx, LORB_E_INVALID, "geom: counts without an init");
  return create_store(ctx, caps, init, geom, out);
}

int lorb_kf_store_geom_view(const lorb_kf_store* S, lorb_kf_store_geom_host* v) {
  if (!S || !v) return LORB_E_INVALID;
  *v = lorb_kf_store_geom_host{S->cap.max_kf, S->cap.max_kf_slots, S->cap.max_obs, S->kf_pose, S->kf_slot_uv, S->obs_slot};
  return LORB_OK;
}

int lorb_kf_store_geom_read(lorb_kf_store* S, const lorb_kf_store_geom_host* g) {
  if (!S || !g) return LORB_E_INVALID;
  lorb_ctx* ctx = S->ctx;
  int32_t cnt[6];
  LORB_TRY(lorb::kf_true_counts(S, cnt));
  const int nk = cnt[0], no = cnt[2], ns = cnt[3];
  if ((g->kf_pose && g->n_kf < nk) || (g->kf_slot_uv && g->n_kf_slots < ns) || (g->obs_slot && g->n_obs < no))
    return lorb::set_error(ctx, LORB_E_INVALID, "an output array is smaller than the store's count (%d kf, %d slots, %d obs)", nk,
                           ns, no);
  LORB_HIP(ctx, lorb::kf_down(S, g->kf_pose, S->kf_pose, (size_t)nk * 24));
  LORB_HIP(ctx, lorb::kf_down(S, g->kf_slot_uv, S->kf_slot_uv, (size_t)ns * 8));
  LORB_HIP(ctx, lorb::kf_down(S, g->obs_slot, S->obs_slot, (size_t)no * 4));
  LORB_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return LORB_OK;
}

}  // extern "C"

namespace {

int create_store(lorb_ctx* ctx, const lorb_kf_store_caps* caps, const lorb_kf_store_host* init,
                 const lorb_kf_store_geom_host* geom, lorb_kf_store** out) {
  if (!ctx) return LORB_E_INVALID;
  if (!out) return lorb::set_error(ctx, LORB_E_INVALID, "null output");
  *out = nullptr;
  if (!caps) return lorb::set_error(ctx, LORB_E_INVALID, "null capacities");
  if (caps->max_kf < 1 || caps->max_points < 1 || caps->max_obs < 1 || caps->max_kf_slots < 1)
    return lorb::set_error(ctx, LORB_E_INVALID, "capacities %d / %d / %d / %d must be positive", caps->max_kf,
                           caps->max_points, caps->max_obs, caps->max_kf_slots);
  if (caps->max_kf > kSortMax)
    return lorb::set_error(ctx, LORB_E_INVALID, "max_kf %d exceeds %d, the keyframe row an insertion sorts in LDS", caps->max_kf,
                           kSortMax);
  const int max_cov = caps->max_kf * caps->max_kf;
  if (init) {
    if (const char* why = init_fault(*caps, max_cov, *init)) return lorb::set_error(ctx, LORB_E_INVALID, "init: %s", why);
    char msg[192];
    if (geom && geom_fault(*init, *geom, msg, sizeof msg)) return lorb::set_error(ctx, LORB_E_INVALID, "geom: %s", msg);
  }
  lorb_kf_store* S = new (std::nothrow) lorb_kf_store;
  if (!S) return lorb::set_error(ctx, LORB_E_NOMEM, "out of host memory");
  struct Guard {
    lorb_kf_store* s;
    ~Guard() { if (s) lorb_kf_store_destroy(s); }
  } guard{S};
  S->ctx = ctx; S->cap = *caps; S->max_cov = max_cov;
  const size_t nk = (size_t)caps->max_kf, np = (size_t)caps->max_points, no = (size_t)caps->max_obs,
               ns = (size_t)caps->max_kf_slots, nc = (size_t)max_cov;
  lorb::Arena& A = S->mem;
  A.add(&S->pos, np * 3); A.add(&S->normal, np * 3); A.add(&S->max_dist, np); A.add(&S->min_dist, np);
  A.add(&S->desc, np * 32); A.add(&S->locked, np); A.add(&S->is_bad, np); A.add(&S->kf_bad, nk);
  A.add(&S->obs_off, np + 1); A.add(&S->obs_kf, no); A.add(&S->kf_slot_off, nk + 1); A.add(&S->kf_slot_point, ns);
  A.add(&S->cov_off, nk + 1); A.add(&S->cov_kf, nc);
  A.add(&S->conn_n, nk); A.add(&S->conn_kf, nc); A.add(&S->conn_w, nc); A.add(&S->ord_n, nk); A.add(&S->ord_kf, nc);
  A.add(&S->cnt, (size_t)8);
  A.add(&S->owner, np); A.add(&S->off2, np + 1); A.add(&S->kf2, no); A.add(&S->tile_cnt, np / kTile + 2);
  A.add(&S->touch, nk); A.add(&S->ctl, (size_t)1);
  A.add(&S->kf_pose, nk * 6); A.add(&S->kf_slot_uv, ns * 2); A.add(&S->obs_slot, no); A.add(&S->slot2, no);
  // the local BA's window and scratch (lorb_kfba.hip)
  const size_t nl = (size_t)lorb::kKfBaMaxLocal;
  A.add(&S->ba_hdr, (size_t)1); A.add(&S->ba_first, np); A.add(&S->ba_rank, nk); A.add(&S->ba_fixed_id, nk);
  A.add(&S->ba_fixed_flag, nk); A.add(&S->ba_seq_off, nl + 1); A.add(&S->ba_tile, ns / kTile + 2);
  A.add(&S->ba_ocnt, np); A.add(&S->ba_ooff, np + 1);
  A.add(&S->w_local, nl); A.add(&S->w_fixed, nk); A.add(&S->w_l2g, np); A.add(&S->w_obs_point, no); A.add(&S->w_obs_frame, no);
  A.add(&S->w_pose, nl * 6); A.add(&S->w_fixed_pose, nk * 6); A.add(&S->w_point, np * 3); A.add(&S->w_uv, no * 2);
  // the points' life and the cull's scratch (lorb_kfcull.hip)
  A.add(&S->life, lorb::KfLife::ints(caps->max_points, caps->max_kf)); A.add(&S->cull_mark, np); A.add(&S->cull_ctl, (size_t)1);
  // a compaction's staging (lorb_kfcompact.hip): 79 bytes of rows (lorb::KfPointRows, whose list this one follows),
  // 4 of map and 1 of hold per point
  A.add(&S->cp_pos, np * 3); A.add(&S->cp_normal, np * 3); A.add(&S->cp_max_dist, np); A.add(&S->cp_min_dist, np);
  A.add(&S->cp_desc, np * 32); A.add(&S->cp_locked, np); A.add(&S->cp_is_bad, np); A.add(&S->cp_recent, np);
  A.add(&S->cp_visible, np); A.add(&S->cp_found, np); A.add(&S->cp_first_fid, np);
  A.add(&S->cp_map, np); A.add(&S->cp_hold, np); A.add(&S->cp_ctl, (size_t)1);
  // the appearance and the refresh's verdicts (lorb_kfrefresh.hip)
  A.add(&S->kf_slot_desc, ns * 32); A.add(&S->kf_slot_octave, ns); A.add(&S->kf_center, nk * 3); A.add(&S->rf_stat, np);
  // a retirement's scratch (lorb_kfretire.hip)
  A.add(&S->rt_mark, nk); A.add(&S->rt_v, (size_t)LORB_KF_RETIRE_MAX_LIST); A.add(&S->rt_ctl, (size_t)1);
  LORB_HIP(ctx, A.commit());
  {
    const lorb::KfLife life(S->life, caps->max_points, caps->max_kf);
    S->visible = life.visible; S->found = life.found; S->first_fid = life.first_fid; S->recent = life.recent;
    S->kf_fid = life.kf_fid; S->frame_word = life.frame_word;
  }
  LORB_HIP(ctx, hipHostMalloc(reinterpret_cast<void**>(&S->h_hdr), sizeof(lorb::KfBaHdr)));
  memset(S->h_hdr, 0, sizeof(lorb::KfBaHdr));
  S->h_hdr->status = 1;  // no window gathered yet
  hipStream_t st = ctx->stream;
  LORB_HIP(ctx, hipMemsetAsync(A.base, 0, A.total, st));
  LORB_HIP(ctx, hipMemsetAsync(S->is_bad, 1, np, st));  // rows past the true counts are inert
  LORB_HIP(ctx, hipMemsetAsync(S->kf_bad, 1, nk, st));
  LORB_HIP(ctx, hipMemsetAsync(S->owner, 0x7f, np * sizeof(int), st));
  LORB_HIP(ctx, hipMemsetAsync(S->ba_first, 0x7f, np * sizeof(int), st));
  std::vector<int32_t> conn_n, conn_kf, conn_w, ord_n, ord_kf, ones;  // alive until the wait below
  int32_t cnt[6] = {0, 0, 0, 0, 0, 0};
  if (init) {
    const lorb_kf_store_host& h = *init;
    const size_t hp = (size_t)h.n_points, hk = (size_t)h.n_kf;
    LORB_HIP(ctx, lorb::kf_up(S, S->pos, h.pos, hp * 12)); LORB_HIP(ctx, lorb::kf_up(S, S->normal, h.normal, hp * 12));
    LORB_HIP(ctx, lorb::kf_up(S, S->max_dist, h.max_dist, hp * 4));
    LORB_HIP(ctx, lorb::kf_up(S, S->min_dist, h.min_dist, hp * 4));
    LORB_HIP(ctx, lorb::kf_up(S, S->desc, h.desc, hp * 32)); LORB_HIP(ctx, lorb::kf_up(S, S->locked, h.locked, hp));
    if (h.is_bad) LORB_HIP(ctx, lorb::kf_up(S, S->is_bad, h.is_bad, hp));
    else if (hp) LORB_HIP(ctx, hipMemsetAsync(S->is_bad, 0, hp, st));
    if (h.kf_bad) LORB_HIP(ctx, lorb::kf_up(S, S->kf_bad, h.kf_bad, hk));
    else if (hk) LORB_HIP(ctx, hipMemsetAsync(S->kf_bad, 0, hk, st));
    ones.assign(hp, 1);  // mnVisible = mnFound = 1 (src/map_point.cpp's constructors); first_fid, recent, kf_fid stay 0
    LORB_HIP(ctx, lorb::kf_up(S, S->visible, ones.data(), hp * 4)); LORB_HIP(ctx, lorb::kf_up(S, S->found, ones.data(), hp * 4));
    if (h.obs_off) LORB_HIP(ctx, lorb::kf_up(S, S->obs_off, h.obs_off, (hp + 1) * 4));
    LORB_HIP(ctx, lorb::kf_up(S, S->obs_kf, h.obs_kf, (size_t)h.n_obs * 4));
    if (hk) {
      LORB_HIP(ctx, lorb::kf_up(S, S->kf_slot_off, h.kf_slot_off, (hk + 1) * 4));
      LORB_HIP(ctx, lorb::kf_up(S, S->kf_slot_point, h.kf_slot_point, (size_t)h.n_kf_slots * 4));
      LORB_HIP(ctx, lorb::kf_up(S, S->cov_off, h.cov_off, (hk + 1) * 4));
      LORB_HIP(ctx, lorb::kf_up(S, S->cov_kf, h.cov_kf, (size_t)h.n_cov * 4));
      // the fixed-stride rows
      conn_n.assign(hk, 0); ord_n.assign(hk, 0);
      conn_kf.assign(hk * nk, 0); conn_w.assign(hk * nk, 0); ord_kf.assign(hk * nk, 0);
      for (size_t k = 0; k < hk; ++k) {
        conn_n[k] = h.conn_off[k + 1] - h.conn_off[k];
        ord_n[k] = h.cov_off[k + 1] - h.cov_off[k];
        for (int i = 0; i < conn_n[k]; ++i) {
          conn_kf[k * nk + i] = h.conn_kf[h.conn_off[k] + i];
          conn_w[k * nk + i] = h.conn_w[h.conn_off[k] + i];
        }
        for (int i = 0; i < ord_n[k]; ++i) ord_kf[k * nk + i] = h.cov_kf[h.cov_off[k] + i];
      }
      LORB_HIP(ctx, lorb::kf_up(S, S->conn_n, conn_n.data(), hk * 4));
      LORB_HIP(ctx, lorb::kf_up(S, S->ord_n, ord_n.data(), hk * 4));
      LORB_HIP(ctx, lorb::kf_up(S, S->conn_kf, conn_kf.data(), hk * nk * 4));
      LORB_HIP(ctx, lorb::kf_up(S, S->conn_w, conn_w.data(), hk * nk * 4));
      LORB_HIP(ctx, lorb::kf_up(S, S->ord_kf, ord_kf.data(), hk * nk * 4));
    }
    if (geom) {
      LORB_HIP(ctx, lorb::kf_up(S, S->kf_pose, geom->kf_pose, hk * 24));
      LORB_HIP(ctx, lorb::kf_up(S, S->kf_slot_uv, geom->kf_slot_uv, (size_t)h.n_kf_slots * 8));
      LORB_HIP(ctx, lorb::kf_up(S, S->obs_slot, geom->obs_slot, (size_t)h.n_obs * 4));
    }
    cnt[0] = h.n_kf; cnt[1] = h.n_points; cnt[2] = h.n_obs; cnt[3] = h.n_kf_slots; cnt[4] = h.n_cov; cnt[5] = h.n_conn;
    LORB_HIP(ctx, lorb::kf_up(S, S->cnt, cnt, sizeof cnt));
  }
  LORB_HIP(ctx, hipStreamSynchronize(st));
  S->b_kf = cnt[0]; S->b_points = cnt[1]; S->b_obs = cnt[2]; S->b_slots = cnt[3]; S->b_cov = cnt[4];
  S->geom_ok = geom != nullptr || cnt[0] == 0;  // an empty store is complete: every insertion writes its own
  S->appear_ok = cnt[0] == 0;                   // initial keyframes: lorb_kf_store_appear_write
  guard.s = nullptr;
  *out = S;
  return LORB_OK;
}

}  // namespace

extern "C" {

int lorb_kf_store_view(const lorb_kf_store* S, lorb_map_store* v) {
  if (!S || !v) return LORB_E_INVALID;
  v->points = lorb_map_points_dev{S->b_points, S->pos, S->normal, S->max_dist, S->min_dist, S->desc, S->locked, S->is_bad,
                                  nullptr};
  v->obs_off = S->obs_off; v->obs_kf = S->obs_kf; v->kf_bad = S->kf_bad;
  v->kf_slot_off = S->kf_slot_off; v->kf_slot_point = S->kf_slot_point; v->cov_off = S->cov_off; v->cov_kf = S->cov_kf;
  v->n_kf = S->b_kf; v->n_obs = S->b_obs; v->n_kf_slots = S->b_slots; v->n_cov = S->b_cov;
  return LORB_OK;
}

int lorb_kf_store_counts(lorb_kf_store* S, int32_t* out, int32_t n) {
  if (!S || !out) return LORB_E_INVALID;
  lorb_ctx* ctx = S->ctx;
  if (n < 1) return lorb::set_error(ctx, LORB_E_INVALID, "%d counts asked for", n);
  int32_t cnt[6];
  LORB_TRY(lorb::kf_true_counts(S, cnt));
  S->b_kf = cnt[0]; S->b_points = cnt[1]; S->b_obs = cnt[2]; S->b_slots = cnt[3]; S->b_cov = cnt[4];
  for (int i = 0; i < std::min(n, 6); ++i) out[i] = cnt[i];
  return LORB_OK;
}

int lorb_kf_store_read(lorb_kf_store* S, const lorb_kf_store_host* h) {
  if (!S || !h) return LORB_E_INVALID;
  lorb_ctx* ctx = S->ctx;
  int32_t cnt[6];
  LORB_TRY(lorb::kf_true_counts(S, cnt));
  const int nk = cnt[0], np = cnt[1], no = cnt[2], ns = cnt[3], nc = cnt[4], nn = cnt[5];
  const bool pts = h->pos || h->normal || h->max_dist || h->min_dist || h->desc || h->locked || h->is_bad || h->obs_off;
  const bool kfs = h->kf_bad || h->kf_slot_off || h->cov_off || h->conn_off;
  if ((pts && h->n_points < np) || (kfs && h->n_kf < nk) || (h->obs_kf && h->n_obs < no) ||
      (h->kf_slot_point && h->n_kf_slots < ns) || (h->cov_kf && h->n_cov < nc) || ((h->conn_kf || h->conn_w) && h->n_conn < nn))
    return lorb::set_error(ctx, LORB_E_INVALID, "an output array is smaller than the store's count (%d kf, %d points, %d obs, "
                           "%d slots, %d cov, %d conn)", nk, np, no, ns, nc, nn);
  const struct { void* host; const void* dev; size_t bytes; } cols[] = {
      {h->pos, S->pos, (size_t)np * 12}, {h->normal, S->normal, (size_t)np * 12}, {h->max_dist, S->max_dist, (size_t)np * 4},
      {h->min_dist, S->min_dist, (size_t)np * 4}, {h->desc, S->desc, (size_t)np * 32}, {h->locked, S->locked, (size_t)np},
      {h->is_bad, S->is_bad, (size_t)np}, {h->obs_off, S->obs_off, ((size_t)np + 1) * 4}, {h->obs_kf, S->obs_kf, (size_t)no * 4},
      {h->kf_bad, S->kf_bad, (size_t)nk}, {h->kf_slot_off, S->kf_slot_off, ((size_t)nk + 1) * 4},
      {h->kf_slot_point, S->kf_slot_point, (size_t)ns * 4}, {h->cov_off, S->cov_off, ((size_t)nk + 1) * 4},
      {h->cov_kf, S->cov_kf, (size_t)nc * 4}};
  for (const auto& c : cols) LORB_HIP(ctx, lorb::kf_down(S, c.host, c.dev, c.bytes));
  const bool conn = h->conn_off || h->conn_kf || h->conn_w;
  const size_t stride = (size_t)S->cap.max_kf;
  std::vector<int32_t> rn, rk, rw;
  if (conn && nk > 0) {
    rn.resize(nk); rk.resize(nk * stride); rw.resize(nk * stride);
    LORB_HIP(ctx, lorb::kf_down(S, rn.data(), S->conn_n, (size_t)nk * 4));
    LORB_HIP(ctx, lorb::kf_down(S, rk.data(), S->conn_kf, nk * stride * 4));
    LORB_HIP(ctx, lorb::kf_down(S, rw.data(), S->conn_w, nk * stride * 4));
  }
  LORB_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (conn) {
    int at = 0;
    for (int k = 0; k < nk; ++k) {
      if (h->conn_off) h->conn_off[k] = at;
      for (int i = 0; i < rn[k] && at < nn; ++i, ++at) {
        if (h->conn_kf) h->conn_kf[at] = rk[k * stride + i];
        if (h->conn_w) h->conn_w[at] = rw[k * stride + i];
      }
    }
    if (h->conn_off) h->conn_off[nk] = at;
  }
  return LORB_OK;
}

int lorb_kf_store_insert_dev(lorb_ctx* ctx, lorb_kf_store* S, const lorb_frame_params* frame, const lorb_frame_out* d_cur,
                             int32_t n_max_cur, const lorb_frame_slots* d_cur_slots, int32_t* d_cur_slot_gid,
                             const lorb_frame_pose* d_cur_pose, const int32_t* d_src_status, int32_t gate,
                             int32_t* d_refer_kf, lorb_local_map_result* d_update, lorb_kf_insert_result* d_result) {
  if (!frame || !d_cur || !d_cur_slots || !d_cur_slot_gid || !d_cur_pose || !d_result) return LORB_E_INVALID;
  LORB_TRY(lorb::kf_enter(ctx, S));
  const int nk = n_max_cur;
  if (nk < 1) return lorb::set_error(ctx, LORB_E_INVALID, "bound %d must be positive", nk);
  if (nk > S->cap.max_kf_slots)
    return lorb::set_error(ctx, LORB_E_INVALID, "bound %d exceeds max_kf_slots %d", nk, S->cap.max_kf_slots);
  if (gate != LORB_KF_GATE_RATIO && gate != LORB_KF_GATE_NONE) return lorb::set_error(ctx, LORB_E_INVALID, "unknown gate %d", gate);
  if (frame->n_levels < 1 || frame->n_levels > LORB_MAX_LEVELS)
    return lorb::set_error(ctx, LORB_E_INVALID, "n_levels %d outside [1, %d]", frame->n_levels, LORB_MAX_LEVELS);
  if (!d_cur->counts || !d_cur->left.x || !d_cur->left.y || !d_cur->left.octave || !d_cur->left.desc || !d_cur->depth ||
      !d_cur_slots->state || !d_cur_slots->pos || !d_cur_slots->desc)
    return lorb::set_error(ctx, LORB_E_INVALID, "null array");
  if ((reinterpret_cast<uintptr_t>(d_cur->left.desc) | reinterpret_cast<uintptr_t>(d_cur_slots->desc)) & 15)
    return lorb::set_error(ctx, LORB_E_INVALID, "a descriptor array is not 16-byte aligned");
  HeadArgs a{};
  a.fp = *frame; a.count = d_cur->counts; a.n_max = nk; a.gate = gate; a.src_status = d_src_status; a.pose = d_cur_pose;
  a.x = d_cur->left.x; a.y = d_cur->left.y; a.depth = d_cur->depth; a.octave = d_cur->left.octave;
  a.fdesc = reinterpret_cast<const uint4*>(d_cur->left.desc);
  a.state = d_cur_slots->state; a.spos = d_cur_slots->pos; a.sdesc = reinterpret_cast<uint4*>(d_cur_slots->desc);
  a.gid = d_cur_slot_gid;
  a.max_kf = S->cap.max_kf; a.max_points = S->cap.max_points; a.max_obs = S->cap.max_obs; a.max_kf_slots = S->cap.max_kf_slots;
  a.pos = S->pos; a.normal = S->normal; a.max_dist = S->max_dist; a.min_dist = S->min_dist;
  a.desc = reinterpret_cast<uint4*>(S->desc); a.locked = S->locked; a.is_bad = S->is_bad; a.kf_bad = S->kf_bad;
  a.kf_slot_off = S->kf_slot_off; a.kf_slot_point = S->kf_slot_point; a.kf_pose = S->kf_pose; a.kf_slot_uv = S->kf_slot_uv;
  a.life = S->life;
  a.kf_slot_desc = reinterpret_cast<uint4*>(S->kf_slot_desc); a.kf_slot_octave = S->kf_slot_octave; a.kf_center = S->kf_center;
  a.cnt = S->cnt; a.owner = S->owner; a.ctl = S->ctl;
  a.refer_kf = d_refer_kf; a.update = d_update; a.rec = d_result;
  hipStream_t st = ctx->stream;
  hipLaunchKernelGGL(k_kf_head, dim3(1), dim3(kWalk), 0, st, a);
  LORB_CHECK_LAUNCH(ctx);
  // grids from the bounds: the kernels read the true counts
  const size_t pb = (size_t)S->b_points, pb1 = std::min(pb + (size_t)nk, (size_t)S->cap.max_points);
  hipLaunchKernelGGL(k_kf_obs_count, dim3(lorb::ceil_div(pb + 1, kTile)), dim3(kTile), 0, st, S->ctl, S->owner, S->obs_off,
                     S->obs_kf, S->obs_slot, S->off2, S->kf2, S->slot2, S->tile_cnt);
  LORB_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(k_kf_obs_scatter, dim3(lorb::ceil_div(pb1 + 1, kTile)), dim3(kTile), 0, st, S->ctl, S->owner, S->off2,
                     S->kf2, S->slot2, S->tile_cnt, S->obs_off, S->obs_kf, S->obs_slot);
  LORB_CHECK_LAUNCH(ctx);
  const int stride = S->cap.max_kf;
  hipLaunchKernelGGL(k_kf_connect, dim3(1), dim3(kWalk), 0, st, S->ctl, S->kf_slot_point, S->is_bad, S->obs_off, S->obs_kf,
                     stride, S->conn_n, S->conn_kf, S->conn_w, S->touch, S->cnt, d_result);
  LORB_CHECK_LAUNCH(ctx);
  const int rows = std::min(S->b_kf + 1, 128);
  hipLaunchKernelGGL(k_kf_order, dim3(rows), dim3(1024), 0, st, S->ctl, S->touch, stride, S->conn_n, S->conn_kf, S->conn_w,
                     S->ord_n, S->ord_kf);
  LORB_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(k_kf_cov, dim3(rows), dim3(1024), 0, st, S->ctl, S->touch, stride, S->ord_n, S->ord_kf, S->cov_off,
                     S->cov_kf, S->cnt);
  LORB_CHECK_LAUNCH(ctx);
  // the bounds after this insertion, whatever the device decides
  S->b_kf = std::min(S->b_kf + 1, S->cap.max_kf);
  S->b_points = (int)pb1;
  S->b_slots = (int)std::min((size_t)S->b_slots + (size_t)nk, (size_t)S->cap.max_kf_slots);
  S->b_obs = S->cap.max_obs;
  S->b_cov = S->max_cov;
  return LORB_OK;
}

}  // extern "C"
