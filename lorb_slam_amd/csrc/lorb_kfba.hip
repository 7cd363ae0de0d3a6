// lorb_kfba.hip -- BA::LocalPoseOptimization(mpCurrFrame) (src/bundle_adjust.cpp:207-330, call site
// src/local_mapping.cpp:32) fed from the keyframe store: lorb_kf_store_ba_gather_dev, lorb_kf_store_local_ba_dev
// and lorb_kf_ba_window_read.  The contract is in lorb_c.h.
//
// The window is gathered in the store's own arena (the w_* arrays of lorb_kfstore.h) and handed to a resident
// device-built plan in place.  The gather is six launches on the ctx stream:
//   k_kfba_head    one workgroup: status; the local frames from K's covisibility row -- the first row position of
//                  every keyframe by atomicMin in LDS, then a scan of the kept positions -- their ranks, their
//                  pose rows, the offsets of their slot rows in the concatenated slot sequence
//   k_kfba_mark    a thread per sequence position: atomicMin of the position on the per-point word ba_first[],
//                  which is at rest (kKfBaNoFirst) between calls
//   k_kfba_count   the positions that own their point, counted per 1024-position tile
//   k_kfba_points  l2g and point_init by the tile scheme of k_kf_obs_scatter; the owner puts its point's word
//                  back to rest; each window point's usable observations counted, the fixed keyframes flagged
//   k_kfba_scan    one workgroup: the fixed keyframes numbered in ascending index with their pose rows, the
//                  observation offsets, the verdict (status 3 / 4) and the record
//   k_kfba_obs     a thread per window point: its observations in list order
// then one copy of the 64-byte header and one wait: the counts pick the plan.  The solve is the plan's; the
// write-back is one launch (k_db_result_rows, lorb_ba_build.hip).  All index arithmetic is integer; the atomics
// are min, max and add on integers, so no result depends on the order they arrive in.
#include <algorithm>

#include "lorb_internal.h"
#include "lorb_kfstore.h"

namespace {

using Hdr = lorb::KfBaHdr;
static_assert(sizeof(Hdr) == 64, "the header is one 64-byte copy");
constexpr int kT = lorb::kKfTile;               // threads per workgroup = positions per tile
constexpr int kMaxLocal = lorb::kKfBaMaxLocal;  // local frames
constexpr int kNoFirst = lorb::kKfBaNoFirst;
constexpr int kRowMax = 4096;                   // the largest max_kf: a covisibility row in LDS
constexpr int kMaxObs = 256;                    // a device plan's point group: a point has fewer usable observations

struct Store {  // what the gather reads of the store, and its scratch
  int max_kf;
  const int* cnt;
  const uint8_t *kf_bad, *is_bad;
  const int *cov_off, *cov_kf, *kf_slot_off, *kf_slot_point, *obs_off, *obs_kf, *obs_slot;
  const float *kf_pose, *kf_slot_uv, *pos;
  Hdr* hdr;
  int *first, *rank, *fixed_id, *fixed_flag, *seq_off, *tile, *ocnt, *ooff;
  int *local, *fixed, *l2g, *obs_point, *obs_frame;
  float *w_pose, *w_fixed_pose, *w_point, *w_uv;
};

// keyframe f's slot row inside the S slots the store holds
__device__ __forceinline__ void slot_row(const Store& s, int f, int S, int* lo, int* len) {
  const auto [l0, l1] = lorb::kf_range(s.kf_slot_off, f, S);
  *lo = l0;
  *len = l1 - l0;
}

__global__ __launch_bounds__(kT) void k_kfba_head(Store s, const int* d_kf, const int* src_status, lorb_kf_ba_result* rec) {
  __shared__ int s_first[kRowMax];  // per keyframe: the first row position that names it
  __shared__ int s_local[kMaxLocal];
  __shared__ lorb::I4 wsum4[16];
  __shared__ int wsum[16];
  __shared__ unsigned long long s_tot;
  const int t = threadIdx.x;
  const int kf = d_kf[0];
  const int nk = s.cnt[0], P = s.cnt[1], O = s.cnt[2], S = s.cnt[3], NC = s.cnt[4];
  // a. status
  if ((src_status && *src_status != 0) || kf < 0 || kf >= nk || nk > s.max_kf) {
    if (t == 0) {
      rec->status = 1;
      s.hdr->status = 1;
      s.hdr->go = 0;
    }
    return;
  }
  // b. the frames (:210-220)
  for (int f = t; f < kRowMax; f += kT) s_first[f] = 0x7fffffff;
  if (t == 0) s_tot = 0ull;
  __syncthreads();
  const auto [lo, hi] = lorb::kf_range(s.cov_off, kf, NC);
  const int len = min(hi - lo, kRowMax);
  for (int q = t; q < len; q += kT) {
    const int f = s.cov_kf[lo + q];
    if ((unsigned)f < (unsigned)nk && f != kf && !s.kf_bad[f]) atomicMin(&s_first[f], q);
  }
  __syncthreads();
  int C = 1, n_bad = 0;  // local[0] = kf, bad or not
  for (int base = 0; base < len; base += kT) {
    const int q = base + t;
    int keep = 0, bad = 0, f = -1;
    if (q < len) {
      f = s.cov_kf[lo + q];
      if ((unsigned)f < (unsigned)nk && f != kf) {
        bad = s.kf_bad[f] != 0;                 // :215-217
        keep = !bad && s_first[f] == q;         // listed once, at its first position
      }
    }
    lorb::I4 tot;
    const lorb::I4 at = lorb::block_excl_scan4<kT>(lorb::I4{{keep, bad, 0, 0}}, wsum4, &tot);
    if (keep && C + at.v[0] < kMaxLocal) s_local[C + at.v[0]] = f;
    C += tot.v[0];
    n_bad += tot.v[1];
  }
  if (C > kMaxLocal) {
    if (t == 0) {
      rec->status = 2;
      s.hdr->status = 2;
      s.hdr->go = 0;
    }
    return;
  }
  if (t == 0) s_local[0] = kf;
  for (int f = t; f < kRowMax; f += kT) s_first[f] = -1;  // from here on: the rank of every keyframe
  __syncthreads();
  if (t < C) s_first[s_local[t]] = t;
  __syncthreads();
  for (int f = t; f < nk; f += kT) {  // one store per word
    s.rank[f] = s_first[f];
    s.fixed_flag[f] = 0;
  }
  int ln = 0;
  if (t < C) {
    const int f = s_local[t];
    s.local[t] = f;
#pragma unroll
    for (int q = 0; q < 6; ++q) s.w_pose[6 * t + q] = s.kf_pose[6 * (size_t)f + q];  // e. pose_init
    int l0;
    slot_row(s, f, S, &l0, &ln);
    atomicAdd(&s_tot, (unsigned long long)ln);
  }
  int T;
  const int so = lorb::block_excl_scan_1024(ln, wsum, &T);
  if (t <= C) s.seq_off[t] = so;  // entry C: the total
  __syncthreads();
  if (t != 0) return;
  if (s_tot > (unsigned long long)S) {  // the rows of distinct keyframes overlap: a damaged store
    rec->status = 1;
    s.hdr->status = 1;
    s.hdr->go = 0;
    return;
  }
  *s.hdr = Hdr{0, 1, C, 0, 0, 0, 0, T, kf, nk, P, O, S, n_bad, 0, 0};
}

// the local frames' tables in LDS, and the point a sequence position holds: -1 for none, outside the store or bad
struct Seq {
  int off[kMaxLocal + 1];
  int kf[kMaxLocal];
};
__device__ __forceinline__ void seq_load(const Store& s, int C, Seq* q) {
  for (int i = threadIdx.x; i <= C; i += kT) q->off[i] = s.seq_off[i];
  for (int i = threadIdx.x; i < C; i += kT) q->kf[i] = s.local[i];
  __syncthreads();
}
__device__ __forceinline__ int seq_point(const Store& s, const Seq& sq, int C, int q, int P, int S) {
  int lo = 0, hi = C - 1;  // the last frame whose row starts at or before q
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (sq.off[mid] <= q) lo = mid; else hi = mid - 1;
  }
  int base, len;
  slot_row(s, sq.kf[lo], S, &base, &len);
  const int j = q - sq.off[lo];
  if (j >= len) return -1;
  const int p = s.kf_slot_point[base + j];
  return ((unsigned)p < (unsigned)P && !s.is_bad[p]) ? p : -1;
}

__global__ __launch_bounds__(kT) void k_kfba_mark(Store s) {
  __shared__ Seq sq;
  const Hdr& h = *s.hdr;
  if (!h.go) return;
  const int q = blockIdx.x * kT + threadIdx.x;
  if (blockIdx.x * kT >= h.T) return;
  seq_load(s, h.C, &sq);
  if (q >= h.T) return;
  const int p = seq_point(s, sq, h.C, q, h.n_pts, h.n_slots);
  if (p >= 0) atomicMin(&s.first[p], q);
}

__global__ __launch_bounds__(kT) void k_kfba_count(Store s) {
  __shared__ Seq sq;
  __shared__ int wsum[16];
  const Hdr& h = *s.hdr;
  if (!h.go) return;
  const int q = blockIdx.x * kT + threadIdx.x;
  if (blockIdx.x * kT >= h.T) return;
  seq_load(s, h.C, &sq);
  const int p = q < h.T ? seq_point(s, sq, h.C, q, h.n_pts, h.n_slots) : -1;
  int tot;
  lorb::block_excl_scan_1024(p >= 0 && s.first[p] == q, wsum, &tot);
  if (threadIdx.x == 0) s.tile[blockIdx.x] = tot;
}

// d's test of observation o: 0 usable (*f, *slot_at: the keyframe and its slot's place in kf_slot_uv), 1 a bad
// keyframe (:278), 2 a keyframe or slot outside the store
__device__ __forceinline__ int obs_kind(const Store& s, int o, int nk, int S, int* f, int* slot_at) {
  const int k = s.obs_kf[o];
  if ((unsigned)k >= (unsigned)nk) return 2;
  if (s.kf_bad[k]) return 1;
  int base, len;
  slot_row(s, k, S, &base, &len);
  const int j = s.obs_slot[o];
  if ((unsigned)j >= (unsigned)len) return 2;
  *f = k;
  *slot_at = base + j;
  return 0;
}

__global__ __launch_bounds__(kT) void k_kfba_points(Store s) {
  __shared__ Seq sq;
  __shared__ int wsum[16];
  Hdr& h = *s.hdr;
  if (!h.go) return;
  const int t = threadIdx.x, b = blockIdx.x, T = h.T;
  if (b * kT >= T) return;
  seq_load(s, h.C, &sq);
  const int n_tiles = (T + kT - 1) / kT;
  int tot;
  const int base = lorb::tile_base_1024(s.tile, b, wsum);
  const int q = b * kT + t;
  const int p = q < T ? seq_point(s, sq, h.C, q, h.n_pts, h.n_slots) : -1;
  const int own = p >= 0 && s.first[p] == q;  // a later position of p sees q or the word at rest: not its own
  const int i = base + lorb::block_excl_scan_1024(own, wsum, &tot);
  if (b == n_tiles - 1 && t == 0) h.P = base + tot;
  if (!own) return;
  s.first[p] = kNoFirst;
  s.l2g[i] = p;
#pragma unroll
  for (int k = 0; k < 3; ++k) s.w_point[3 * (size_t)i + k] = s.pos[3 * (size_t)p + k];  // e. point_init
  const int O = h.n_obs_store;
  const auto [lo, hi] = lorb::kf_range(s.obs_off, p, O);
  int n = 0, bad_kf = 0, bad_slot = 0;
  for (int o = lo; o < hi; ++o) {
    int f, at;
    const int kind = obs_kind(s, o, h.n_kf, h.n_slots, &f, &at);
    bad_kf += kind == 1;
    bad_slot += kind == 2;
    if (kind) continue;
    ++n;
    if (s.rank[f] < 0) s.fixed_flag[f] = 1;  // every writer stores the same value
  }
  s.ocnt[i] = n;
  atomicMax(&h.maxk, n);
  if (bad_kf) atomicAdd(&h.n_obs_bad_kf, bad_kf);
  if (bad_slot) atomicAdd(&h.n_obs_bad_slot, bad_slot);
}

__global__ __launch_bounds__(kT) void k_kfba_scan(Store s, lorb_kf_ba_result* rec) {
  __shared__ int wsum[16];
  Hdr& h = *s.hdr;
  if (!h.go) return;
  const int t = threadIdx.x, nk = h.n_kf, Pw = h.P;
  int F = 0, K = 0;
  for (int base = 0; base < nk; base += kT) {  // the fixed frames in ascending keyframe index
    const int f = base + t, flag = f < nk && s.fixed_flag[f];
    int tot;
    const int at = F + lorb::block_excl_scan_1024(flag, wsum, &tot);
    if (flag) {
      s.fixed_id[f] = at;
      s.fixed[at] = f;
#pragma unroll
      for (int q = 0; q < 6; ++q) s.w_fixed_pose[6 * (size_t)at + q] = s.kf_pose[6 * (size_t)f + q];
    }
    F += tot;
  }
  for (int base = 0; base < Pw; base += kT) {
    const int i = base + t;
    int tot;
    const int at = K + lorb::block_excl_scan_1024(i < Pw ? s.ocnt[i] : 0, wsum, &tot);
    if (i < Pw) s.ooff[i] = at;
    K += tot;
  }
  if (t != 0) return;
  s.ooff[Pw] = K;
  const int status = (Pw == 0 || K == 0) ? 3 : h.maxk >= kMaxObs ? 4 : 0;
  h.status = status;
  h.go = status == 0;
  h.F = F;
  h.K = K;
  *rec = lorb_kf_ba_result{status, h.kf, h.C, F, Pw, K, h.n_cov_bad, h.n_obs_bad_kf, h.n_obs_bad_slot, 0};
}

__global__ __launch_bounds__(kT) void k_kfba_obs(Store s) {
  const Hdr& h = *s.hdr;
  if (!h.go) return;
  const int O = h.n_obs_store;
  for (int i = blockIdx.x * kT + threadIdx.x; i < h.P; i += gridDim.x * kT) {
    const int p = s.l2g[i];
    const auto [lo, hi] = lorb::kf_range(s.obs_off, p, O);
    int at = s.ooff[i];
    for (int o = lo; o < hi; ++o) {
      int f, uv;
      if (obs_kind(s, o, h.n_kf, h.n_slots, &f, &uv)) continue;
      const int r = s.rank[f];
      s.obs_point[at] = i;
      s.obs_frame[at] = r >= 0 ? r : -1 - s.fixed_id[f];
      s.w_uv[2 * (size_t)at] = s.kf_slot_uv[2 * (size_t)uv];
      s.w_uv[2 * (size_t)at + 1] = s.kf_slot_uv[2 * (size_t)uv + 1];
      ++at;
    }
  }
}

Store store_args(const lorb_kf_store* S) {
  Store s{};
  s.max_kf = S->cap.max_kf; s.cnt = S->cnt; s.kf_bad = S->kf_bad; s.is_bad = S->is_bad;
  s.cov_off = S->cov_off; s.cov_kf = S->cov_kf; s.kf_slot_off = S->kf_slot_off; s.kf_slot_point = S->kf_slot_point;
  s.obs_off = S->obs_off; s.obs_kf = S->obs_kf; s.obs_slot = S->obs_slot;
  s.kf_pose = S->kf_pose; s.kf_slot_uv = S->kf_slot_uv; s.pos = S->pos;
  s.hdr = S->ba_hdr; s.first = S->ba_first; s.rank = S->ba_rank; s.fixed_id = S->ba_fixed_id; s.fixed_flag = S->ba_fixed_flag;
  s.seq_off = S->ba_seq_off; s.tile = S->ba_tile; s.ocnt = S->ba_ocnt; s.ooff = S->ba_ooff;
  s.local = S->w_local; s.fixed = S->w_fixed; s.l2g = S->w_l2g; s.obs_point = S->w_obs_point; s.obs_frame = S->w_obs_frame;
  s.w_pose = S->w_pose; s.w_fixed_pose = S->w_fixed_pose; s.w_point = S->w_point; s.w_uv = S->w_uv;
  return s;
}

// the six launches, the header copy and the wait; LORB_E_UNSUPPORTED for status 2 and 4
int gather(lorb_ctx* ctx, lorb_kf_store* S, const lorb_frame_params* frame, const int32_t* d_kf, const int32_t* d_src_status,
           lorb_kf_ba_result* d_result) {
  if (!frame || !d_kf || !d_result) return LORB_E_INVALID;
  LORB_TRY(lorb::kf_enter(ctx, S, lorb::kKfNeedGeom));
  const Store s = store_args(S);
  hipStream_t st = ctx->stream;
  // grids from the host's bounds: the kernels read the true counts
  const unsigned seq_blocks = std::max(1u, lorb::ceil_div((size_t)S->b_slots, kT));
  const unsigned pt_blocks = std::max(1u, lorb::ceil_div((size_t)std::min(S->b_points, S->b_slots), kT));
  hipLaunchKernelGGL(k_kfba_head, dim3(1), dim3(kT), 0, st, s, d_kf, d_src_status, d_result);
  LORB_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(k_kfba_mark, dim3(seq_blocks), dim3(kT), 0, st, s);
  LORB_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(k_kfba_count, dim3(seq_blocks), dim3(kT), 0, st, s);
  LORB_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(k_kfba_points, dim3(seq_blocks), dim3(kT), 0, st, s);
  LORB_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(k_kfba_scan, dim3(1), dim3(kT), 0, st, s, d_result);
  LORB_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(k_kfba_obs, dim3(pt_blocks), dim3(kT), 0, st, s);
  LORB_CHECK_LAUNCH(ctx);
  LORB_HIP(ctx, hipMemcpyAsync(S->h_hdr, S->ba_hdr, sizeof(Hdr), hipMemcpyDeviceToHost, st));
  LORB_HIP(ctx, lorb::spin_sync(ctx));
  S->window_current = true;  // until a compaction renumbers the points (lorb_kf_store_refresh_dev)
  const Hdr& h = *S->h_hdr;
  if (h.status == 2)
    return lorb::set_error(ctx, LORB_E_UNSUPPORTED, "keyframe %d has more than %d local frames", h.kf, kMaxLocal);
  if (h.status == 4)
    return lorb::set_error(ctx, LORB_E_UNSUPPORTED, "a window point has %d usable observations (device plans hold <= %d)",
                           h.maxk, kMaxObs - 1);
  return LORB_OK;
}

}  // namespace

extern "C" {

int lorb_kf_store_ba_gather_dev(lorb_ctx* ctx, lorb_kf_store* S, const lorb_frame_params* frame, const int32_t* d_kf,
                                const int32_t* d_src_status, lorb_kf_ba_result* d_result) {
  return gather(ctx, S, frame, d_kf, d_src_status, d_result);
}

int lorb_kf_store_local_ba_dev(lorb_ctx* ctx, lorb_kf_store* S, const lorb_frame_params* frame, const int32_t* d_kf,
                               const int32_t* d_src_status, const lorb_lm_options* opt, lorb_kf_ba_result* d_result,
                               lorb_ba_summary* summary) {
  if (!ctx || !S || !frame || !d_kf || !opt || !d_result) return LORB_E_INVALID;
  LORB_TRY(gather(ctx, S, frame, d_kf, d_src_status, d_result));
  const Hdr h = *S->h_hdr;
  if (summary) *summary = lorb_ba_summary{};
  if (h.status != 0) return LORB_OK;  // 1, 3: nothing to solve
  // f. the resident plan of this camera count; its capacities never pass the store's
  lorb::PlanSlot* sl = nullptr;
  LORB_TRY(S->plans.pick(ctx, h.C, h.F, h.P, h.K, &sl, S->cap.max_kf, S->cap.max_points, S->cap.max_obs));
  lorb_ba_window_dev w{};
  w.n_poses = h.C; w.n_fixed = sl->F_cap; w.max_points = sl->P_cap; w.max_obs = sl->K_cap;
  w.d_n_points = &S->ba_hdr->P; w.d_n_obs = &S->ba_hdr->K;
  w.fx = frame->fx; w.fy = frame->fy; w.cx = frame->cx; w.cy = frame->cy;
  w.d_pose_init = S->w_pose; w.d_fixed_pose = S->w_fixed_pose; w.d_point_init = S->w_point;
  w.d_obs_point = S->w_obs_point; w.d_obs_frame = S->w_obs_frame; w.d_obs_uv = S->w_uv;
  const int rc = S->plans.build(ctx, sl, &w, true);  // d's observations are sorted by point
  if (rc != LORB_OK) {
    if (!sl->plan) S->plans.release(*sl);
    return rc;
  }
  LORB_TRY(lorb_ba_plan_solve(sl->plan, opt));
  // g. the write-back, one launch
  LORB_TRY(lorb::ba_plan_result_rows_dev(sl->plan, S->w_local, S->kf_pose, S->w_l2g, S->pos, &d_result->written));
  if (summary) LORB_TRY(lorb_ba_plan_read(sl->plan, nullptr, nullptr, summary));
  return LORB_OK;
}

int lorb_kf_ba_window_read(lorb_kf_store* S, const lorb_kf_ba_window_host* out) {
  if (!S || !out) return LORB_E_INVALID;
  lorb_ctx* ctx = S->ctx;
  LORB_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const Hdr h = *S->h_hdr;
  if (h.status != 0 && h.status != 3) return lorb::set_error(ctx, LORB_E_INVALID, "no window was gathered (status %d)", h.status);
  const bool cams = out->local_kf || out->pose_init, fixed = out->fixed_kf || out->fixed_pose,
             pts = out->l2g || out->point_init, obs = out->obs_point || out->obs_frame || out->obs_uv;
  if ((cams && out->n_poses < h.C) || (fixed && out->n_fixed < h.F) || (pts && out->n_points < h.P) || (obs && out->n_obs < h.K))
    return lorb::set_error(ctx, LORB_E_INVALID, "an output array is smaller than the window (%d poses, %d fixed, %d points, "
                           "%d obs)", h.C, h.F, h.P, h.K);
  LORB_HIP(ctx, lorb::kf_down(S, out->local_kf, S->w_local, (size_t)h.C * 4));
  LORB_HIP(ctx, lorb::kf_down(S, out->pose_init, S->w_pose, (size_t)h.C * 24));
  LORB_HIP(ctx, lorb::kf_down(S, out->fixed_kf, S->w_fixed, (size_t)h.F * 4));
  LORB_HIP(ctx, lorb::kf_down(S, out->fixed_pose, S->w_fixed_pose, (size_t)h.F * 24));
  LORB_HIP(ctx, lorb::kf_down(S, out->l2g, S->w_l2g, (size_t)h.P * 4));
  LORB_HIP(ctx, lorb::kf_down(S, out->point_init, S->w_point, (size_t)h.P * 12));
  LORB_HIP(ctx, lorb::kf_down(S, out->obs_point, S->w_obs_point, (size_t)h.K * 4));
  LORB_HIP(ctx, lorb::kf_down(S, out->obs_frame, S->w_obs_frame, (size_t)h.K * 4));
  LORB_HIP(ctx, lorb::kf_down(S, out->obs_uv, S->w_uv, (size_t)h.K * 8));
  LORB_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return LORB_OK;
}

}  // extern "C"
