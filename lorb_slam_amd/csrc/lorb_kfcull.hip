// lorb_kfcull.hip -- the life of the store's points and LocalMapping::MapPointsCulling on the keyframe store:
// lorb_kf_store_life_write / _read / _view, lorb_kf_store_observe_dev (the tracker's two IncreaseVisible sites,
// src/visual_odometry.cpp:153-171 and :176-195) and lorb_kf_store_cull_dev (src/local_mapping.cpp:82-108 in the
// verdict order of include/lorb/local_mapping.hpp:63-74, with MapPoint::SetBadFlag, src/map_point.cpp:184-199,
// and Frame::EraseMapPoint, src/frame.cpp:896-899).  The contract is in lorb_c.h.
//
// The life state (visible, found, first_fid, recent per point; kf_fid per keyframe; the frame word) lives in the
// store's arena; k_kf_head (lorb_kfstore.hip) writes it for keyframe K and its new points.
//
// observe is ONE launch on the ctx stream:
//   k_kf_observe      one workgroup walking the slots, then the local rows: status, the frame word, the integer
//                     atomics on visible[] and found[], the record
// cull is FOUR launches:
//   k_kf_cull_head    one wavefront: status, kf_fid[kf], the true counts into KfCullCtl, the record at zero
//   k_kf_cull_verdict a thread per point: the verdict; a culled point's is_bad, recent, mark, the -1 in every
//                     keyframe slot its observations name; the observations it gives up per 1024-point tile; the
//                     record's counters and the true n_obs by integer atomics
//   k_kf_cull_frame   the tracker's frame: slots that hold a marked point become EMPTY; the observation CSR
//                     (offsets, keyframes, slots) copied to the insertion's scratch
//   k_kf_cull_scatter the CSR back: every list moves left by the observations given up in front of it (base = the
//                     sum of the earlier tiles, then a scan inside the tile); the marks go back to rest
// The last two return at once when no point was culled (KfCullCtl::n_culled): the CSR is not rewritten.  All
// counting is integer: no result depends on the order the atomics arrive in.
#include <algorithm>
#include <cmath>

#include "lorb_internal.h"
#include "lorb_kfstore.h"

namespace {

constexpr int kT = lorb::kKfTile;  // threads per workgroup = points per tile
using Ctl = lorb::KfCullCtl;

struct ObserveArgs {
  int frame_id, n_max, max_local, found_rule;
  const int* count;  // the frame's counts (entry 0)
  const uint8_t* state;
  const int *gid, *lid, *l2g;
  const lorb_local_map_result* update;
  const uint8_t* in_view;
  const int* local_status;  // or null
  const int* cnt;
  int *visible, *found, *frame_word;
  lorb_kf_observe_result* rec;
};

__global__ __launch_bounds__(kT) void k_kf_observe(ObserveArgs a) {
  __shared__ lorb::I4 wsum4[16];
  const int t = threadIdx.x;
  const int n = a.count[0], n_local = a.update->n_local;
  // a. status
  if (n < 0 || n > a.n_max || (a.local_status && *a.local_status != 0) || a.update->status != 0 || n_local < 0 ||
      n_local > a.max_local) {
    if (t == 0) a.rec->status = 1;
    return;
  }
  const int P = a.cnt[1];
  if (t == 0) a.frame_word[0] = a.frame_id;  // b. mCurrFrame->mnId
  lorb::I4 c = {{0, 0, 0, 0}}, tot;
  for (int j = t; j < n; j += kT) {  // c. :153-171, per slot
    const int g = a.gid[j];
    if ((unsigned)g >= (unsigned)P) continue;
    atomicAdd(&a.visible[g], 1);
    ++c.v[0];
  }
  for (int k = t; k < n_local; k += kT) {  // d. :188-194
    if (!a.in_view[k]) continue;
    const int g = a.l2g[k];
    if ((unsigned)g >= (unsigned)P) continue;
    atomicAdd(&a.visible[g], 1);
    ++c.v[1];
  }
  if (a.found_rule == LORB_KF_FOUND_SLOTS) {  // e. ORB-SLAM2's TrackLocalMap; the reference never calls IncreaseFound
    for (int j = t; j < n; j += kT) {
      if (a.state[j] == LORB_SLOT_EMPTY) continue;
      const int l = a.lid[j];
      int g = -1;
      if (l < 0) g = a.gid[j];
      else if (l < n_local) g = a.l2g[l];
      if ((unsigned)g >= (unsigned)P) continue;
      atomicAdd(&a.found[g], 1);
      ++c.v[2];
    }
  }
  lorb::block_excl_scan4<kT>(c, wsum4, &tot);
  if (t == 0) *a.rec = lorb_kf_observe_result{0, tot.v[0], tot.v[1], tot.v[2]};
}

struct CullArgs {
  lorb_kf_cull_params par;
  int max_kf, n_max;  // n_max: the frame group's bound, 0 without the group
  const int *d_kf, *src_status;
  int* cnt;
  uint8_t *is_bad, *recent, *mark;
  const int *visible, *found, *first_fid, *kf_fid;
  int *obs_off, *obs_kf, *obs_slot;
  const int* kf_slot_off;
  int* kf_slot_point;
  int *off2, *kf2, *slot2, *tile;
  // the tracker's frame, or null
  const int* count;
  uint8_t* state;
  int* gid;
  Ctl* ctl;
  lorb_kf_cull_result* rec;
};

__global__ __launch_bounds__(64) void k_kf_cull_head(CullArgs a) {
  if (threadIdx.x != 0) return;
  const int kf = a.d_kf[0], nk = a.cnt[0];
  // a. status
  if ((a.src_status && *a.src_status != 0) || kf < 0 || kf >= nk || nk > a.max_kf) {
    a.rec->status = 1;
    a.ctl->go = 0;
    a.ctl->n_culled = 0;
    return;
  }
  const int P = a.cnt[1], O = a.cnt[2], S = a.cnt[3];
  *a.ctl = Ctl{1, kf, a.kf_fid[kf], nk, P, O, S, 0};
  *a.rec = lorb_kf_cull_result{0, kf, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, O};
}

// b + c. the verdict of point p in the order of include/lorb/local_mapping.hpp:66-71, and SetBadFlag
enum { cExamined = 0, cBadBefore, cRatio, cObs, cAgedOut, cStays, cObsGone, cErased, cBadSlot, cCount };

__global__ __launch_bounds__(kT) void k_kf_cull_verdict(CullArgs a) {
  __shared__ int s_c[cCount];  // this tile's counters: integer adds in LDS
  const Ctl& h = *a.ctl;
  if (!h.go) return;
  const int t = threadIdx.x, p = blockIdx.x * kT + t;
  const int P = h.P, O = h.O, S = h.S, nk = h.nk;
  if (blockIdx.x * kT >= P) return;
  if (t < cCount) s_c[t] = 0;
  __syncthreads();
  if (p < P && a.recent[p]) {
    const auto [lo, hi] = lorb::kf_range(a.obs_off, p, O);
    const unsigned age = (unsigned)(h.cur - a.first_fid[p]);
    int kind;
    if (a.is_bad[p]) kind = cBadBefore;  // 1. it leaves the list
    else if ((float)a.found[p] / (float)a.visible[p] < a.par.min_found_ratio) kind = cRatio;  // 2. GetFoundRatio()
    else if (age >= (unsigned)a.par.age_obs && hi - lo < a.par.min_obs) kind = cObs;          // 3.
    else if (age >= (unsigned)a.par.age_out) kind = cAgedOut;                                 // 4. it leaves the list
    else kind = cStays;                                                                       // 5.
    atomicAdd(&s_c[cExamined], 1);
    atomicAdd(&s_c[kind], 1);
    if (kind != cStays) a.recent[p] = 0;
    if (kind == cRatio || kind == cObs) {  // MapPoint::SetBadFlag (src/map_point.cpp:184-199)
      a.is_bad[p] = 1;
      a.mark[p] = 1;
      int erased = 0;
      for (int o = lo; o < hi; ++o) {  // Frame::EraseMapPoint(it->second), bad keyframe or not
        const int f = a.obs_kf[o], s = a.obs_slot[o];
        if ((unsigned)f >= (unsigned)nk) continue;
        const auto [l0, l1] = lorb::kf_range(a.kf_slot_off, f, S);
        if ((unsigned)s >= (unsigned)(l1 - l0) || a.kf_slot_point[l0 + s] != p) continue;
        a.kf_slot_point[l0 + s] = -1;
        ++erased;
      }
      if (hi > lo) atomicAdd(&s_c[cObsGone], hi - lo);
      if (erased) atomicAdd(&s_c[cErased], erased);
      if (hi - lo > erased) atomicAdd(&s_c[cBadSlot], hi - lo - erased);
    }
  }
  __syncthreads();
  if (t != 0) return;
  const int gone = s_c[cObsGone], culled = s_c[cRatio] + s_c[cObs];
  a.tile[blockIdx.x] = gone;  // the observations this tile gives up
  lorb_kf_cull_result* r = a.rec;
  if (s_c[cExamined]) atomicAdd(&r->n_examined, s_c[cExamined]);
  if (s_c[cBadBefore]) atomicAdd(&r->n_bad_before, s_c[cBadBefore]);
  if (s_c[cRatio]) atomicAdd(&r->n_culled_ratio, s_c[cRatio]);
  if (s_c[cObs]) atomicAdd(&r->n_culled_obs, s_c[cObs]);
  if (s_c[cAgedOut]) atomicAdd(&r->n_aged_out, s_c[cAgedOut]);
  if (s_c[cStays]) atomicAdd(&r->n_recent, s_c[cStays]);
  if (s_c[cErased]) atomicAdd(&r->n_slots_erased, s_c[cErased]);
  if (s_c[cBadSlot]) atomicAdd(&r->n_obs_bad_slot, s_c[cBadSlot]);
  if (culled) atomicAdd(&a.ctl->n_culled, culled);
  if (gone) {  // e. the true count and the record's
    atomicAdd(&r->n_obs_removed, gone);
    atomicSub(&r->n_obs, gone);
    atomicSub(&a.cnt[2], gone);
  }
}

// d. K's Frame is the tracker's frame: its slots that hold a point culled by this call; and the CSR as it stands
// into scratch
__global__ __launch_bounds__(kT) void k_kf_cull_frame(CullArgs a) {
  __shared__ int wsum[16];
  const Ctl& h = *a.ctl;
  if (!h.go || h.n_culled == 0) return;
  const int t = threadIdx.x, P = h.P, O = h.O;
  const long long i0 = (long long)blockIdx.x * kT + t, step = (long long)gridDim.x * kT;
  int n = a.count ? a.count[0] : 0;
  if (n < 0 || n > a.n_max) n = 0;  // a count out of range: no slot is touched
  int emptied = 0;
  for (long long j = i0; j < n; j += step) {
    const int g = a.gid[j];
    if ((unsigned)g < (unsigned)P && a.mark[g]) {
      a.state[j] = LORB_SLOT_EMPTY;
      a.gid[j] = -1;
      ++emptied;
    }
  }
  int tot;
  lorb::block_excl_scan_1024(emptied, wsum, &tot);
  if (t == 0 && tot) atomicAdd(&a.rec->n_frame_slots_emptied, tot);
  for (long long p = i0; p <= P; p += step) a.off2[p] = a.obs_off[p];
  for (long long o = i0; o < O; o += step) {
    a.kf2[o] = a.obs_kf[o];
    a.slot2[o] = a.obs_slot[o];
  }
}

// c, the lists: point p's list moves left by the observations the culled points in front of it gave up; a culled
// point's list becomes empty.  Launched over the bound on n_points + 1.
__global__ __launch_bounds__(kT) void k_kf_cull_scatter(CullArgs a) {
  __shared__ int wsum[16];
  const Ctl& h = *a.ctl;
  if (!h.go || h.n_culled == 0) return;
  const int t = threadIdx.x, b = blockIdx.x, P = h.P, O = h.O;
  if ((long long)b * kT > P) return;
  const int n_tiles = (P + kT - 1) / kT;
  int tot;
  const int base = lorb::tile_base_1024(a.tile, min(b, n_tiles), wsum);
  const int p = b * kT + t;
  int lo = 0, hi = 0, gone = 0;
  if (p < P) {
    const lorb::KfRange r = lorb::kf_range(a.off2, p, O);
    lo = r.lo; hi = r.hi;
    gone = a.mark[p] != 0;
  }
  const int before = base + lorb::block_excl_scan_1024(gone ? hi - lo : 0, wsum, &tot);
  if (p < P) {
    if (gone) a.mark[p] = 0;  // back at rest
    const int at = lo - before;
    if (before && at >= 0) {
      a.obs_off[p] = at;
      if (!gone)
        for (int o = lo; o < hi; ++o) {
          a.obs_kf[at + (o - lo)] = a.kf2[o];
          a.obs_slot[at + (o - lo)] = a.slot2[o];
        }
    }
  } else if (p == P) {
    a.obs_off[P] = max(lorb::clampi(a.off2[P], 0, O) - before, 0);
  }
}

CullArgs cull_args(const lorb_kf_store* S) {
  CullArgs a{};
  a.max_kf = S->cap.max_kf; a.cnt = S->cnt; a.is_bad = S->is_bad; a.recent = S->recent; a.mark = S->cull_mark;
  a.visible = S->visible; a.found = S->found; a.first_fid = S->first_fid; a.kf_fid = S->kf_fid;
  a.obs_off = S->obs_off; a.obs_kf = S->obs_kf; a.obs_slot = S->obs_slot;
  a.kf_slot_off = S->kf_slot_off; a.kf_slot_point = S->kf_slot_point;
  a.off2 = S->off2; a.kf2 = S->kf2; a.slot2 = S->slot2; a.tile = S->tile_cnt; a.ctl = S->cull_ctl;
  return a;
}

}  // namespace

extern "C" {

int lorb_kf_store_life_view(const lorb_kf_store* S, lorb_kf_store_life_host* v) {
  if (!S || !v) return LORB_E_INVALID;
  *v = lorb_kf_store_life_host{S->cap.max_kf, S->cap.max_points, S->visible, S->found, S->first_fid, S->recent, S->kf_fid};
  return LORB_OK;
}

int lorb_kf_store_frame_word_view(const lorb_kf_store* S, int32_t** d_word) {
  if (!S || !d_word) return LORB_E_INVALID;
  *d_word = S->frame_word;
  return LORB_OK;
}

int lorb_kf_store_life_read(lorb_kf_store* S, const lorb_kf_store_life_host* h) {
  if (!S || !h) return LORB_E_INVALID;
  lorb_ctx* ctx = S->ctx;
  int32_t cnt[6];
  LORB_TRY(lorb::kf_true_counts(S, cnt));
  const int nk = cnt[0], np = cnt[1];
  const bool pts = h->visible || h->found || h->first_fid || h->recent;
  if ((pts && h->n_points < np) || (h->kf_fid && h->n_kf < nk))
    return lorb::set_error(ctx, LORB_E_INVALID, "an output array is smaller than the store's count (%d kf, %d points)", nk, np);
  LORB_HIP(ctx, lorb::kf_down(S, h->visible, S->visible, (size_t)np * 4));
  LORB_HIP(ctx, lorb::kf_down(S, h->found, S->found, (size_t)np * 4));
  LORB_HIP(ctx, lorb::kf_down(S, h->first_fid, S->first_fid, (size_t)np * 4));
  LORB_HIP(ctx, lorb::kf_down(S, h->recent, S->recent, (size_t)np));
  LORB_HIP(ctx, lorb::kf_down(S, h->kf_fid, S->kf_fid, (size_t)nk * 4));
  LORB_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return LORB_OK;
}

int lorb_kf_store_life_write(lorb_kf_store* S, const lorb_kf_store_life_host* h) {
  if (!S || !h) return LORB_E_INVALID;
  lorb_ctx* ctx = S->ctx;
  int32_t cnt[6];
  LORB_TRY(lorb::kf_true_counts(S, cnt));
  const int nk = cnt[0], np = cnt[1];
  if (h->n_kf != nk || h->n_points != np)
    return lorb::set_error(ctx, LORB_E_INVALID, "life: counts %d / %d differ from the store's %d / %d (kf, points)", h->n_kf,
                           h->n_points, nk, np);
  for (int p = 0; p < np; ++p) {
    if (h->visible && h->visible[p] < 1)
      return lorb::set_error(ctx, LORB_E_INVALID, "life: visible[%d] = %d must be at least 1", p, h->visible[p]);
    if (h->found && h->found[p] < 0)
      return lorb::set_error(ctx, LORB_E_INVALID, "life: found[%d] = %d must not be negative", p, h->found[p]);
  }
  LORB_HIP(ctx, lorb::kf_up(S, S->visible, h->visible, (size_t)np * 4));
  LORB_HIP(ctx, lorb::kf_up(S, S->found, h->found, (size_t)np * 4));
  LORB_HIP(ctx, lorb::kf_up(S, S->first_fid, h->first_fid, (size_t)np * 4));
  LORB_HIP(ctx, lorb::kf_up(S, S->recent, h->recent, (size_t)np));
  LORB_HIP(ctx, lorb::kf_up(S, S->kf_fid, h->kf_fid, (size_t)nk * 4));
  LORB_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return LORB_OK;
}

int lorb_kf_store_observe_dev(lorb_ctx* ctx, lorb_kf_store* S, int32_t frame_id, const lorb_frame_out* d_cur,
                              int32_t n_max_cur, const lorb_frame_slots* d_cur_slots, const int32_t* d_cur_slot_gid,
                              const int32_t* d_cur_slot_id, const lorb_local_map_arrays* lmap,
                              const lorb_local_map_result* d_update, const uint8_t* d_in_view,
                              const int32_t* d_local_status, int32_t found_rule, lorb_kf_observe_result* d_result) {
  if (!d_cur || !d_cur_slots || !d_cur_slot_gid || !d_cur_slot_id || !lmap || !d_update || !d_in_view || !d_result)
    return LORB_E_INVALID;
  LORB_TRY(lorb::kf_enter(ctx, S));
  if (n_max_cur < 1) return lorb::set_error(ctx, LORB_E_INVALID, "bound %d must be positive", n_max_cur);
  if (found_rule != LORB_KF_FOUND_NEVER && found_rule != LORB_KF_FOUND_SLOTS)
    return lorb::set_error(ctx, LORB_E_INVALID, "unknown found rule %d", found_rule);
  if (!d_cur->counts || !d_cur_slots->state || !lmap->l2g) return lorb::set_error(ctx, LORB_E_INVALID, "null array");
  if (lmap->max_local < 1) return lorb::set_error(ctx, LORB_E_INVALID, "max_local %d must be positive", lmap->max_local);
  ObserveArgs a{};
  a.frame_id = frame_id; a.n_max = n_max_cur; a.max_local = lmap->max_local; a.found_rule = found_rule;
  a.count = d_cur->counts; a.state = d_cur_slots->state; a.gid = d_cur_slot_gid; a.lid = d_cur_slot_id; a.l2g = lmap->l2g;
  a.update = d_update; a.in_view = d_in_view; a.local_status = d_local_status;
  a.cnt = S->cnt; a.visible = S->visible; a.found = S->found; a.frame_word = S->frame_word; a.rec = d_result;
  hipLaunchKernelGGL(k_kf_observe, dim3(1), dim3(kT), 0, ctx->stream, a);
  LORB_CHECK_LAUNCH(ctx);
  return LORB_OK;
}

int lorb_kf_store_cull_dev(lorb_ctx* ctx, lorb_kf_store* S, const int32_t* d_kf, const int32_t* d_src_status,
                           const lorb_kf_cull_params* par, const lorb_frame_out* d_cur, int32_t n_max_cur,
                           const lorb_frame_slots* d_cur_slots, int32_t* d_cur_slot_gid, lorb_kf_cull_result* d_result) {
  if (!d_kf || !par || !d_result) return LORB_E_INVALID;
  LORB_TRY(lorb::kf_enter(ctx, S, lorb::kKfNeedGeom));
  if (par->age_obs < 0 || par->age_out < 0 || std::isnan(par->min_found_ratio))
    return lorb::set_error(ctx, LORB_E_INVALID, "cull parameters: ratio %g, ages %d / %d", (double)par->min_found_ratio,
                           par->age_obs, par->age_out);
  const bool any = d_cur || d_cur_slots || d_cur_slot_gid, all = d_cur && d_cur_slots && d_cur_slot_gid;
  if (any && !all) return lorb::set_error(ctx, LORB_E_INVALID, "the frame group is given in part");
  if (all) {
    if (n_max_cur < 1) return lorb::set_error(ctx, LORB_E_INVALID, "bound %d must be positive", n_max_cur);
    if (!d_cur->counts || !d_cur_slots->state) return lorb::set_error(ctx, LORB_E_INVALID, "null array");
  }
  CullArgs a = cull_args(S);
  a.par = *par; a.d_kf = d_kf; a.src_status = d_src_status; a.rec = d_result;
  if (all) {
    a.n_max = n_max_cur; a.count = d_cur->counts; a.state = d_cur_slots->state; a.gid = d_cur_slot_gid;
  }
  hipStream_t st = ctx->stream;
  // grids from the host's bounds: the kernels read the true counts
  const unsigned pt_blocks = lorb::ceil_div((size_t)S->b_points + 1, kT);
  const unsigned fr_blocks = std::max(pt_blocks, all ? lorb::ceil_div((size_t)n_max_cur, kT) : 1u);
  hipLaunchKernelGGL(k_kf_cull_head, dim3(1), dim3(64), 0, st, a);
  LORB_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(k_kf_cull_verdict, dim3(pt_blocks), dim3(kT), 0, st, a);
  LORB_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(k_kf_cull_frame, dim3(fr_blocks), dim3(kT), 0, st, a);
  LORB_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(k_kf_cull_scatter, dim3(pt_blocks), dim3(kT), 0, st, a);
  LORB_CHECK_LAUNCH(ctx);
  return LORB_OK;
}

}  // extern "C"
