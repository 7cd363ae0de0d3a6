// lorb_kfretire.hip -- retiring keyframes on the keyframe store: lorb_kf_store_retire_dev, which is Frame::SetBadFlag
// (src/frame.cpp:684-714) for a set of keyframes, with Frame::EraseConnection and its re-sort (:791-798, :754-774),
// MapPoint::EraseObservation with the mpRefKF hand-over and the cascade into MapPoint::SetBadFlag
// (src/map_point.cpp:141-153, :184-199).  Which keyframes go is the caller's: the reference's KeyFramesCulling is
// empty (src/local_mapping.cpp:110-113).  The contract is in lorb_c.h.
//
// The list is retired as a SET V: a point's observation count only falls and a retired keyframe's own maps are
// cleared whatever its neighbours did before, so the store is the one the reference leaves after retiring the list
// one keyframe after another, in any order.  Membership of V is a byte per keyframe (rt_mark, at rest between calls);
// the points' marks ride in the cull's cull_mark (1: loses entries, 2: dies), the CSR copy in the insertion's
// off2 / kf2 / slot2, the tile counts in tile_cnt.
//
// retire is SIX launches on the ctx stream:
//   k_kf_retire_head    one workgroup, a thread per list entry: status, the class of every entry (outside the store,
//                       duplicate, bad, kf_fid 0, protected, V), V in list order and its marks, the true counts into
//                       KfRetireCtl, the record
//   k_kf_retire_points  a thread per point: the observations it loses; a point left with two or fewer is
//                       MapPoint::SetBadFlag -- is_bad, the -1 in every surviving keyframe's slot; the observations
//                       given up per 1024-point tile; the CSR (offsets, keyframes, slots) copied to scratch; the
//                       record's counters and the true n_obs by integer atomics
//   k_kf_retire_scatter the CSR back: every list moves left by the observations given up in front of it, a trimmed
//                       list keeps its order without V's entries; the points' marks go back to rest
//   k_kf_retire_conn    one workgroup per keyframe outside V: the keys of its weight map that are in V and whose own
//                       map names it (binary search) leave the row, order kept; a row that lost one is re-sorted from
//                       ALL of its map by (weight, index) into its ordered list (k_kf_order's key and order)
//   k_kf_retire_rows    one workgroup per keyframe of V: its slot row becomes -1, conn_n = ord_n = 0, kf_bad = 1,
//                       its mark goes back to rest
//   k_kf_retire_cov     the covisibility CSR from the ordered rows, from the first changed row on (k_kf_cov's scheme);
//                       the true n_cov and n_conn; the record's counts
// Every kernel after the first returns at once on an empty V (KfRetireCtl::go), the scatter also when no point lost an
// observation: the CSR is not rewritten.  All counting is integer: no result depends on the order the atomics arrive
// in.  No kernel uses floating point.
#include <algorithm>

#include "lorb_internal.h"
#include "lorb_kfstore.h"

namespace {

constexpr int kT = lorb::kKfTile;  // threads per workgroup = points per tile = the longest list
constexpr int kRowMax = 4096;      // keys of one weight map sort in LDS = the largest max_kf (lorb_kfstore.hip's kSortMax)
constexpr int kMaxRows = 128;      // workgroups of the grid-stride kernels over keyframes
static_assert(LORB_KF_RETIRE_MAX_LIST == kT, "one list entry per thread of k_kf_retire_head");
using Ctl = lorb::KfRetireCtl;

struct RetireArgs {
  int max_kf, max_points, max_obs, max_kf_slots, max_cov;
  int n_max_list, n_protect;
  const int *list, *n_list, *src_status;  // src_status: or null
  const int* protect;                     // n_protect words, or null
  int* cnt;
  uint8_t *is_bad, *kf_bad, *pmark, *kmark;
  const int* kf_fid;
  int *obs_off, *obs_kf, *obs_slot;
  const int* kf_slot_off;
  int* kf_slot_point;
  int *off2, *kf2, *slot2, *tile;
  int *conn_n, *conn_kf, *conn_w, *ord_n, *ord_kf, *cov_off, *cov_kf;
  int* v;
  Ctl* ctl;
  lorb_kf_retire_result* rec;
};

// a + b. status, then the class of every list entry in the contract's order
enum { cRange = 0, cDup, cBad, cFirst, cProtect, cTake, cClasses };

__global__ __launch_bounds__(kT) void k_kf_retire_head(RetireArgs a) {
  __shared__ int s_list[kT];
  __shared__ int s_c[cClasses];
  __shared__ int wsum[16];
  const int t = threadIdx.x;
  const int n = a.n_list[0];
  const int nk = a.cnt[0], P = a.cnt[1], O = a.cnt[2], S = a.cnt[3], nc = a.cnt[4], nn = a.cnt[5];
  // a. status: nothing but the record's word is written
  const bool ok = !(a.src_status && *a.src_status != 0) && n >= 0 && n <= a.n_max_list && nk >= 0 && nk <= a.max_kf &&
                  P >= 0 && P <= a.max_points && O >= 0 && O <= a.max_obs && S >= 0 && S <= a.max_kf_slots && nc >= 0 &&
                  nc <= a.max_cov && nn >= 0 && nn <= a.max_cov;
  if (!ok) {
    if (t == 0) {
      a.rec->status = 1;
      a.ctl->go = 0;
    }
    return;
  }
  const int e = t < n ? a.list[t] : -1;
  s_list[t] = e;
  if (t < cClasses) s_c[t] = 0;
  __syncthreads();
  int cls = -1;
  if (t < n) {
    if ((unsigned)e >= (unsigned)nk) cls = cRange;  // 1.
    else {
      bool dup = false, prot = false;
      for (int j = 0; j < t; ++j) dup |= s_list[j] == e;
      for (int j = 0; j < a.n_protect; ++j) prot |= a.protect[j] == e;
      if (dup) cls = cDup;                    // 2. equal to an earlier entry
      else if (a.kf_bad[e]) cls = cBad;       // 3.
      else if (a.kf_fid[e] == 0) cls = cFirst;  // 4. if(mnId == 0) return; (src/frame.cpp:686-687)
      else if (prot) cls = cProtect;          // 5.
      else cls = cTake;
    }
    atomicAdd(&s_c[cls], 1);
  }
  int n_v;
  const int at = lorb::block_excl_scan_1024(cls == cTake, wsum, &n_v);  // its barriers settle s_c
  if (cls == cTake) {  // V in list order; an entry of V is unique, so no two threads meet
    a.v[at] = e;
    a.kmark[e] = 1;
  }
  if (t != 0) return;
  *a.ctl = Ctl{n_v > 0, nk, P, O, S, n_v, 0, nk};
  *a.rec = lorb_kf_retire_result{0, s_c[cRange], s_c[cDup], s_c[cBad], s_c[cFirst], s_c[cProtect], n_v, 0, 0, 0, 0, 0, 0, 0,
                                 O, nc, nn};
}

// c. MapPoint::EraseObservation of every keyframe of V (src/map_point.cpp:141-153), from the lists alone
enum { pErased = 0, pBad, pGone, pSlots, pBadSlot, pAffected, pCount };

__device__ __forceinline__ bool in_v(const RetireArgs& a, int f, int nk) { return (unsigned)f < (unsigned)nk && a.kmark[f]; }

__global__ __launch_bounds__(kT) void k_kf_retire_points(RetireArgs a) {
  __shared__ int s_c[pCount];
  const Ctl& h = *a.ctl;
  if (!h.go) return;
  const int t = threadIdx.x, P = h.P, O = h.O, S = h.S, nk = h.nk;
  // the CSR as it stands into scratch
  const long long i0 = (long long)blockIdx.x * kT + t, step = (long long)gridDim.x * kT;
  for (long long p = i0; p <= P; p += step) a.off2[p] = a.obs_off[p];
  for (long long o = i0; o < O; o += step) {
    a.kf2[o] = a.obs_kf[o];
    a.slot2[o] = a.obs_slot[o];
  }
  if ((long long)blockIdx.x * kT >= P) return;
  if (t < pCount) s_c[t] = 0;
  __syncthreads();
  const int p = blockIdx.x * kT + t;
  if (p < P) {
    const auto [lo, hi] = lorb::kf_range(a.obs_off, p, O);
    int r = 0;
    for (int o = lo; o < hi; ++o) r += in_v(a, a.obs_kf[o], nk);
    if (r > 0) {
      const int len = hi - lo;
      atomicAdd(&s_c[pAffected], 1);
      if (len - r > 2) {  // the entries leave; mpRefKF stays the first entry of the list (:147-148)
        a.pmark[p] = 1;
        atomicAdd(&s_c[pErased], r);
        atomicAdd(&s_c[pGone], r);
      } else {  // if(mnObs <= 2) SetBadFlag(); (:151-152, :184-199)
        a.pmark[p] = 2;
        a.is_bad[p] = 1;
        int erased = 0;
        for (int o = lo; o < hi; ++o) {  // Frame::EraseMapPoint(it->second) of the observations that remain
          const int f = a.obs_kf[o], s = a.obs_slot[o];
          if (in_v(a, f, nk)) continue;  // its whole row is cleared (k_kf_retire_rows)
          if ((unsigned)f >= (unsigned)nk) continue;
          const auto [l0, l1] = lorb::kf_range(a.kf_slot_off, f, S);
          if ((unsigned)s >= (unsigned)(l1 - l0) || a.kf_slot_point[l0 + s] != p) continue;
          a.kf_slot_point[l0 + s] = -1;
          ++erased;
        }
        atomicAdd(&s_c[pBad], 1);
        atomicAdd(&s_c[pGone], len);
        if (erased) atomicAdd(&s_c[pSlots], erased);
        if (len - r > erased) atomicAdd(&s_c[pBadSlot], len - r - erased);
      }
    }
  }
  __syncthreads();
  if (t != 0) return;
  const int gone = s_c[pGone];
  a.tile[blockIdx.x] = gone;  // the observations this tile gives up
  lorb_kf_retire_result* r = a.rec;
  if (s_c[pErased]) atomicAdd(&r->n_obs_erased, s_c[pErased]);
  if (s_c[pBad]) atomicAdd(&r->n_points_bad, s_c[pBad]);
  if (s_c[pSlots]) atomicAdd(&r->n_slots_erased, s_c[pSlots]);
  if (s_c[pBadSlot]) atomicAdd(&r->n_obs_bad_slot, s_c[pBadSlot]);
  if (s_c[pAffected]) atomicAdd(&a.ctl->n_affected, s_c[pAffected]);
  if (gone) {
    atomicAdd(&r->n_obs_removed, gone);
    atomicSub(&a.cnt[2], gone);
  }
}

// c, the lists: point p's list moves left by the observations given up in front of it; a trimmed list keeps its
// order without V's entries, a dead point's list becomes empty.  Launched over the bound on n_points + 1.
__global__ __launch_bounds__(kT) void k_kf_retire_scatter(RetireArgs a) {
  __shared__ int wsum[16];
  const Ctl& h = *a.ctl;
  if (!h.go || h.n_affected == 0) return;
  const int t = threadIdx.x, b = blockIdx.x, P = h.P, O = h.O, nk = h.nk;
  if ((long long)b * kT > P) return;
  const int n_tiles = (P + kT - 1) / kT;
  int tot;
  const int base = lorb::tile_base_1024(a.tile, min(b, n_tiles), wsum);
  const int p = b * kT + t;
  int lo = 0, hi = 0, m = 0, gone = 0;
  if (p < P) {
    const lorb::KfRange r = lorb::kf_range(a.off2, p, O);
    lo = r.lo; hi = r.hi;
    m = a.pmark[p];
    if (m == 2) gone = hi - lo;
    else if (m == 1)
      for (int o = lo; o < hi; ++o) gone += in_v(a, a.kf2[o], nk);
  }
  const int before = base + lorb::block_excl_scan_1024(gone, wsum, &tot);
  if (p < P) {
    if (m) a.pmark[p] = 0;  // back at rest
    const int at = lo - before;
    if ((before || m) && at >= 0) {
      a.obs_off[p] = at;
      if (m != 2) {
        int w = at;
        for (int o = lo; o < hi; ++o) {
          const int f = a.kf2[o];
          if (m == 1 && in_v(a, f, nk)) continue;
          a.obs_kf[w] = f;
          a.obs_slot[w] = a.slot2[o];
          ++w;
        }
      }
    }
  } else if (p == P) {
    a.obs_off[P] = max(lorb::clampi(a.off2[P], 0, O) - before, 0);
  }
}

// d. Frame::EraseConnection(f) on every g outside V that f's weight map names (src/frame.cpp:690-693, :791-798):
// g loses the key f when its own map has it, and UpdateBestCovisibleFrames (:754-774) re-sorts ALL of g's map
__global__ __launch_bounds__(kT) void k_kf_retire_conn(RetireArgs a) {
  __shared__ unsigned long long s_key[kRowMax];
  __shared__ int wsum[16];
  const Ctl& h = *a.ctl;
  if (!h.go) return;
  const int t = threadIdx.x, nk = h.nk, stride = a.max_kf;
  for (int g = blockIdx.x; g < nk; g += gridDim.x) {
    if (a.kmark[g]) continue;
    const size_t row = (size_t)g * stride;
    const int m = lorb::clampi(a.conn_n[g], 0, stride);
    int kept = 0;
    for (int base = 0; base < m; base += kT) {  // the row in ascending key order, 1024 keys at a time
      const int q = base + t;
      int keep = 0;
      unsigned long long key = 0;
      if (q < m) {
        const int f = a.conn_kf[row + q], w = a.conn_w[row + q];
        key = ((unsigned long long)(unsigned)w << 32) | (unsigned)f;
        keep = 1;
        if (in_v(a, f, nk)) {  // the reference iterates f's map: does it name g?
          const int* fr = a.conn_kf + (size_t)f * stride;
          int l = 0, r = lorb::clampi(a.conn_n[f], 0, stride);
          while (l < r) {
            const int mid = (l + r) >> 1;
            if (fr[mid] < g) l = mid + 1;
            else r = mid;
          }
          if (l < lorb::clampi(a.conn_n[f], 0, stride) && fr[l] == g) keep = 0;
        }
      }
      int tot;
      const int at = kept + lorb::block_excl_scan_1024(keep, wsum, &tot);
      if (keep) s_key[at] = key;
      kept += tot;
    }
    __syncthreads();
    if (kept == m) continue;  // nothing erased: the row and its ordered list stay
    for (int q = t; q < kept; q += kT) {  // the row back, still ascending by key
      const unsigned long long key = s_key[q];
      a.conn_kf[row + q] = (int)(unsigned)(key & 0xffffffffull);
      a.conn_w[row + q] = (int)(unsigned)(key >> 32);
    }
    int np2 = 1;
    while (np2 < kept) np2 <<= 1;
    for (int q = kept + t; q < np2; q += kT) s_key[q] = ~0ull;
    __syncthreads();
    lorb::kf_sort_keys_1024(s_key, np2);
    for (int q = t; q < kept; q += kT) a.ord_kf[row + q] = (int)(unsigned)(s_key[q] & 0xffffffffull);
    if (t == 0) {
      a.conn_n[g] = kept;
      a.ord_n[g] = kept;
      atomicAdd(&a.rec->n_conn_erased, m - kept);
      atomicAdd(&a.rec->n_rows_reordered, 1);
      atomicMin(&a.ctl->first_row, g);
    }
    __syncthreads();  // s_key is the next row's
  }
}

// e. the retired keyframes (src/frame.cpp:705-711); the whole slot row becomes -1 so that it holds no dead point
// against a compaction
__global__ __launch_bounds__(kT) void k_kf_retire_rows(RetireArgs a) {
  const Ctl& h = *a.ctl;
  if (!h.go) return;
  const int t = threadIdx.x;
  for (int i = blockIdx.x; i < h.n_v; i += gridDim.x) {
    const int f = a.v[i];
    const auto [l0, l1] = lorb::kf_range(a.kf_slot_off, f, h.S);
    for (int s = l0 + t; s < l1; s += kT) a.kf_slot_point[s] = -1;
    if (t == 0) {
      a.conn_n[f] = 0;
      a.ord_n[f] = 0;
      a.kf_bad[f] = 1;
      a.kmark[f] = 0;  // back at rest
      atomicMin(&a.ctl->first_row, f);
    }
  }
}

// e + f. mvpOrderedKeyFrames as the view's CSR from the first changed row on: every workgroup scans the row lengths,
// then copies its share of the rows (k_kf_cov's scheme); the true n_cov and n_conn; the record's counts
__global__ __launch_bounds__(kT) void k_kf_retire_cov(RetireArgs a) {
  __shared__ int s_off[kRowMax + 1];
  __shared__ int wsum[16];
  const Ctl& h = *a.ctl;
  if (!h.go) return;
  const int t = threadIdx.x, nk = h.nk, stride = a.max_kf;
  int run = 0, conn = 0;
  for (int base = 0; base < nk; base += kT) {
    const int k = base + t;
    int tot;
    const int at = run + lorb::block_excl_scan_1024(k < nk ? a.ord_n[k] : 0, wsum, &tot);
    if (k < nk) s_off[k] = at;
    run += tot;
    lorb::block_excl_scan_1024(k < nk ? a.conn_n[k] : 0, wsum, &tot);
    conn += tot;
  }
  if (t == 0) s_off[nk] = run;
  __syncthreads();
  const int first = lorb::clampi(h.first_row, 0, nk);
  if (blockIdx.x == 0) {
    for (int k = first + t; k <= nk; k += kT) a.cov_off[k] = s_off[k];
    if (t == 0) {
      a.cnt[4] = run;
      a.cnt[5] = conn;
      a.rec->n_obs = a.cnt[2];
      a.rec->n_cov = run;
      a.rec->n_conn = conn;
    }
  }
  for (int f = first + blockIdx.x; f < nk; f += gridDim.x) {
    const int lo = s_off[f], len = s_off[f + 1] - lo;
    for (int q = t; q < len; q += kT) a.cov_kf[lo + q] = a.ord_kf[(size_t)f * stride + q];
  }
}

}  // namespace

extern "C" {

int lorb_kf_store_retire_dev(lorb_ctx* ctx, lorb_kf_store* S, const int32_t* d_list, const int32_t* d_n_list,
                             int32_t n_max_list, const int32_t* d_protect, int32_t n_protect, const int32_t* d_src_status,
                             lorb_kf_retire_result* d_result) {
  if (!d_list || !d_n_list || !d_result) return LORB_E_INVALID;
  LORB_TRY(lorb::kf_enter(ctx, S, lorb::kKfNeedGeom));
  if (n_max_list < 1 || n_max_list > LORB_KF_RETIRE_MAX_LIST)
    return lorb::set_error(ctx, LORB_E_INVALID, "list bound %d outside [1, %d]", n_max_list, LORB_KF_RETIRE_MAX_LIST);
  if (n_protect < 0 || n_protect > LORB_KF_RETIRE_MAX_PROTECT)
    return lorb::set_error(ctx, LORB_E_INVALID, "%d protected words outside [0, %d]", n_protect, LORB_KF_RETIRE_MAX_PROTECT);
  if (n_protect > 0 && !d_protect) return lorb::set_error(ctx, LORB_E_INVALID, "null protected words");
  RetireArgs a{};
  a.max_kf = S->cap.max_kf; a.max_points = S->cap.max_points; a.max_obs = S->cap.max_obs; a.max_kf_slots = S->cap.max_kf_slots;
  a.max_cov = S->max_cov; a.n_max_list = n_max_list; a.n_protect = n_protect;
  a.list = d_list; a.n_list = d_n_list; a.src_status = d_src_status; a.protect = d_protect;
  a.cnt = S->cnt; a.is_bad = S->is_bad; a.kf_bad = S->kf_bad; a.pmark = S->cull_mark; a.kmark = S->rt_mark; a.kf_fid = S->kf_fid;
  a.obs_off = S->obs_off; a.obs_kf = S->obs_kf; a.obs_slot = S->obs_slot;
  a.kf_slot_off = S->kf_slot_off; a.kf_slot_point = S->kf_slot_point;
  a.off2 = S->off2; a.kf2 = S->kf2; a.slot2 = S->slot2; a.tile = S->tile_cnt;
  a.conn_n = S->conn_n; a.conn_kf = S->conn_kf; a.conn_w = S->conn_w; a.ord_n = S->ord_n; a.ord_kf = S->ord_kf;
  a.cov_off = S->cov_off; a.cov_kf = S->cov_kf;
  a.v = S->rt_v; a.ctl = S->rt_ctl; a.rec = d_result;
  hipStream_t st = ctx->stream;
  // grids from the host's bounds: the kernels read the true counts
  const unsigned pt_blocks = lorb::ceil_div((size_t)S->b_points + 1, kT);
  const unsigned kf_blocks = (unsigned)std::clamp(S->b_kf, 1, kMaxRows);
  const unsigned v_blocks = (unsigned)std::min(n_max_list, kMaxRows);
  hipLaunchKernelGGL(k_kf_retire_head, dim3(1), dim3(kT), 0, st, a);
  LORB_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(k_kf_retire_points, dim3(pt_blocks), dim3(kT), 0, st, a);
  LORB_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(k_kf_retire_scatter, dim3(pt_blocks), dim3(kT), 0, st, a);
  LORB_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(k_kf_retire_conn, dim3(kf_blocks), dim3(kT), 0, st, a);
  LORB_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(k_kf_retire_rows, dim3(v_blocks), dim3(kT), 0, st, a);
  LORB_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(k_kf_retire_cov, dim3(kf_blocks), dim3(kT), 0, st, a);
  LORB_CHECK_LAUNCH(ctx);
  return LORB_OK;
}

}  // extern "C"
