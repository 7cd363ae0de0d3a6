// lorb_localmap.hip -- VisualOdometry::UpdateLocalMap (src/visual_odometry.cpp:234-340) on the device,
// between the two tracking stages of the frame chain: lorb_local_map_create / _destroy / _view,
// lorb_local_map_update_dev and lorb_local_map_ids_back_dev.
//
// The map store is the caller's (lorb_map_store: device arrays, host counts); the local map is an
// object that owns its table, its index maps and its scratch (lorb::Arena), so the unit takes no ctx
// scratch slot.  An update is five launches on the ctx stream:
//   k_lm_vote     one workgroup: the status; the clear of the point flags; the slots' global ids and
//                 step 1.1 (bad held points nulled, one vote per observing keyframe, counted in LDS);
//                 steps 1.2-1.3 (ordered compaction of the voted keyframes, first-wins arg-max, the
//                 expansion by one wavefront); the record's counts
//   k_lm_mark     step 2's membership: a flag per point held by a local keyframe (same-value writes)
//   k_lm_count    flagged points per 1024-point tile
//   k_lm_compact  the ordered compaction over all points -- a tile's base is the sum of the tile
//                 counts before it, so the order holds across tiles -- with the table rows gathered
//                 by the thread that placed them, the is_bad padding, n_local and status 2
//   k_lm_ids      the slots' local rows
// Every kernel after the first returns on the first one's verdict (Ctl::ok), so status 1 writes nothing.
// All index arithmetic is integer: the results do not depend on the order the atomics arrive in.
#include <algorithm>

#include "lorb_internal.h"

namespace {

constexpr int kTile = 1024;     // points per compaction tile = threads per workgroup
constexpr int kVoteWin = 4096;  // keyframes whose votes are counted in LDS at a time

struct Ctl {
  int ok;          // k_lm_vote's verdict on the status
  int n_local_kf;  // the list's length after the expansion
  int over;        // n_local > max_local
  int pad;
};

}  // namespace

struct lorb_local_map {
  lorb_ctx* ctx = nullptr;
  int max_local = 0, max_kf = 0, max_points = 0;
  lorb::Arena mem;
  // the local table
  float *pos = nullptr, *normal = nullptr, *max_dist = nullptr, *min_dist = nullptr;
  uint8_t *desc = nullptr, *locked = nullptr, *is_bad = nullptr;
  int *l2g = nullptr, *g2l = nullptr, *kf_votes = nullptr, *local_kf = nullptr;
  // scratch
  uint8_t* flag = nullptr;  // max_points rounded up to 16: the point is held by a local keyframe
  int* tile_cnt = nullptr;  // flagged points per tile
  Ctl* ctl = nullptr;
};

namespace {

struct VoteArgs {
  const int* count;  // the frame's counts (entry 0)
  int n_max;
  const int* src_status;  // or null
  uint8_t* state;         // n_max: the frame's slot states
  int* gid;               // n_max
  // the store
  int n_points, n_kf, n_obs, n_cov;
  const uint8_t* pt_bad;  // or null
  const int *obs_off, *obs_kf;
  const uint8_t* kf_bad;
  const int *cov_off, *cov_kf;
  // the object
  int* votes;
  int* local_kf;
  uint8_t* flag;
  Ctl* ctl;
  lorb_local_map_result* rec;
  // the id source (motion_assign null: none)
  const int* motion_assign;
  const lorb_track_frames_result* motion_rec;
  const int* last_gid;
  int n_max_last, given;
};

// [off[i], off[i + 1]) clipped to [0, len)
__device__ __forceinline__ void csr_range(const int* off, int i, int len, int* lo, int* hi) {
  const int a = off[i], b = off[i + 1];
  *lo = min(max(a, 0), len);
  *hi = min(max(b, *lo), len);
}

__global__ __launch_bounds__(1024) void k_lm_vote(VoteArgs a) {
  __shared__ lorb::I4 wsum4[16];
  __shared__ int wsum[16];
  __shared__ unsigned long long wkey[16];
  __shared__ int s_list[16];  // the list's first entries: all of it whenever the expansion runs
  __shared__ int s_votes[kVoteWin];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int n = a.count[0];
  const bool ok = n >= 0 && n <= a.n_max && !(a.src_status && *a.src_status != 0);
  if (t == 0) {
    a.rec->status = ok ? 0 : 1;
    a.ctl->ok = ok;
  }
  if (!ok) return;
  uint4* f4 = reinterpret_cast<uint4*>(a.flag);
  for (int q = t; q < (a.n_points + 15) / 16; q += 1024) f4[q] = make_uint4(0, 0, 0, 0);
  const bool keep = a.motion_assign && a.given && a.motion_rec->motion.pass == 1;
  // b + c: the slots' global ids, and step 1.1's emptying of the slots that hold a bad point (:254-257)
  lorb::I4 c = {{0, 0, 0, 0}};
  for (int j = t; j < n; j += 1024) {
    int g = a.gid[j];
    if (a.motion_assign) g = lorb::motion_entry_id(g, a.motion_assign[j], keep, a.last_gid, a.n_max_last);
    if ((unsigned)g >= (unsigned)a.n_points) g = -1;  // a point outside the store
    if (a.state[j] != LORB_SLOT_EMPTY) {
      if (g >= 0 && a.pt_bad && a.pt_bad[g]) {
        a.state[j] = LORB_SLOT_EMPTY;
        g = -1;
        c.v[1]++;
      } else {
        c.v[0]++;
      }
    }
    a.gid[j] = g;
  }
  lorb::I4 tot4;
  lorb::block_excl_scan4<1024>(c, wsum4, &tot4);
  // c + d: the votes (:248-252) and steps 1.2-1.3.1 (:263-280), kVoteWin keyframes at a time: the window's
  // counters live in LDS (a few keyframes take every vote, and LDS atomics on one address are cheap where
  // global ones queue at the L2); every thread walks the slots it wrote above (its own stores: no fence),
  // then the window's voted keyframes that are not bad join the list in ascending index
  int n0 = 0, best_v = 0, best_k = 0;
  for (int w0 = 0; w0 < a.n_kf; w0 += kVoteWin) {
    const int wn = min(kVoteWin, a.n_kf - w0);
    for (int k = t; k < wn; k += 1024) s_votes[k] = 0;
    __syncthreads();
    for (int j = t; j < n; j += 1024) {
      const int g = a.gid[j];
      if (g < 0 || a.state[j] == LORB_SLOT_EMPTY) continue;
      int lo, hi;
      csr_range(a.obs_off, g, a.n_obs, &lo, &hi);
      for (int o = lo; o < hi; ++o) {
        const int kf = a.obs_kf[o] - w0;
        if ((unsigned)kf < (unsigned)wn) atomicAdd(&s_votes[kf], 1);
      }
    }
    __syncthreads();
    for (int base = 0; base < wn; base += 1024) {
      const int k = base + t;
      const int v = k < wn ? s_votes[k] : 0;
      if (k < wn) a.votes[w0 + k] = v;
      const int in = v > 0 && !a.kf_bad[w0 + k];
      int tot;
      const int at = n0 + lorb::block_excl_scan_1024(in, wsum, &tot);
      if (in) {
        a.local_kf[at] = w0 + k;
        if (at < 16) s_list[at] = w0 + k;
        if (v > best_v) { best_v = v; best_k = w0 + k; }  // ascending k per thread: the first of equals stays
      }
      n0 += tot;
    }
  }
  // pFMax: the strictly largest vote, the lowest index among equals (:274)
  unsigned long long key = best_v > 0 ? ((unsigned long long)best_v << 32) | (unsigned)(0x7fffffff - best_k) : 0ull;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) key = max(key, (unsigned long long)__shfl_xor((long long)key, o, 64));
  if (lane == 0) wkey[wv] = key;
  __syncthreads();  // wkey and s_list are complete
  if (wv != 0) return;
  // the expansion (:282-307) as an index loop over the growing list, by wavefront 0: lane c looks at
  // entry c of the visited frame's first 10 covisibles, the lowest eligible lane's frame is appended
  int nl = n0;
  for (int i = 0; i < nl && nl <= 10; ++i) {
    const int f = s_list[i];
    int lo, hi;
    csr_range(a.cov_off, f, a.n_cov, &lo, &hi);
    int b = -1;
    if (lane < min(hi - lo, 10)) {
      b = a.cov_kf[lo + lane];
      if ((unsigned)b >= (unsigned)a.n_kf || a.kf_bad[b]) b = -1;
      for (int q = 0; q < nl; ++q)
        if (s_list[q] == b) b = -1;
    }
    const unsigned long long m = __ballot(b >= 0);
    if (m) {
      const int nb = __shfl(b, __ffsll((long long)m) - 1, 64);
      if (lane == 0) {
        s_list[nl] = nb;
        a.local_kf[nl] = nb;
      }
      nl++;
    }
  }
  if (t == 0) {
    unsigned long long kmax = 0;
    for (int w = 0; w < 16; ++w) kmax = max(kmax, wkey[w]);
    a.rec->n_cur = n;
    a.rec->n_held = tot4.v[0];
    a.rec->n_nulled = tot4.v[1];
    a.rec->n_voted = n0;
    a.rec->n_local_kf = nl;
    a.rec->refer_kf = kmax ? 0x7fffffff - (int)(unsigned)(kmax & 0xffffffffull) : -1;
    a.ctl->n_local_kf = nl;
  }
}

// e, membership: every non-bad point in a slot of a local keyframe (:316-328)
__global__ __launch_bounds__(256) void k_lm_mark(const Ctl* ctl, const int* local_kf, const int* kf_slot_off,
                                                 const int* kf_slot_point, int n_kf_slots, int n_points,
                                                 const uint8_t* pt_bad, uint8_t* flag) {
  if (!ctl->ok) return;
  const int nl = ctl->n_local_kf;
  for (int li = blockIdx.x; li < nl; li += gridDim.x) {
    int lo, hi;
    csr_range(kf_slot_off, local_kf[li], n_kf_slots, &lo, &hi);
    for (int s = lo + threadIdx.x; s < hi; s += 256) {
      const int p = kf_slot_point[s];
      if ((unsigned)p < (unsigned)n_points && !(pt_bad && pt_bad[p])) flag[p] = 1;
    }
  }
}

__global__ __launch_bounds__(kTile) void k_lm_count(const Ctl* ctl, const uint8_t* flag, int n_points, int* tile_cnt) {
  __shared__ int wsum[16];
  if (!ctl->ok) return;
  const int p = blockIdx.x * kTile + threadIdx.x;
  int tot;
  lorb::block_excl_scan_1024(p < n_points && flag[p], wsum, &tot);
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = tot;
}

struct CompactArgs {
  Ctl* ctl;
  const uint8_t* flag;
  const int* tile_cnt;
  int n_points, n_tiles, max_local;
  lorb_map_points_dev src;
  float *pos, *normal, *max_dist, *min_dist;
  uint8_t *desc, *locked, *is_bad;
  int *l2g, *g2l;
  lorb_local_map_result* rec;
};

// e, order: the local points in ascending global index.  Launched over max(point tiles, table tiles).
__global__ __launch_bounds__(kTile) void k_lm_compact(CompactArgs a) {
  __shared__ lorb::I4 wsum4[16];
  __shared__ int wsum[16];
  if (!a.ctl->ok) return;
  const int t = threadIdx.x, b = blockIdx.x;
  lorb::I4 s = {{0, 0, 0, 0}};  // [0] flagged points in the tiles before this one, [1] in all tiles
  for (int i = t; i < a.n_tiles; i += kTile) {
    const int c = a.tile_cnt[i];
    s.v[0] += i < b ? c : 0;
    s.v[1] += c;
  }
  lorb::I4 tot4;
  lorb::block_excl_scan4<kTile>(s, wsum4, &tot4);
  const int base = tot4.v[0], n_local = tot4.v[1];
  const bool over = n_local > a.max_local;
  const int p = b * kTile + t;
  const int f = p < a.n_points && a.flag[p];
  int tot;
  const int r = base + lorb::block_excl_scan_1024(f, wsum, &tot);
  if (p < a.n_points) a.g2l[p] = f && !over ? r : -1;
  if (f && !over) {
    a.l2g[r] = p;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      a.pos[3 * r + k] = a.src.pos[3 * (size_t)p + k];
      a.normal[3 * r + k] = a.src.normal[3 * (size_t)p + k];
    }
    a.max_dist[r] = a.src.max_dist[p];
    a.min_dist[r] = a.src.min_dist[p];
    const uint4* sd = reinterpret_cast<const uint4*>(a.src.desc) + 2 * (size_t)p;
    uint4* dd = reinterpret_cast<uint4*>(a.desc) + 2 * (size_t)r;
    const uint4 d0 = sd[0], d1 = sd[1];
    dd[0] = d0;
    dd[1] = d1;
    a.locked[r] = a.src.locked[p];
    a.is_bad[r] = 0;
  }
  if (p < a.max_local && (over || p >= n_local)) a.is_bad[p] = 1;
  if (b == 0 && t == 0) {
    a.rec->n_local = n_local;
    if (over) a.rec->status = 2;
    a.ctl->over = over;
  }
}

// f: the slots' local rows
__global__ __launch_bounds__(256) void k_lm_ids(const Ctl* ctl, const int* count, const uint8_t* state, const int* gid,
                                                const int* g2l, int n_points, int* slot_id) {
  if (!ctl->ok || ctl->over) return;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= count[0]) return;
  const int g = gid[j];
  slot_id[j] = state[j] != LORB_SLOT_EMPTY && (unsigned)g < (unsigned)n_points ? g2l[g] : -1;
}

__global__ __launch_bounds__(256) void k_lm_ids_back(const int* count, int n_max, const int* status, const uint8_t* state,
                                                     const int* slot_id, const int* l2g, int max_local, int* gid) {
  const int n = count[0];
  if (n < 0 || n > n_max || (status && *status != 0)) return;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const int lid = slot_id[j];
  if ((unsigned)lid < (unsigned)max_local) gid[j] = l2g[lid];
  else if (state[j] == LORB_SLOT_EMPTY) gid[j] = -1;
}

bool frame_ok(const lorb_frame_out* f, const lorb_frame_slots* s) { return f->counts && s->state && s->pos && s->desc; }

}  // namespace

extern "C" {

int lorb_local_map_destroy(lorb_local_map* M) {
  if (!M) return LORB_E_INVALID;
  M->mem.release();
  delete M;
  return LORB_OK;
}

int lorb_local_map_create(lorb_ctx* ctx, int32_t max_local, int32_t max_kf, int32_t max_points, lorb_local_map** out) {
  if (!ctx) return LORB_E_INVALID;
  if (!out) return lorb::set_error(ctx, LORB_E_INVALID, "null output");
  *out = nullptr;
  if (max_local < 1 || max_kf < 1 || max_points < 1)
    return lorb::set_error(ctx, LORB_E_INVALID, "capacities %d / %d / %d must be positive", max_local, max_kf, max_points);
  lorb_local_map* M = new (std::nothrow) lorb_local_map;
  if (!M) return lorb::set_error(ctx, LORB_E_NOMEM, "out of host memory");
  struct Guard {
    lorb_local_map* m;
    ~Guard() { if (m) lorb_local_map_destroy(m); }
  } guard{M};
  M->ctx = ctx; M->max_local = max_local; M->max_kf = max_kf; M->max_points = max_points;
  const size_t nl = (size_t)max_local, np = (size_t)max_points;
  lorb::Arena& A = M->mem;
  A.add(&M->pos, nl * 3); A.add(&M->normal, nl * 3); A.add(&M->max_dist, nl); A.add(&M->min_dist, nl);
  A.add(&M->desc, nl * 32); A.add(&M->locked, nl); A.add(&M->is_bad, nl);
  A.add(&M->l2g, nl); A.add(&M->g2l, np); A.add(&M->kf_votes, (size_t)max_kf); A.add(&M->local_kf, (size_t)max_kf);
  A.add(&M->flag, (np + 15) & ~size_t(15)); A.add(&M->tile_cnt, (np + kTile - 1) / kTile); A.add(&M->ctl, (size_t)1);
  LORB_HIP(ctx, A.commit());
  LORB_HIP(ctx, hipMemsetAsync(A.base, 0, A.total, ctx->stream));
  LORB_HIP(ctx, hipMemsetAsync(M->is_bad, 1, nl, ctx->stream));
  LORB_HIP(ctx, hipStreamSynchronize(ctx->stream));
  guard.m = nullptr;
  *out = M;
  return LORB_OK;
}

int lorb_local_map_view(const lorb_local_map* M, lorb_local_map_arrays* v) {
  if (!M || !v) return LORB_E_INVALID;
  v->points = lorb_map_points_dev{M->max_local, M->pos, M->normal, M->max_dist, M->min_dist, M->desc, M->locked, M->is_bad,
                                  nullptr};
  v->l2g = M->l2g; v->g2l = M->g2l; v->kf_votes = M->kf_votes; v->local_kf = M->local_kf;
  v->max_local = M->max_local; v->max_kf = M->max_kf; v->max_points = M->max_points;
  return LORB_OK;
}

int lorb_local_map_update_dev(lorb_ctx* ctx, lorb_local_map* M, const lorb_map_store* S, const lorb_frame_out* d_cur,
                              int32_t n_max_cur, const lorb_frame_slots* d_cur_slots, int32_t* d_cur_slot_gid,
                              int32_t* d_cur_slot_id, const int32_t* d_src_status, const lorb_track_local_id_source* ids,
                              lorb_local_map_result* d_result) {
  if (!ctx || !M || !S || !d_cur || !d_cur_slots || !d_cur_slot_gid || !d_cur_slot_id || !d_result) return LORB_E_INVALID;
  if (M->ctx != ctx) return lorb::set_error(ctx, LORB_E_INVALID, "the local map belongs to another context");
  const int nk = n_max_cur, np = S->points.n, nkf = S->n_kf;
  if (nk < 1) return lorb::set_error(ctx, LORB_E_INVALID, "bound %d must be positive", nk);
  if (np < 0 || nkf < 0 || S->n_obs < 0 || S->n_kf_slots < 0 || S->n_cov < 0)
    return lorb::set_error(ctx, LORB_E_INVALID, "negative sizes");
  if (np > M->max_points) return lorb::set_error(ctx, LORB_E_INVALID, "%d points exceed max_points %d", np, M->max_points);
  if (nkf > M->max_kf) return lorb::set_error(ctx, LORB_E_INVALID, "%d keyframes exceed max_kf %d", nkf, M->max_kf);
  // the local stage's candidate list is allocated from the bounds
  if ((int64_t)M->max_local * (int64_t)nk > (int64_t(8) << 20))
    return lorb::set_error(ctx, LORB_E_INVALID, "max_local %d x bound %d exceed the asynchronous limit of 8M candidates",
                           M->max_local, nk);
  const lorb_map_points_dev& P = S->points;
  if (P.in_frame) return lorb::set_error(ctx, LORB_E_INVALID, "points.in_frame must be NULL");
  if (!frame_ok(d_cur, d_cur_slots) ||
      (ids && (!ids->d_motion_assign || !ids->d_motion_result || !ids->d_last_slot_id || ids->n_max_last < 1)) ||
      (np > 0 && (!P.pos || !P.normal || !P.max_dist || !P.min_dist || !P.desc || !P.locked || !S->obs_off)) ||
      (S->n_obs > 0 && !S->obs_kf) || (nkf > 0 && (!S->kf_bad || !S->kf_slot_off || !S->cov_off)) ||
      (S->n_kf_slots > 0 && !S->kf_slot_point) || (S->n_cov > 0 && !S->cov_kf))
    return lorb::set_error(ctx, LORB_E_INVALID, "null array");
  if (reinterpret_cast<uintptr_t>(P.desc) & 15)
    return lorb::set_error(ctx, LORB_E_INVALID, "points.desc is not 16-byte aligned");
  VoteArgs v{};
  v.count = d_cur->counts; v.n_max = nk; v.src_status = d_src_status; v.state = d_cur_slots->state; v.gid = d_cur_slot_gid;
  v.n_points = np; v.n_kf = nkf; v.n_obs = S->n_obs; v.n_cov = S->n_cov; v.pt_bad = P.is_bad;
  v.obs_off = S->obs_off; v.obs_kf = S->obs_kf; v.kf_bad = S->kf_bad; v.cov_off = S->cov_off; v.cov_kf = S->cov_kf;
  v.votes = M->kf_votes; v.local_kf = M->local_kf; v.flag = M->flag; v.ctl = M->ctl; v.rec = d_result;
  if (ids) {
    v.motion_assign = ids->d_motion_assign; v.motion_rec = ids->d_motion_result; v.last_gid = ids->d_last_slot_id;
    v.n_max_last = ids->n_max_last; v.given = ids->cur_slots_given != 0;
  }
  hipStream_t st = ctx->stream;
  hipLaunchKernelGGL(k_lm_vote, dim3(1), dim3(1024), 0, st, v);
  LORB_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(k_lm_mark, dim3(std::min(std::max(nkf, 1), 128)), dim3(256), 0, st, M->ctl, M->local_kf, S->kf_slot_off,
                     S->kf_slot_point, S->n_kf_slots, np, P.is_bad, M->flag);
  LORB_CHECK_LAUNCH(ctx);
  const int n_tiles = (int)lorb::ceil_div((size_t)np, kTile);
  if (n_tiles > 0) {
    hipLaunchKernelGGL(k_lm_count, dim3(n_tiles), dim3(kTile), 0, st, M->ctl, M->flag, np, M->tile_cnt);
    LORB_CHECK_LAUNCH(ctx);
  }
  CompactArgs c{};
  c.ctl = M->ctl; c.flag = M->flag; c.tile_cnt = M->tile_cnt;
  c.n_points = np; c.n_tiles = n_tiles; c.max_local = M->max_local; c.src = P;
  c.pos = M->pos; c.normal = M->normal; c.max_dist = M->max_dist; c.min_dist = M->min_dist;
  c.desc = M->desc; c.locked = M->locked; c.is_bad = M->is_bad; c.l2g = M->l2g; c.g2l = M->g2l; c.rec = d_result;
  hipLaunchKernelGGL(k_lm_compact, dim3(std::max(n_tiles, (int)lorb::ceil_div((size_t)M->max_local, kTile))), dim3(kTile), 0,
                     st, c);
  LORB_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(k_lm_ids, dim3(lorb::ceil_div((size_t)nk, 256)), dim3(256), 0, st, M->ctl, d_cur->counts,
                     d_cur_slots->state, d_cur_slot_gid, M->g2l, np, d_cur_slot_id);
  LORB_CHECK_LAUNCH(ctx);
  return LORB_OK;
}

int lorb_local_map_ids_back_dev(lorb_ctx* ctx, const lorb_local_map* M, const lorb_frame_out* d_cur, int32_t n_max_cur,
                                const lorb_frame_slots* d_cur_slots, const int32_t* d_cur_slot_id,
                                const int32_t* d_local_status, int32_t* d_cur_slot_gid) {
  if (!ctx || !M || !d_cur || !d_cur_slots || !d_cur_slot_id || !d_cur_slot_gid) return LORB_E_INVALID;
  if (M->ctx != ctx) return lorb::set_error(ctx, LORB_E_INVALID, "the local map belongs to another context");
  if (n_max_cur < 1) return lorb::set_error(ctx, LORB_E_INVALID, "bound %d must be positive", n_max_cur);
  if (!d_cur->counts || !d_cur_slots->state) return lorb::set_error(ctx, LORB_E_INVALID, "null array");
  hipLaunchKernelGGL(k_lm_ids_back, dim3(lorb::ceil_div((size_t)n_max_cur, 256)), dim3(256), 0, ctx->stream, d_cur->counts,
                     n_max_cur, d_local_status, d_cur_slots->state, d_cur_slot_id, M->l2g, M->max_local, d_cur_slot_gid);
  LORB_CHECK_LAUNCH(ctx);
  return LORB_OK;
}

}  // extern "C"
