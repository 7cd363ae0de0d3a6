// lorb_window.hip -- windowed (projection) ORB matching on gfx950 + its frame-side callees.
//
// (a4) Matcher::SearchByProjection(Frame*, Frame*, th)          src/matcher.cpp:64-218
// (a5) Matcher::SearchByProjection(Frame*, set<MapPoint*>, th)  src/matcher.cpp:220-316
// (a7) Frame::AssignFeaturesToGrid / GetFeaturesInArea          src/frame.cpp:87-115, 370-423
// (a8) Frame::IsInFrustum + MapPoint::PredictScale              src/frame.cpp:425-494, map_point.cpp:267-284
// (a20) Frame::UnprojectStereo                                  src/frame.cpp:335-356
//
// The reference resolves map points sequentially: a keypoint slot already holding a map point
// with mnObs>0 is skipped by every LATER point (src/matcher.cpp:149-151, 273-275).  That order
// dependence is reproduced exactly and in parallel by a Jacobi fixpoint:
//   round r: every point picks best/second over its candidate list, skipping slots that were
//            locked before the call or claimed (accepted + mnObs>0) by an EARLIER point in
//            round r-1's results;  claims = min point index per slot.
// Point 0 is exact in round 1, point j depends only on points < j, so after round k points
// 0..k-1 are final; a round with no change is the unique sequential answer.  Rounds are bounded
// by n+1 and in practice end after a handful.  All float expressions follow the reference's
// operation order (built with -ffp-contract=off) so candidate sets are bit-identical.
#include "lorb_internal.h"

#include <cmath>

namespace {

constexpr int kCells = LORB_GRID_COLS * LORB_GRID_ROWS;
constexpr uint32_t kNoClaim = 0x7fffffff;

struct WinParams {  // per-call scalars (device copy of lorb_frame_params)
  lorb_frame_params fp;
  float th;
  int mode_forward, mode_backward;  // a4 only
  float Rcw[9], tcw[3];             // a4 only
  int oct_limit;                    // a4 only: a last-frame point with an octave outside [0, oct_limit) is inactive
};

__device__ __forceinline__ int hamming(const uint4* a, const uint4* b) {
  const uint4 a0 = a[0], a1 = a[1], b0 = b[0], b1 = b[1];
  return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
         __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// Frame::PosInGrid: the cell of a keypoint, or -1 outside the grid
__device__ __forceinline__ int pos_in_grid(float x, float y, const lorb_frame_params& fp) {
  const int px = (int)roundf((x - fp.min_x) * fp.grid_w_inv);
  const int py = (int)roundf((y - fp.min_y) * fp.grid_h_inv);
  if (px < 0 || px >= LORB_GRID_COLS || py < 0 || py >= LORB_GRID_ROWS) return -1;
  return px * LORB_GRID_ROWS + py;
}

// The grid of n <= kGridLds keypoints built by one NT-thread workgroup in its own LDS (off: kCells + 1,
// cur: kCells, idx: n), lists in keypoint order: the candidate kernels of the host-array calls build
// it per workgroup instead of reading a grid built by a launch of its own.
template <int NT>
__device__ __forceinline__ void grid_lds(const float* __restrict__ x, const float* __restrict__ y, int n,
                                         const lorb_frame_params& fp, int* off, int* cur, int* idx) {
  constexpr int CPT = kCells / NT;  // consecutive cells per thread in the scan
  static_assert(kCells % NT == 0, "cells per thread");
  __shared__ int wsum[NT / 64];
  const int t = threadIdx.x;
  for (int c = t; c < kCells; c += NT) off[c] = 0;
  __syncthreads();
  for (int i = t; i < n; i += NT) {
    const int c = pos_in_grid(x[i], y[i], fp);
    if (c >= 0) atomicAdd(&off[c], 1);
  }
  __syncthreads();
  int v[CPT], sum = 0;
#pragma unroll
  for (int k = 0; k < CPT; ++k) { v[k] = off[CPT * t + k]; sum += v[k]; }
  int tot;
  int run = lorb::block_excl_scan<NT>(sum, wsum, &tot);
#pragma unroll
  for (int k = 0; k < CPT; ++k) { off[CPT * t + k] = run; cur[CPT * t + k] = run; run += v[k]; }
  if (t == NT - 1) off[kCells] = tot;
  __syncthreads();
  for (int i = t; i < n; i += NT) {
    const int c = pos_in_grid(x[i], y[i], fp);
    if (c >= 0) idx[atomicAdd(&cur[c], 1)] = i;
  }
  __syncthreads();
  for (int c = t; c < kCells; c += NT) {  // insertion (keypoint) order inside every cell
    const int a = off[c], b = off[c + 1];
    for (int i = a + 1; i < b; ++i) {
      const int w = idx[i];
      int j = i;
      while (j > a) {
        const int u = idx[j - 1];
        if (u <= w) break;
        idx[j] = u;
        --j;
      }
      idx[j] = w;
    }
  }
  __syncthreads();
}

// (a7) grid: one workgroup; cell = PosInGrid; per-cell lists in keypoint (insertion) order.  The
// offsets and (up to kGridLds keypoints) the lists are built in LDS and stored once, coalesced.
constexpr int kGridLds = 6144;
// scatter keypoints into their cells' lists (atomics: any order), then restore insertion (index)
// order inside every cell (cells hold a handful of entries); indices only, never a pointer below a
// cell's first entry
__device__ __forceinline__ void grid_place(int* idx, const int* off, int* cur, const int* __restrict__ kp_cell,
                                           int n, int t) {
  for (int i = t; i < n; i += 1024) {
    const int c = kp_cell[i];
    if (c >= 0) idx[atomicAdd(&cur[c], 1)] = i;
  }
  __syncthreads();
  for (int c = t; c < kCells; c += 1024) {
    const int a = off[c], b = off[c + 1];
    for (int i = a + 1; i < b; ++i) {
      const int v = idx[i];
      int j = i;
      while (j > a) {
        const int u = idx[j - 1];
        if (u <= v) break;
        idx[j] = u;
        --j;
      }
      idx[j] = v;
    }
  }
}
// kDevCount (the frames chain): n is the current frame's count in device memory, dc.max_cur bounds
// it and sizes cell_idx / kp_cell
template <bool kDevCount = false>
__global__ __launch_bounds__(1024) void k_grid_build(const float* __restrict__ x, const float* __restrict__ y,
                                                     int n, lorb_frame_params fp,
                                                     int* __restrict__ cell_off,  // kCells+1
                                                     int* __restrict__ cell_idx, int* __restrict__ kp_cell,
                                                     lorb::FrameCounts dc = {}) {
  if (kDevCount) {
    int nl;
    if (!lorb::frame_counts(dc, &nl, &n)) return;
  }
  __shared__ int off[kCells + 1];  // counts, then offsets
  __shared__ int cur[kCells];
  __shared__ int s_idx[kGridLds];
  const bool lds = n <= kGridLds;
  const int t = threadIdx.x;
  for (int c = t; c < kCells; c += 1024) off[c] = 0;
  __syncthreads();
  for (int i = t; i < n; i += 1024) {
    const int c = pos_in_grid(x[i], y[i], fp);
    kp_cell[i] = c;
    if (c >= 0) atomicAdd(&off[c], 1);
  }
  __syncthreads();
  {  // 3072-entry exclusive scan: three consecutive cells per thread
    static_assert(kCells == 3 * 1024, "grid scan assumes 64 x 48 cells");
    __shared__ int wsum[16];
    const int c0 = 3 * t;
    const int a = off[c0], b = off[c0 + 1], c = off[c0 + 2];
    int tot;
    const int ex = lorb::block_excl_scan_1024(a + b + c, wsum, &tot);
    off[c0] = ex; off[c0 + 1] = ex + a; off[c0 + 2] = ex + a + b;
    cur[c0] = ex; cur[c0 + 1] = ex + a; cur[c0 + 2] = ex + a + b;
    if (t == 1023) off[kCells] = tot;
  }
  __syncthreads();
  // separate instantiations for the LDS and the global list: a pointer that may be either is a flat
  // pointer, and the sort's walk below a cell's first entry must not be formed on the LDS aperture
  if (lds) grid_place(s_idx, off, cur, kp_cell, n, t);
  else grid_place(cell_idx, off, cur, kp_cell, n, t);
  for (int c = t; c <= kCells; c += 1024) cell_off[c] = off[c];
  if (lds) {
    __syncthreads();
    const int tot = off[kCells];
    for (int i = t; i < tot; i += 1024) cell_idx[i] = s_idx[i];
  }
}

struct FeatArea {  // Frame::GetFeaturesInArea window
  int x0, x1, y0, y1;
  bool empty;
};
__device__ __forceinline__ FeatArea feat_area(const lorb_frame_params& fp, float x, float y, float r) {
  FeatArea a;
  a.empty = true;
  a.x0 = max(0, (int)floorf((x - fp.min_x - r) * fp.grid_w_inv));
  if (a.x0 >= LORB_GRID_COLS) return a;
  a.x1 = min(LORB_GRID_COLS - 1, (int)ceilf((x - fp.min_x + r) * fp.grid_w_inv));
  if (a.x1 < 0) return a;
  a.y0 = max(0, (int)floorf((y - fp.min_y - r) * fp.grid_h_inv));
  if (a.y0 >= LORB_GRID_ROWS) return a;
  a.y1 = min(LORB_GRID_ROWS - 1, (int)ceilf((y - fp.min_y + r) * fp.grid_h_inv));
  if (a.y1 < 0) return a;
  a.empty = false;
  return a;
}

struct KpDev {
  const float *x, *y, *angle, *uR;
  const int* octave;
  const uint4* desc;
  const uint8_t* slot_state;
  const int *cell_off, *cell_idx;
  int n;
};

// The candidate kernels of the host-array calls (k_cand_*<., true>, n <= kStageKps keypoints) build
// the frame's grid in their own LDS instead of reading one built by a launch of its own.  (Staging
// the keypoints' coordinates, octaves and descriptors into LDS as well measured slower: 11.5 ->
// 12.2 us per a4 launch.)
constexpr int kStageKps = 1024;
struct KpLds {
  int off[kCells + 1], cur[kCells], idx[kStageKps];
};
template <int NT>
__device__ __forceinline__ KpDev stage_grid(const KpDev& G, const lorb_frame_params& fp, KpLds& L) {
  grid_lds<NT>(G.x, G.y, G.n, fp, L.off, L.cur, L.idx);  // ends with a barrier
  KpDev K = G;
  K.cell_off = L.off;
  K.cell_idx = L.idx;
  return K;
}


// Walk GetFeaturesInArea in reference order (ix outer, iy inner, cell insertion order) and apply
// the level / window / stereo filters -- one WAVEFRONT per query.  The window's cells are taken 64
// at a time (lane = cell); a wave scan of their sizes flattens the cell lists into one entry
// sequence in reference order, the entries are taken 64 at a time (lane = entry, owner cell by a
// 6-step binary search over the scanned sizes), and survivors are compacted with a ballot, so
// candidate k of the query is the k-th survivor of the reference's loop.  WRITE=false counts,
// WRITE=true emits (keypoint, distance | octave << 16).  All arguments are wave-uniform; returns the count.
template <bool WRITE>
__device__ __forceinline__ int walk_candidates_wave(const KpDev& K, const lorb_frame_params& fp, float x,
                                                    float y, float r, int minLevel, int maxLevel,
                                                    float stereo_u, float stereo_r, const uint4* qdesc,
                                                    int2* out) {
  const FeatArea a = feat_area(fp, x, y, r);
  if (a.empty) return 0;
  const int lane = threadIdx.x & 63;
  const bool bCheckLevels = (minLevel > 0) || (maxLevel >= 0);
  const int ny = a.y1 - a.y0 + 1;
  const int ncell = (a.x1 - a.x0 + 1) * ny;
  const unsigned long long lt = (1ull << lane) - 1ull;
  int n = 0;
  for (int cb = 0; cb < ncell; cb += 64) {
    const int ci = cb + lane;
    int beg = 0, len = 0;
    if (ci < ncell) {
      const int c = (a.x0 + ci / ny) * LORB_GRID_ROWS + (a.y0 + ci % ny);
      beg = K.cell_off[c];
      len = K.cell_off[c + 1] - beg;
    }
    int incl = len;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(incl, o, 64);
      if (lane >= o) incl += u;
    }
    const int ex = incl - len;
    const int total = __shfl(incl, 63, 64);
    for (int eb = 0; eb < total; eb += 64) {
      const int e = eb + lane;
      int src = 0;  // last lane (cell) whose first entry is <= e: the owner (ex is non-decreasing)
#pragma unroll
      for (int st = 32; st >= 1; st >>= 1) {
        const int cand = src + st;
        const int exc = __shfl(ex, cand & 63, 64);
        if (cand < 64 && exc <= e) src = cand;
      }
      const int sbeg = __shfl(beg, src, 64), sex = __shfl(ex, src, 64);
      bool pass = false;
      int j = 0, oc = 0;
      if (e < total) {
        j = K.cell_idx[sbeg + (e - sex)];
        oc = K.octave[j];
        // slots locked before the call (mnObs > 0) are skipped by every point (src/matcher.cpp:
        // 149-151, 273-275): a pure filter, applied here once instead of in every resolver round
        pass = K.slot_state[j] != LORB_SLOT_LOCKED;
        pass = pass && !(bCheckLevels && (oc < minLevel || (maxLevel >= 0 && oc > maxLevel)));
        const float distx = K.x[j] - x;
        const float disty = K.y[j] - y;
        pass = pass && (fabsf(distx) < r && fabsf(disty) < r);
        if (pass && K.uR) {  // stereo consistency (checked after occupancy in the reference;
                             // both are pure filters so the order is immaterial)
          const float uRj = K.uR[j];
          if (uRj > 0) pass = !(fabsf(stereo_u - uRj) > stereo_r);
        }
      }
      const unsigned long long m = __ballot(pass);
      if (WRITE && pass) out[n + __popcll(m & lt)] = make_int2(j, hamming(qdesc, K.desc + 2 * (size_t)j) | (oc << 16));
      n += __popcll(m);
    }
  }
  return n;
}

constexpr int kCandWaves = 4;  // queries (wavefronts) per 256-thread workgroup

// (a5) candidates of each local map point, one wavefront per point
// (the body, shared with k_cand_local_dc)
template <bool WRITE, bool GRID>
__device__ __forceinline__ void cand_local_run(KpDev K, const WinParams& P, int np,
                                               const uint8_t* __restrict__ in_view,
                                               const uint8_t* __restrict__ is_bad,
                                               const float* __restrict__ px, const float* __restrict__ py,
                                               const float* __restrict__ pxr, const int* __restrict__ plev,
                                               const float* __restrict__ vcos, const uint4* __restrict__ pdesc,
                                               int* __restrict__ cand_cnt, const int* __restrict__ cand_off,
                                               int2* __restrict__ cand, int stride) {
  const int m = blockIdx.x * kCandWaves + (threadIdx.x >> 6);
  // the query's scalars requested first (GRID: they arrive while the keypoints are staged)
  const int mq = min(m, np - 1);
  const bool act = in_view[mq] && !(is_bad && is_bad[mq]);
  const int lev = plev[mq];
  const float vc = vcos[mq], qx = px[mq], qy = py[mq], qxr = pxr[mq];
  if constexpr (GRID) {
    __shared__ KpLds L;
    K = stage_grid<64 * kCandWaves>(K, P.fp, L);
  }
  if (m >= np) return;
  int cnt = 0;
  if (act) {
    float r = ((double)vc > 0.998) ? 2.5f : 4.0f;  // RadiusByViewingCos
    if (P.th != 1.0f) r *= P.th;
    const float rs = r * P.fp.scale_factors[lev];
    cnt = walk_candidates_wave<WRITE>(K, P.fp, qx, qy, rs, lev - 1, lev, qxr, rs, pdesc + 2 * (size_t)m,
                                      WRITE ? cand + (stride > 0 ? (size_t)m * stride : (size_t)cand_off[m]) : nullptr);
  }
  if ((!WRITE || stride > 0) && (threadIdx.x & 63) == 0) cand_cnt[m] = cnt;
}
template <bool WRITE, bool GRID = false>
__global__ __launch_bounds__(64 * kCandWaves) void k_cand_local(KpDev K, WinParams P, int np,
                                                    const uint8_t* __restrict__ in_view,
                                                    const uint8_t* __restrict__ is_bad,
                                                    const float* __restrict__ px, const float* __restrict__ py,
                                                    const float* __restrict__ pxr, const int* __restrict__ plev,
                                                    const float* __restrict__ vcos, const uint4* __restrict__ pdesc,
                                                    int* __restrict__ cand_cnt, const int* __restrict__ cand_off,
                                                    int2* __restrict__ cand, int stride = 0) {
  cand_local_run<WRITE, GRID>(K, P, np, in_view, is_bad, px, py, pxr, plev, vcos, pdesc, cand_cnt, cand_off, cand, stride);
}
// the device-count form of k_cand_local<true, false> (the local-map frames chain's write pass):
// launched over the bound np = dc.max_last, the counts read first as k_cand_frame<., ., true> does
__global__ __launch_bounds__(64 * kCandWaves) void k_cand_local_dc(KpDev K, WinParams P, int np,
                                                    const uint8_t* __restrict__ in_view,
                                                    const uint8_t* __restrict__ is_bad,
                                                    const float* __restrict__ px, const float* __restrict__ py,
                                                    const float* __restrict__ pxr, const int* __restrict__ plev,
                                                    const float* __restrict__ vcos, const uint4* __restrict__ pdesc,
                                                    int* __restrict__ cand_cnt, const int* __restrict__ cand_off,
                                                    int2* __restrict__ cand, int stride, lorb::FrameCounts dc) {
  if (!lorb::frame_counts(dc, &np, &K.n)) return;
  if ((int)blockIdx.x * kCandWaves >= np) return;
  cand_local_run<true, false>(K, P, np, in_view, is_bad, px, py, pxr, plev, vcos, pdesc, cand_cnt, cand_off, cand, stride);
}

// (a4) projection of last-frame map points + candidates, one wavefront per point
__device__ __forceinline__ float gemv3(const float* R, float a, float b, float c, float t) {
  const double s = (double)R[0] * (double)a + (double)R[1] * (double)b + (double)R[2] * (double)c;
  return (float)(s + (double)t);
}
// WRITE: emit at cand_off[i] (two passes: count, scan, write); STRIDE > 0: one pass, emit at
// i * STRIDE and write the count (STRIDE bounds a query's candidates: the frame's keypoint count)
// the candidates of last-frame point i (one wavefront; returns the count, written at `out` if WRITE)
struct FrameQuery {  // a last-frame point's inputs
  bool act;          // has a map point and is not an outlier
  float X, Y, Z;
  int o;             // octave
};
__device__ __forceinline__ FrameQuery frame_query(int i, const uint8_t* __restrict__ has_mp,
                                                  const uint8_t* __restrict__ outlier, const float* __restrict__ pos,
                                                  const int* __restrict__ loct) {
  FrameQuery q;
  q.act = has_mp[i] && !(outlier && outlier[i]);
  q.X = pos[3 * i]; q.Y = pos[3 * i + 1]; q.Z = pos[3 * i + 2];
  q.o = loct[i];
  return q;
}
// (kDevPose: Rcw, tcw and the two modes are the MotionPose block's, not P's -- P stays the kernel
// argument it is either way: scale_factors is indexed by the octave)
template <bool WRITE, bool kDevPose = false>
__device__ __forceinline__ int cand_frame_one(const KpDev& K, const WinParams& P, const FrameQuery& q,
                                              const uint4* qdesc, int2* out, const lorb::MotionPose* mp = nullptr) {
  int cnt = 0;
  if (q.act) {
    const float X = q.X, Y = q.Y, Z = q.Z;
    const float* Rcw = kDevPose ? mp->Rcw : P.Rcw;
    const float* tcw = kDevPose ? mp->tcw : P.tcw;
    const float xc = gemv3(Rcw + 0, X, Y, Z, tcw[0]);
    const float yc = gemv3(Rcw + 3, X, Y, Z, tcw[1]);
    const float zc = gemv3(Rcw + 6, X, Y, Z, tcw[2]);
    const float invzc = (float)(1.0 / (double)zc);
    if (!(invzc < 0)) {
      const float u = P.fp.fx * xc * invzc + P.fp.cx;
      const float v = P.fp.fy * yc * invzc + P.fp.cy;
      if (!(u < P.fp.min_x || u > P.fp.max_x) && !(v < P.fp.min_y || v > P.fp.max_y)) {
        const int o = q.o;
        const float radius = P.th * P.fp.scale_factors[o];
        int mn, mx;
        if (kDevPose ? mp->mode_forward : P.mode_forward) { mn = o; mx = -1; }
        else if (kDevPose ? mp->mode_backward : P.mode_backward) { mn = 0; mx = o; }
        else { mn = o - 1; mx = o + 1; }
        const float ur = u - P.fp.bf * invzc;
        cnt = walk_candidates_wave<WRITE>(K, P.fp, u, v, radius, mn, mx, ur, radius, qdesc, out);
      }
    }
  }
  return cnt;
}
// kDevCount (the frames chain): launched over the bounds (nl = dc.max_last, K.n = dc.max_cur, which
// is also the stride); the counts are read first, a workgroup wholly past n_last leaves before it
// stages anything, a wave past it loads no query
// kDevPose (that chain's device-pose form): P's pose part -- Rcw, tcw, the two modes -- is read from the
// block the chain's first kernel left, and dc.last points at that block's n_last
template <bool WRITE, bool GRID = false, bool kDevCount = false, bool kDevPose = false>
__global__ __launch_bounds__(64 * kCandWaves) void k_cand_frame(KpDev K, WinParams P, int nl,
                                                    const uint8_t* __restrict__ has_mp,
                                                    const uint8_t* __restrict__ outlier,
                                                    const float* __restrict__ pos,
                                                    const int* __restrict__ loct,
                                                    const uint4* __restrict__ ldesc,
                                                    int* __restrict__ cand_cnt, const int* __restrict__ cand_off,
                                                    int2* __restrict__ cand, int stride = 0,
                                                    const int* __restrict__ skip_unless = nullptr, int skip_max = 0,
                                                    lorb::FrameCounts dc = {},
                                                    const lorb::MotionPose* __restrict__ mp = nullptr) {
  if (kDevCount) {
    if (!lorb::frame_counts(dc, &nl, &K.n)) return;
    if ((int)blockIdx.x * kCandWaves >= nl) return;
  }
  // a predicated pass (the motion chain's retry): runs only if *skip_unless <= skip_max
  if (skip_unless && *skip_unless > skip_max) return;
  const int i = blockIdx.x * kCandWaves + (threadIdx.x >> 6);
  // the query's inputs requested first (GRID: they arrive while the keypoints are staged)
  // (kDevCount: a workgroup that got here has blockIdx.x * kCandWaves < nl, so nl - 1 >= 0)
  FrameQuery q = frame_query(min(i, nl - 1), has_mp, outlier, pos, loct);
  q.act = q.act && (unsigned)q.o < (unsigned)P.oct_limit;
  if constexpr (GRID) {
    __shared__ KpLds L;
    K = stage_grid<64 * kCandWaves>(K, P.fp, L);
  }
  if (i >= nl) return;
  const int cnt = cand_frame_one<WRITE, kDevPose>(
      K, P, q, ldesc + 2 * (size_t)i,
      WRITE ? cand + (stride > 0 ? (size_t)i * stride : (size_t)cand_off[i]) : nullptr, mp);
  if ((!WRITE || stride > 0) && (threadIdx.x & 63) == 0) cand_cnt[i] = cnt;
}

// exclusive scan of candidate counts (one workgroup, chunked)
// kDevCount (the frames chain): n is the last frame's count in device memory (cnt holds nothing past it)
template <bool kDevCount = false>
__global__ __launch_bounds__(1024) void k_scan(const int* __restrict__ cnt, int n, int* __restrict__ off,
                                               lorb::FrameCounts dc = {}) {
  if (kDevCount) {
    int nk;
    if (!lorb::frame_counts(dc, &n, &nk)) return;
  }
  __shared__ int wsum[16];
  int carry = 0;
  for (int base = 0; base < n; base += 1024) {
    const int i = base + (int)threadIdx.x;
    const int v = i < n ? cnt[i] : 0;
    int tot;
    const int ex = lorb::block_excl_scan_1024(v, wsum, &tot);
    if (i < n) off[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) off[n] = carry;
}

// one-pass candidate lists of the host-array matchers (a4, a5): up to this many entries (n_queries *
// nk) the candidates go to a fixed stride per query
constexpr size_t kCandStrided = size_t(1) << 20;

// Candidate list of a windowed match: a query has at most nk candidates, so `bound` = n_queries *
// nk entries always suffice.  Up to kCandBound entries that bound is allocated and the call needs
// no host round trip; past it the exact total (d_total, written by k_scan) is read back.
int alloc_candidates(lorb_ctx* ctx, const int* d_total, size_t bound, int2** cand) {
  constexpr size_t kCandBound = size_t(8) << 20;
  size_t cap = bound;
  if (cap > kCandBound) {
    int total = 0;
    LORB_HIP(ctx, hipMemcpyAsync(&total, d_total, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    LORB_HIP(ctx, hipStreamSynchronize(ctx->stream));
    cap = (size_t)total;
  }
  return lorb::scratch_t(ctx, S_W9, std::max<size_t>(cap, 1), cand);
}

// Jacobi fixpoint resolver (one workgroup per call).  MODE 0 = a5 (best/second + ratio test),
// MODE 1 = a4 (best only + rotation histogram / ComputeThreeMaxima null-out).  out != null: assign
// and the count are also copied there (nk + 1 ints) at the end.
template <int MODE>
__device__ __forceinline__ void resolve_run(int np, int nk, const int* cand_off, const int2* __restrict__ cand,
                                            const uint8_t* __restrict__ pt_locked,
                                            const float* __restrict__ last_angle,
                                            const float* cur_angle,
                                            int* res,      // np: accepted slot or -1
                                            int* claim,    // nk
                                            int* assign,   // nk: the working assignment
                                            int* bins,     // np scratch (MODE 1)
                                            int* nulls,    // nk scratch (MODE 1)
                                            int* __restrict__ assign_g,  // nk: where the assignment goes (or null)
                                            int* __restrict__ nmatches, int stride, int* __restrict__ out) {
  __shared__ int s_changed;
  __shared__ int hist[LORB_HISTO_LENGTH];
  __shared__ int s_ind[3];
  __shared__ int s_acc, s_rej;
  const int t = threadIdx.x;
  // np <= 1024 (one query per thread): the first kRegCand candidates of the thread's query, its lock
  // flag and (MODE 1) its angle are loaded once, all together, into registers; every round then reads
  // them (and their claims, from LDS) without a global round trip.  Later candidates, if any, come
  // from global.
  constexpr int kRegCand = 8;
  const bool regc = np <= 1024;
  int2 rc[kRegCand];
  int rn = 0;
  bool lk_t = false;
  float la_t = 0.0f;
  if (regc && t < np) {
    lk_t = pt_locked[t];
    if (MODE == 1) la_t = last_angle[t];
    if (stride > 0) {
      // strided lists: the first slots are requested together with the count (one round trip)
      const int a = t * stride, kmax = min(kRegCand, stride);
#pragma unroll
      for (int k = 0; k < kRegCand; ++k) rc[k] = cand[a + min(k, kmax - 1)];
      rn = min(cand_off[t], kmax);
    } else {
      const int a = cand_off[t], b = cand_off[t + 1];
      rn = min(b - a, kRegCand);
      if (rn > 0) {
#pragma unroll
        for (int k = 0; k < kRegCand; ++k) rc[k] = cand[a + min(k, rn - 1)];
      }
    }
  }
  for (int c = t; c < nk; c += 1024) claim[c] = kNoClaim;
  for (int m = t; m < np; m += 1024) res[m] = -2;  // "never computed"
  if (t == 0) { s_acc = 0; s_rej = 0; }
  __syncthreads();
  for (int round = 0; round <= np; ++round) {
    if (t == 0) s_changed = 0;
    __syncthreads();
    for (int m = t; m < np; m += 1024) {
      // stride > 0: query m's candidates at [m stride, m stride + count), cand_off holds the counts
      const int a = stride > 0 ? m * stride : cand_off[m], b = stride > 0 ? a + cand_off[m] : cand_off[m + 1];
      int bestDist = 256, bestIdx = -1;
      int bestLevel = -1, bestDist2 = 256, bestLevel2 = -1;
      // candidates in list order (ties keep the first, as the reference's loop)
      auto consider = [&](const int2 cd) {  // (slot, distance | octave << 16); pre-call locked slots removed
        const int j = cd.x;
        if ((int)claim[j] < m) return;  // locked by an earlier point during this call
        const int dist = cd.y & 0xffff;
        if (MODE == 0) {
          const int oc = cd.y >> 16;
          if (dist < bestDist) {
            bestDist2 = bestDist; bestDist = dist;
            bestLevel2 = bestLevel; bestLevel = oc; bestIdx = j;
          } else if (dist < bestDist2) {
            bestLevel2 = oc; bestDist2 = dist;
          }
        } else {
          if (dist < bestDist) { bestDist = dist; bestIdx = j; }
        }
      };
      int e0 = a;
      if (regc) {
#pragma unroll
        for (int k = 0; k < kRegCand; ++k)
          if (k < rn) consider(rc[k]);
        e0 = a + rn;
      }
      for (int e = e0; e < b; ++e) consider(cand[e]);
      int r = -1;
      if (bestDist <= LORB_TH_HIGH) {
        r = bestIdx;
        if (MODE == 0 && bestLevel == bestLevel2 && (double)bestDist > 0.8 * (double)bestDist2) r = -1;
      }
      if (r != res[m]) { res[m] = r; s_changed = 1; }
    }
    __syncthreads();
    if (!s_changed) break;
    for (int c = t; c < nk; c += 1024) claim[c] = kNoClaim;
    __syncthreads();
    for (int m = t; m < np; m += 1024)
      if (res[m] >= 0 && (regc ? lk_t : pt_locked[m] != 0)) atomicMin(&claim[res[m]], m);
    __syncthreads();
  }
  // final slot assignment: last accepted writer per slot
  for (int c = t; c < nk; c += 1024) { assign[c] = LORB_ASSIGN_UNCHANGED; if (MODE == 1) nulls[c] = 0; }
  if (MODE == 1 && t < LORB_HISTO_LENGTH) hist[t] = 0;
  __syncthreads();
  for (int m = t; m < np; m += 1024) {
    const int r = res[m];
    if (r >= 0) {
      atomicMax(&assign[r], m);
      atomicAdd(&s_acc, 1);
      if (MODE == 1) {
        float rot = (regc ? la_t : last_angle[m]) - cur_angle[r];
        if (rot < 0.0) rot += 360.0f;
        const float factor = LORB_HISTO_LENGTH / 360.0f;
        int bin = (int)roundf(rot * factor);
        if (bin == LORB_HISTO_LENGTH) bin = 0;
        bins[m] = bin;
        atomicAdd(&hist[bin], 1);
      }
    }
  }
  __syncthreads();
  if (MODE == 1) {
    if (t < 64) {  // Matcher::ComputeThreeMaxima, src/matcher.cpp:387-428, on one wavefront
      // The reference's insertion loop (strict >, bins in order, counts starting at 0) keeps the
      // three largest non-zero counts, ties to the lower bin.  Lane = bin; three wave argmax rounds
      // over the key count * 64 + (63 - bin) (largest count, then lowest bin) give the same bins.
      static_assert(LORB_HISTO_LENGTH <= 64, "one bin per lane");
      const int cnt = t < LORB_HISTO_LENGTH ? hist[t] : 0;
      int key = cnt > 0 ? cnt * 64 + (63 - t) : -1;
      int ind[3], mx[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        int k = key;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) k = max(k, __shfl_xor(k, o, 64));
        ind[r] = k >= 0 ? 63 - (k & 63) : -1;
        mx[r] = k >= 0 ? k >> 6 : 0;
        if (k >= 0 && t == ind[r]) key = -1;  // taken
      }
      if ((float)mx[1] < 0.1f * (float)mx[0]) { ind[1] = -1; ind[2] = -1; }
      else if ((float)mx[2] < 0.1f * (float)mx[0]) { ind[2] = -1; }
      if (t == 0) { s_ind[0] = ind[0]; s_ind[1] = ind[1]; s_ind[2] = ind[2]; }
    }
    __syncthreads();
    for (int m = t; m < np; m += 1024) {
      const int r = res[m];
      if (r >= 0) {
        const int b = bins[m];
        if (b != s_ind[0] && b != s_ind[1] && b != s_ind[2]) { nulls[r] = 1; atomicAdd(&s_rej, 1); }
      }
    }
    __syncthreads();
    for (int c = t; c < nk; c += 1024)
      if (nulls[c]) assign[c] = LORB_ASSIGN_NULL;
  }
  __syncthreads();
  if (t == 0) *nmatches = s_acc - s_rej;
  for (int c = t; c < nk; c += 1024) {
    const int v = assign[c];
    if (assign_g && assign_g != assign) assign_g[c] = v;
    if (out) out[c] = v;  // the host-array calls: the mapped result block, plain stores
  }
  if (out && t == 0) out[nk] = s_acc - s_rej;
}
// LDS modes of k_resolve: 1 = claim and res (nk + np ints); 2 = also the working assignment, the
// MODE-1 bins / nulls and a copy of the current frame's keypoint angles (4 nk + 2 np words).
inline int resolve_lds_mode(int np, int nk, size_t* bytes) {
  const size_t b2 = sizeof(int) * (4 * (size_t)nk + 2 * (size_t)np), b1 = sizeof(int) * ((size_t)np + (size_t)nk);
  if (b2 <= 120 * 1024) { *bytes = b2; return 2; }
  if (b1 <= 120 * 1024) { *bytes = b1; return 1; }
  *bytes = 0;
  return 0;
}
// kDevCount (the frames chain): np and nk are the two counts in device memory; the bounds chose
// lds_mode, the stride and the sizes of the global working arrays, so whatever the counts are fits
template <int MODE, bool kDevCount = false>
__global__ __launch_bounds__(1024) void k_resolve(int np, int nk, const int* __restrict__ cand_off,
                                                  const int2* __restrict__ cand,
                                                  const uint8_t* __restrict__ pt_locked,
                                                  const float* __restrict__ last_angle,
                                                  const float* __restrict__ cur_angle,
                                                  int* __restrict__ res, int* __restrict__ claim,
                                                  int* __restrict__ assign, int* __restrict__ bins,
                                                  int* __restrict__ nulls, int* __restrict__ nmatches, int lds_mode,
                                                  int stride = 0, int* __restrict__ out = nullptr,
                                                  const int* __restrict__ skip_unless = nullptr, int skip_max = 0,
                                                  lorb::FrameCounts dc = {}) {
  if (kDevCount && !lorb::frame_counts(dc, &np, &nk)) return;
  if (skip_unless && *skip_unless > skip_max) return;  // a predicated pass, as k_cand_frame
  // the working set in LDS (dynamic shared memory) as far as it fits (resolve_lds_mode), else global
  extern __shared__ int s_dyn[];
  int* wassign = assign;
  const float* ca = cur_angle;
  if (lds_mode >= 1) { claim = s_dyn; res = s_dyn + nk; }
  if (lds_mode == 2) {
    wassign = res + np;
    nulls = wassign + nk;
    bins = nulls + nk;
    float* s_ca = reinterpret_cast<float*>(bins + np);
    if (MODE == 1)
      for (int c = threadIdx.x; c < nk; c += 1024) s_ca[c] = cur_angle[c];
    ca = s_ca;  // resolve_run's first barrier orders these stores before any read
  }
  resolve_run<MODE>(np, nk, cand_off, cand, pt_locked, last_angle, ca, res, claim, wassign, bins, nulls, assign,
                    nmatches, stride, out);
}

// (a8) Frame::IsInFrustum + PredictScale for map point m: false if the point is skipped or out of
// view, else its tracking fields.  One body for k_frustum (one thread per point) and the local-map
// chain's candidate kernel (one wavefront per point, every lane the same values): same expression in
// the same unit, so both store the same bits.
struct TrackFields {
  float x, y, xr, cos;
  int lev;
};
__device__ __forceinline__ bool frustum_point(const lorb_frame_params& fp, const float* __restrict__ T,
                                              const float* __restrict__ Ow, int m, const float* __restrict__ pos,
                                              const float* __restrict__ nrm, const float* __restrict__ maxd,
                                              const float* __restrict__ mind, float cos_limit,
                                              const uint8_t* __restrict__ skip_a, const uint8_t* __restrict__ skip_b,
                                              TrackFields* f) {
  // EstimatePoseLocal skips points already matched in the frame and bad points before calling
  // IsInFrustum (src/visual_odometry.cpp:181-184); they leave tracking with mbTrackInView false
  if ((skip_a && skip_a[m]) || (skip_b && skip_b[m])) return false;
  const float P0 = pos[3 * m], P1 = pos[3 * m + 1], P2 = pos[3 * m + 2];
  float Pc[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double s = (double)T[4 * r] * P0 + (double)T[4 * r + 1] * P1 + (double)T[4 * r + 2] * P2 + (double)T[4 * r + 3] * 1.0f;
    Pc[r] = (float)s;
  }
  if (Pc[2] < 0.0f) return false;
  const float invz = 1.0f / Pc[2];
  const float u = fp.fx * Pc[0] * invz + fp.cx;
  const float v = fp.fy * Pc[1] * invz + fp.cy;
  if (u < fp.min_x || u > fp.max_x) return false;
  if (v < fp.min_y || v > fp.max_y) return false;
  const float maxDistance = 1.2f * maxd[m];
  const float minDistance = 0.8f * mind[m];
  const float PO0 = P0 - Ow[0], PO1 = P1 - Ow[1], PO2 = P2 - Ow[2];
  const float dist = (float)sqrt((double)PO0 * PO0 + (double)PO1 * PO1 + (double)PO2 * PO2);
  if (dist < minDistance || dist > maxDistance) return false;
  const float dot = PO0 * nrm[3 * m] + PO1 * nrm[3 * m + 1] + PO2 * nrm[3 * m + 2];
  const float viewCos = dot / dist;
  if (viewCos < cos_limit) return false;
  const float ratio = maxd[m] / dist;
  int nScale = (int)ceilf((float)log((double)ratio) / fp.log_scale_factor);
  if (nScale < 0) nScale = 0;
  else if (nScale >= fp.n_levels) nScale = fp.n_levels - 1;
  f->x = u;
  f->xr = u - fp.bf * invz;
  f->y = v;
  f->lev = nScale;
  f->cos = viewCos;
  return true;
}
__global__ __launch_bounds__(256) void k_frustum(lorb_frame_params fp, const float* __restrict__ T,
                                                 const float* __restrict__ Ow, int n,
                                                 const float* __restrict__ pos, const float* __restrict__ nrm,
                                                 const float* __restrict__ maxd, const float* __restrict__ mind,
                                                 float cos_limit, uint8_t* __restrict__ in_view,
                                                 float* __restrict__ ox, float* __restrict__ oy,
                                                 float* __restrict__ oxr, int* __restrict__ olev,
                                                 float* __restrict__ ocos,
                                                 const uint8_t* __restrict__ skip_a,
                                                 const uint8_t* __restrict__ skip_b) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= n) return;
  TrackFields f;
  const bool iv = frustum_point(fp, T, Ow, m, pos, nrm, maxd, mind, cos_limit, skip_a, skip_b, &f);
  in_view[m] = iv;
  if (!iv) return;
  ox[m] = f.x;
  oxr[m] = f.xr;
  oy[m] = f.y;
  olev[m] = f.lev;
  ocos[m] = f.cos;
}

// The local-map chain's candidate kernel (lorb_track_local*): k_cand_local with a8 fused in.  One
// wavefront per map point evaluates frustum_point for it, lane 0 stores the tracking fields (and a
// second copy into the host form's mapped result block, `mir`), and the candidates are walked
// straight from those registers.  WRITE: one strided pass (candidates at m * stride, counts in
// cand_cnt); !WRITE: the count pass of the count / scan / write sequence, whose write pass is
// k_cand_local<true> reading the fields stored here.
struct FrustumIn {  // a8's inputs; the pose and the camera centre travel as kernel arguments (the
                    // device-pose form reads them from a lorb::LocalPose block and leaves T / Ow unused)
  float T[16], Ow[3];
  const float *pos, *nrm, *maxd, *mind;
  const uint8_t *skip_a, *skip_b;
  float cos_limit;
};
struct FieldsOut {
  uint8_t* in_view;  // np
  float* track;      // 4 planes of np: x, y, xr, cos
  int* level;        // np
};
// (the body, shared with k_cand_local_fr_dc; T, Ow: the pose and the camera centre, wherever they live)
template <bool WRITE, bool GRID>
__device__ __forceinline__ void cand_local_fr_run(KpDev K, const WinParams& P, int np, const FrustumIn& F,
                                                  const float* __restrict__ T, const float* __restrict__ Ow,
                                                  const FieldsOut& o, const FieldsOut& mir,
                                                  const uint4* __restrict__ pdesc, int* __restrict__ cand_cnt,
                                                  int2* __restrict__ cand, int stride) {
  const int m = blockIdx.x * kCandWaves + (threadIdx.x >> 6);
  // the query's fields first (GRID: its loads are in flight while the grid is staged)
  TrackFields f;
  const bool act = frustum_point(P.fp, T, Ow, min(m, np - 1), F.pos, F.nrm, F.maxd, F.mind, F.cos_limit, F.skip_a,
                                 F.skip_b, &f);
  if constexpr (GRID) {
    __shared__ KpLds L;
    K = stage_grid<64 * kCandWaves>(K, P.fp, L);
  }
  if (m >= np) return;
  const bool lane0 = (threadIdx.x & 63) == 0;
  if (lane0) {
    o.in_view[m] = act;
    if (mir.in_view) mir.in_view[m] = act;
    if (act) {
      o.track[m] = f.x; o.track[np + m] = f.y; o.track[2 * np + m] = f.xr; o.track[3 * np + m] = f.cos;
      o.level[m] = f.lev;
      if (mir.in_view) {
        mir.track[m] = f.x; mir.track[np + m] = f.y; mir.track[2 * np + m] = f.xr; mir.track[3 * np + m] = f.cos;
        mir.level[m] = f.lev;
      }
    }
  }
  int cnt = 0;
  if (act && K.n > 0) {  // a frame without keypoints has no grid to walk
    float r = ((double)f.cos > 0.998) ? 2.5f : 4.0f;  // RadiusByViewingCos
    if (P.th != 1.0f) r *= P.th;
    const float rs = r * P.fp.scale_factors[f.lev];
    cnt = walk_candidates_wave<WRITE>(K, P.fp, f.x, f.y, rs, f.lev - 1, f.lev, f.xr, rs, pdesc + 2 * (size_t)m,
                                      WRITE ? cand + (size_t)m * stride : nullptr);
  }
  if (lane0) cand_cnt[m] = cnt;
}
template <bool WRITE, bool GRID = false>
__global__ __launch_bounds__(64 * kCandWaves) void k_cand_local_fr(KpDev K, WinParams P, int np, FrustumIn F,
                                                                   FieldsOut o, FieldsOut mir,
                                                                   const uint4* __restrict__ pdesc,
                                                                   int* __restrict__ cand_cnt, int2* __restrict__ cand,
                                                                   int stride) {
  cand_local_fr_run<WRITE, GRID>(K, P, np, F, F.T, F.Ow, o, mir, pdesc, cand_cnt, cand, stride);
}
// The device-count, device-pose form (lorb_track_local_frames_dev): launched over the bound np =
// dc.max_last with K.n = dc.max_cur (also the stride); the counts are read first, a workgroup wholly
// past np leaves before it stages anything; the pose and the camera centre come from the block
// k_local_head left (F.T / F.Ow are unused).
template <bool WRITE, bool GRID = false>
__global__ __launch_bounds__(64 * kCandWaves) void k_cand_local_fr_dc(KpDev K, WinParams P, int np, FrustumIn F,
                                                                      FieldsOut o, const uint4* __restrict__ pdesc,
                                                                      int* __restrict__ cand_cnt,
                                                                      int2* __restrict__ cand, int stride,
                                                                      const lorb::LocalPose* __restrict__ pose,
                                                                      lorb::FrameCounts dc) {
  if (!lorb::frame_counts(dc, &np, &K.n)) return;
  if ((int)blockIdx.x * kCandWaves >= np) return;
  cand_local_fr_run<WRITE, GRID>(K, P, np, F, pose->T, pose->Ow, o, FieldsOut{nullptr, nullptr, nullptr}, pdesc, cand_cnt,
                                 cand, stride);
}

// one thread per keypoint; Twc = mTcw.inv() given
__global__ __launch_bounds__(256) void k_unproject(lorb_frame_params fp, lorb::Mat4f Twc, int n,
                                                   const float* __restrict__ x, const float* __restrict__ y,
                                                   const float* __restrict__ depth, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  lorb::unproject_kp(fp, Twc, x[i], y[i], depth[i], out + 3 * i);
}

// The map-point slots of a built frame (lorb_frame_slots_fill_dev; the first launch of
// lorb_track_motion_frames_dev), one 1024-thread workgroup walking the frame's n_left keypoints:
// the count of created points is then a workgroup sum -- no atomic, no counter to clear -- and a
// frame has a few thousand keypoints at most.
//   MODE LORB_SLOTS_UPDATE_FRAME (src/visual_odometry.cpp:215-230): an EMPTY slot becomes FREE with
//     the unprojected keypoint and the frame's descriptor; others are left alone.
//   MODE LORB_SLOTS_INITIALIZE (:86-99): depth >= 0 -> LOCKED with the same; depth < 0 -> EMPTY.
// CHAIN (the frames chain): both counts are checked and the record's status, counts and n_created
// written here, the chain's first kernel; `locked` receives state == LOCKED (a4's mp_locked).
// POSE (that chain's device-pose form, lorb_track_motion_frames_pose_dev): the status also covers the
// two blocks' status words; thread 0 -- beside the slot walk, as in k_local_head -- runs the
// motion-model prediction (src/visual_odometry.cpp:119, then Frame::SetPose(Tcw)) into the current
// frame's block when a model is given, and leaves a4's motion direction and the LM's start in the
// MotionPose block for the kernels behind it; the fill's Twc is the last frame's block's.
struct PoseChain {
  lorb_frame_pose* cur;
  const lorb_frame_pose* last;
  const lorb_motion_model* model;  // or null: *cur as given
  lorb::MotionPose* blk;
};
// (one thread) the prediction where a model is given, then what the chain reads of the two poses
__device__ __forceinline__ void motion_predict(const PoseChain& pc, float baseline) {
  float Tcw[16], pose[6];
  if (pc.model) {
    float Twc[16];
    lorb::gemm4_f32(pc.last->Tcw, pc.model->Tcc, Tcw);  // pF->GetPose() * mTcc
    lorb::inv4_lu32f(Tcw, Twc);
    lorb::Tcw_to_rvec(Tcw, pose);
    pose[3] = Tcw[3]; pose[4] = Tcw[7]; pose[5] = Tcw[11];
#pragma unroll
    for (int k = 0; k < 16; ++k) { pc.cur->Tcw[k] = Tcw[k]; pc.cur->Twc[k] = Twc[k]; }
#pragma unroll
    for (int k = 0; k < 6; ++k) pc.cur->pose[k] = pose[k];
    pc.cur->status = 0;
  } else {
#pragma unroll
    for (int k = 0; k < 16; ++k) Tcw[k] = pc.cur->Tcw[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) pose[k] = pc.cur->pose[k];
  }
  float Rcw[9], tcw[3];
  int fwd, bwd;
  lorb::a4_motion_direction(Tcw, pc.last->Tcw, baseline, Rcw, tcw, &fwd, &bwd);
#pragma unroll
  for (int k = 0; k < 9; ++k) pc.blk->Rcw[k] = Rcw[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) pc.blk->tcw[k] = tcw[k];
#pragma unroll
  for (int k = 0; k < 6; ++k) pc.blk->pose_init[k] = pose[k];
  pc.blk->mode_forward = fwd;
  pc.blk->mode_backward = bwd;
}
struct SlotFill {
  lorb_frame_params fp;
  lorb::Mat4f Twc;
  const int* count;  // the frame's counts (entry 0); !CHAIN only
  int n_max;
  const float *x, *y, *depth;
  const uint4* desc;
  uint8_t* state;
  float* pos;
  uint4* sdesc;
  uint8_t* locked;  // or null
  int* n_created;   // or null
};
// REFER (the second motion attempt, lorb_track_motion_refer_pose_dev: src/visual_odometry.cpp:50-54): the
// POSE form on the refer frame behind a head that decides, from the first attempt's record in device
// memory, whether the attempt runs at all.  In this order: (a) a first attempt with status != 0 zeroes
// the refer record and ends the call; (b) the reference-frame word follows the previous frame's
// UpdateLocalMap (:311-312); (c) the current slots' ids by the first attempt's codes (motion_entry_id);
// (d) due = the first attempt's pass == 0, stale = due and the word is not the caller's refer frame.
// Not due, or stale, ends the call: n_last = -1 in the MotionPose block, on which every kernel behind
// this one returns, and nothing of the refer frame is examined.  Every thread reads the first attempt's
// record before the barrier; thread 0 overwrites its status only behind it.
struct ReferHead {
  const int* assign;  // the first attempt's final codes
  int first_given;    // cur_slots_given of the first attempt
  const int* last_gid;  // the gid group (cur_gid null: none)
  int n_max_last;
  int* cur_gid;
  int refer_kf;  // the guard pair (kf_word null: none)
  int* kf_word;
  const lorb_local_map_result* prev_update;
  lorb_track_refer_result* out;
};
template <int MODE, bool CHAIN, bool POSE = false, bool REFER = false>
__global__ __launch_bounds__(1024) void k_slots_fill(SlotFill a, lorb::FrameCounts dc,
                                                     lorb_track_frames_result* __restrict__ rec, PoseChain pc = {},
                                                     ReferHead rh = {}) {
  __shared__ int wsum[16];
  const int t = threadIdx.x;
  int n, n_cur = 0;
  lorb::Mat4f twc_blk;  // POSE only
  if constexpr (REFER) {
    static_assert(POSE, "the second attempt is a form of the device-pose chain");
    const bool first_ok = rec->status == 0;
    const int first_pass = rec->motion.pass, nm_first = rec->motion.nmatches_first, nm_retry = rec->motion.nmatches_retry;
    int kf = 0;
    if (rh.kf_word) {
      kf = *rh.kf_word;
      if (rh.prev_update->status == 0 && rh.prev_update->refer_kf >= 0) kf = rh.prev_update->refer_kf;
    }
    __syncthreads();
    if (!first_ok) {  // a
      if (t == 0) {
        *rh.out = lorb_track_refer_result{0, 0, 0, 0, 0};
        pc.blk->n_last = -1;
      }
      return;
    }
    if (t == 0 && rh.kf_word) *rh.kf_word = kf;  // b
    if (rh.cur_gid) {                            // c
      const int nc = min(dc.cur[0], dc.max_cur);
      const bool keep = rh.first_given && first_pass == 1;
      for (int j = t; j < nc; j += 1024)
        rh.cur_gid[j] = lorb::motion_entry_id(rh.cur_gid[j], rh.assign[j], keep, rh.last_gid, rh.n_max_last);
    }
    const bool due = first_pass == 0, stale = due && rh.kf_word && kf != rh.refer_kf;  // d
    if (t == 0) *rh.out = lorb_track_refer_result{due, due && !stale, stale, nm_first, nm_retry};
    if (!due || stale) {
      if (t == 0) pc.blk->n_last = -1;
      return;
    }
  }
  if constexpr (POSE) {
    static_assert(CHAIN, "the device-pose form is a form of the chain");
    const bool ok = lorb::frame_counts(dc, &n, &n_cur) && pc.last->status == 0 && !(pc.model && pc.model->status != 0);
    if (t == 0) {
      rec->status = ok ? 0 : 1;
      pc.blk->n_last = ok ? n : -1;
      if (!ok) pc.cur->status = 1;
    }
    if (!ok) return;
#pragma unroll
    for (int k = 0; k < 16; ++k) twc_blk.v[k] = pc.last->Twc[k];
    if (t == 0) motion_predict(pc, a.fp.b);
  } else if (CHAIN) {
    const bool ok = lorb::frame_counts(dc, &n, &n_cur);
    if (t == 0) rec->status = ok ? 0 : 1;
    if (!ok) return;
  } else {
    n = a.count[0];
    if (n < 0 || n > a.n_max) {
      if (t == 0 && a.n_created) *a.n_created = -1;
      return;
    }
  }
  int made = 0;
  for (int i = t; i < n; i += 1024) {
    uint8_t st;
    bool fill;
    if (MODE == LORB_SLOTS_UPDATE_FRAME) {
      st = a.state[i];
      fill = st == LORB_SLOT_EMPTY;
      if (fill) st = LORB_SLOT_FREE;
    } else {
      fill = a.depth[i] >= 0;
      st = fill ? LORB_SLOT_LOCKED : LORB_SLOT_EMPTY;
    }
    if (fill) {
      lorb::unproject_kp(a.fp, POSE ? twc_blk : a.Twc, a.x[i], a.y[i], a.depth[i], a.pos + 3 * (size_t)i);
      a.sdesc[2 * (size_t)i] = a.desc[2 * (size_t)i];
      a.sdesc[2 * (size_t)i + 1] = a.desc[2 * (size_t)i + 1];
      made++;
    }
    if (fill || MODE == LORB_SLOTS_INITIALIZE) a.state[i] = st;
    if (a.locked) a.locked[i] = st == LORB_SLOT_LOCKED;
  }
  int tot;
  lorb::block_excl_scan_1024(made, wsum, &tot);
  if (t == 0) {
    if (a.n_created) *a.n_created = tot;
    if (CHAIN) { rec->n_last = n; rec->n_cur = n_cur; rec->n_created = tot; }
  }
}

}  // namespace

namespace {
using lorb::inv4_lu32f;

// The first launch of lorb_track_local_frames_dev, one 1024-thread workgroup (as k_slots_fill):
//   a. the status: the count against its bound and the source's status; a failing one stores status 1
//      and, in the chain's own block, np = -1, on which every later kernel returns (frame_counts);
//   b. the pose hand-over, by thread 0 while the others walk the slots: the six doubles rounded to
//      float, Tcw_in, the camera centre, into the LocalPose block and the record;
//   c. the slots' ids (given, or derived from the motion stage's codes), then the held-slot loop of
//      src/visual_odometry.cpp:153-171: a slot holding a bad point is emptied, every other held point
//      of the table is flagged in the in_frame mask, which the kernel clears first.
struct LocalHead {
  const int* count;  // the frame's counts (entry 0)
  int n_max, np;
  const int* src_status;  // or null
  const double* pose;     // 6
  uint8_t* state;         // n_max: the frame's slot states
  int* slot_id;           // n_max
  const uint8_t* is_bad;  // np, or null
  uint8_t* in_frame;      // np: the mask (scratch)
  lorb::LocalPose* blk;
  lorb_track_local_frames_result* rec;
  // the id source (motion_assign null: none)
  const int* motion_assign;
  const lorb_track_frames_result* motion_rec;
  const int* last_slot_id;
  int n_max_last, given;
};
__global__ __launch_bounds__(1024) void k_local_head(LocalHead a) {
  __shared__ int wsum[16];
  const int t = threadIdx.x;
  const int n = a.count[0];
  const bool ok = n >= 0 && n <= a.n_max && !(a.src_status && *a.src_status != 0);
  if (t == 0) {
    a.rec->status = ok ? 0 : 1;
    a.blk->np = ok ? a.np : -1;
  }
  if (!ok) return;
  if (t == 0) {
    float p[6], T[16], Twc[16];
    for (int k = 0; k < 6; ++k) p[k] = (float)a.pose[k];  // src/bundle_adjust.cpp:198-201
    lorb::pose_to_Tcw(p, p + 3, T);
    inv4_lu32f(T, Twc);
    for (int k = 0; k < 6; ++k) { a.blk->pose_in[k] = p[k]; a.rec->pose_in[k] = p[k]; }
    for (int k = 0; k < 16; ++k) { a.blk->T[k] = T[k]; a.rec->Tcw_in[k] = T[k]; }
    a.blk->Ow[0] = Twc[3]; a.blk->Ow[1] = Twc[7]; a.blk->Ow[2] = Twc[11];
    a.rec->n_cur = n;
  }
  for (int m = t; m < a.np; m += 1024) a.in_frame[m] = 0;
  const bool keep = a.motion_assign && a.given && a.motion_rec->motion.pass == 1;
  __syncthreads();  // the mask is clear
  int held = 0;
  for (int j = t; j < n; j += 1024) {
    int id = a.slot_id[j];
    if (a.motion_assign) id = lorb::motion_entry_id(id, a.motion_assign[j], keep, a.last_slot_id, a.n_max_last);
    if ((unsigned)id >= (unsigned)a.np) id = -1;  // a point outside the table
    const uint8_t st = a.state[j];
    if (st != LORB_SLOT_EMPTY) {
      if (id >= 0 && a.is_bad && a.is_bad[id]) {
        a.state[j] = LORB_SLOT_EMPTY;
        id = -1;
      } else {
        held++;
        if (id >= 0) a.in_frame[id] = 1;
      }
    }
    a.slot_id[j] = id;
  }
  int n_held;
  lorb::block_excl_scan_1024(held, wsum, &n_held);  // its barriers: the mask is complete
  int inf = 0;
  for (int m = t; m < a.np; m += 1024) inf += a.in_frame[m];
  int n_inf;
  lorb::block_excl_scan_1024(inf, wsum, &n_inf);
  if (t == 0) { a.rec->n_held = n_held; a.rec->n_in_frame = n_inf; }
}

// VisualOdometry::Run :65-66 after the local stage, one thread: the frame's block from the local
// record (Frame::SetPose of the optimised pose) and mTcc = last.Twc * cur.Tcw
struct PoseFinish {
  const lorb_track_local_frames_result* rec;
  const lorb_frame_pose* last;
  lorb_frame_pose* cur;
  lorb_motion_model* model;
};
__global__ __launch_bounds__(64) void k_pose_finish(PoseFinish a) {
  if (threadIdx.x != 0) return;
  if (a.rec->status != 0) {
    a.cur->status = 1;
    return;
  }
  float Tcw[16], Twc[16], Tcc[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) Tcw[k] = a.rec->Tcw[k];
  inv4_lu32f(Tcw, Twc);
  lorb::gemm4_f32(a.last->Twc, Tcw, Tcc);
  const bool ok = a.rec->local.ok != 0;
#pragma unroll
  for (int k = 0; k < 6; ++k) a.cur->pose[k] = ok ? (float)a.rec->local.pose[k] : a.rec->pose_in[k];
#pragma unroll
  for (int k = 0; k < 16; ++k) { a.cur->Tcw[k] = Tcw[k]; a.cur->Twc[k] = Twc[k]; a.model->Tcc[k] = Tcc[k]; }
  a.cur->status = 0;
  a.model->status = 0;
}

// a frame's keypoints (Frame::mvKeysUn, mDescriptors, slot states) for the host-array entry points:
// packed into their InPack (one pull for every input), then the device grid built
struct KpParts {
  int x, y, ang, oc, desc, ur, ss;
  std::vector<uint8_t> zeros;
};
// pack_empty = false: a null slot_state packs nothing and K->slot_state comes out null (a chain that
// reads the context's own all-EMPTY buffer)
void kps_add(lorb::InPack& in, const lorb_keypoints* k, const uint8_t* slot_state, KpParts& p, bool pack_empty = true) {
  const size_t n = (size_t)k->n;
  p.x = in.add_t(k->x, n); p.y = in.add_t(k->y, n); p.ang = in.add_t(k->angle, n);
  p.oc = in.add_t(k->octave, n); p.desc = in.add_t(k->desc, n * 32); p.ur = in.add_t(k->u_right, n);
  if (!slot_state && pack_empty) { p.zeros.assign(n, 0); slot_state = p.zeros.data(); }
  p.ss = in.add_t(slot_state, n);
}
// the committed pack's keypoints, without a grid: the search builds one where it needs it (search_issue)
KpDev kps_finish(const lorb::InPack& in, const KpParts& p, int n) {
  KpDev K;
  K.x = in.dev<float>(p.x); K.y = in.dev<float>(p.y); K.angle = in.dev<float>(p.ang); K.uR = in.dev<float>(p.ur);
  K.octave = in.dev<int>(p.oc); K.desc = in.dev<const uint4>(p.desc); K.slot_state = in.dev<uint8_t>(p.ss);
  K.cell_off = nullptr; K.cell_idx = nullptr; K.n = n;
  return K;
}
// The keypoint grid of a frame (src/frame.cpp:87-115) for a *K that has none yet: the one place that
// launches k_grid_build.  A second search over the same *K reuses the grid.  dc (the frames chain):
// K->n is the bound, the count is read on the device.
int ensure_grid(lorb_ctx* ctx, KpDev* K, const lorb_frame_params& fp, const lorb::FrameCounts* dc = nullptr) {
  if (K->cell_off) return LORB_OK;
  const size_t n = (size_t)std::max(K->n, 1);
  int *cell_off, *cell_idx, *kp_cell;
  LORB_TRY(lorb::scratch_t(ctx, slot<S_KP, 7>(), kCells + 1, &cell_off));
  LORB_TRY(lorb::scratch_t(ctx, slot<S_KP, 8>(), n, &cell_idx));
  LORB_TRY(lorb::scratch_t(ctx, slot<S_KP, 9>(), n, &kp_cell));
  if (dc)
    hipLaunchKernelGGL(k_grid_build<true>, dim3(1), dim3(1024), 0, ctx->stream, K->x, K->y, K->n, fp, cell_off, cell_idx,
                       kp_cell, *dc);
  else
    hipLaunchKernelGGL(k_grid_build<false>, dim3(1), dim3(1024), 0, ctx->stream, K->x, K->y, K->n, fp, cell_off, cell_idx,
                       kp_cell);
  LORB_CHECK_LAUNCH(ctx);
  K->cell_off = cell_off; K->cell_idx = cell_idx;
  return LORB_OK;
}

// a4's per-call scalars.  src/matcher.cpp:74-87: motion direction from the two poses (cv::gemm:
// double accumulation)
WinParams frame_params_a4(const lorb_frame_params* cur, const float* cur_Tcw, const float* last_Tcw, float th,
                          int oct_limit) {
  WinParams P{};
  P.fp = *cur;
  P.th = th;
  P.oct_limit = std::min(std::max(oct_limit, 0), LORB_MAX_LEVELS);
  // (null poses: the chain's device-pose form, whose candidate kernel reads this part from its block)
  if (cur_Tcw) lorb::a4_motion_direction(cur_Tcw, last_Tcw, cur->b, P.Rcw, P.tcw, &P.mode_forward, &P.mode_backward);
  return P;
}

struct LastDev {  // lorb_last_frame's arrays on the device
  int n;
  const uint8_t *hm, *ol, *lk;
  const float *pos, *la;
  const int* lo;
  const uint4* ld;
};
LastDev last_dev(const lorb_last_frame* l) {
  return {l->n, l->has_mp, l->outlier, l->mp_locked, l->mp_pos, l->angle, l->octave,
          reinterpret_cast<const uint4*>(l->mp_desc)};
}
KpDev kp_dev(const lorb_keypoints* k, const uint8_t* slot_state) {
  KpDev K;
  K.x = k->x; K.y = k->y; K.angle = k->angle; K.uR = k->u_right; K.octave = k->octave;
  K.desc = reinterpret_cast<const uint4*>(k->desc); K.slot_state = slot_state;
  K.cell_off = nullptr; K.cell_idx = nullptr; K.n = k->n;
  return K;
}
// argument checks shared by the device-pointer a4 and the motion chain
int frame_dev_check(lorb_ctx* ctx, const lorb_frame_params* cur, const lorb_keypoints* k, const lorb_last_frame* l) {
  const int nk = k->n, nl = l->n;
  if (nk < 0 || nl < 0) return lorb::set_error(ctx, LORB_E_INVALID, "negative sizes");
  if (cur->n_levels < 1 || cur->n_levels > LORB_MAX_LEVELS)
    return lorb::set_error(ctx, LORB_E_INVALID, "n_levels %d out of range", cur->n_levels);
  if (!l->Tcw || (nk > 0 && (!k->x || !k->y || !k->octave || !k->angle || !k->desc)) ||
      (nl > 0 && (!l->has_mp || !l->mp_locked || !l->mp_pos || !l->mp_desc || !l->octave || !l->angle)))
    return lorb::set_error(ctx, LORB_E_INVALID, "null array");
  return LORB_OK;
}
// n all-EMPTY slot states: a buffer cleared when it is (re)allocated and never written afterwards
int empty_slots(lorb_ctx* ctx, int n, const uint8_t** out) {
  uint8_t* z;
  LORB_TRY(lorb::scratch_t(ctx, S_TM_ZERO, (size_t)std::max(n, 1), &z));
  if (ctx->zero_ss != z || ctx->zero_ss_sz != ctx->scratch_sz[S_TM_ZERO]) {  // a grown buffer may reuse the address
    LORB_HIP(ctx, hipMemsetAsync(z, 0, ctx->scratch_sz[S_TM_ZERO], ctx->stream));
    ctx->zero_ss = z;
    ctx->zero_ss_sz = ctx->scratch_sz[S_TM_ZERO];
  }
  *out = z;
  return LORB_OK;
}

// The launches of one projection search (MODE 1: a4, MODE 0: a5) on device-resident inputs, shared
// by every caller: the keypoint grid where the candidate kernel does not build its own (once per *K),
// the candidate lists of the nq queries (one strided pass up to kCandStrided entries, else count /
// scan / write), the resolver.  What differs per search is `launch`: called as launch(CandPass<WRITE,
// GRID>, workgroups, cnt, off, cand, stride), it launches that instantiation of its candidate kernel.
// The working buffers (S_WX, S_W9) are the same for every search.  dc (the frames chains): nq and
// K->n are the caller's bounds -- they size the grids, the stride, the LDS mode and every buffer --
// and each kernel reads the two counts from device memory (its kDevCount form); `launch` passes *dc
// on to its candidate kernel.  MODE 1: dc->last is the last frame's count.  MODE 0
// (lorb_track_local_frames_dev): the query count is a host value, so dc->last points at a device int
// that the call's first kernel stores it into (or -1: every kernel then returns).
template <bool WRITE, bool GRID>
struct CandPass {
  static constexpr bool write = WRITE, grid = GRID;
};
struct SearchOut {
  int *assign, *nmatches;  // the nk codes and the count
  int* out;                // or null: the mapped result block of a host-array call (nk + 1 ints)
  const int* skip_unless;  // or null: a predicated search, whose kernels return at once unless
  int skip_max;            // *skip_unless <= skip_max
};
template <int MODE, typename Launch>
int search_issue(lorb_ctx* ctx, KpDev* K, const lorb_frame_params& fp, int nq, const uint8_t* locked,
                 const float* last_angle, const SearchOut& o, Launch&& launch, const lorb::FrameCounts* dc = nullptr) {
  const int nk = K->n;
  // a query has at most nk candidates: up to kCandStrided entries one pass writes them at i * nk
  // (no count pass, no scan); past it the count / scan / write passes size the list exactly
  const bool strided = (size_t)nq * (size_t)nk <= kCandStrided;
  const bool lds_grid = strided && nk <= kStageKps;  // the candidate kernel builds the grid itself
  if (!lds_grid) LORB_TRY(ensure_grid(ctx, K, fp, dc));
  int *cnt, *off, *res, *claim, *bins = nullptr, *nulls = nullptr;
  LORB_TRY(lorb::scratch_t(ctx, slot<S_WX, 0>(), (size_t)nq + 1, &cnt));
  LORB_TRY(lorb::scratch_t(ctx, slot<S_WX, 1>(), (size_t)nq + 1, &off));
  LORB_TRY(lorb::scratch_t(ctx, slot<S_WX, 2>(), (size_t)nq + 1, &res));
  LORB_TRY(lorb::scratch_t(ctx, slot<S_WX, 3>(), (size_t)nk + 1, &claim));
  if constexpr (MODE == 1) {  // the rotation histogram
    LORB_TRY(lorb::scratch_t(ctx, slot<S_WX, 5>(), (size_t)nq + 1, &bins));
    LORB_TRY(lorb::scratch_t(ctx, slot<S_WX, 6>(), (size_t)nk + 1, &nulls));
  }
  const unsigned g = lorb::ceil_div(std::max(nq, 1), kCandWaves);
  int2* cand;
  if (strided) {
    LORB_TRY(lorb::scratch_t(ctx, S_W9, std::max<size_t>((size_t)nq * nk, 1), &cand));
    if (nq > 0) {
      lorb::KernelTimer kt(ctx, LORB_K_WINDOW_CAND);
      if (lds_grid) launch(CandPass<true, true>{}, g, cnt, (const int*)nullptr, cand, nk);
      else launch(CandPass<true, false>{}, g, cnt, (const int*)nullptr, cand, nk);
    }
  } else {
    if (nq > 0) {
      lorb::KernelTimer kt(ctx, LORB_K_WINDOW_CAND);
      launch(CandPass<false, false>{}, g, cnt, (const int*)nullptr, (int2*)nullptr, 0);
    }
    // a skipped pass leaves cnt as the pass before wrote it: the scan then sizes a list nobody fills
    if (dc) hipLaunchKernelGGL(k_scan<true>, dim3(1), dim3(1024), 0, ctx->stream, cnt, nq, off, *dc);
    else hipLaunchKernelGGL(k_scan<false>, dim3(1), dim3(1024), 0, ctx->stream, cnt, nq, off);
    LORB_TRY(alloc_candidates(ctx, off + nq, (size_t)nq * (size_t)nk, &cand));
    if (nq > 0) launch(CandPass<true, false>{}, g, cnt, (const int*)off, cand, 0);
  }
  size_t rlds = 0;
  const int rmode = resolve_lds_mode(nq, nk, &rlds);
  if (dc)
    hipLaunchKernelGGL((k_resolve<MODE, true>), dim3(1), dim3(1024), rlds, ctx->stream, nq, nk,
                       strided ? (const int*)cnt : (const int*)off, cand, locked, last_angle,
                       MODE == 1 ? K->angle : (const float*)nullptr, res, claim, o.assign, bins, nulls, o.nmatches, rmode,
                       strided ? nk : 0, o.out, o.skip_unless, o.skip_max, *dc);
  else
    hipLaunchKernelGGL((k_resolve<MODE, false>), dim3(1), dim3(1024), rlds, ctx->stream, nq, nk,
                       strided ? (const int*)cnt : (const int*)off, cand, locked, last_angle,
                       MODE == 1 ? K->angle : (const float*)nullptr, res, claim, o.assign, bins, nulls, o.nmatches, rmode,
                       strided ? nk : 0, o.out, o.skip_unless, o.skip_max);
  LORB_CHECK_LAUNCH(ctx);
  return LORB_OK;
}

// a4 on device-resident inputs, for the host-array call, the device-pointer call and the motion
// chain (whose second pass over the same *K is predicated on the first's count)
int a4_issue(lorb_ctx* ctx, KpDev* K, const WinParams& P, const LastDev& L, int* dassign, int* dnm, int* out,
             const int* skip_unless = nullptr, int skip_max = 0, const lorb::FrameCounts* dc = nullptr,
             const lorb::MotionPose* mp = nullptr) {  // mp (with dc): P's pose part lives in that block
  return search_issue<1>(
      ctx, K, P.fp, L.n, L.lk, L.la, {dassign, dnm, out, skip_unless, skip_max},
      [&](auto pass, unsigned g, int* cnt, const int* off, int2* cand, int stride) {
        using Pass = decltype(pass);
        if (dc && mp)
          hipLaunchKernelGGL((k_cand_frame<Pass::write, Pass::grid, true, true>), dim3(g), dim3(256), 0, ctx->stream, *K, P,
                             L.n, L.hm, L.ol, L.pos, L.lo, L.ld, cnt, off, cand, stride, skip_unless, skip_max, *dc, mp);
        else if (dc)
          hipLaunchKernelGGL((k_cand_frame<Pass::write, Pass::grid, true>), dim3(g), dim3(256), 0, ctx->stream, *K, P, L.n,
                             L.hm, L.ol, L.pos, L.lo, L.ld, cnt, off, cand, stride, skip_unless, skip_max, *dc);
        else
          hipLaunchKernelGGL((k_cand_frame<Pass::write, Pass::grid, false>), dim3(g), dim3(256), 0, ctx->stream, *K, P, L.n,
                             L.hm, L.ol, L.pos, L.lo, L.ld, cnt, off, cand, stride, skip_unless, skip_max);
      },
      dc);
}

struct LocalDev {  // a5's queries on the device: lorb_local_points' arrays, or a8's output
  int n;
  const uint8_t *iv, *bad, *lk;
  const float *px, *py, *pxr, *vc;
  const int* pl;
  const uint4* pd;
};
template <bool WRITE, bool GRID>
void launch_cand_local(lorb_ctx* ctx, unsigned g, const KpDev& K, const WinParams& P, const LocalDev& Q, int* cnt,
                       const int* off, int2* cand, int stride) {
  hipLaunchKernelGGL((k_cand_local<WRITE, GRID>), dim3(g), dim3(256), 0, ctx->stream, K, P, Q.n, Q.iv, Q.bad, Q.px, Q.py,
                     Q.pxr, Q.pl, Q.vc, Q.pd, cnt, off, cand, stride);
}
// a5 on device-resident inputs, for the host-array call and lorb_track_local_map_dev
int a5_issue(lorb_ctx* ctx, KpDev* K, const WinParams& P, const LocalDev& Q, int* dassign, int* dnm, int* out) {
  return search_issue<0>(ctx, K, P.fp, Q.n, Q.lk, nullptr, {dassign, dnm, out, nullptr, 0},
                         [&](auto pass, unsigned g, int* cnt, const int* off, int2* cand, int stride) {
                           using Pass = decltype(pass);
                           launch_cand_local<Pass::write, Pass::grid>(ctx, g, *K, P, Q, cnt, off, cand, stride);
                         });
}

}  // namespace

extern "C" {

int lorb_search_by_projection_local(lorb_ctx* ctx, const lorb_frame_params* frame, const lorb_keypoints* kps,
                                    const uint8_t* slot_state, const lorb_local_points* pts, float th,
                                    int32_t* assign, int32_t* nmatches) {
  if (!ctx || !frame || !kps || !pts || !assign || !nmatches) return LORB_E_INVALID;
  const int nk = kps->n, np = pts->n;
  if (nk < 0 || np < 0) return lorb::set_error(ctx, LORB_E_INVALID, "negative sizes");
  if (nk == 0) { *nmatches = 0; return LORB_OK; }
  for (int i = 0; i < np; ++i)
    if (pts->track_in_view[i] && !(pts->is_bad && pts->is_bad[i]) &&
        (pts->pred_level[i] < 0 || pts->pred_level[i] >= LORB_MAX_LEVELS))
      return lorb::set_error(ctx, LORB_E_INVALID, "point %d: predicted level %d out of range", i, pts->pred_level[i]);
  // every input in one pull, the result stored straight into pinned memory by k_resolve
  lorb::InPack in(ctx);
  KpParts kp;
  kps_add(in, kps, slot_state, kp);
  const int i_iv = in.add_t(pts->track_in_view, np), i_bad = in.add_t(pts->is_bad, np), i_lk = in.add_t(pts->locked, np),
            i_px = in.add_t(pts->proj_x, np), i_py = in.add_t(pts->proj_y, np), i_pxr = in.add_t(pts->proj_xr, np),
            i_pl = in.add_t(pts->pred_level, np), i_vc = in.add_t(pts->view_cos, np),
            i_pd = in.add_t(pts->desc, (size_t)np * 32);
  LORB_TRY(in.commit());
  KpDev K = kps_finish(in, kp, nk);
  const LocalDev Q = {np, in.dev<uint8_t>(i_iv), in.dev<uint8_t>(i_bad), in.dev<uint8_t>(i_lk), in.dev<float>(i_px),
                      in.dev<float>(i_py), in.dev<float>(i_pxr), in.dev<float>(i_vc), in.dev<int>(i_pl),
                      in.dev<const uint4>(i_pd)};
  WinParams P{};
  P.fp = *frame;
  P.th = th;
  int* dassign;
  LORB_TRY(lorb::scratch_t(ctx, slot<S_WX, 4>(), (size_t)nk + 1, &dassign));
  lorb::OutPack out(ctx);
  const int o_as = out.add(sizeof(int) * ((size_t)nk + 1));
  LORB_TRY(out.alloc(true));  // k_resolve writes assign + count into the mapped block
  LORB_TRY(a5_issue(ctx, &K, P, Q, dassign, dassign + nk, out.dev<int>(o_as)));
  LORB_TRY(out.fetch());
  memcpy(assign, out.host<int>(o_as), sizeof(int) * nk);
  *nmatches = out.host<int>(o_as)[nk];
  return LORB_OK;
}

int lorb_search_by_projection_frame(lorb_ctx* ctx, const lorb_frame_params* cur, const float cur_Tcw[16],
                                    const lorb_keypoints* cur_kps, const uint8_t* cur_slot_state,
                                    const lorb_last_frame* last, float th, int32_t* assign, int32_t* nmatches) {
  if (!ctx || !cur || !cur_Tcw || !cur_kps || !last || !assign || !nmatches) return LORB_E_INVALID;
  const int nk = cur_kps->n, nl = last->n;
  if (nk < 0 || nl < 0) return lorb::set_error(ctx, LORB_E_INVALID, "negative sizes");
  if (nk == 0) { *nmatches = 0; return LORB_OK; }
  for (int i = 0; i < nl; ++i)
    if (last->has_mp[i] && (last->octave[i] < 0 || last->octave[i] >= LORB_MAX_LEVELS))
      return lorb::set_error(ctx, LORB_E_INVALID, "last keypoint %d: octave %d out of range", i, last->octave[i]);
  const WinParams P = frame_params_a4(cur, cur_Tcw, last->Tcw, th, LORB_MAX_LEVELS);  // octaves checked above
  // every input in one pull, the result stored straight into pinned memory by k_resolve
  lorb::InPack in(ctx);
  KpParts kp;
  kps_add(in, cur_kps, cur_slot_state, kp);
  const int i_hm = in.add_t(last->has_mp, nl), i_ol = in.add_t(last->outlier, nl), i_lk = in.add_t(last->mp_locked, nl),
            i_pos = in.add_t(last->mp_pos, (size_t)nl * 3), i_ld = in.add_t(last->mp_desc, (size_t)nl * 32),
            i_lo = in.add_t(last->octave, nl), i_la = in.add_t(last->angle, nl);
  LORB_TRY(in.commit());
  KpDev K = kps_finish(in, kp, nk);
  const LastDev L = {nl, in.dev<uint8_t>(i_hm), in.dev<uint8_t>(i_ol), in.dev<uint8_t>(i_lk), in.dev<float>(i_pos),
                     in.dev<float>(i_la), in.dev<int>(i_lo), in.dev<const uint4>(i_ld)};
  int* dassign;
  LORB_TRY(lorb::scratch_t(ctx, slot<S_WX, 4>(), (size_t)nk + 1, &dassign));
  lorb::OutPack out(ctx);
  const int o_as = out.add(sizeof(int) * ((size_t)nk + 1));
  LORB_TRY(out.alloc(true));  // k_resolve writes assign + count into the mapped block
  LORB_TRY(a4_issue(ctx, &K, P, L, dassign, dassign + nk, out.dev<int>(o_as)));
  LORB_TRY(out.fetch());
  memcpy(assign, out.host<int>(o_as), sizeof(int) * nk);
  *nmatches = out.host<int>(o_as)[nk];
  return LORB_OK;
}

int lorb_search_by_projection_frame_dev(lorb_ctx* ctx, const lorb_frame_params* cur, const float cur_Tcw[16],
                                        const lorb_keypoints* d_cur_kps, const uint8_t* d_cur_slot_state,
                                        const lorb_last_frame* d_last, float th, int32_t* d_assign,
                                        int32_t* d_nmatches) {
  if (!ctx || !cur || !cur_Tcw || !d_cur_kps || !d_last || !d_nmatches) return LORB_E_INVALID;
  const int nk = d_cur_kps->n;
  LORB_TRY(frame_dev_check(ctx, cur, d_cur_kps, d_last));
  if (nk == 0) {
    LORB_HIP(ctx, hipMemsetAsync(d_nmatches, 0, sizeof(int32_t), ctx->stream));
    return LORB_OK;
  }
  if (!d_assign) return lorb::set_error(ctx, LORB_E_INVALID, "null array");
  WinParams P = frame_params_a4(cur, cur_Tcw, d_last->Tcw, th, cur->n_levels);
  const uint8_t* ss = d_cur_slot_state;
  if (!ss) LORB_TRY(empty_slots(ctx, nk, &ss));
  KpDev K = kp_dev(d_cur_kps, ss);
  return a4_issue(ctx, &K, P, last_dev(d_last), d_assign, d_nmatches, nullptr);
}

// VisualOdometry::EstimatePoseMotion (src/visual_odometry.cpp:117-138) on device-resident data:
// a4 at th_first into d_assign, a4 at th_retry over all-EMPTY slots into a buffer of its own --
// always enqueued, its kernels returning at once unless the first pass found <= min_matches --
// then the tail kernel (pass decision, final codes, residual gathering, pose-only LM).  The second
// pass reuses the first's keypoint grid and working buffers (the stream orders them).
// fr (lorb_track_motion_frames_dev): K.n and L.n are the caller's bounds (both >= 1), every kernel
// reads the counts of fr->dc, and the tail is k_track_frames_tail, which also applies the codes to
// the current frame's slots.  mp (with fr: lorb_track_motion_frames_pose_dev): cur_Tcw, pose_init and
// last_Tcw are null, the candidate kernels and the tail read the MotionPose block *mp instead.  rg (with
// mp: lorb_track_motion_refer_pose_dev): the tail is the form that also writes the slots' ids.
static int track_motion_issue(lorb_ctx* ctx, const lorb_frame_params* cur, const float* cur_Tcw,
                              const float* pose_init, KpDev K, const float* slot_pos, const LastDev& L,
                              const float* last_Tcw, const lorb_track_motion_params* par,
                              const lorb_lm_options* opt, int* d_assign, lorb_track_motion_result* rec,
                              int* assign_out, const lorb::FramesTail* fr = nullptr,
                              const lorb::MotionPose* mp = nullptr, const lorb::ReferGids* rg = nullptr) {
  const int nk = K.n;
  const lorb::FrameCounts* dc = fr ? &fr->dc : nullptr;
  int* tm;  // pass 2's codes (nk) | its count | pass 1's count
  float* list;
  LORB_TRY(lorb::scratch_t(ctx, slot<S_TM, 0>(), (size_t)nk + 2, &tm));
  LORB_TRY(lorb::scratch_t(ctx, slot<S_TM, 1>(), (size_t)std::max(nk, 1) * 5, &list));
  int *nm2 = tm + nk, *nm1 = tm + nk + 1;
  const uint8_t* given = K.slot_state;
  if (nk == 0) {
    LORB_HIP(ctx, hipMemsetAsync(nm2, 0, 2 * sizeof(int), ctx->stream));  // nothing to match: both passes find 0
  } else {
    const uint8_t* z;
    LORB_TRY(empty_slots(ctx, nk, &z));
    if (!given) K.slot_state = z;
    LORB_TRY(a4_issue(ctx, &K, frame_params_a4(cur, cur_Tcw, last_Tcw, par->th_first, cur->n_levels), L, d_assign, nm1,
                      nullptr, nullptr, 0, dc, mp));
    K.slot_state = z;  // src/visual_odometry.cpp:128: the retry starts from emptied slots
    LORB_TRY(a4_issue(ctx, &K, frame_params_a4(cur, cur_Tcw, last_Tcw, par->th_retry, cur->n_levels), L, tm, nm2, nullptr,
                      nm1, par->min_matches, dc, mp));
  }
  lorb::TrackTail t{};
  t.nk = nk; t.nm1 = nm1; t.nm2 = nm2; t.assign2 = tm; t.assign = d_assign;
  t.slot_state = given; t.slot_pos = slot_pos; t.last_pos = L.pos; t.x = K.x; t.y = K.y;
  t.min_matches = par->min_matches;
  t.fx = cur->fx; t.fy_eff = par->fy_eff; t.cx = cur->cx; t.cy = cur->cy;
  if (pose_init) memcpy(t.pose_init, pose_init, sizeof(t.pose_init));
  t.list = list; t.rec = rec; t.assign_out = assign_out;
  if (fr && mp && rg) return lorb::launch_track_frames_tail_refer(ctx, t, *fr, mp, *rg, opt);
  if (fr && mp) return lorb::launch_track_frames_tail_pose(ctx, t, *fr, mp, opt);
  if (fr) return lorb::launch_track_frames_tail(ctx, t, *fr, opt);
  return lorb::launch_track_tail(ctx, t, opt);
}

int lorb_track_motion_dev(lorb_ctx* ctx, const lorb_frame_params* cur, const float cur_Tcw[16],
                          const float pose_init[6], const lorb_keypoints* d_cur_kps, const uint8_t* d_slot_state,
                          const float* d_slot_pos, const lorb_last_frame* d_last,
                          const lorb_track_motion_params* par, const lorb_lm_options* opt, int32_t* d_assign,
                          lorb_track_motion_result* d_result) {
  if (!ctx || !cur || !cur_Tcw || !pose_init || !d_cur_kps || !d_last || !par || !opt || !d_result) return LORB_E_INVALID;
  LORB_TRY(frame_dev_check(ctx, cur, d_cur_kps, d_last));
  if (par->min_matches < 0) return lorb::set_error(ctx, LORB_E_INVALID, "min_matches %d is negative", par->min_matches);
  if ((d_cur_kps->n > 0 && !d_assign) || (d_slot_state && !d_slot_pos))
    return lorb::set_error(ctx, LORB_E_INVALID, "null array");
  return track_motion_issue(ctx, cur, cur_Tcw, pose_init, kp_dev(d_cur_kps, d_slot_state), d_slot_pos, last_dev(d_last),
                            d_last->Tcw, par, opt, d_assign, d_result, nullptr);
}

int lorb_track_motion(lorb_ctx* ctx, const lorb_frame_params* cur, const float cur_Tcw[16], const float pose_init[6],
                      const lorb_keypoints* cur_kps, const uint8_t* slot_state, const float* slot_pos,
                      const lorb_last_frame* last, const lorb_track_motion_params* par, const lorb_lm_options* opt,
                      int32_t* assign, lorb_track_motion_result* result, float* Tcw_out) {
  if (!ctx || !cur || !cur_Tcw || !pose_init || !cur_kps || !last || !par || !opt || !result) return LORB_E_INVALID;
  LORB_TRY(frame_dev_check(ctx, cur, cur_kps, last));
  const int nk = cur_kps->n, nl = last->n;
  if (par->min_matches < 0) return lorb::set_error(ctx, LORB_E_INVALID, "min_matches %d is negative", par->min_matches);
  if ((nk > 0 && !assign) || (slot_state && !slot_pos)) return lorb::set_error(ctx, LORB_E_INVALID, "null array");
  for (int i = 0; i < nl; ++i)
    if (last->has_mp[i] && (last->octave[i] < 0 || last->octave[i] >= LORB_MAX_LEVELS))
      return lorb::set_error(ctx, LORB_E_INVALID, "last keypoint %d: octave %d out of range", i, last->octave[i]);
  // every input in one pull; the tail kernel stores assign and the record into the mapped block
  lorb::InPack in(ctx);
  KpParts kp;
  kps_add(in, cur_kps, slot_state, kp);
  const int i_sp = in.add_t(slot_state ? slot_pos : nullptr, (size_t)nk * 3);
  const int i_hm = in.add_t(last->has_mp, nl), i_ol = in.add_t(last->outlier, nl), i_lk = in.add_t(last->mp_locked, nl),
            i_pos = in.add_t(last->mp_pos, (size_t)nl * 3), i_ld = in.add_t(last->mp_desc, (size_t)nl * 32),
            i_lo = in.add_t(last->octave, nl), i_la = in.add_t(last->angle, nl);
  LORB_TRY(in.commit());
  KpDev K = kps_finish(in, kp, nk);
  if (!slot_state) K.slot_state = nullptr;  // all EMPTY: the chain reads its own zeroed buffer
  const LastDev L = {nl, in.dev<uint8_t>(i_hm), in.dev<uint8_t>(i_ol), in.dev<uint8_t>(i_lk), in.dev<float>(i_pos),
                     in.dev<float>(i_la), in.dev<int>(i_lo), in.dev<const uint4>(i_ld)};
  int* dassign;
  LORB_TRY(lorb::scratch_t(ctx, slot<S_TM, 2>(), (size_t)nk + 1, &dassign));
  lorb::OutPack out(ctx);
  const int o_rec = out.add(sizeof(lorb_track_motion_result)), o_as = out.add(sizeof(int) * ((size_t)nk + 1));
  LORB_TRY(out.alloc(true));
  LORB_TRY(track_motion_issue(ctx, cur, cur_Tcw, pose_init, K, in.dev<float>(i_sp), L, last->Tcw, par, opt, dassign,
                              out.dev<lorb_track_motion_result>(o_rec), out.dev<int>(o_as)));
  LORB_TRY(out.fetch());
  if (nk > 0) memcpy(assign, out.host<int>(o_as), sizeof(int) * nk);
  *result = *out.host<lorb_track_motion_result>(o_rec);
  if (Tcw_out) {
    const float R[3] = {(float)result->pose[0], (float)result->pose[1], (float)result->pose[2]};
    const float T[3] = {(float)result->pose[3], (float)result->pose[4], (float)result->pose[5]};
    lorb_pose_to_Tcw(R, T, Tcw_out);
  }
  return LORB_OK;
}

// the fill launch of lorb_frame_slots_fill_dev and of the frames chain (dc / rec given; pc: its
// device-pose form, Tcw null)
static int slots_fill_issue(lorb_ctx* ctx, const lorb_frame_params* frame, const float* Tcw, const lorb_frame_out* f,
                            int n_max, int mode, const lorb_frame_slots* s, uint8_t* locked, int* n_created,
                            const lorb::FrameCounts* dc, lorb_track_frames_result* rec, const PoseChain* pc = nullptr,
                            const ReferHead* rh = nullptr) {  // rh (with pc): the second attempt's head
  SlotFill a{};
  a.fp = *frame;
  if (Tcw) {
    float Twc[16];
    inv4_lu32f(Tcw, Twc);
    memcpy(a.Twc.v, Twc, sizeof(a.Twc.v));
  }
  a.count = f->counts; a.n_max = n_max;
  a.x = f->left.x; a.y = f->left.y; a.depth = f->depth; a.desc = reinterpret_cast<const uint4*>(f->left.desc);
  a.state = s->state; a.pos = s->pos; a.sdesc = reinterpret_cast<uint4*>(s->desc);
  a.locked = locked; a.n_created = n_created;
  if (dc && pc && rh)
    hipLaunchKernelGGL((k_slots_fill<LORB_SLOTS_UPDATE_FRAME, true, true, true>), dim3(1), dim3(1024), 0, ctx->stream, a, *dc,
                       rec, *pc, *rh);
  else if (dc && pc)
    hipLaunchKernelGGL((k_slots_fill<LORB_SLOTS_UPDATE_FRAME, true, true>), dim3(1), dim3(1024), 0, ctx->stream, a, *dc, rec,
                       *pc);
  else if (dc)
    hipLaunchKernelGGL((k_slots_fill<LORB_SLOTS_UPDATE_FRAME, true>), dim3(1), dim3(1024), 0, ctx->stream, a, *dc, rec);
  else if (mode == LORB_SLOTS_UPDATE_FRAME)
    hipLaunchKernelGGL((k_slots_fill<LORB_SLOTS_UPDATE_FRAME, false>), dim3(1), dim3(1024), 0, ctx->stream, a,
                       lorb::FrameCounts{}, (lorb_track_frames_result*)nullptr);
  else
    hipLaunchKernelGGL((k_slots_fill<LORB_SLOTS_INITIALIZE, false>), dim3(1), dim3(1024), 0, ctx->stream, a,
                       lorb::FrameCounts{}, (lorb_track_frames_result*)nullptr);
  LORB_CHECK_LAUNCH(ctx);
  return LORB_OK;
}
static bool slots_ok(const lorb_frame_slots* s) { return s && s->state && s->pos && s->desc; }
static bool frame_left_ok(const lorb_frame_out* f) {
  return f && f->counts && f->depth && f->left.x && f->left.y && f->left.desc;
}

int lorb_frame_slots_fill_dev(lorb_ctx* ctx, const lorb_frame_params* frame, const float Tcw[16],
                              const lorb_frame_out* d_frame, int32_t n_max, int32_t mode,
                              const lorb_frame_slots* d_slots, int32_t* d_n_created) {
  if (!ctx || !frame || !Tcw || !d_frame || !d_slots) return LORB_E_INVALID;
  if (n_max < 0) return lorb::set_error(ctx, LORB_E_INVALID, "negative bound %d", n_max);
  if (mode != LORB_SLOTS_UPDATE_FRAME && mode != LORB_SLOTS_INITIALIZE)
    return lorb::set_error(ctx, LORB_E_INVALID, "unknown fill mode %d", mode);
  if (!frame_left_ok(d_frame) || !slots_ok(d_slots)) return lorb::set_error(ctx, LORB_E_INVALID, "null array");
  return slots_fill_issue(ctx, frame, Tcw, d_frame, n_max, mode, d_slots, nullptr, d_n_created, nullptr, nullptr);
}

// VisualOdometry::EstimatePoseMotion(pF) after its SetPose (src/visual_odometry.cpp:121-137) on two
// built frames whose counts stay in device memory: the UpdateFrame fill of the last frame's slots
// (which also checks the counts and writes the record's status), the motion chain in its device-count
// form over the caller's bounds, and the tail that applies the codes to the current frame's slots.
// (both forms: the host poses, or pose -- cur, last and model of the device-pose form, blk unset; rh and
// rg with pose: the second attempt, whose "last" objects are the refer frame's)
static int track_frames_issue(lorb_ctx* ctx, const lorb_frame_params* cur, const float* cur_Tcw, const float* pose_init,
                              const float* last_Tcw, const PoseChain* pose, const lorb_frame_out* d_cur, int32_t n_max_cur,
                              const lorb_frame_slots* d_cur_slots, int32_t cur_slots_given, const lorb_frame_out* d_last,
                              int32_t n_max_last, const lorb_frame_slots* d_last_slots, const uint8_t* d_last_outlier,
                              const lorb_track_motion_params* par, const lorb_lm_options* opt, int32_t* d_assign,
                              lorb_track_frames_result* d_result, const ReferHead* rh = nullptr,
                              const lorb::ReferGids* rg = nullptr) {
  if (n_max_cur < 1 || n_max_last < 1)
    return lorb::set_error(ctx, LORB_E_INVALID, "bounds %d / %d must be positive", n_max_last, n_max_cur);
  // a4's candidate list is allocated from the bounds: past this it would need the total read back
  if ((int64_t)n_max_last * (int64_t)n_max_cur > (int64_t(8) << 20))
    return lorb::set_error(ctx, LORB_E_INVALID, "bounds %d x %d exceed the asynchronous limit of 8M candidates",
                           n_max_last, n_max_cur);
  if (cur->n_levels < 1 || cur->n_levels > LORB_MAX_LEVELS)
    return lorb::set_error(ctx, LORB_E_INVALID, "n_levels %d out of range", cur->n_levels);
  if (par->min_matches < 0) return lorb::set_error(ctx, LORB_E_INVALID, "min_matches %d is negative", par->min_matches);
  if (!frame_left_ok(d_cur) || !frame_left_ok(d_last) || !slots_ok(d_cur_slots) || !slots_ok(d_last_slots) ||
      !d_cur->left.octave || !d_cur->left.angle || !d_cur->u_right || !d_last->left.octave || !d_last->left.angle)
    return lorb::set_error(ctx, LORB_E_INVALID, "null array");
  lorb::FramesTail fr{};
  fr.dc = {d_last->counts, d_cur->counts, n_max_last, n_max_cur};
  fr.cur = *d_cur_slots; fr.last = *d_last_slots; fr.given = cur_slots_given != 0;
  uint8_t* lk;
  LORB_TRY(lorb::scratch_t(ctx, slot<S_TF, 0>(), (size_t)n_max_last, &lk));
  PoseChain pc{};
  if (pose) {  // the fill reads the last frame's own count; the kernels behind it the copy in the block (-1: status 1)
    pc = *pose;
    LORB_TRY(lorb::scratch_t(ctx, slot<S_TP, 0>(), 1, &pc.blk));
  }
  LORB_TRY(slots_fill_issue(ctx, cur, last_Tcw, d_last, n_max_last, LORB_SLOTS_UPDATE_FRAME, d_last_slots, lk, nullptr,
                            &fr.dc, d_result, pose ? &pc : nullptr, rh));
  if (pose) fr.dc.last = &pc.blk->n_last;
  KpDev K;
  K.x = d_cur->left.x; K.y = d_cur->left.y; K.angle = d_cur->left.angle; K.uR = d_cur->u_right;
  K.octave = d_cur->left.octave; K.desc = reinterpret_cast<const uint4*>(d_cur->left.desc);
  K.slot_state = fr.given ? d_cur_slots->state : nullptr;
  K.cell_off = nullptr; K.cell_idx = nullptr; K.n = n_max_cur;
  // has_mp is "state != EMPTY": the kernels test the byte for non-zero, so the states serve as they are
  static_assert(LORB_SLOT_EMPTY == 0, "the slot states are read as has_mp flags");
  const LastDev L = {n_max_last, d_last_slots->state, d_last_outlier, lk, d_last_slots->pos, d_last->left.angle,
                     d_last->left.octave, reinterpret_cast<const uint4*>(d_last_slots->desc)};
  return track_motion_issue(ctx, cur, cur_Tcw, pose_init, K, d_cur_slots->pos, L, last_Tcw, par, opt, d_assign,
                            &d_result->motion, nullptr, &fr, pc.blk, rg);
}

int lorb_track_motion_frames_dev(lorb_ctx* ctx, const lorb_frame_params* cur, const float cur_Tcw[16],
                                 const float pose_init[6], const lorb_frame_out* d_cur, int32_t n_max_cur,
                                 const lorb_frame_slots* d_cur_slots, int32_t cur_slots_given,
                                 const float last_Tcw[16], const lorb_frame_out* d_last, int32_t n_max_last,
                                 const lorb_frame_slots* d_last_slots, const uint8_t* d_last_outlier,
                                 const lorb_track_motion_params* par, const lorb_lm_options* opt,
                                 int32_t* d_assign, lorb_track_frames_result* d_result) {
  if (!ctx || !cur || !cur_Tcw || !pose_init || !d_cur || !d_cur_slots || !last_Tcw || !d_last || !d_last_slots || !par ||
      !opt || !d_assign || !d_result)
    return LORB_E_INVALID;
  return track_frames_issue(ctx, cur, cur_Tcw, pose_init, last_Tcw, nullptr, d_cur, n_max_cur, d_cur_slots, cur_slots_given,
                            d_last, n_max_last, d_last_slots, d_last_outlier, par, opt, d_assign, d_result);
}

// The same chain with the three poses in device memory (VisualOdometry::Run's hand-over between
// frames): the first launch is k_slots_fill's POSE form -- status over the counts and the blocks, the
// motion-model prediction on thread 0, the MotionPose block -- and the candidate kernels and the tail
// are the forms that read that block.  The same number of launches as the host-pose call.
int lorb_track_motion_frames_pose_dev(lorb_ctx* ctx, const lorb_frame_params* cur, lorb_frame_pose* d_cur_pose,
                                      const lorb_frame_out* d_cur, int32_t n_max_cur,
                                      const lorb_frame_slots* d_cur_slots, int32_t cur_slots_given,
                                      const lorb_frame_pose* d_last_pose, const lorb_motion_model* d_model,
                                      const lorb_frame_out* d_last, int32_t n_max_last,
                                      const lorb_frame_slots* d_last_slots, const uint8_t* d_last_outlier,
                                      const lorb_track_motion_params* par, const lorb_lm_options* opt,
                                      int32_t* d_assign, lorb_track_frames_result* d_result) {
  if (!ctx || !cur || !d_cur_pose || !d_cur || !d_cur_slots || !d_last_pose || !d_last || !d_last_slots || !par || !opt ||
      !d_assign || !d_result)
    return LORB_E_INVALID;
  const PoseChain pose = {d_cur_pose, d_last_pose, d_model, nullptr};
  return track_frames_issue(ctx, cur, nullptr, nullptr, nullptr, &pose, d_cur, n_max_cur, d_cur_slots, cur_slots_given,
                            d_last, n_max_last, d_last_slots, d_last_outlier, par, opt, d_assign, d_result);
}

// VisualOdometry::Run :50-54, the second attempt on the reference keyframe, decided on the device: the
// device-pose chain with the refer frame's objects as the last frame's, the current slots given, and
// k_slots_fill's REFER form in front, which ends the call -- every later kernel returns at once -- unless
// the first attempt's record says pass 0 and the reference-frame word is the caller's refer frame.  The
// tail is the form that also applies the final codes to the slots' global ids.  The same launches as
// lorb_track_motion_frames_pose_dev for the same bounds.
int lorb_track_motion_refer_pose_dev(lorb_ctx* ctx, const lorb_frame_params* cur, lorb_frame_pose* d_cur_pose,
                                     const lorb_frame_out* d_cur, int32_t n_max_cur, const lorb_frame_slots* d_cur_slots,
                                     int32_t first_slots_given, const lorb_frame_pose* d_refer_pose,
                                     const lorb_motion_model* d_model, const lorb_frame_out* d_refer, int32_t n_max_refer,
                                     const lorb_frame_slots* d_refer_slots, const uint8_t* d_refer_outlier,
                                     const int32_t* d_last_slot_gid, int32_t n_max_last, const int32_t* d_refer_slot_gid,
                                     int32_t* d_cur_slot_gid, int32_t refer_kf, int32_t* d_refer_kf,
                                     const lorb_local_map_result* d_prev_update, const lorb_track_motion_params* par,
                                     const lorb_lm_options* opt, int32_t* d_assign, lorb_track_frames_result* d_result,
                                     lorb_track_refer_result* d_refer_result) {
  if (!ctx || !cur || !d_cur_pose || !d_cur || !d_cur_slots || !d_refer_pose || !d_model || !d_refer || !d_refer_slots ||
      !par || !opt || !d_assign || !d_result || !d_refer_result)
    return LORB_E_INVALID;
  // the two optional groups are given whole or not at all (checked before the context is touched)
  const int n_gid = (d_last_slot_gid != nullptr) + (d_refer_slot_gid != nullptr) + (d_cur_slot_gid != nullptr);
  if (n_gid != 0 && n_gid != 3) return LORB_E_INVALID;
  if ((d_refer_kf != nullptr) != (d_prev_update != nullptr)) return LORB_E_INVALID;
  if (n_gid && n_max_last < 1) return lorb::set_error(ctx, LORB_E_INVALID, "bound %d must be positive", n_max_last);
  const PoseChain pose = {d_cur_pose, d_refer_pose, d_model, nullptr};
  const ReferHead rh = {d_assign, first_slots_given != 0, d_last_slot_gid, n_max_last,    d_cur_slot_gid,
                        refer_kf, d_refer_kf,             d_prev_update,   d_refer_result};
  const lorb::ReferGids rg = {d_refer_slot_gid, n_max_refer, d_cur_slot_gid};
  return track_frames_issue(ctx, cur, nullptr, nullptr, nullptr, &pose, d_cur, n_max_cur, d_cur_slots, 1, d_refer,
                            n_max_refer, d_refer_slots, d_refer_outlier, par, opt, d_assign, d_result, &rh, &rg);
}

int lorb_frame_pose_finish_dev(lorb_ctx* ctx, const lorb_track_local_frames_result* d_local_result,
                               const lorb_frame_pose* d_last_pose, lorb_frame_pose* d_cur_pose,
                               lorb_motion_model* d_model) {
  if (!ctx || !d_local_result || !d_last_pose || !d_cur_pose || !d_model) return LORB_E_INVALID;
  hipLaunchKernelGGL(k_pose_finish, dim3(1), dim3(64), 0, ctx->stream, PoseFinish{d_local_result, d_last_pose, d_cur_pose, d_model});
  LORB_CHECK_LAUNCH(ctx);
  return LORB_OK;
}

int lorb_is_in_frustum(lorb_ctx* ctx, const lorb_frame_params* frame, const float Tcw[16],
                       const lorb_frustum_points* pts, float viewing_cos_limit, uint8_t* in_view,
                       float* proj_x, float* proj_y, float* proj_xr, int32_t* pred_level, float* view_cos) {
  if (!ctx || !frame || !Tcw || !pts) return LORB_E_INVALID;
  const int n = pts->n;
  if (n <= 0) return LORB_OK;
  float Twc[16];
  inv4_lu32f(Tcw, Twc);
  const float Ow[3] = {Twc[3], Twc[7], Twc[11]};
  float *dT, *dO, *pos, *nrm, *mx, *mn, *outf;
  uint8_t* iv;
  int* lev;
  LORB_TRY(lorb::upload_t(ctx, S_W0, Tcw, 16, &dT));
  LORB_TRY(lorb::upload_t(ctx, S_W1, Ow, 3, &dO));
  LORB_TRY(lorb::upload_t(ctx, S_W2, pts->pos, (size_t)n * 3, &pos));
  LORB_TRY(lorb::upload_t(ctx, S_W3, pts->normal, (size_t)n * 3, &nrm));
  LORB_TRY(lorb::upload_t(ctx, S_W4, pts->max_dist, n, &mx));
  LORB_TRY(lorb::upload_t(ctx, S_W5, pts->min_dist, n, &mn));
  LORB_TRY(lorb::scratch_t(ctx, S_W6, (size_t)n * 4, &outf));
  LORB_TRY(lorb::scratch_t(ctx, S_W7, (size_t)n, &iv));
  LORB_TRY(lorb::scratch_t(ctx, S_W8, (size_t)n, &lev));
  hipLaunchKernelGGL(k_frustum, dim3(lorb::ceil_div(n, 256)), dim3(256), 0, ctx->stream, *frame, dT, dO, n, pos, nrm, mx,
                     mn, viewing_cos_limit, iv, outf, outf + n, outf + 2 * n, lev, outf + 3 * n,
                     (const uint8_t*)nullptr, (const uint8_t*)nullptr);
  LORB_CHECK_LAUNCH(ctx);
  LORB_HIP(ctx, hipMemcpyAsync(in_view, iv, n, hipMemcpyDeviceToHost, ctx->stream));
  LORB_HIP(ctx, hipMemcpyAsync(proj_x, outf, sizeof(float) * n, hipMemcpyDeviceToHost, ctx->stream));
  LORB_HIP(ctx, hipMemcpyAsync(proj_y, outf + n, sizeof(float) * n, hipMemcpyDeviceToHost, ctx->stream));
  LORB_HIP(ctx, hipMemcpyAsync(proj_xr, outf + 2 * n, sizeof(float) * n, hipMemcpyDeviceToHost, ctx->stream));
  LORB_HIP(ctx, hipMemcpyAsync(view_cos, outf + 3 * n, sizeof(float) * n, hipMemcpyDeviceToHost, ctx->stream));
  LORB_HIP(ctx, hipMemcpyAsync(pred_level, lev, sizeof(int) * n, hipMemcpyDeviceToHost, ctx->stream));
  LORB_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return LORB_OK;
}

// the tracking sequence of VisualOdometry::EstimatePoseLocal
// (src/visual_odometry.cpp:173-201) on device-resident frame and map data: IsInFrustum for every
// local map point not already in the frame and not bad, then SearchByProjection(F, localMPs, th).
int lorb_track_local_map_dev(lorb_ctx* ctx, const lorb_frame_params* frame, const float Tcw[16],
                             const lorb_keypoints* d_kps, const uint8_t* d_slot_state,
                             const lorb_map_points_dev* pts, float viewing_cos_limit, float th,
                             uint8_t* d_in_view, float* d_track, int32_t* d_level,
                             int32_t* d_assign, int32_t* d_nmatches) {
  if (!ctx || !frame || !Tcw || !d_kps || !pts || !d_in_view || !d_track || !d_level || !d_assign || !d_nmatches)
    return LORB_E_INVALID;
  const int nk = d_kps->n, np = pts->n;
  if (nk < 0 || np < 0) return lorb::set_error(ctx, LORB_E_INVALID, "negative sizes");
  if (frame->n_levels < 1 || frame->n_levels > LORB_MAX_LEVELS)
    return lorb::set_error(ctx, LORB_E_INVALID, "n_levels %d out of range", frame->n_levels);
  float Twc[16];
  inv4_lu32f(Tcw, Twc);
  const float TO[19] = {Tcw[0], Tcw[1], Tcw[2], Tcw[3], Tcw[4], Tcw[5], Tcw[6], Tcw[7], Tcw[8], Tcw[9],
                        Tcw[10], Tcw[11], Tcw[12], Tcw[13], Tcw[14], Tcw[15], Twc[3], Twc[7], Twc[11]};
  float* dTO;
  LORB_TRY(lorb::upload_t(ctx, slot<S_WX, 7>(), TO, 19, &dTO));
  if (np > 0)
    hipLaunchKernelGGL(k_frustum, dim3(lorb::ceil_div(np, 256)), dim3(256), 0, ctx->stream, *frame, dTO, dTO + 16, np,
                       pts->pos, pts->normal, pts->max_dist, pts->min_dist, viewing_cos_limit, d_in_view, d_track,
                       d_track + np, d_track + 2 * np, d_level, d_track + 3 * np, pts->in_frame, pts->is_bad);
  if (nk == 0) {
    LORB_HIP(ctx, hipMemsetAsync(d_nmatches, 0, sizeof(int32_t), ctx->stream));
    LORB_CHECK_LAUNCH(ctx);
    return LORB_OK;
  }
  const uint8_t* ss = d_slot_state;
  if (!ss) LORB_TRY(empty_slots(ctx, nk, &ss));
  KpDev K = kp_dev(d_kps, ss);
  WinParams P{};
  P.fp = *frame;
  P.th = th;
  const LocalDev Q = {np, d_in_view, pts->is_bad, pts->locked, d_track, d_track + np, d_track + 2 * np, d_track + 3 * np,
                      d_level, reinterpret_cast<const uint4*>(pts->desc)};
  return a5_issue(ctx, &K, P, Q, d_assign, d_nmatches, nullptr);
}

int lorb_track_local_map(lorb_ctx* ctx, const lorb_frame_params* frame, const float Tcw[16], const lorb_keypoints* kps,
                         const uint8_t* slot_state, const lorb_map_points_dev* pts, float viewing_cos_limit, float th,
                         uint8_t* in_view, float* track, int32_t* level, int32_t* assign, int32_t* nmatches) {
  if (!ctx || !frame || !Tcw || !kps || !pts || !nmatches) return LORB_E_INVALID;
  const int nk = kps->n, np = pts->n;
  if (nk < 0 || np < 0) return lorb::set_error(ctx, LORB_E_INVALID, "negative sizes");
  if ((np > 0 && (!in_view || !track || !level || !pts->pos || !pts->normal || !pts->max_dist || !pts->min_dist ||
                  !pts->desc || !pts->locked)) ||
      (nk > 0 && (!assign || !kps->x || !kps->y || !kps->octave || !kps->angle || !kps->desc)))
    return lorb::set_error(ctx, LORB_E_INVALID, "null array");
  lorb_keypoints K{};
  lorb_map_points_dev M{};
  K.n = nk; M.n = np;
  LORB_TRY(lorb::upload_t(ctx, slot<S_TL, 0>(), kps->x, (size_t)nk, const_cast<float**>(&K.x)));
  LORB_TRY(lorb::upload_t(ctx, slot<S_TL, 1>(), kps->y, (size_t)nk, const_cast<float**>(&K.y)));
  LORB_TRY(lorb::upload_t(ctx, slot<S_TL, 2>(), kps->octave, (size_t)nk, const_cast<int32_t**>(&K.octave)));
  LORB_TRY(lorb::upload_t(ctx, slot<S_TL, 3>(), kps->angle, (size_t)nk, const_cast<float**>(&K.angle)));
  LORB_TRY(lorb::upload_t(ctx, slot<S_TL, 4>(), kps->u_right, kps->u_right ? (size_t)nk : 0, const_cast<float**>(&K.u_right)));
  LORB_TRY(lorb::upload_t(ctx, slot<S_TL, 5>(), kps->desc, (size_t)nk * 32, const_cast<uint8_t**>(&K.desc)));
  uint8_t* dss;
  LORB_TRY(lorb::upload_t(ctx, slot<S_TL, 6>(), slot_state, slot_state ? (size_t)nk : 0, &dss));
  LORB_TRY(lorb::upload_t(ctx, slot<S_TL, 7>(), pts->pos, (size_t)np * 3, const_cast<float**>(&M.pos)));
  LORB_TRY(lorb::upload_t(ctx, slot<S_TL, 8>(), pts->normal, (size_t)np * 3, const_cast<float**>(&M.normal)));
  LORB_TRY(lorb::upload_t(ctx, slot<S_TL, 9>(), pts->max_dist, (size_t)np, const_cast<float**>(&M.max_dist)));
  LORB_TRY(lorb::upload_t(ctx, slot<S_TL, 10>(), pts->min_dist, (size_t)np, const_cast<float**>(&M.min_dist)));
  LORB_TRY(lorb::upload_t(ctx, slot<S_TL, 11>(), pts->desc, (size_t)np * 32, const_cast<uint8_t**>(&M.desc)));
  LORB_TRY(lorb::upload_t(ctx, slot<S_TL, 12>(), pts->locked, (size_t)np, const_cast<uint8_t**>(&M.locked)));
  LORB_TRY(lorb::upload_t(ctx, slot<S_TL, 13>(), pts->is_bad, pts->is_bad ? (size_t)np : 0, const_cast<uint8_t**>(&M.is_bad)));
  LORB_TRY(lorb::upload_t(ctx, slot<S_TL, 14>(), pts->in_frame, pts->in_frame ? (size_t)np : 0,
                          const_cast<uint8_t**>(&M.in_frame)));
  uint8_t* div;
  float* dtr;
  int32_t *dlv, *das, *dnm;
  LORB_TRY(lorb::scratch_t(ctx, slot<S_TL, 15>(), (size_t)std::max(np, 1), &div));
  LORB_TRY(lorb::scratch_t(ctx, slot<S_TL, 16>(), (size_t)std::max(np, 1) * 4, &dtr));
  LORB_TRY(lorb::scratch_t(ctx, slot<S_TL, 17>(), (size_t)std::max(np, 1), &dlv));
  LORB_TRY(lorb::scratch_t(ctx, slot<S_TL, 18>(), (size_t)std::max(nk, 1), &das));
  LORB_TRY(lorb::scratch_t(ctx, slot<S_TL, 19>(), 1, &dnm));
  LORB_TRY(lorb_track_local_map_dev(ctx, frame, Tcw, &K, dss, &M, viewing_cos_limit, th, div, dtr, dlv, das, dnm));
  if (np > 0) {
    LORB_HIP(ctx, hipMemcpyAsync(in_view, div, (size_t)np, hipMemcpyDeviceToHost, ctx->stream));
    LORB_HIP(ctx, hipMemcpyAsync(track, dtr, sizeof(float) * 4 * np, hipMemcpyDeviceToHost, ctx->stream));
    LORB_HIP(ctx, hipMemcpyAsync(level, dlv, sizeof(int32_t) * np, hipMemcpyDeviceToHost, ctx->stream));
  }
  if (nk > 0) LORB_HIP(ctx, hipMemcpyAsync(assign, das, sizeof(int32_t) * nk, hipMemcpyDeviceToHost, ctx->stream));
  LORB_HIP(ctx, hipMemcpyAsync(nmatches, dnm, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  LORB_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return LORB_OK;
}

// VisualOdometry::EstimatePoseLocal after UpdateLocalMap (src/visual_odometry.cpp:173-209) on
// device-resident data: a8 fused into a5's candidate kernel, the resolver, then the tail kernel
// (in-view count, gate, residual gathering, pose-only LM).  Launches: candidates + resolver + tail
// while np * nk <= kCandStrided and nk <= kStageKps; the grid build is added past kStageKps, the
// count / scan / write sequence replaces the one candidate pass past kCandStrided.  o: the tracking
// fields on the device; mir (or nulls): the host form's copy in its mapped result block.
static int track_local_issue(lorb_ctx* ctx, const lorb_frame_params* frame, const float* Tcw, const float* pose_init,
                             KpDev K, const float* slot_pos, const lorb_map_points_dev* pts,
                             const lorb_track_local_params* par, const lorb_lm_options* opt, const FieldsOut& o,
                             const FieldsOut& mir, int* d_assign, lorb_track_local_result* rec, int* assign_out) {
  const int nk = K.n, np = pts->n;
  int* nm;
  float* list;
  LORB_TRY(lorb::scratch_t(ctx, slot<S_TLC, 0>(), 1, &nm));
  LORB_TRY(lorb::scratch_t(ctx, slot<S_TLC, 1>(), (size_t)std::max(nk, 1) * 5, &list));
  const uint8_t* given = K.slot_state;
  FrustumIn F{};
  float Twc[16];
  inv4_lu32f(Tcw, Twc);
  memcpy(F.T, Tcw, sizeof(F.T));
  F.Ow[0] = Twc[3]; F.Ow[1] = Twc[7]; F.Ow[2] = Twc[11];
  F.pos = pts->pos; F.nrm = pts->normal; F.maxd = pts->max_dist; F.mind = pts->min_dist;
  F.skip_a = pts->in_frame; F.skip_b = pts->is_bad;
  F.cos_limit = par->viewing_cos_limit;
  WinParams P{};
  P.fp = *frame;
  P.th = par->th;
  const uint4* pdesc = reinterpret_cast<const uint4*>(pts->desc);
  if (nk == 0) {
    // no keypoints: the fields are still computed (the count pass walks nothing), nothing matches
    if (np > 0) {
      int* cnt;
      LORB_TRY(lorb::scratch_t(ctx, slot<S_WX, 0>(), (size_t)np + 1, &cnt));
      hipLaunchKernelGGL(k_cand_local_fr<false>, dim3(lorb::ceil_div(np, kCandWaves)), dim3(256), 0, ctx->stream, K, P, np,
                         F, o, mir, pdesc, cnt, (int2*)nullptr, 0);
    }
    LORB_HIP(ctx, hipMemsetAsync(nm, 0, sizeof(int), ctx->stream));
    LORB_CHECK_LAUNCH(ctx);
  } else {
    if (!given) LORB_TRY(empty_slots(ctx, nk, &K.slot_state));
    // the fused kernel is the first candidate pass; the write pass of the count / scan / write
    // sequence (off given) is k_cand_local reading the fields the count pass stored
    const LocalDev Q = {np, o.in_view, pts->is_bad, pts->locked, o.track, o.track + np, o.track + 2 * np,
                        o.track + 3 * np, o.level, pdesc};
    LORB_TRY(search_issue<0>(ctx, &K, P.fp, np, pts->locked, nullptr, {d_assign, nm, nullptr, nullptr, 0},
                             [&](auto pass, unsigned g, int* cnt, const int* off, int2* cand, int stride) {
                               using Pass = decltype(pass);
                               if (off)
                                 launch_cand_local<true, false>(ctx, g, K, P, Q, cnt, off, cand, stride);
                               else
                                 hipLaunchKernelGGL((k_cand_local_fr<Pass::write, Pass::grid>), dim3(g), dim3(256), 0,
                                                    ctx->stream, K, P, np, F, o, mir, pdesc, cnt, cand, stride);
                             }));
  }
  lorb::LocalTail t{};
  t.nk = nk; t.np = np; t.nm = nm; t.assign = d_assign; t.in_view = o.in_view;
  t.slot_state = given; t.slot_pos = slot_pos; t.pt_pos = pts->pos; t.x = K.x; t.y = K.y;
  t.min_matches = par->min_matches;
  t.fx = frame->fx; t.fy_eff = par->fy_eff; t.cx = frame->cx; t.cy = frame->cy;
  memcpy(t.pose_init, pose_init, sizeof(t.pose_init));
  t.list = list; t.rec = rec; t.assign_out = assign_out;
  return lorb::launch_local_tail(ctx, t, opt);
}

// argument checks shared by both forms of the local-map chain
static int track_local_check(lorb_ctx* ctx, const lorb_frame_params* frame, const lorb_keypoints* k,
                             const uint8_t* slot_state, const float* slot_pos, const lorb_map_points_dev* p,
                             const lorb_track_local_params* par, const uint8_t* in_view, const float* track,
                             const int32_t* level, const int32_t* assign) {
  const int nk = k->n, np = p->n;
  if (nk < 0 || np < 0) return lorb::set_error(ctx, LORB_E_INVALID, "negative sizes");
  if (frame->n_levels < 1 || frame->n_levels > LORB_MAX_LEVELS)
    return lorb::set_error(ctx, LORB_E_INVALID, "n_levels %d out of range", frame->n_levels);
  if (par->min_matches < 0) return lorb::set_error(ctx, LORB_E_INVALID, "min_matches %d is negative", par->min_matches);
  if ((np > 0 && (!in_view || !track || !level || !p->pos || !p->normal || !p->max_dist || !p->min_dist || !p->desc ||
                  !p->locked)) ||
      (nk > 0 && (!assign || !k->x || !k->y || !k->octave || !k->angle || !k->desc)) || (slot_state && !slot_pos))
    return lorb::set_error(ctx, LORB_E_INVALID, "null array");
  return LORB_OK;
}

int lorb_track_local_dev(lorb_ctx* ctx, const lorb_frame_params* frame, const float Tcw[16], const float pose_init[6],
                         const lorb_keypoints* d_kps, const uint8_t* d_slot_state, const float* d_slot_pos,
                         const lorb_map_points_dev* d_pts, const lorb_track_local_params* par,
                         const lorb_lm_options* opt, uint8_t* d_in_view, float* d_track, int32_t* d_level,
                         int32_t* d_assign, lorb_track_local_result* d_result) {
  if (!ctx || !frame || !Tcw || !pose_init || !d_kps || !d_pts || !par || !opt || !d_result) return LORB_E_INVALID;
  LORB_TRY(track_local_check(ctx, frame, d_kps, d_slot_state, d_slot_pos, d_pts, par, d_in_view, d_track, d_level,
                             d_assign));
  const FieldsOut o = {d_in_view, d_track, d_level}, none = {nullptr, nullptr, nullptr};
  return track_local_issue(ctx, frame, Tcw, pose_init, kp_dev(d_kps, d_slot_state), d_slot_pos, d_pts, par, opt, o, none,
                           d_assign, d_result, nullptr);
}

int lorb_track_local(lorb_ctx* ctx, const lorb_frame_params* frame, const float Tcw[16], const float pose_init[6],
                     const lorb_keypoints* kps, const uint8_t* slot_state, const float* slot_pos,
                     const lorb_map_points_dev* pts, const lorb_track_local_params* par, const lorb_lm_options* opt,
                     uint8_t* in_view, float* track, int32_t* level, int32_t* assign, lorb_track_local_result* result,
                     float* Tcw_out) {
  if (!ctx || !frame || !Tcw || !pose_init || !kps || !pts || !par || !opt || !result) return LORB_E_INVALID;
  LORB_TRY(track_local_check(ctx, frame, kps, slot_state, slot_pos, pts, par, in_view, track, level, assign));
  const int nk = kps->n, np = pts->n;
  // every input in one pull; the candidate kernel stores the tracking fields, the tail kernel assign
  // and the record, into the mapped block
  lorb::InPack in(ctx);
  KpParts kp;
  kps_add(in, kps, slot_state, kp, false);  // all EMPTY: nothing packed, the chain reads its own zeroed buffer
  const int i_sp = in.add_t(slot_state ? slot_pos : nullptr, (size_t)nk * 3);
  const int i_pos = in.add_t(pts->pos, (size_t)np * 3), i_nrm = in.add_t(pts->normal, (size_t)np * 3),
            i_mx = in.add_t(pts->max_dist, np), i_mn = in.add_t(pts->min_dist, np),
            i_pd = in.add_t(pts->desc, (size_t)np * 32), i_lk = in.add_t(pts->locked, np),
            i_bad = in.add_t(pts->is_bad, np), i_inf = in.add_t(pts->in_frame, np);
  LORB_TRY(in.commit());
  const KpDev K = kps_finish(in, kp, nk);
  lorb_map_points_dev M{};
  M.n = np;
  M.pos = in.dev<float>(i_pos); M.normal = in.dev<float>(i_nrm); M.max_dist = in.dev<float>(i_mx);
  M.min_dist = in.dev<float>(i_mn); M.desc = in.dev<uint8_t>(i_pd); M.locked = in.dev<uint8_t>(i_lk);
  M.is_bad = in.dev<uint8_t>(i_bad); M.in_frame = in.dev<uint8_t>(i_inf);
  int* dassign;
  FieldsOut o;
  LORB_TRY(lorb::scratch_t(ctx, slot<S_TLC, 2>(), (size_t)nk + 1, &dassign));
  LORB_TRY(lorb::scratch_t(ctx, slot<S_TLC, 3>(), (size_t)std::max(np, 1), &o.in_view));
  LORB_TRY(lorb::scratch_t(ctx, slot<S_TLC, 4>(), (size_t)std::max(np, 1) * 4, &o.track));
  LORB_TRY(lorb::scratch_t(ctx, slot<S_TLC, 5>(), (size_t)std::max(np, 1), &o.level));
  lorb::OutPack out(ctx);
  const int o_rec = out.add(sizeof(lorb_track_local_result)), o_as = out.add(sizeof(int) * ((size_t)nk + 1)),
            o_iv = out.add((size_t)np + 1), o_tr = out.add(sizeof(float) * 4 * ((size_t)np + 1)),
            o_lv = out.add(sizeof(int) * ((size_t)np + 1));
  LORB_TRY(out.alloc(true));
  const FieldsOut mir = {out.dev<uint8_t>(o_iv), out.dev<float>(o_tr), out.dev<int>(o_lv)};
  LORB_TRY(track_local_issue(ctx, frame, Tcw, pose_init, K, in.dev<float>(i_sp), &M, par, opt, o, mir, dassign,
                             out.dev<lorb_track_local_result>(o_rec), out.dev<int>(o_as)));
  LORB_TRY(out.fetch());
  if (np > 0) {
    // as the device form, only the fields of points in view are defined: the others are left as given
    const uint8_t* iv = out.host<uint8_t>(o_iv);
    const float* tr = out.host<float>(o_tr);
    const int* lv = out.host<int>(o_lv);
    memcpy(in_view, iv, (size_t)np);
    for (int m = 0; m < np; ++m)
      if (iv[m]) {
        for (int q = 0; q < 4; ++q) track[(size_t)q * np + m] = tr[(size_t)q * np + m];
        level[m] = lv[m];
      }
  }
  if (nk > 0) memcpy(assign, out.host<int>(o_as), sizeof(int) * nk);
  *result = *out.host<lorb_track_local_result>(o_rec);
  if (Tcw_out) {
    const float R[3] = {(float)result->pose[0], (float)result->pose[1], (float)result->pose[2]};
    const float T[3] = {(float)result->pose[3], (float)result->pose[4], (float)result->pose[5]};
    lorb_pose_to_Tcw(R, T, Tcw_out);
  }
  return LORB_OK;
}

// VisualOdometry::EstimatePoseLocal after UpdateLocalMap (src/visual_odometry.cpp:153-209) on a built
// frame whose count, pose and slots stay in device memory: k_local_head (status, pose hand-over,
// held-slot loop), then track_local_issue's launches in their device-count, device-pose forms over the
// caller's bounds (np = d_pts->n is a host value: k_local_head stores it where FrameCounts::last
// points, or -1 on a failing status), and the tail that also applies the codes to the slots.
// Launches: head + candidates + resolver + tail while np * n_max_cur <= kCandStrided and n_max_cur <=
// kStageKps; the grid build is added past kStageKps, the count / scan / write sequence replaces the
// one candidate pass past kCandStrided.
int lorb_track_local_frames_dev(lorb_ctx* ctx, const lorb_frame_params* frame, const lorb_frame_out* d_cur,
                                int32_t n_max_cur, const lorb_frame_slots* d_cur_slots, int32_t* d_cur_slot_id,
                                const double* d_pose, const int32_t* d_src_status,
                                const lorb_track_local_id_source* ids, const lorb_map_points_dev* d_pts,
                                const lorb_track_local_params* par, const lorb_lm_options* opt, uint8_t* d_in_view,
                                float* d_track, int32_t* d_level, int32_t* d_assign,
                                lorb_track_local_frames_result* d_result) {
  if (!ctx || !frame || !d_cur || !d_cur_slots || !d_cur_slot_id || !d_pose || !d_pts || !par || !opt || !d_in_view ||
      !d_track || !d_level || !d_assign || !d_result)
    return LORB_E_INVALID;
  const int nk = n_max_cur, np = d_pts->n;
  if (nk < 1) return lorb::set_error(ctx, LORB_E_INVALID, "bound %d must be positive", nk);
  if (np < 0) return lorb::set_error(ctx, LORB_E_INVALID, "negative sizes");
  // a5's candidate list is allocated from the bounds: past this it would need the total read back
  if ((int64_t)np * (int64_t)nk > (int64_t(8) << 20))
    return lorb::set_error(ctx, LORB_E_INVALID, "%d points x bound %d exceed the asynchronous limit of 8M candidates", np,
                           nk);
  if (frame->n_levels < 1 || frame->n_levels > LORB_MAX_LEVELS)
    return lorb::set_error(ctx, LORB_E_INVALID, "n_levels %d out of range", frame->n_levels);
  if (par->min_matches < 0) return lorb::set_error(ctx, LORB_E_INVALID, "min_matches %d is negative", par->min_matches);
  if (d_pts->in_frame) return lorb::set_error(ctx, LORB_E_INVALID, "d_pts->in_frame must be NULL: the call derives it");
  if (!d_cur->counts || !d_cur->left.x || !d_cur->left.y || !d_cur->left.octave || !d_cur->left.angle ||
      !d_cur->left.desc || !d_cur->u_right || !slots_ok(d_cur_slots) ||
      (ids && (!ids->d_motion_assign || !ids->d_motion_result || !ids->d_last_slot_id || ids->n_max_last < 1)) ||
      (np > 0 && (!d_pts->pos || !d_pts->normal || !d_pts->max_dist || !d_pts->min_dist || !d_pts->desc || !d_pts->locked)))
    return lorb::set_error(ctx, LORB_E_INVALID, "null array");
  int* nm;
  float* list;
  lorb::LocalPose* blk;
  uint8_t* in_frame;
  LORB_TRY(lorb::scratch_t(ctx, slot<S_TLC, 0>(), 1, &nm));
  LORB_TRY(lorb::scratch_t(ctx, slot<S_TLC, 1>(), (size_t)nk * 5, &list));
  LORB_TRY(lorb::scratch_t(ctx, slot<S_TLF, 0>(), 1, &blk));
  LORB_TRY(lorb::scratch_t(ctx, slot<S_TLF, 1>(), (size_t)std::max(np, 1), &in_frame));
  LocalHead h{};
  h.count = d_cur->counts; h.n_max = nk; h.np = np; h.src_status = d_src_status; h.pose = d_pose;
  h.state = d_cur_slots->state; h.slot_id = d_cur_slot_id; h.is_bad = d_pts->is_bad; h.in_frame = in_frame;
  h.blk = blk; h.rec = d_result;
  if (ids) {
    h.motion_assign = ids->d_motion_assign; h.motion_rec = ids->d_motion_result; h.last_slot_id = ids->d_last_slot_id;
    h.n_max_last = ids->n_max_last; h.given = ids->cur_slots_given != 0;
  }
  hipLaunchKernelGGL(k_local_head, dim3(1), dim3(1024), 0, ctx->stream, h);
  LORB_CHECK_LAUNCH(ctx);
  const lorb::FrameCounts dc = {&blk->np, d_cur->counts, np, nk};
  KpDev K;
  K.x = d_cur->left.x; K.y = d_cur->left.y; K.angle = d_cur->left.angle; K.uR = d_cur->u_right;
  K.octave = d_cur->left.octave; K.desc = reinterpret_cast<const uint4*>(d_cur->left.desc);
  K.slot_state = d_cur_slots->state;
  K.cell_off = nullptr; K.cell_idx = nullptr; K.n = nk;
  FrustumIn F{};  // T and Ow stay zero: the device form reads them from blk
  F.pos = d_pts->pos; F.nrm = d_pts->normal; F.maxd = d_pts->max_dist; F.mind = d_pts->min_dist;
  F.skip_a = in_frame; F.skip_b = d_pts->is_bad;
  F.cos_limit = par->viewing_cos_limit;
  WinParams P{};
  P.fp = *frame;
  P.th = par->th;
  const FieldsOut o = {d_in_view, d_track, d_level};
  const uint4* pdesc = reinterpret_cast<const uint4*>(d_pts->desc);
  const LocalDev Q = {np, d_in_view, d_pts->is_bad, d_pts->locked, d_track, d_track + np, d_track + 2 * np,
                      d_track + 3 * np, d_level, pdesc};
  LORB_TRY(search_issue<0>(
      ctx, &K, P.fp, np, d_pts->locked, nullptr, {d_assign, nm, nullptr, nullptr, 0},
      [&](auto pass, unsigned g, int* cnt, const int* off, int2* cand, int stride) {
        using Pass = decltype(pass);
        if (off)
          hipLaunchKernelGGL(k_cand_local_dc, dim3(g), dim3(256), 0, ctx->stream, K, P, np, Q.iv, Q.bad, Q.px, Q.py,
                             Q.pxr, Q.pl, Q.vc, Q.pd, cnt, off, cand, stride, dc);
        else
          hipLaunchKernelGGL((k_cand_local_fr_dc<Pass::write, Pass::grid>), dim3(g), dim3(256), 0, ctx->stream, K, P, np, F,
                             o, pdesc, cnt, cand, stride, (const lorb::LocalPose*)blk, dc);
      },
      &dc));
  lorb::LocalTail t{};
  t.nk = nk; t.np = np; t.nm = nm; t.assign = d_assign; t.in_view = d_in_view;
  t.slot_state = d_cur_slots->state; t.slot_pos = d_cur_slots->pos; t.pt_pos = d_pts->pos; t.x = K.x; t.y = K.y;
  t.min_matches = par->min_matches;
  t.fx = frame->fx; t.fy_eff = par->fy_eff; t.cx = frame->cx; t.cy = frame->cy;
  t.list = list; t.rec = &d_result->local; t.assign_out = nullptr;
  lorb::LocalFramesTail f{};
  f.dc = dc; f.pose = blk; f.cur = *d_cur_slots; f.slot_id = d_cur_slot_id;
  f.pt_locked = d_pts->locked; f.pt_desc = d_pts->desc; f.rec = d_result;
  return lorb::launch_local_frames_tail(ctx, t, f, opt);
}

int lorb_unproject_stereo_dev(lorb_ctx* ctx, const lorb_frame_params* frame, const float Tcw[16], int32_t n,
                              const float* d_x, const float* d_y, const float* d_depth, float* d_out) {
  if (!ctx || !frame || !Tcw) return LORB_E_INVALID;
  if (n <= 0) return LORB_OK;
  float Twc[16];
  inv4_lu32f(Tcw, Twc);
  lorb::Mat4f T;
  memcpy(T.v, Twc, sizeof(T.v));
  hipLaunchKernelGGL(k_unproject, dim3(lorb::ceil_div(n, 256)), dim3(256), 0, ctx->stream, *frame, T, n, d_x, d_y,
                     d_depth, d_out);
  LORB_CHECK_LAUNCH(ctx);
  return LORB_OK;
}

int lorb_unproject_stereo(lorb_ctx* ctx, const lorb_frame_params* frame, const float Tcw[16], int32_t n,
                          const float* x, const float* y, const float* depth, float* out_xyz) {
  if (!ctx || !frame || !Tcw) return LORB_E_INVALID;
  if (n <= 0) return LORB_OK;
  float Twc[16];
  inv4_lu32f(Tcw, Twc);
  float *dx, *dy, *dd, *o;
  lorb::Mat4f T;
  memcpy(T.v, Twc, sizeof(T.v));
  LORB_TRY(lorb::upload_t(ctx, S_W1, x, n, &dx));
  LORB_TRY(lorb::upload_t(ctx, S_W2, y, n, &dy));
  LORB_TRY(lorb::upload_t(ctx, S_W3, depth, n, &dd));
  LORB_TRY(lorb::scratch_t(ctx, S_W4, (size_t)n * 3, &o));
  hipLaunchKernelGGL(k_unproject, dim3(lorb::ceil_div(n, 256)), dim3(256), 0, ctx->stream, *frame, T, n, dx, dy, dd, o);
  LORB_CHECK_LAUNCH(ctx);
  LORB_HIP(ctx, hipMemcpyAsync(out_xyz, o, sizeof(float) * 3 * n, hipMemcpyDeviceToHost, ctx->stream));
  LORB_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return LORB_OK;
}

}  // extern "C"
