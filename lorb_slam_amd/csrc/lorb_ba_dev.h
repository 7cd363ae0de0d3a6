// lorb_ba_dev.h -- device-side types and inline helpers shared by the bundle-adjustment units
// (lorb_ba.hip, lorb_ba_build.hip, lorb_ba_chol.hip): the structs the kernels take as arguments,
// the wave / block reductions, the small index helpers, the iteration head that both k_ba_lm_begin
// and the fused Cholesky run, the Cholesky's LDS sizes and the Cholesky unit's host launchers.
//
// Included after the unit's `#pragma clang fp contract(fast)` block (see lorb_ba.hip), so the inline
// device code here is compiled under the including unit's contraction setting.
#pragma once
#include "lorb_ba_math.h"
#include "lorb_internal.h"

namespace lorb {
namespace ba {

constexpr int kGB = 256;  // observations per point group (one workgroup), see K1

struct BaWin {
  int pose_base, n_poses, point_base, n_points;
  int pblk_base, n_pblk;
  int env_base, env_size, n, row_base, bw;  // S band: row i holds cols [i-bw, i]
  int obs_base, n_obs;
  int n_obs_all;  // observations of the window over all ranks (== n_obs unless sharded)
  // point-major path: the window's group partials start at part_base, part_stride doubles per group
  // (camera terms at part_cam within it); bwc = the camera-level half band
  int part_stride, part_cam, bwc, pad_;
  // partial runs ("super-groups"): F consecutive point groups of the window processed by one
  // k_ba_ls workgroup into ONE partial (F = 1: one per group); super-groups [sg_base, sg_base + n_sg)
  int sg_base, n_sg;
  long long part_base;
  double fx, fy, cx, cy;
};
struct PBlk { int win, p0, cnt, o0, no; };  // point group: points [p0, p0+cnt), obs [o0, o0+no)
struct BlockPair { int win, ch, cl, off, cnt; };  // global camera indices, pair list range
struct WinState {
  double radius, decrease_factor, cost, x_norm, gmax, initial_cost;
  int iter, n_success, n_invalid, done, relin, cur, last_successful, term, chol_fail, pad;
};
struct LMOpt {
  int max_iter, max_invalid, jacobi;
  double ftol, gtol, ptol, init_radius, max_radius, min_radius, min_rel, min_diag, max_diag;
};

// Wave reductions, butterfly xor 32, 16, 8, 4, 2, 1, with no LDS traffic.  The cross-row steps
// use gfx950's v_permlane32_swap / v_permlane16_swap on two copies of the value: afterwards lane i
// holds {v_i, v_(i^32)} (resp. i^16) across the two copies.  The in-row steps are DPP moves:
// row_ror:8 is xor 8 within a 16-lane row, and once lanes i and i^8 agree row_ror:4 delivers the
// xor-4 partner's value; quad_perm does xor 2 and xor 1.  Every step combines a lane and its
// partner with a commutative op, so all lanes end with the bits of the plain shuffle butterfly.
template <int CTRL>
__device__ __forceinline__ double dpp_d(double v) {
  const unsigned long long u = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_mov_dpp((int)(u & 0xffffffffu), CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_mov_dpp((int)(u >> 32), CTRL, 0xF, 0xF, false);
  return __longlong_as_double(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}
// {v_i, v_partner} for partner i^32 (W32) or i^16
template <bool W32>
__device__ __forceinline__ void xrow_pair(double v, double& a, double& b) {
  const unsigned long long u = __double_as_longlong(v);
  const unsigned lo = (unsigned)(u & 0xffffffffu), hi = (unsigned)(u >> 32);
  const auto l = W32 ? __builtin_amdgcn_permlane32_swap(lo, lo, false, false)
                     : __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
  const auto h = W32 ? __builtin_amdgcn_permlane32_swap(hi, hi, false, false)
                     : __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
  a = __longlong_as_double(((unsigned long long)h[0] << 32) | l[0]);
  b = __longlong_as_double(((unsigned long long)h[1] << 32) | l[1]);
}
__device__ __forceinline__ double wave_sum(double v) {
  double a, b;
  xrow_pair<true>(v, a, b); v = a + b;
  xrow_pair<false>(v, a, b); v = a + b;
  v += dpp_d<0x128>(v);  // row_ror:8
  v += dpp_d<0x124>(v);  // row_ror:4
  v += dpp_d<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_d<0xB1>(v);   // quad_perm [1,0,3,2]
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
  double a, b;
  xrow_pair<true>(v, a, b); v = fmax(a, b);
  xrow_pair<false>(v, a, b); v = fmax(a, b);
  v = fmax(v, dpp_d<0x128>(v));
  v = fmax(v, dpp_d<0x124>(v));
  v = fmax(v, dpp_d<0x4E>(v));
  v = fmax(v, dpp_d<0xB1>(v));
  return v;
}
// Reduce-scatter of N <= 32 per-lane values (padded to 32): each step halves the values a lane
// keeps -- the half its partner does not keep goes to the partner, which adds it to its own copy --
// so 32 sums cost 31 exchanges instead of 32 full butterflies.  Partners: lane ^ 32, ^ 16
// (permlane swaps of two different registers), ^ 8 (row_ror:8), the mirrored lane of the half row
// (row_half_mirror: the other quad), ^ 2; a last ^ 1 step completes every sum, and sum k ends in
// lanes 2k, 2k + 1, from where v_readlane broadcasts it.  Every lane returns all N sums.
__device__ __forceinline__ double readlane_d(double v, int l);
__device__ __forceinline__ void swap_pair(double x, double y, bool w32, double& r0, double& r1) {
  const unsigned long long ux = __double_as_longlong(x), uy = __double_as_longlong(y);
  const unsigned xl = (unsigned)ux, xh = (unsigned)(ux >> 32), yl = (unsigned)uy, yh = (unsigned)(uy >> 32);
  const auto l = w32 ? __builtin_amdgcn_permlane32_swap(xl, yl, false, false)
                     : __builtin_amdgcn_permlane16_swap(xl, yl, false, false);
  const auto h = w32 ? __builtin_amdgcn_permlane32_swap(xh, yh, false, false)
                     : __builtin_amdgcn_permlane16_swap(xh, yh, false, false);
  r0 = __longlong_as_double(((unsigned long long)h[0] << 32) | l[0]);
  r1 = __longlong_as_double(((unsigned long long)h[1] << 32) | l[1]);
}
template <int CTRL, int BIT, int H>
__device__ __forceinline__ void rs_dpp_step(double (&v)[32], int lane) {
  const bool up = (lane >> BIT) & 1;
#pragma unroll
  for (int k = 0; k < H; ++k) {
    const double keep = up ? v[k + H] : v[k], send = up ? v[k] : v[k + H];
    v[k] = keep + dpp_d<CTRL>(send);
  }
}
// in place: v[0 .. N) in, the N sums out in every lane (v[N .. 32) are scratch)
template <int N>
__device__ __forceinline__ void wave_sum_all(double (&v)[32]) {
  static_assert(N <= 32, "at most 32 values");
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int k = N; k < 32; ++k) v[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {  // ^32: lanes < 32 keep k, lanes >= 32 keep k + 16
    double a, b;
    swap_pair(v[k], v[k + 16], true, a, b);
    v[k] = a + b;
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {   // ^16 (rows of 16): even rows keep k, odd rows k + 8
    double a, b;
    swap_pair(v[k], v[k + 8], false, a, b);
    v[k] = a + b;
  }
  rs_dpp_step<0x128, 3, 4>(v, lane);  // row_ror:8 = ^8
  rs_dpp_step<0x141, 2, 2>(v, lane);  // row_half_mirror: the other quad of the half row
  rs_dpp_step<0x4E, 1, 1>(v, lane);   // quad_perm [2,3,0,1] = ^2
  v[0] += dpp_d<0xB1>(v[0]);          // quad_perm [1,0,3,2] = ^1
  // lane l now holds sum (16 b5 + 8 b4 + 4 b3 + 2 b2 + b1) = l >> 1
  const double r = v[0];
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = readlane_d(r, 2 * k);
}
template <int N>
__device__ __forceinline__ void block_sum(double (&v)[N], double* sh /* [N*256] */) {
  // deterministic fixed tree over a 256-thread block
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < N; ++k) sh[k * 256 + t] = v[k];
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int k = 0; k < N; ++k) sh[k * 256 + t] += sh[k * 256 + t + s];
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = sh[k * 256];
  __syncthreads();
}

// sym 3x3 packed (xx,xy,xz,yy,yz,zz) inverse via Cholesky; returns false if not PD
__device__ __forceinline__ bool inv3(const double a[6], double inv[6]) {
  const double l00 = a[0];
  if (!(l00 > 0.0)) return false;
  const double L00 = sqrt(l00);
  const double L10 = a[1] / L00, L20 = a[2] / L00;
  const double d1 = a[3] - L10 * L10;
  if (!(d1 > 0.0)) return false;
  const double L11 = sqrt(d1);
  const double L21 = (a[4] - L20 * L10) / L11;
  const double d2 = a[5] - L20 * L20 - L21 * L21;
  if (!(d2 > 0.0)) return false;
  const double L22 = sqrt(d2);
  // inverse of L (lower)
  const double i00 = 1.0 / L00, i11 = 1.0 / L11, i22 = 1.0 / L22;
  const double i10 = -L10 * i00 * i11;
  const double i21 = -L21 * i11 * i22;
  const double i20 = -(L20 * i00 + L21 * i10) * i22;
  // A^-1 = Li^T Li
  inv[0] = i00 * i00 + i10 * i10 + i20 * i20;
  inv[1] = i10 * i11 + i20 * i21;
  inv[2] = i20 * i22;
  inv[3] = i11 * i11 + i21 * i21;
  inv[4] = i21 * i22;
  inv[5] = i22 * i22;
  return true;
}
__device__ __forceinline__ double s3(const double m[6], int a, int b) {
  if (a > b) { const int t = a; a = b; b = t; }
  return m[a * 3 - (a * (a - 1)) / 2 + (b - a)];  // packed (xx,xy,xz,yy,yz,zz)
}

// ------------------------------------------------------------------------------------------
struct BaDev {
  lorb::RotJet* rot_lin;           // 2 x rot_stride: rotation state (with d/daa) of x_pose[k] at k rot_stride
                                   // (rot_off): k = 0 by k_ba_init, cur ^ 1 by the Cholesky's epilogue with
                                   // the candidate pose (one array: the kernels index it as they did one buffer)
  lorb::RotVal* rot_cand;          // Ctot: rotation state of the candidate pose x_pose[cur ^ 1]
  lorb::RotJet* rot_fix;           // NF: rotation states of the fixed poses (k_ba_init; they never change)
  lorb::RotVal* rotv_fix;          // NF: the same, value only (the candidate cost)
  const BaWin* win;
  const PBlk* pblk;
  const int* obs_pt;         // K  (global point of each observation)
  const BlockPair* bp;
  const int* pt_obs_off;     // Ptot+1
  const int* obs_cam;        // K  (global optimised camera or -1)
  const int* obs_fix;        // K  (global fixed pose or -1)
  const double2* obs_uv;     // K
  const double* fixed_pose;  // NF*6
  double* x_init_pose;       // Ctot*6 (initial values, never written)
  double* x_init_pt;         // Ptot*3
  double* x_pose[2];         // Ctot*6
  double* x_pt[2];           // Ptot*3
  double* scale_pose;        // Ctot*6
  double* scale_pt;          // Ptot*3
  double* etb;               // Ptot*3 (unscaled)
  double* pinv;              // Ptot*6
  double* U;                 // Ctot*21 (unscaled, packed upper row-major)
  double* V;                 // Ctot*6
  double* env;               // S envelopes (all-reduced when sharded)
  double* rhs;               // sum n
  // sharded plans: kernels write the *_part buffers, the all-reduce produces the
  // global ones (unsharded: *_part == global).  Contiguous per exchange:
  //   lin   [U | V | wlin (2W: cost, point |x|^2)]  sum;   wmax (W: point gradient max)  max
  //   solve [env | rhs | wfail (W)]                 sum
  //   step  wstep (3W: model cost change, candidate cost, point |step|^2)  sum
  double *U_part, *V_part, *wlin, *wlin_part, *wmax, *wmax_part;
  double *env_part, *rhs_part, *wfail, *wfail_part, *wstep, *wstep_part;
  const int* cam_active;     // Ctot: camera observed by some rank
  int sharded, rank0;
  double* ycam;              // sum n (solution, scaled space, y = -step)
  double* part;              // n_pblk * 8 partials
  unsigned long long* dbg;   // diagnostic stamps (LORB_LS_STAMPS and LORB_CHOL_TRACE builds only)
  double* kco;               // k_ba_chol_2s back-substitution operators: per window
                             // ((row_base >> 4) + w) * 1024 doubles, top side's blocks then the
                             // bottom side's, [block][16][64] (BandSide::bsk_block)
  WinState* st;
  // The folded iteration tail (k_ba_ls<FOLD>): the window's first point group stores the state it
  // decided to st2 (the other groups of that launch still read the undecided st); k_ba_red and the
  // Cholesky's head of that iteration read st2 (fold != 0 in their copy of BaDev), the head stores
  // to st again.  ls_fail: a point block of that linearisation was not invertible (st.chol_fail
  // is an input of the same launch); the head moves it into st.chol_fail and clears it.
  WinState* st2;
  int* ls_fail;
  int fold;  // 0; 1 a folding iteration; 2 of a plan of one window
  int rot_stride;
  // partials (k_ba_ls -> k_ba_red), per super-group (its first camera - pose_base, camera span)
  double* gpart;
  int2* gspan;
  const int4* sgrp;          // per super-group: window, first point group, point groups
  lorb_lm_iteration* trace;  // per window LORB_LM_TRACE_CAP records (lm_decide)
  // [0] point groups, [1] block pairs, [2] super-groups in use.  Launch grids may be larger (device-built plans
  // launch at capacity so that the captured LM graph survives a rebuild); the extra workgroups exit.
  const int* live;
};

__device__ __forceinline__ int u21(int a, int b) {  // packed upper index of 6x6 sym
  if (a > b) { const int t = a; a = b; b = t; }
  return a * 6 - (a * (a - 1)) / 2 + (b - a);
}

// first entry of x_pose[k]'s rotation states in rot_lin
__device__ __forceinline__ int rot_off(const BaDev& d, int k) { return k ? d.rot_stride : 0; }

// broadcast lane `l` (wave-uniform) of a double through two v_readlane_b32
__device__ __forceinline__ double readlane_d(double v, int l) {
  const unsigned long long u = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)(u & 0xffffffffu), l);
  const int hi = __builtin_amdgcn_readlane((int)(u >> 32), l);
  return __longlong_as_double(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}

// entry (i, j), j in [i - bw, i], of a band stored row by row
__device__ __forceinline__ double& band(double* A, int bw, int i, int j) {
  return A[(size_t)i * (bw + 1) + (j - i + bw)];
}
// slot of block (a, a - dd) of a point group's camera window ("Point-major Schur path", lorb_ba.hip); a window's slots
__host__ __device__ __forceinline__ int pm_slot(int a, int dd, int bwc) {
  return a <= bwc ? a * (a + 1) / 2 + dd : (bwc + 1) * (bwc + 2) / 2 + (a - bwc - 1) * (bwc + 1) + dd;
}
__host__ __device__ __forceinline__ int pm_nslots(int span, int bwc) {
  return span <= 0 ? 0 : pm_slot(span - 1, span - 1 < bwc ? span - 1 : bwc, bwc) + 1;
}

// v_rsq_f64 is accurate to about 2^-22 relative; each Newton step squares the error.  Two steps
// reach full double precision; LORB_RSQ_STEPS=1 stops at ~1e-14.
#ifndef LORB_RSQ_STEPS
#define LORB_RSQ_STEPS 2
#endif
__device__ __forceinline__ double rsqrt_refined(double a) {
  double y = __builtin_amdgcn_rsq(a);
#pragma unroll
  for (int s = 0; s < LORB_RSQ_STEPS; ++s) {
    const double e = fma(-a * y, y, 1.0);
    y = fma(0.5 * y, e, y);
  }
  return y;
}

// Lane-strided partial sums over a window's point groups (b = lane, lane + 64, ... in that order,
// the per-lane order of a plain loop) with the loads of kPU groups issued before any is added: the
// partials come from the previous kernel (another XCD's L2), so a load-add loop pays one memory
// round trip per step.  F0..F2 pick the fields; M1: field 1 is a max.
template <int F0, int F1, int F2, bool M1>
__device__ __forceinline__ void group_partials(const double* __restrict__ part, int base, int n, int lane,
                                               double& a, double& b, double& c) {
  constexpr int kPU = 8;
  for (int b0 = lane; b0 < n; b0 += 64 * kPU) {
    double v0[kPU], v1[kPU], v2[kPU];
#pragma unroll
    for (int u = 0; u < kPU; ++u) {
      const int g = b0 + 64 * u;
      const double* P = part + 8 * (base + (g < n ? g : 0));
      v0[u] = P[F0]; v1[u] = P[F1]; v2[u] = P[F2];
    }
#pragma unroll
    for (int u = 0; u < kPU; ++u)
      if (b0 + 64 * u < n) {
        a += v0[u];
        b = M1 ? fmax(b, v1[u]) : b + v1[u];
        c += v2[u];
      }
  }
}

// K3: per-window iteration head: finalise the (re)linearisation, termination checks
// Camera terms (gradient max, |x|^2, iteration-0 Jacobi scale) come from the (all-reduced)
// U / V blocks; point terms from the point-group partials (SH: from the exchange buffers).
// One wavefront; returns the state after the head (lane 0 has stored it).  k_ba_lm_begin runs it
// as a kernel; the fused iteration runs it on an otherwise idle wave of the Cholesky (lm_head).
template <bool SH>
__device__ __forceinline__ WinState lm_head(const BaDev& d, const LMOpt& o, int w, int lane, WinState S, const BaWin& W) {
  if (S.relin) {
    // fixed lane assignment + fixed butterfly => deterministic
    double cost = 0.0, gm = 0.0, xn2 = 0.0;
    if (!SH) group_partials<0, 1, 2, true>(d.part, W.pblk_base, W.n_pblk, lane, cost, gm, xn2);
    const int cur = S.cur;
    for (int c = W.pose_base + lane; c < W.pose_base + W.n_poses; c += 64) {
      if (S.iter == 0) {
        const int dg[6] = {0, 6, 11, 15, 18, 20};
        for (int k = 0; k < 6; ++k) d.scale_pose[6 * c + k] = 1.0 / (1.0 + sqrt(d.U[21 * c + dg[k]]));
      }
      if (!d.cam_active[c]) continue;
      for (int k = 0; k < 6; ++k) {
        const double x = d.x_pose[cur][6 * c + k];
        gm = fmax(gm, fabs(x - (x + -d.V[6 * c + k])));
        xn2 += x * x;
      }
    }
    cost = wave_sum(cost); gm = wave_max(gm); xn2 = wave_sum(xn2);
    if (SH) { cost += d.wlin[2 * w]; xn2 += d.wlin[2 * w + 1]; gm = fmax(gm, d.wmax[w]); }
    S.cost = cost;
    S.gmax = gm;
    S.x_norm = sqrt(xn2);
    if (S.iter == 0) S.initial_cost = cost;
    S.last_successful = 1;
    S.relin = 0;
  }
  if (lane == 0) {
    if (S.iter >= o.max_iter) { S.done = 1; S.term = LORB_TERM_NO_CONVERGENCE; }
    else if (S.last_successful && S.gmax <= o.gtol) { S.done = 1; S.term = LORB_TERM_GRADIENT_TOL; }
    else if (S.radius <= o.min_radius) { S.done = 1; S.term = LORB_TERM_MIN_RADIUS; }
    else S.iter++;
    d.st[w] = S;
  }
  return S;
}

// LDS words of k_ba_chol_2s: band (n16 rows), both sides' rhs (n16 + 48), two 64 x 18 exchanges
// (together the 48 x 48 combine), zX (48), two 64 x 17 panel hand-off buffers, a zero word
__host__ __device__ constexpr int chol2s_words(int n16, int bw) {
  return n16 * (bw + 1) + (n16 + 48) + 2 * 64 * 18 + 48 + 2 * 64 * 17 + 2;
}
// LDS words a plan reserves for a band (max_env_w): the largest of the one-sided K6w (band + z + invd +
// exchange), the two-sided K6t ((n16 + 48) band rows, z, invd, two exchanges, zX) and k_ba_chol_2s
constexpr int chol_lds_words(int n16, int bw) {
  const int w1 = n16 * (bw + 1) + 2 * n16 + 64 * 18, w2 = (n16 + 48) * (bw + 2) + 2 * 64 * 18 + 48;
  const int w3 = chol2s_words(n16, bw);
  return w1 > w2 ? (w1 > w3 ? w1 : w3) : (w2 > w3 ? w2 : w3);
}

// ==========================================================================================
// Plan groups (lorb_ba_group_*): the LM solves of up to kGrpMax plans -- the device-built plans of
// several LocalMapping windows -- launched as ONE set of kernels on one stream, the way a plan of
// several windows is.  Each launch deals its workgroups to the member plans by a block prefix
// (GrpGrid); a workgroup runs the one-plan kernel's code on its member's BaDev (kernel arguments),
// so every member's results are bit-identical to its own solve (the block-pair sums do not depend
// on the k_ba_red width, k_ba_red's note).
// ==========================================================================================
constexpr int kGrpMax = 4;
struct BaGrp {
  BaDev d[kGrpMax];
  int n;
};
struct GrpGrid {
  int pre[kGrpMax + 1];  // workgroups of members [0, k); pre[n] = the launch's workgroups
};
struct GrpInit {  // k_ba_init's per-plan arguments
  int W[kGrpMax], ctot[kGrpMax], n_pt[kGrpMax], nf[kGrpMax];
};
// the member running workgroup b, and b's index in that member's own launch (members without
// workgroups in this launch are skipped: the last member whose prefix is <= b)
__device__ __forceinline__ int grp_member(const GrpGrid& G, int n, unsigned b, unsigned& lb) {
  int k = 0;
#pragma unroll
  for (int i = 1; i < kGrpMax; ++i) k += (i < n && (int)b >= G.pre[i]) ? 1 : 0;
  lb = b - (unsigned)G.pre[k];
  return k;
}

// ------------------------------------------------------------------------------------------
// Host launchers of lorb_ba_chol.hip (a kernel is launched from the unit that defines it).

// LDS a Cholesky workgroup may take
constexpr int kLdsBudget = 160 * 1024 - 2048;
// what the Cholesky launch needs of a plan: windows, doubles of the widest window's band in
// k_ba_chol's layout (max_env) and in k_ba_chol_w / _2s's (max_env_w), widest band
struct CholShape { int W, max_env, max_env_w, max_bw; };
// kind (chol_kind_of): 2 k_ba_chol_2s (head: <true>, the fused iteration), 1 k_ba_chol_w,
// 0 k_ba_chol<in LDS or not, panel rows per lane>
void launch_chol(int kind, const CholShape& sh, hipStream_t s, const BaDev& d, const LMOpt& o, bool head);
// k_ba_chol_2s_g, G.pre[g.n] workgroups dealt to the group's members; lds: bytes of the widest band
void launch_chol_2s_g(hipStream_t s, const BaGrp& g, const GrpGrid& G, const LMOpt& o, bool head, size_t lds);

}  // namespace ba
}  // namespace lorb
