// lorb_ba_chol.hip -- band Cholesky of the reduced camera system with the forward / back
// substitution, one workgroup per window.  Three kernels, each for a band shape the others refuse
// (chol_kind_of in lorb_ba.hip picks by the plan's band): k_ba_chol (any band, panel in registers, band in LDS or global), k_ba_chol_w
// (band <= 48, one wave) and k_ba_chol_2s (two-sided, band >= 15 and >= 128 rows; the fused
// iteration runs the LM head inside it), plus k_ba_chol_2s_g for plan groups.
//
// FP64 contraction as in every BA unit, before any include (lorb_ba.hip's header says why): the
// inline device code of lorb_ba_math.h and lorb_ba_dev.h is compiled under it.
#ifndef LORB_NO_CONTRACT  // A/B builds only (tools/isa_fma.py, tools/build_variant.sh nofma -DLORB_NO_CONTRACT)
#pragma clang fp contract(fast)
#endif
#include "lorb_ba_math.h"
#include "lorb_internal.h"
#include "lorb_ba_dev.h"

namespace {

using namespace lorb::ba;

// The second pass of k_ba_chol's and k_ba_chol_w's epilogues: the linearisation state of candidate
// camera c, which its own thread has just stored to x_pose[k], into rot_lin[k] (k = cur ^ 1; an
// accepted step then only flips cur).  A pass of its own: rot_jet beside rot_val in one block would
// share subexpressions with it, and the candidate's rot_val must stay the code it is.  (k_ba_chol_2s
// forms these states on other threads, beside the candidates' pass.)
__device__ __forceinline__ void rot_lin_of(const BaDev& d, int k, int c) {
  double x[6];
#pragma unroll
  for (int q = 0; q < 6; ++q) x[q] = d.x_pose[k][6 * c + q];
  d.rot_lin[rot_off(d, k) + c] = lorb::rot_jet(x);
}

typedef double v4d __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void wave_sync_lds() {
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
  __builtin_amdgcn_wave_barrier();
}

// K6: banded Cholesky of S + forward/back substitution; one 256-thread workgroup per window.
// Right-looking with panel width NB.  Wave 0 factors the panel entirely in registers (lane l
// owns panel rows kb+l+64r, r < RPL; the pivot column is broadcast with v_readlane), with the
// forward substitution fused in; rsqrt-refined pivots keep IEEE div/sqrt off the critical
// path.  All four waves then apply the rank-NB trailing update from LDS.
constexpr int NB = 16;

// One 16x16 tile (I, J) of the panel's trailing update (SYRK): A(i, j) -= sum_k L(i, k) L(j, k)
// for ke <= j <= i <= rlast, k in [kb, kb + NB), on v_mfma_f64_16x16x4f64 (K = NB = 4 MFMAs).
// Operand lane l holds row (l & 15), k = l >> 4; accumulator register r holds row
// 4r + (l >> 4), column l & 15.  Entries outside the band / triangle are fed as 0 and never
// stored.
__device__ __forceinline__ void chol_trail_tile(double* A, int bw, int kb, int ke, int rlast,
                                                int I, int J, int lane) {
  if (16 * (I - J) - 15 > bw) return;  // tile entirely outside the band
  const int ci = lane & 15, ck = lane >> 4;
  const int i0 = ke + 16 * I, j0 = ke + 16 * J;
  v4d acc;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + ck + 4 * r, j = j0 + ci;
    const bool ok = i <= rlast && j <= i && i - j <= bw;
    const double v = band(A, bw, ok ? i : ke, ok ? j : ke);
    acc[r] = ok ? v : 0.0;
  }
#pragma unroll
  for (int kk = 0; kk < NB / 4; ++kk) {
    const int k = kb + 4 * kk + ck;
    const int ia = i0 + ci, jb = j0 + ci;
    const bool oka = ia <= rlast && ia - k <= bw, okb = jb <= rlast && jb - k <= bw;
    const double a = band(A, bw, oka ? ia : k, k), b = band(A, bw, okb ? jb : k, k);
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(oka ? -a : 0.0, okb ? b : 0.0, acc, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + ck + 4 * r, j = j0 + ci;
    if (i <= rlast && j <= i && i - j <= bw) band(A, bw, i, j) = acc[r];
  }
}

template <bool IN_LDS, int RPL>
__global__ __launch_bounds__(256) void k_ba_chol(BaDev d) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  __shared__ int s_fail;
  __shared__ __attribute__((aligned(16))) double s_col[80];
  __shared__ double s_l[NB][NB + 1], s_zk[NB], s_y[NB];  // a factored panel's diagonal block (extra rows)
  const int w = blockIdx.x;
  if (d.st[w].done) return;
  if (d.sharded && d.wfail[w] > 0.0) {  // a rank's point block was not PD: the step is invalid
    if (threadIdx.x == 0) d.st[w].chol_fail = 1;
    return;
  }
  const BaWin W = d.win[w];
  const int n = W.n, bw = W.bw;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  double *A, *z, *invd;
  if (IN_LDS) {
    A = smem;
    z = smem + (size_t)n * (bw + 1);
    invd = z + n;
    const double* src = d.env + W.env_base;
    for (int k = t; k < n * (bw + 1); k += 256) A[k] = src[k];
    for (int k = t; k < n; k += 256) z[k] = d.rhs[W.row_base + k];
  } else {
    A = d.env + W.env_base;
    z = d.rhs + W.row_base;
    invd = d.ycam + W.row_base;  // scratch, overwritten with the solution at the end
  }
  if (t == 0) s_fail = 0;
  __syncthreads();
  // Lookahead: panel p's trailing update is split into the tiles covering panel p+1's columns
  // (J = 0, all four waves, before panel p+1) and the rest (J >= 1), which waves 1-3 apply
  // while wave 0 factors panel p+1 -- they touch disjoint columns.
  int pkb = -1, pke = 0, prl = 0;  // previous panel (deferred tiles), pkb < 0: none
  for (int kb = 0; kb < n; kb += NB) {
    const int ke = min(kb + NB, n);
    const int rlast = min(n - 1, ke - 1 + bw);
    if (wv != 0 && pkb >= 0) {
      const int m = ((prl - pke + 1 + 15) >> 4) - 1;  // J >= 1 tiles: triangle of side m
      for (int tt = wv - 1; tt < m * (m + 1) / 2; tt += 3) {
        int I = 0;
        while ((I + 1) * (I + 2) / 2 <= tt) ++I;
        chol_trail_tile(A, bw, pkb, pke, prl, I + 1, tt - I * (I + 1) / 2 + 1, lane);
      }
    }
    if (wv == 0) {
      double P[RPL][NB], zr[RPL];
#pragma unroll
      for (int r = 0; r < RPL; ++r) {
        const int row = kb + lane + 64 * r;
        const bool vr = row <= rlast;
#pragma unroll
        for (int q = 0; q < NB; ++q) {
          const int col = kb + q;
          P[r][q] = (vr && col < ke && col <= row && row - col <= bw) ? band(A, bw, row, col) : 0.0;
        }
        zr[r] = vr ? z[row] : 0.0;
      }
      bool bad = false;
      if (ke - kb == NB) {
        // Full panel: one basic block (no per-column branches, pivots via v_readlane), so the
        // compiler can overlap column q+1's pivot chain with column q's bulk updates.  A
        // non-positive pivot turns into NaNs that are never stored: `bad` aborts below.
        // Lanes l < q hold finished or upper-triangle garbage in P[0][q..]; those entries are
        // never read as a pivot/head and never stored, so only z needs masking.
        double yq = 0.0;
#pragma unroll
        for (int q = 0; q < NB; ++q) {
          const double akk = readlane_d(P[0][q], q);
          bad |= !(akk > 0.0);
          const double y = rsqrt_refined(akk);
#pragma unroll
          for (int r = 0; r < RPL; ++r) P[r][q] *= y;  // lane q: akk * y = L(k, k)
          yq = lane == q ? y : yq;
          const double zk = readlane_d(zr[0], q) * y;
          zr[0] = lane > q ? fma(-P[0][q], zk, zr[0]) : (lane == q ? zk : zr[0]);
#pragma unroll
          for (int r = 1; r < RPL; ++r) zr[r] = fma(-P[r][q], zk, zr[r]);
#pragma unroll
          for (int q2 = q + 1; q2 < NB; ++q2) {
            const double l = readlane_d(P[0][q], q2);
#pragma unroll
            for (int r = 0; r < RPL; ++r) P[r][q2] = fma(-P[r][q], l, P[r][q2]);
          }
        }
        if (lane < NB) invd[kb + lane] = yq;
      } else {
#pragma unroll
      for (int q = 0; q < NB; ++q) {
        const int k = kb + q;
        if (k < ke && !bad) {
          const double akk = readlane_d(P[0][q], q);
          if (!(akk > 0.0)) {
            bad = true;
          } else {
            const double y = rsqrt_refined(akk);
#pragma unroll
            for (int r = 0; r < RPL; ++r) {
              const int row = kb + lane + 64 * r;
              if (row > k) P[r][q] *= y;
            }
            if (lane == q) { P[0][q] = akk * y; zr[0] *= y; invd[k] = y; s_col[64] = zr[0]; }
            // broadcast the column head L(kb+q2, k) and z_k through LDS (one write, wide reads)
            s_col[lane] = P[0][q];
            wave_sync_lds();
            const double zk = s_col[64];
            double l[NB];
#pragma unroll
            for (int q2 = q + 1; q2 < NB; ++q2) l[q2] = s_col[q2];
#pragma unroll
            for (int r = 0; r < RPL; ++r) {
              const int row = kb + lane + 64 * r;
              if (row > k) zr[r] -= P[r][q] * zk;
            }
#pragma unroll
            for (int q2 = q + 1; q2 < NB; ++q2) {
#pragma unroll
              for (int r = 0; r < RPL; ++r) {
                const int row = kb + lane + 64 * r;
                if (row >= kb + q2) P[r][q2] -= P[r][q] * l[q2];
              }
            }
            wave_sync_lds();  // all reads of s_col done before the next column overwrites it
          }
        }
      }
      }
#pragma unroll
      for (int r = 0; r < RPL; ++r) {
        const int row = kb + lane + 64 * r;
        if (row <= rlast) {
#pragma unroll
          for (int q = 0; q < NB; ++q) {
            const int col = kb + q;
            if (col < ke && col <= row && row - col <= bw) band(A, bw, row, col) = P[r][q];
          }
          z[row] = zr[r];
        }
      }
      // Rows below the register panel (bw + NB > 64 RPL: a dense window of more than ~80 cameras):
      // the panel's column operations replayed 64 rows at a time from its diagonal block (L(kb+q2,
      // kb+q) in lane q2's P[0][q], z_k in lane q's zr[0], 1 / L(k, k) in invd) -- per row the same
      // operations in the same order as a register row's.
      if (!bad && kb + 64 * RPL <= rlast) {
        const int nq = ke - kb;
        if (lane < NB) {
#pragma unroll
          for (int q = 0; q < NB; ++q) s_l[lane][q] = P[0][q];
          s_zk[lane] = zr[0];
          s_y[lane] = lane < nq ? invd[kb + lane] : 0.0;
        }
        wave_sync_lds();
        for (int r0 = kb + 64 * RPL; r0 <= rlast; r0 += 64) {
          const int row = r0 + lane;
          const bool vr = row <= rlast;
          double X[NB], zx = vr ? z[row] : 0.0;
#pragma unroll
          for (int q = 0; q < NB; ++q) X[q] = (vr && q < nq && row - (kb + q) <= bw) ? band(A, bw, row, kb + q) : 0.0;
#pragma unroll
          for (int q = 0; q < NB; ++q) {
            if (q < nq) {
              X[q] *= s_y[q];
              zx = fma(-X[q], s_zk[q], zx);
#pragma unroll
              for (int q2 = q + 1; q2 < NB; ++q2) X[q2] = fma(-X[q], s_l[q2][q], X[q2]);
            }
          }
          if (vr) {
#pragma unroll
            for (int q = 0; q < NB; ++q)
              if (q < nq && row - (kb + q) <= bw) band(A, bw, row, kb + q) = X[q];
            z[row] = zx;
          }
        }
        wave_sync_lds();
      }
      if (bad && lane == 0) s_fail = 1;
    }
    __syncthreads();
    if (s_fail) break;
    // trailing tiles over panel p+1's columns (J = 0); the rest is deferred (see above)
    {
      const int nt = (rlast - ke + 1 + 15) >> 4;
      for (int I = wv; I < nt; I += 4) chol_trail_tile(A, bw, kb, ke, rlast, I, 0, lane);
      pkb = kb; pke = ke; prl = rlast;
    }
    __syncthreads();
  }
  if (s_fail) {
    if (t == 0) d.st[w].chol_fail = 1;
    return;
  }
  // back substitution L^T y = z, 64-row register blocks from the bottom (wave 0)
  if (wv == 0) {
    for (int bb = ((n - 1) / 64) * 64; bb >= 0; bb -= 64) {
      const int row = bb + lane;
      const int be = min(n - 1, bb + 63);
      double zr = row < n ? z[row] : 0.0;
      // 8-row chunks: the chunk's L(k, row) and 1/L(k, k) are loaded before the serial
      // readlane chain so LDS/global latency is paid once per chunk, not once per row.
      constexpr int BC = 8;
      for (int k0 = be; k0 >= bb; k0 -= BC) {
        double lk[BC], iv[BC];
#pragma unroll
        for (int u = 0; u < BC; ++u) {
          const int k = max(k0 - u, bb);
          const bool ok = k0 - u >= bb && row < k && k - row <= bw;
          lk[u] = band(A, bw, k, ok ? row : k);
          lk[u] = ok ? lk[u] : 0.0;
          iv[u] = invd[k];
        }
#pragma unroll
        for (int u = 0; u < BC; ++u) {
          const int k = k0 - u;
          if (k >= bb) {
            const double yk = readlane_d(zr, k - bb) * iv[u];
            zr = lane == k - bb ? yk : fma(-lk[u], yk, zr);
          }
        }
      }
      if (row < n) z[row] = zr;
      wave_sync_lds();
      // rows above the block: z_i -= sum_k L(k, i) y_k, k in [bb, be], k - i <= bw
      for (int i = max(0, bb - bw) + lane; i < bb; i += 64) {
        double acc = 0.0;
        const int kend = min(be, i + bw);
        for (int k = bb; k <= kend; k += BC) {
          double a[BC], zk[BC];
#pragma unroll
          for (int u = 0; u < BC; ++u) {
            const int kk = min(k + u, kend);
            a[u] = band(A, bw, kk, i);
            zk[u] = z[kk];
          }
#pragma unroll
          for (int u = 0; u < BC; ++u) acc = fma(k + u <= kend ? a[u] : 0.0, zk[u], acc);
        }
        z[i] -= acc;
      }
      wave_sync_lds();
    }
  }
  __syncthreads();
  for (int k = t; k < n; k += 256) d.ycam[W.row_base + k] = z[k];
  // candidate cameras x + D^-1 delta (into x_pose[cur ^ 1]) and their rotation states
  {
    const int cur = d.st[w].cur;
    for (int ci = t; ci < W.n_poses; ci += 256) {
      const int c = W.pose_base + ci;
      double xn[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        xn[k] = d.x_pose[cur][6 * c + k] + (-z[6 * ci + k]) * d.scale_pose[6 * c + k];
        d.x_pose[cur ^ 1][6 * c + k] = xn[k];
      }
      d.rot_cand[c] = lorb::rot_val(xn);
    }
    for (int ci = t; ci < W.n_poses; ci += 256) rot_lin_of(d, cur ^ 1, W.pose_base + ci);
  }
}

// K6w: banded Cholesky for band <= 48 on ONE wavefront per window, no workgroup barrier.
// The active 64 x 64 trailing window (rows/cols kb .. kb+63) lives in registers as ten 16 x 16
// tiles (I, J), J <= I < 4, in the v_mfma_f64_16x16x4f64 accumulator layout (register r of
// lane l: row 4r + (l >> 4), column l & 15).  Per 16-column panel:
//   1. the panel tiles (I, 0) go through a 64 x 17 LDS exchange to lane = row layout;
//   2. the 64 x 16 panel is factored in registers (v_readlane pivots, rsqrt + Newton, the
//      forward substitution fused);
//   3. L is stored into the LDS band (for the back-substitution) and re-read as MFMA operands
//      (A and B fragments of a tile are the same registers: B = L_J^T);
//   4. the rank-16 trailing update of tiles (I, J >= 1) runs as 24 MFMAs;
//   5. the window slides by 16: tiles move up-left, and the new bottom tile row comes straight
//      from S, because no earlier panel reaches it (L(i, k) = 0 for i - k > bw <= 48).
// Rows n .. n16-1 are an identity pad, so every panel is full; the next bottom tile row is
// prefetched one panel ahead.
__device__ __forceinline__ constexpr int tri4(int I, int J) { return I * (I + 1) / 2 + J; }

__global__ __launch_bounds__(256) void k_ba_chol_w(BaDev d) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int w = blockIdx.x;
  if (d.st[w].done) return;
  if (d.sharded && d.wfail[w] > 0.0) {  // a rank's point block was not PD: the step is invalid
    if (threadIdx.x == 0) d.st[w].chol_fail = 1;
    return;
  }
  const BaWin W = d.win[w];
  const int n = W.n, bw = W.bw;
  const int n16 = (n + 15) & ~15;
  const int t = threadIdx.x, lane = t & 63, ci = lane & 15, ck = lane >> 4;
  double* A = smem;                          // S band, overwritten in place by L: n16 x (bw + 1)
  double* z = A + (size_t)n16 * (bw + 1);    // rhs, overwritten by the forward substitution
  double* invd = z + n16;                    // n16
  double* xch = invd + n16;                  // 64 x 17 exchange
  const int dummy = (int)(xch + 64 * 17 + lane - A);  // 64 per-lane dummy slots after xch
  {  // stage S (+ identity pad rows) and rhs with all four waves, then wave 0 works alone
    const double* __restrict__ S = d.env + W.env_base;
    const int ne = n * (bw + 1);
    for (int k = t; k < ne; k += 256) A[k] = S[k];
    for (int k = ne + t; k < n16 * (bw + 1); k += 256) A[k] = (k % (bw + 1)) == bw ? 1.0 : 0.0;
    for (int k = t; k < n16; k += 256) z[k] = k < n ? d.rhs[W.row_base + k] : 0.0;
  }
  __syncthreads();
  if (t >= 64) return;
  auto sget = [&](int i, int j) -> double {  // band entry (i, j) of the staged matrix; branch-free
    const bool ok = j <= i && i - j <= bw && i < n16;
    const double v = A[ok ? i * (bw + 1) + (j - i + bw) : 0];
    return ok ? v : 0.0;
  };
  v4d T[10], Tn[4];
#pragma unroll
  for (int I = 0; I < 4; ++I)
#pragma unroll
    for (int J = 0; J <= I; ++J)
#pragma unroll
      for (int r = 0; r < 4; ++r) T[tri4(I, J)][r] = sget(16 * I + ck + 4 * r, 16 * J + ci);
  double zr = z[lane];
  bool bad = false;
  for (int kb = 0; kb < n16; kb += 16) {
    // the tile row that enters at the end of this panel (rows kb+64 .. kb+79): untouched S
#pragma unroll
    for (int J = 0; J < 4; ++J)
#pragma unroll
      for (int r = 0; r < 4; ++r) Tn[J][r] = sget(kb + 64 + ck + 4 * r, kb + 16 + 16 * J + ci);
    const double zin = kb + 16 + lane < n16 ? z[kb + 16 + lane] : 0.0;  // used by lanes >= 48
    // 1. panel tiles -> lane = row
#pragma unroll
    for (int I = 0; I < 4; ++I)
#pragma unroll
      for (int r = 0; r < 4; ++r) xch[(16 * I + ck + 4 * r) * 17 + ci] = T[tri4(I, 0)][r];
    wave_sync_lds();
    double P[NB];
#pragma unroll
    for (int q = 0; q < NB; ++q) P[q] = xch[lane * 17 + q];
    wave_sync_lds();
    // 2. factor the panel (lane = row kb + lane; entries above the diagonal are never stored)
    double yq = 0.0;
#pragma unroll
    for (int q = 0; q < NB; ++q) {
      const double akk = readlane_d(P[q], q);
      bad |= !(akk > 0.0);
      const double y = rsqrt_refined(akk);
      P[q] *= y;  // lane q: akk * y = L(k, k)
      yq = lane == q ? y : yq;
      const double zk = readlane_d(zr, q) * y;
      zr = lane > q ? fma(-P[q], zk, zr) : (lane == q ? zk : zr);
#pragma unroll
      for (int q2 = q + 1; q2 < NB; ++q2) {
        const double l = readlane_d(P[q], q2);
        P[q2] = fma(-P[q], l, P[q2]);
      }
    }
    // 3. L into the band (rows kb .. kb+63 have left S's use) + exchange; final z of the panel
    {
      const int row = kb + lane;
#pragma unroll
      for (int q = 0; q < NB; ++q) {
        const int col = kb + q;
        // branch-free: entries outside the band / above the diagonal go to a per-lane dummy slot
        const bool ok = row < n16 && col <= row && row - col <= bw;
        A[ok ? row * (bw + 1) + (col - row + bw) : dummy] = P[q];
        xch[lane * 17 + q] = P[q];
      }
      if (lane < NB) { z[row] = zr; invd[row] = yq; }
    }
    wave_sync_lds();
    double opA[4][4];  // [I][kk] = L(kb + 16 I + ci, kb + 4 kk + ck), I >= 1
#pragma unroll
    for (int I = 1; I < 4; ++I)
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) opA[I][kk] = xch[(16 * I + ci) * 17 + 4 * kk + ck];
    // 4. rank-16 trailing update (J = 1 first: it is the next panel)
#pragma unroll
    for (int J = 1; J < 4; ++J)
#pragma unroll
      for (int I = J; I < 4; ++I)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
          T[tri4(I, J)] = __builtin_amdgcn_mfma_f64_16x16x4f64(-opA[I][kk], opA[J][kk], T[tri4(I, J)], 0, 0, 0);
    // 5. slide the window by 16 rows / columns
    {
      const double zs = __shfl_down(zr, 16, 64);  // rows kb+16 .. kb+63 move up
      zr = lane < 48 ? zs : zin;                  // rows kb+64 .. kb+79 enter (raw rhs)
    }
    T[tri4(0, 0)] = T[tri4(1, 1)];
    T[tri4(1, 0)] = T[tri4(2, 1)]; T[tri4(1, 1)] = T[tri4(2, 2)];
    T[tri4(2, 0)] = T[tri4(3, 1)]; T[tri4(2, 1)] = T[tri4(3, 2)]; T[tri4(2, 2)] = T[tri4(3, 3)];
#pragma unroll
    for (int J = 0; J < 4; ++J) T[tri4(3, J)] = Tn[J];
  }
  if (bad) {
    if (lane == 0) d.st[w].chol_fail = 1;
    return;
  }
  wave_sync_lds();
  // back substitution L^T y = z by 16-row blocks from the bottom.  Lane (g, j) = (lane >> 4,
  // lane & 15): the block's column j gathers sum_i L(i, j) y_i over the rows below (split over
  // the four lane groups, butterfly-reduced), then the 16 x 16 triangle is solved with
  // v_readlane broadcasts.
  {
    const int jc = lane & 15, g = lane >> 4;
    for (int c0 = n16 - 16; c0 >= 0; c0 -= 16) {
      const int j = c0 + jc;
      double lk[NB];
#pragma unroll
      for (int k = 0; k < NB; ++k) {  // L(c0 + k, j), k > jc, inside the band (bw < 15: not all of them)
        const bool ok = k > jc && k - jc <= bw;
        const double v = A[ok ? (c0 + k) * (bw + 1) + (j - (c0 + k) + bw) : 0];
        lk[k] = ok ? v : 0.0;
      }
      // rows i = c0+16+g+4u (u < 16) cover every row below the block that reaches column j
      // (i - j <= bw <= 48); all loads are issued before the FMAs, four independent chains
      const int iend = min(n16 - 1, j + bw);
      double av[16], zv[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int i = c0 + 16 + g + 4 * u;
        const bool ok = i <= iend;
        av[u] = A[ok ? i * (bw + 1) + (j - i + bw) : 0];
        zv[u] = z[ok ? i : 0];
        av[u] = ok ? av[u] : 0.0;
      }
      double a4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int u = 0; u < 16; ++u) a4[u & 3] = fma(av[u], zv[u], a4[u & 3]);
      double acc = (a4[0] + a4[1]) + (a4[2] + a4[3]);
      {  // butterfly xor 16, xor 32 (permlane swaps, no LDS)
        double a, b;
        xrow_pair<false>(acc, a, b); acc = a + b;
        xrow_pair<true>(acc, a, b); acc = a + b;
      }
      double zb = z[j] - acc;
      const double iv = invd[j];
#pragma unroll
      for (int k = NB - 1; k >= 0; --k) {
        const double yk = readlane_d(zb, k) * readlane_d(iv, k);
        zb = jc == k ? yk : fma(-lk[k], yk, zb);
      }
      if (g == 0) z[j] = zb;
      wave_sync_lds();
    }
  }
  for (int k = lane; k < n; k += 64) d.ycam[W.row_base + k] = z[k];
  const int cur = d.st[w].cur;
  for (int ci2 = lane; ci2 < W.n_poses; ci2 += 64) {
    const int c = W.pose_base + ci2;
    double xn[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      xn[k] = d.x_pose[cur][6 * c + k] + (-z[6 * ci2 + k]) * d.scale_pose[6 * c + k];
      d.x_pose[cur ^ 1][6 * c + k] = xn[k];
    }
    d.rot_cand[c] = lorb::rot_val(xn);
  }
  for (int ci2 = lane; ci2 < W.n_poses; ci2 += 64) rot_lin_of(d, cur ^ 1, W.pose_base + ci2);
}

// K6t: two-sided ("twisted") banded Cholesky for band <= 48 and n >= 128.  The chain of
// dependent panels is the cost of K6w (one wavefront is latency/issue bound), so the matrix is
// split into T = [0, m), M = [m, m+48) and B = [m+48, n16): T and B do not couple (band <= 48).
// Wave 0 eliminates T top-down and wave 1 eliminates B bottom-up concurrently: the bottom part
// is staged REVERSED (row i' = n16-1-i; the band of the reversed matrix is the same), so both
// waves run the identical panel code on their own LDS band.  Their windows end on M holding
// S_MM - L_MT L_MT^T and S_MM - L_MB L_MB^T; wave 0 combines them (minus S_MM) and factors M
// (3 panels).  Back-substitution: M, then T (wave 0) and B (wave 1) concurrently.  Rows
// n .. n16-1 are an identity pad.
// Progressive staging (k_ba_chol_2s): bit b of the workgroup's mask = rows [16 b, 16 b + 16) of the
// band are in LDS.  Waves 2 / 3 publish with release, the factoring waves wait with acquire.
__device__ __forceinline__ void wait_bit(unsigned long long* mask, int b) {
  while (!((__hip_atomic_load(mask, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) >> b) & 1ull))
    __builtin_amdgcn_s_sleep(1);
}
// SLEEP: the waiting wave backs off between polls so that it does not compete for LDS with the
// chain it waits on; the chain wave's own wait is short and spins
template <bool SLEEP>
__device__ __forceinline__ void wait_ge(int* c, int v) {
  while (__hip_atomic_load(c, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < v)
    if (SLEEP) __builtin_amdgcn_s_sleep(1);
}

// 1: the update waves spin on the chain's L post instead of sleeping between polls (same-box A/B
// 46.2 / 46.1 vs 46.1 / 45.5 us: inside the noise, off)
// Column stride of the chain's L columns in xch, padded against bank conflicts when the update
// wave reads them in MFMA operand layout.
constexpr int kCS = 65;
struct BandSide {
  double* A;     // band storage of the whole matrix (row-major, rows x (bw + 1), row i holds cols
                 // i-bw .. i); the diagonal slot holds 1 / L(i, i) (its only use is the
                 // back-substitution).  Element (i, j) of this side's view is A[base + si*i + sj*j]:
                 // the top side views it as is (si = bw, sj = 1, base = bw); the bottom side views
                 // it reversed, (i', j') = (n16-1-j, n16-1-i) (si = -1, sj = -bw, base =
                 // (n16-1)(bw+1) + bw), so both sides run the same panel code on one staging.
  double* z;     // rows: rhs -> forward substitution -> solution
  double* xch;   // 64 x 17 exchange (column 16 of each row: dummy store slot of that lane)
  int rows, bw, lane;
  int base, si, sj;
  unsigned long long* mask = nullptr;  // progressive staging (null: the whole band is staged)
  int* pdone = nullptr;                // panels whose L is in the band (release-counted, for linv)
  int nbk = 0, dir = 0;                // row blocks; +1 top view, -1 reversed bottom view
  int zslot = 0;                       // A[zslot] == 0.0 (out-of-band reads of the back-substitution)
  double* kco = nullptr;               // this side's back-substitution operators (bsk_block)
  unsigned long long* trace = nullptr;   // LORB_CHOL_TRACE diagnostics: per-panel event times
  int tslot = 0;                         // (slot of this wave's next panel; cycles since t0)
  int bslot = 320;                       // (slot of this wave's next back-substitution block)
  unsigned long long t0 = 0;
  __device__ __forceinline__ void tr(int k) const {
#ifdef LORB_CHOL_TRACE
    if (trace && lane == 0) trace[tslot + k] = __builtin_amdgcn_s_memtime() - t0;
#endif
  }

  __device__ __forceinline__ int idx(int i, int j) const { return base + si * i + sj * j; }

  __device__ __forceinline__ double get(int i, int j) const {  // branch-free; 0 outside band / rows
    const bool ok = j <= i && i - j <= bw && i < rows;
    const double v = A[ok ? idx(i, j) : base];
    return ok ? v : 0.0;
  }
  __device__ __forceinline__ void init_tiles(v4d (&T)[10]) const {  // column 0 is the chain wave's
#pragma unroll
    for (int I = 1; I < 4; ++I)
#pragma unroll
      for (int J = 1; J <= I; ++J)
#pragma unroll
        for (int r = 0; r < 4; ++r) T[tri4(I, J)][r] = get(16 * I + (lane >> 4) + 4 * r, 16 * J + (lane & 15));
  }
  __device__ __forceinline__ void init_panel(double (&P)[NB], double& zr) const {
#pragma unroll
    for (int q = 0; q < NB; ++q) P[q] = get(lane, q);
    zr = lane < rows ? z[lane] : 0.0;
  }
  // Lookahead split of the panel loop over two wavefronts of one side.  The CHAIN wave factors
  // panels kb = kb0, kb0+16, ... < kend (lane = panel row): v_readlane pivots, rsqrt-refined, the
  // forward substitution fused; it writes L to the band and to xch and posts *lrd.  The UPDATE
  // wave holds the 64 x 64 trailing window as ten 16 x 16 MFMA accumulator tiles: on each posted
  // panel it first applies the rank-16 update to the next panel's column (tiles (1..3, 1)), hands
  // that column to the chain wave through pb (lane = row) and posts *prd, and only then updates
  // the rest of the window and slides it by 16 -- off the chain's critical path.
  //   chain(): P = the first panel when `pre` (else it comes from pb); pwant counts the pb posts
  //   consumed so far (continues across phases).
  __device__ __forceinline__ void chain(double (&P)[NB], double& zr, bool& bad, int kb0, int kend, bool pre,
                                        int* lrd, int* prd, int& pwant, const double* pb) const {
    const int dstep = 16 * (si + sj);  // address step of one panel along the diagonal
    unsigned l_ok = 0;
#pragma unroll
    for (int q = 0; q < NB; ++q) l_ok |= (unsigned)(q <= lane && lane - q <= bw) << q;
    int l_base = idx(kb0 + lane, kb0);  // slot of (kb0 + lane, kb0 + q) = l_base + q sj
    // L column q of the panel at colbuf[q * kCS + row]: the chain's multipliers and what the
    // update wave reads (in MFMA operand layout)
    double* colbuf = xch;
    // dummy target of the masked band stores (outside colbuf)
    double* dummy = xch + 16 * kCS + lane;
    for (int kb = kb0; kb < kend; kb += 16) {
      // Opaque per-iteration copies of the lane constants: otherwise every lane comparison of the
      // unrolled panel is hoisted out of the loop as an SGPR mask and the masks spill.
      int lane = this->lane, lok = (int)l_ok;
      asm volatile("" : "+v"(lane), "+v"(lok));
      if (!(pre && kb == kb0)) {
        wait_ge<false>(prd, ++pwant);
#pragma unroll
        for (int q = 0; q < NB; ++q) P[q] = pb[lane * 17 + q];  // lanes < q: upper garbage, never used
      }
      tr(0);
      const double zin = kb + 16 + lane < rows ? z[kb + 16 + lane] : 0.0;
      double yq = 0.0;
      // Software-pipelined columns: column q-1's updates of the later columns (multipliers loaded
      // from colbuf at the end of iteration q-1) are issued inside column q's pivot chain, behind
      // a scheduling barrier after the first Newton step of its rsqrt, so the chain no longer
      // waits on LDS.  Every P[q2] still receives its FMAs in column order (same bits).
      double mp[NB];
#pragma unroll
      for (int q2 = 0; q2 < NB; ++q2) mp[q2] = 0.0;
      double akk = readlane_d(P[0], 0);
#pragma unroll
      for (int q = 0; q < NB; ++q) {
        bad |= !(akk > 0.0);
        double y = __builtin_amdgcn_rsq(akk);
        __builtin_amdgcn_sched_barrier(0);
        if (q >= 1) {
#pragma unroll
          for (int q2 = q + 1; q2 < NB; ++q2) P[q2] = fma(-P[q - 1], mp[q2], P[q2]);
        }
        // The chain wave is VALU-issue bound (about 45 instructions per column): one Newton step on
        // v_rsq_f64 (about 2^-23 relative) leaves ~1e-14, far inside north_star's 1e-5
        {
          const double e = fma(-akk * y, y, 1.0);
          y = fma(0.5 * y, e, y);
        }
        P[q] *= y;  // lane q: akk * y = L(k, k)
        yq = lane == q ? y : yq;
        const double zk = readlane_d(zr, q) * y;
        zr = lane > q ? fma(-P[q], zk, zr) : (lane == q ? zk : zr);
        colbuf[q * kCS + lane] = P[q];
        if (q + 1 < NB) {
          const double l1 = readlane_d(P[q], q + 1);
          P[q + 1] = fma(-P[q], l1, P[q + 1]);
          akk = readlane_d(P[q + 1], q + 1);
#pragma unroll
          for (int q2 = q + 2; q2 < NB; ++q2) mp[q2] = colbuf[q * kCS + q2];
        }
      }
      tr(1);
      const bool rowvalid = kb + lane < rows;
      // the update wave reads L from colbuf: post it now, then store L to the band (for the
      // diagonal-block inverses and the back-substitution) while the update runs
      if (lane == 0) __hip_atomic_fetch_add(lrd, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
#pragma unroll
      for (int q = 0; q < NB; ++q) {
        const bool ok = rowvalid && (((unsigned)lok >> q) & 1u);
        *(ok ? A + l_base + q * sj : dummy) = q == lane ? yq : P[q];
      }
      l_base += dstep;
      if (lane < NB) z[kb + lane] = zr;
      if (lane == 0 && pdone) __hip_atomic_fetch_add(pdone, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
      const double zs = __shfl_down(zr, 16, 64);
      zr = lane < 48 ? zs : zin;
      tr(2);
      const_cast<BandSide*>(this)->tslot += 3;
    }
  }
  //   update(): T = the window at kb0 (column 0 unused); on return the window at kend (all ten
  //   tiles).  lwant counts the L posts consumed so far.
  __device__ __forceinline__ void update(v4d (&T)[10], int kb0, int kend, int* lrd, int* prd, int& lwant,
                                         double* pb) const {
    const int ci = lane & 15, ck = lane >> 4;
    const int dstep = 16 * (si + sj);
    int tn_addr = idx(kb0 + 64 + ck, kb0 + 16 + ci);  // entering tile (J, r) adds 4 r si + 16 J sj (below)
    unsigned tn_ok = 0;
#pragma unroll
    for (int J = 0; J < 4; ++J)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 64 + ck + 4 * r, j = 16 + 16 * J + ci;
        tn_ok |= (unsigned)(j <= i && i - j <= bw) << (4 * J + r);
      }
    for (int kb = kb0; kb < kend; kb += 16) {
      int tok = (int)tn_ok;
      asm volatile("" : "+v"(tok));
      // the tile row entering at the end of this panel (view rows kb+64 .. kb+79): untouched S,
      // loaded while the chain wave factors the panel
      if (mask) {
        const int b = dir > 0 ? kb / 16 + 4 : nbk - 5 - kb / 16;
        if (b >= 0 && b < nbk) wait_bit(mask, b);
      }
      v4d Tn[4];
#pragma unroll
      for (int J = 0; J < 4; ++J)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          // (kb+64+ck+4r, kb+16+16J+ci): row offset 4r, column offset 16J relative to tn_addr
          const bool ok = (((unsigned)tok >> (4 * J + r)) & 1u) && kb + 64 + ck + 4 * r < rows;
          const double v = A[ok ? tn_addr + 4 * r * si + 16 * J * sj : base];
          Tn[J][r] = ok ? v : 0.0;
        }
      tn_addr += dstep;
      const bool nxt = kb + 16 < kend;
      tr(0);
      wait_ge<true>(lrd, ++lwant);
      tr(1);
      double opA[4][4];
#pragma unroll
      for (int I = 1; I < 4; ++I)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
          opA[I][kk] = xch[(4 * kk + ck) * kCS + 16 * I + ci];  // L(kb + 16 I + ci, kb + 4 kk + ck)
      // the next panel's column first, then hand it over
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
#pragma unroll
        for (int I = 1; I < 4; ++I)
          T[tri4(I, 1)] = __builtin_amdgcn_mfma_f64_16x16x4f64(-opA[I][kk], opA[1][kk], T[tri4(I, 1)], 0, 0, 0);
      if (nxt) {
#pragma unroll
        for (int I = 1; I < 4; ++I)
#pragma unroll
          for (int r = 0; r < 4; ++r) pb[(16 * (I - 1) + ck + 4 * r) * 17 + ci] = T[tri4(I, 1)][r];
#pragma unroll
        for (int r = 0; r < 4; ++r) pb[(48 + ck + 4 * r) * 17 + ci] = Tn[0][r];
        if (lane == 0) __hip_atomic_fetch_add(prd, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      tr(2);
      // k-step outer: the three tiles' accumulation chains interleave
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
#pragma unroll
        for (int J = 2; J < 4; ++J)
#pragma unroll
          for (int I = J; I < 4; ++I)
            T[tri4(I, J)] = __builtin_amdgcn_mfma_f64_16x16x4f64(-opA[I][kk], opA[J][kk], T[tri4(I, J)], 0, 0, 0);
      T[tri4(0, 0)] = T[tri4(1, 1)];
      T[tri4(1, 0)] = T[tri4(2, 1)]; T[tri4(1, 1)] = T[tri4(2, 2)];
      T[tri4(2, 0)] = T[tri4(3, 1)]; T[tri4(2, 1)] = T[tri4(3, 2)]; T[tri4(2, 2)] = T[tri4(3, 3)];
#pragma unroll
      for (int J = 0; J < 4; ++J) T[tri4(3, J)] = Tn[J];
      tr(3);
      const_cast<BandSide*>(this)->tslot += 4;
    }
  }
  // The 16 x 16 diagonal block of L at view rows c0 .. c0+15 replaced in place by its inverse X
  // (lower triangular; the diagonal slot already holds 1 / L(i, i) = X(i, i)):
  // X(i, j) = -X(i, i) sum_{k=j}^{i-1} L(i, k) X(k, j).  Only the back-substitution reads the
  // block afterwards.  All 64 lanes: lane = 4 j + r holds column j's rows i = 4 m + r (acc[m]).  Step k: the lane
  // of row k (r = k & 3) forms X(k, j) and stores it, a quad broadcast hands it to the column's
  // four lanes, each adds L(i, k) X(k, j) to its rows.  The L loads (about 30 per lane) are all
  // issued before the sweep.  Per row the FMAs run in k order (the bits of a column sweep).
  template <int K>
  __device__ __forceinline__ void linv_step(int c0, int j, int r, double (&acc)[4], const double (&dv)[4],
                                            const double (&lv)[16][4]) const {
    constexpr int rk = K & 3, mk = K >> 2;
    const double xo = K == j ? dv[mk] : (K > j ? -dv[mk] * acc[mk] : 0.0);
    if (r == rk && K > j && K - j <= bw) A[idx(c0 + K, c0 + j)] = xo;
    const double xk = dpp_d<rk * 0x55>(xo);
#pragma unroll
    for (int m = 0; m < 4; ++m)
      if (4 * m + 3 > K) acc[m] = fma(lv[K][m], xk, acc[m]);  // lv == 0 where 4 m + r <= K
  }
  template <int K>
  __device__ __forceinline__ void linv_sweep(int c0, int j, int r, double (&acc)[4], const double (&dv)[4],
                                             const double (&lv)[16][4]) const {
    linv_step<K>(c0, j, r, acc, dv, lv);
    if constexpr (K + 1 < 16) linv_sweep<K + 1>(c0, j, r, acc, dv, lv);
  }
  __device__ __forceinline__ void linv(int c0) const {
    const int j = lane >> 2, r = lane & 3;
    double acc[4] = {0.0, 0.0, 0.0, 0.0}, dv[4], lv[16][4];
#pragma unroll
    for (int m = 0; m < 4; ++m) dv[m] = A[idx(c0 + 4 * m + r, c0 + 4 * m + r)];
#pragma unroll
    for (int k = 0; k < 16; ++k)
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        if (4 * m + 3 > k) {
          const int i = 4 * m + r;
          lv[k][m] = A[(i > k && i - k <= bw) ? idx(c0 + i, c0 + k) : zslot];
        } else {
          lv[k][m] = 0.0;
        }
      }
    linv_sweep<0>(c0, j, r, acc, dv, lv);
  }
  // Back-substitution L^T y = z, push style: the 64 rows c0-48 .. c0+15 of the current block c0
  // live in registers (row r in lane r & 63, so sliding the window needs no shuffle).  A block
  // solves its 16 x 16 triangle -- as a v_readlane chain (c0 >= c_inv) or as one product with the
  // inverted diagonal block X from linv (c0 < c_inv) -- writes y to z, pushes y into the rows above
  // it within the band, and its lanes load the rows that enter the window above.
  __device__ __forceinline__ int bs_row(int c0) const { return c0 - 48 + ((lane - (c0 - 48)) & 63); }
  // window of block c_hi; `known` rows c_hi+16 .. c_hi+15+known already hold final y in z and are
  // pushed into it first
  __device__ __forceinline__ double bs_init(int c_hi, int known) const {
    const int row = bs_row(c_hi);
    double zw = row >= 0 ? z[row] : 0.0;
    for (int i0 = 0; i0 < known; i0 += 16) {
      double l[16], y[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int ri = c_hi + 16 + i0 + k;
        const bool ok = i0 + k < known && row >= 0 && ri - row <= bw;
        l[k] = A[ok ? idx(ri, row) : base];
        l[k] = ok ? l[k] : 0.0;
        y[k] = z[i0 + k < known ? ri : 0];
      }
#pragma unroll
      for (int k = 0; k < 16; ++k) zw = fma(-l[k], y[k], zw);
    }
    return zw;
  }
  struct BsWin {
    double zw;         // the window
    double zin = 0.0;  // rows that entered above (loaded by the last block's lanes), merged late
    bool pend = false;
  };
  // blocks c_from, c_from - 16, ..., c_to; INV: multiply by the inverted diagonal block, else a
  // v_readlane chain through the triangle.  The rows entering above are merged only before the
  // next block's pushes, so their loads are off the chain.  Addresses are per-lane linear in the
  // block index; the lane constants are kept opaque (VGPRs) so the unrolled block does not
  // hoist dozens of uniform values into SGPRs.
  template <bool INV>
  __device__ __forceinline__ void bs_run(BsWin& S, int c_from, int c_to) const {
    for (int c0 = c_from; c0 >= c_to; c0 -= 16) {
      int row = bs_row(c0);
      const int j = row - c0, b0 = c0 & 63;
      const bool blk = j >= 0;
      // L(c0 + k, row) at aL + si k, valid for 1 <= c0 - row + k <= bw (and row >= 0; INV: not a
      // block lane); X(c0 + k, c0 + j) at aX + si k, valid for k >= j.  Invalid entries read the
      // zero word, so a load needs one compare and one address select.
      int aL = base + si * c0 + sj * row;
      int aX = base + si * c0 + sj * (c0 + j);
      int eL = c0 - row - 1 + ((row < 0 || (INV && blk)) ? (1 << 20) : 0);
      int eX = blk ? -j : (1 << 20);
      asm volatile("" : "+v"(aL), "+v"(aX), "+v"(eL), "+v"(eX), "+v"(row));
      double Lp[16], xv[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) Lp[k] = A[(unsigned)(eL + k) < (unsigned)bw ? aL + si * k : zslot];
      double zw = S.zw;
      if (!INV) {
#pragma unroll
        for (int k = 0; k < 16; ++k) xv[k] = A[base + si * (c0 + k) + sj * (c0 + k)];  // 1 / L(i, i)
        zw = S.pend ? S.zin : zw;
#pragma unroll
        for (int k = 15; k >= 0; --k) {
          const double yk = readlane_d(zw, (b0 + k) & 63) * xv[k];
          zw = (j == k) ? yk : fma(-Lp[k], yk, zw);
        }
        if (blk) z[row] = zw;
      } else {
#pragma unroll
        for (int k = 0; k < 16; ++k) xv[k] = A[(unsigned)(eX + k) < 16u ? aX + si * k : zslot];
        // z_b and then y_b go through z in LDS (broadcast reads)
        if (blk) z[row] = zw;
        wave_sync_lds();
        double a4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < 16; ++k) a4[k & 3] = fma(xv[k], z[c0 + k], a4[k & 3]);
        const double y = (a4[0] + a4[1]) + (a4[2] + a4[3]);
        wave_sync_lds();
        if (blk) z[row] = y;
        wave_sync_lds();
        zw = S.pend ? S.zin : zw;
        double p4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < 16; ++k) p4[k & 3] = fma(Lp[k], z[c0 + k], p4[k & 3]);
        zw = blk ? y : zw - ((p4[0] + p4[1]) + (p4[2] + p4[3]));
      }
      if (blk) S.zin = row - 64 >= 0 ? z[row - 64] : 0.0;  // the row entering above
      S.pend = blk;
      S.zw = zw;
    }
  }
  // Back-substitution operator of T / B block c0, built off the critical path (after the block's
  // diagonal inverse X): the block's step -- y = X^T z_b, then the push of y into the 47 rows
  // above -- folded into ONE product with z_b.  Lane l (window row r = bs_row(c0)) gets
  //   block rows (j = r - c0 >= 0):  coef[k] = X(k, j)                          (y_j = sum_k coef[k] z_k)
  //   rows above:                    coef[k] = sum_{j <= k} L(c0 + j, r) X(k, j) (zw_r -= sum_k coef[k] z_k)
  // at kco[(c0 / 16) * 1024 + 64 k + l].  The bs_run_k step is then one LDS round trip (publish z_b,
  // 16 broadcast reads) where bs_run<true> has two.  X is the full 16 x 16 block: bw >= 15.
  // On the matrix cores: C(k, r) = sum_j X(k, j) Lx(j, r), rows r = c0-48 .. c0+15 as four 16-row
  // tiles (N), j in four steps of 4 (K), 16 v_mfma_f64_16x16x4f64; Lx(j, r) = L(c0 + j, r) above the
  // block (0 outside the band / matrix) and the identity on the block's own rows.  Per lane 4 + 12
  // independent LDS loads (no broadcasts); C lands as kco[64 k + (r & 63)], the lane of row r in
  // bs_run_k's window.
  __device__ __forceinline__ void bsk_block(int c0) const {
    const int ci = lane & 15, ck = lane >> 4;
    double xa[4], lb[3][4];
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      const int j = 4 * st + ck;  // A: X(ci, j), lower triangle
      xa[st] = A[j <= ci ? idx(c0 + ci, c0 + j) : zslot];
#pragma unroll
      for (int t = 0; t < 3; ++t) {  // B: L(c0 + j, r) for the rows above
        const int r = c0 - 48 + 16 * t + ci, dd = c0 + j - r;
        lb[t][st] = A[(r >= 0 && dd >= 1 && dd <= bw) ? idx(c0 + j, r) : zslot];
      }
    }
    v4d acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int st = 0; st < 4; ++st) {
#pragma unroll
      for (int t = 0; t < 3; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[st], lb[t][st], acc[t], 0, 0, 0);
      const double id = (4 * st + ck) == ci ? 1.0 : 0.0;  // the block's rows: X(k, r - c0)
      acc[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[st], id, acc[3], 0, 0, 0);
    }
    double* o = kco + (c0 >> 4) * 1024;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k = 4 * q + ck;  // coefficient pairs (k, k + 1) of a lane adjacent: 16-byte loads
        o[128 * (k >> 1) + 2 * ((c0 - 48 + 16 * t + ci) & 63) + (k & 1)] = acc[t][q];
      }
  }
  __device__ __forceinline__ void bsk_load(int c0, double (&cf)[16]) const {
    const double2* p = reinterpret_cast<const double2*>(kco + (c0 >> 4) * 1024) + lane;
#pragma unroll
    for (int k2 = 0; k2 < 8; ++k2) {
      const double2 v = p[64 * k2];
      cf[2 * k2] = v.x; cf[2 * k2 + 1] = v.y;
    }
  }
  // blocks c_from, c_from - 16, ..., c_to through their bsk_block operators; cf holds block
  // c_from's on entry.  Two coefficient sets alternate, so the next block's loads (L2) stay in
  // flight while this block runs (a copy between sets would wait for them).  Rows entering above
  // are merged before the product, as in bs_run.
  __device__ __forceinline__ void tr_bs(int k) const {  // LORB_CHOL_TRACE: back-substitution steps
#ifdef LORB_CHOL_TRACE
    if (trace && lane == 0 && bslot + k < 512) trace[bslot + k] = __builtin_amdgcn_s_memtime() - t0;
#endif
  }
  // cn: the next block's operator is requested into cg once z_b is published (the issue of its
  // loads overlaps the publish's round trip instead of sitting between two blocks)
  __device__ __forceinline__ void bsk_step(BsWin& S, int c0, const double (&cf)[16], int cn, double (&cg)[16]) const {
    tr_bs(0);
    int row = bs_row(c0);
    asm volatile("" : "+v"(row));
    const int j = row - c0;
    const bool blk = j >= 0;
    // branch-free: the other lanes' stores go to their dummy slot (xch column 16), their entering-
    // row load to the zero word (an exec-masked branch made the compiler wait for that load on the
    // chain right after the product)
    double* pub = blk ? z + row : xch + 17 * lane + 16;
    const double* ent = (blk && row >= 64) ? z + (row - 64) : A + zslot;
    double zw = S.zw;
    *pub = zw;  // z_b is final: publish it
    zw = S.pend ? S.zin : zw;
    const double zin = *ent;  // the row entering above (never pushed yet: off the chain)
    bsk_load(cn, cg);
    wave_sync_lds();
    tr_bs(1);
    const double2* zb2 = reinterpret_cast<const double2*>(z + c0);
    double a4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k2 = 0; k2 < 8; ++k2) {
      const double2 v = zb2[k2];
      a4[(2 * k2) & 3] = fma(cf[2 * k2], v.x, a4[(2 * k2) & 3]);
      a4[(2 * k2 + 1) & 3] = fma(cf[2 * k2 + 1], v.y, a4[(2 * k2 + 1) & 3]);
    }
    const double sum = (a4[0] + a4[1]) + (a4[2] + a4[3]);
    zw = blk ? sum : zw - sum;
    tr_bs(2);
    const_cast<BandSide*>(this)->bslot += 3;
    *pub = zw;  // y_b (after every lane's broadcast read: a wave's LDS operations stay in order)
    S.zin = zin;
    S.pend = blk;
    S.zw = zw;
  }
  // fully unrolled (at most kBskMax blocks): in a loop the compiler drains every load at the loop
  // head (vmcnt(0)), which would make each block wait for its successor's prefetch
  static constexpr int kBskMax = 32;
  __device__ __forceinline__ void bs_run_k(BsWin& S, int c_from, int c_to, double (&cf)[16]) const {
    double cg[16];
    int c0 = c_from;
#pragma unroll
    for (int it = 0; it < kBskMax; it += 2) {
      if (c0 < c_to) return;
      bsk_step(S, c0, cf, c0 - 16 >= c_to ? c0 - 16 : c0, cg);
      if (c0 - 16 < c_to) return;
      bsk_step(S, c0 - 16, cg, c0 - 32 >= c_to ? c0 - 32 : c0, cf);
      c0 -= 32;
    }
    for (; c0 >= c_to; c0 -= 16) {  // more than kBskMax blocks (narrow bands of ~1000 rows)
      bsk_step(S, c0, cf, c0 - 16 >= c_to ? c0 - 16 : c0, cg);
#pragma unroll
      for (int k = 0; k < 16; ++k) cf[k] = cg[k];
    }
  }
};

// Flat copy of band chunks [j0, j1) (16-byte chunks of the row-major n x (bw + 1) band) by nthr
// threads, U chunks per thread per batch with all loads of a batch issued before any store.
// Element (i, off) keeps S's value inside the matrix; the left triangle of the first bw rows is
// zeroed and rows n .. n16-1 are an identity pad.
template <int U>
__device__ __forceinline__ void stage_band(const double2* __restrict__ S2, double* Ab, int j0, int j1, int tid,
                                           int nthr, int n, int bw, int nsrc) {
  const int B1 = bw + 1;
  for (int jb = j0 + tid; jb < j1; jb += nthr * U) {
    double2 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = jb + nthr * u;
      v[u] = S2[(j < j1 && j < nsrc) ? j : 0];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = jb + nthr * u;
      if (j < j1) {
        int i = (2 * j) / B1, off = (2 * j) % B1;
        double e[2] = {v[u].x, v[u].y};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const bool in = i < n && i - (bw - off) >= 0;
          e[h] = in ? e[h] : ((i >= n && off == bw) ? 1.0 : 0.0);
          if (++off == B1) { off = 0; ++i; }
        }
        reinterpret_cast<double2*>(Ab)[j] = double2{e[0], e[1]};
      }
    }
  }
}


// the fused iteration's camera-block terms (stage_fix's), added by the staging thread itself
// the same over two chunk ranges [a0, a1) and [b0, b1), all loads of a batch before any store;
template <int U>
__device__ __forceinline__ void stage_band2(const double2* __restrict__ S2, double* Ab, int a0, int a1, int b0, int b1,
                                            int tid, int nthr, int n, int bw, int nsrc) {
  const int B1 = bw + 1, la = a1 - a0, tot = la + (b1 - b0);
  for (int vb = tid; vb < tot; vb += nthr * U) {
    double2 v[U];
    int jj[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int vv = vb + nthr * u;
      jj[u] = vv < la ? a0 + vv : b0 + (vv - la);
      v[u] = S2[(vv < tot && jj[u] < nsrc) ? jj[u] : 0];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = jj[u];
      if (vb + nthr * u < tot) {
        int i = (2 * j) / B1, off = (2 * j) % B1;
        double e[2] = {v[u].x, v[u].y};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const bool in = i < n && i - (bw - off) >= 0;
          e[h] = in ? e[h] : ((i >= n && off == bw) ? 1.0 : 0.0);
          if (++off == B1) { off = 0; ++i; }
        }
        reinterpret_cast<double2*>(Ab)[j] = double2{e[0], e[1]};
      }
    }
  }
}

// The fused iteration's camera blocks: k_ba_red<2> stages sc (U - A) sc^T on the diagonal camera
// blocks, so rows [r0, r1) of the staged band only get D^2 = clamp(U_ii sc_i^2) / radius on the
// diagonal.  Threads tid, tid + nthr, ... of the caller.
__device__ __forceinline__ void stage_fix(const BaDev& d, const LMOpt& o, double* Ab, const BaWin& W, double radius,
                                          int r0, int r1, int tid, int nthr) {
  r1 = min(r1, W.n);
  const int B1 = W.bw + 1;
  for (int q = tid; q < (r1 - r0) * 6; q += nthr) {
    const int i = r0 + q / 6, i6 = i % 6, j6 = q % 6;
    if (j6 != i6) continue;
    const int c = W.pose_base + i / 6;
    const double* sc = d.scale_pose + 6 * c;
    double v = d.U[21 * c + u21(i6, j6)] * sc[i6] * sc[j6];
    v = 0.0 + fmin(fmax(v, o.min_diag), o.max_diag) / radius;
    double& e = Ab[i * B1 + (j6 - i6 + W.bw)];
    e = e + v;
  }
}

// stage_fix's term for item q of rows [r0, r1) (one item per thread when (r1 - r0) * 6 <= the
// threads): its value, and in `at` the band word it is added to (-1: none).  Computed before the
// band copy, so its loads share the copy's round trip; the same expression, the same bits.
__device__ __forceinline__ double stage_fix_val(const BaDev& d, const LMOpt& o, const BaWin& W, double radius,
                                                int r0, int r1, int q, int& at) {
  r1 = min(r1, W.n);
  at = -1;
  if (q >= (r1 - r0) * 6) return 0.0;
  const int i = r0 + q / 6, i6 = i % 6, j6 = q % 6;
  if (j6 != i6) return 0.0;
  const int c = W.pose_base + i / 6;
  const double* sc = d.scale_pose + 6 * c;
  double v = d.U[21 * c + u21(i6, j6)] * sc[i6] * sc[j6];
  v = 0.0 + fmin(fmax(v, o.min_diag), o.max_diag) / radius;
  at = i * (W.bw + 1) + (j6 - i6 + W.bw);
  return v;
}

// One 16-row block of the band (8 (bw + 1) <= 64 x 7 chunks for bw <= 48) staged by one wavefront
// of the progressive staging in ONE global round trip: the fused iteration's camera-block operands
// (stage_fix's) are requested with the band chunks, and the term is formed when the block is
// written.  With stage_band + stage_fix a block took two round trips and two integer divisions per
// chunk, 5.8-6.9 k cycles, more than a panel of the chains: the update waves waited for their
// entering rows.  The values and the expressions are stage_band's and stage_fix's: the same bits.
struct StageBlk {
  static __device__ __forceinline__ double pinned_load(const double* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
  }
  double2 v[7];
  double fu[2], fs[2];  // U_ii and sc_i of this lane's diagonal entries
  int fa[2];            // the band words they are added to (-1: none)
  template <bool FIX>
  __device__ __forceinline__ void load(const BaDev& d, const BaWin& W, const double2* __restrict__ S2, int b, int cpb,
                                       int nch, int nsrc, int lane) {
    const int j0 = b * cpb, j1 = min(j0 + cpb, nch);
    // Relaxed wavefront-scope atomic loads (plain global_load_dwordx2): they are issued here, all
    // before the first wait.  Ordinary loads of the camera-block operands are sunk to their use,
    // below the band's LDS stores (which do not alias them): a second round trip
    const double* Sd = reinterpret_cast<const double*>(S2);
#pragma unroll
    for (int u = 0; u < 7; ++u) {
      const int j = j0 + lane + 64 * u;
      const int js = (j < j1 && j < nsrc) ? j : 0;
      v[u].x = pinned_load(Sd + 2 * js);
      v[u].y = pinned_load(Sd + 2 * js + 1);
    }
    if (FIX) {  // stage_fix's 96 items of 16 rows, two per lane; branch-free (the others load item 0's)
      const int rows = min(16 * b + 16, W.n) - 16 * b;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int q = lane + 64 * h;
        const int i = 16 * b + q / 6, i6 = i % 6, j6 = q % 6;
        const bool on = q < rows * 6 && j6 == i6;
        const int c = W.pose_base + (on ? i / 6 : 0);
        fu[h] = pinned_load(&d.U[21 * c + (on ? u21(i6, i6) : 0)]);
        fs[h] = pinned_load(&d.scale_pose[6 * c + (on ? i6 : 0)]);
        fa[h] = on ? i * (W.bw + 1) + W.bw : -1;
      }
    }
  }
  // Only for blocks 4 <= b < n16 / 16 - 4 (the progressive ones): their rows 64 <= i < n16 - 64 < n
  // lie below the band's zeroed left triangle (i > bw) and above the identity pad, so stage_band's
  // per-element row / offset arithmetic (two integer divisions per chunk, which made the staging
  // wave slower than the chains) reduces to a copy.
  template <bool FIX>
  __device__ __forceinline__ void store(const LMOpt& o, double radius, double* Ab, int b, int cpb, int nch,
                                        int lane) const {
    const int j0 = b * cpb, j1 = min(j0 + cpb, nch);
#pragma unroll
    for (int u = 0; u < 7; ++u) {
      const int j = j0 + lane + 64 * u;
      if (j < j1) reinterpret_cast<double2*>(Ab)[j] = v[u];
    }
    if (FIX) {
      wave_sync_lds();
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        double t = fu[h] * fs[h] * fs[h];
        t = 0.0 + fmin(fmax(t, o.min_diag), o.max_diag) / radius;
        if (fa[h] >= 0) Ab[fa[h]] = Ab[fa[h]] + t;
      }
    }
  }
};

constexpr int kChol2sThreads = 512;
// The T / B back-substitution runs one LDS round trip per block (BandSide::bsk_block / bs_run_k).
// (Measured and removed: the epilogue's pose state loaded at the kernel's start, 232 -> 256 VGPRs,
// no gain; y_T / y_B as w - G y_M with G and w formed during the M phase, 115 k cycles against
// 97 k -- DESIGN §4.)

// Waves: 0 / 1 chain (top / bottom side), 2 / 3 their update waves, 4 / 5 the inverses of L's
// diagonal blocks (for the back-substitution), 6 / 7 the progressive staging of the band.
// HEAD (the fused iteration): wave 4 first runs the iteration head (lm_head, k_ba_lm_begin's work)
// while the first panels factor; a head that ends the solve leaves the candidate unwritten.
template <bool HEAD>
__device__ __forceinline__ void chol_2s_run(const BaDev& d, const LMOpt& o, const int w) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  __shared__ int s_bad;
  __shared__ int s_head_done;

  // window, state and failure flag requested together (one round trip before the band copy)
  // (a folding iteration, d.fold: the state k_ba_ls decided, and its point-block failure flag)
  const bool fold = HEAD && d.fold;
  const BaWin W = d.win[w];
  const int ls_fail = fold ? d.ls_fail[w] : 0;
  const WinState S0 = [&] {
    WinState S = (fold ? d.st2 : d.st)[w];
    if (fold) S.chol_fail = ls_fail;
    return S;
  }();
  const int done = S0.done;
  const double wfail = d.sharded ? d.wfail[w] : 0.0;
  if (fold) {
    // a solve the head ended earlier has st done (k_ba_ls decides nothing then: st2 is stale); one
    // the tail has just ended is done in st2 alone, and st takes it here, as k_ba_lm_end stores it
    if (d.st[w].done) return;
    if (done && threadIdx.x == 0) d.st[w] = S0;
  }
  if (done) return;
  if (wfail > 0.0) {  // a rank's point block was not PD: the step is invalid
    if (HEAD) {       // the fused sharded iteration's head still runs (it advances the iteration)
      if (threadIdx.x < 64) {
        const WinState S = lm_head<true>(d, o, w, threadIdx.x, S0, W);
        if (threadIdx.x == 0 && !S.done) d.st[w].chol_fail = 1;
      }
    } else if (threadIdx.x == 0) {
      d.st[w].chol_fail = 1;
    }
    return;
  }
#ifdef LORB_CHOL_TRACE
  if (threadIdx.x == 0) d.dbg[512 * w + 250] = __builtin_amdgcn_s_memtime();  // raw: state loaded
#endif
  constexpr int NT = kChol2sThreads;
  const int n = W.n, bw = W.bw, B1 = bw + 1;
  const int n16 = (n + 15) & ~15;
  const int m = 16 * ((n16 - 48) / 32);  // T = [0, m), M = [m, m+48), B = [m+48, n16)
  const int nB = n16 - m - 48;
  const int rt = m + 48, rb = nB + 48;    // rows of the top / reversed-bottom bands
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  double* Ab = smem;          // the whole band once, n16 rows (rows n .. n16-1: identity pad)
  double* zt = Ab + n16 * B1;
  double* zb = zt + rt;
  double* xt = zb + rb;       // 64 x 18 per side (rows of 17); both together hold X (48 x 48)
  double* xb = xt + 64 * 18;
  double* zX = xb + 64 * 18;  // 48
  double* pbt = zX + 48;      // 64 x 17 panel hand-off, top / bottom
  double* pbb = pbt + 64 * 17;
  double* zero = pbb + 64 * 17;  // one 0.0
  // Staging.  The rows each side's first panel reads (view rows 0 .. 79 of both sides) are copied
  // by all waves; the rest of the band by waves 6 / 7 while the chains run, in the order the
  // update waves need it (a block mask in LDS).  Waves 4 / 5 invert the diagonal 16 x 16 blocks
  // of L as the panels finish, for the back-substitution.
  __shared__ unsigned long long s_mask;
  __shared__ int s_pdone[2];
  __shared__ int s_linv[2];           // diagonal-block inverses done, per side
  __shared__ int s_lrd[2], s_prd[2];  // per side: L panels posted (chain), panel columns posted (update)
  __shared__ int s_hand[3];           // T / B -> M hand-over (below)
  __shared__ int s_kdone[2];          // operator builders done, per side
  const double2* __restrict__ S2 = reinterpret_cast<const double2*>(d.env + W.env_base);
  const int nch = n16 * B1 / 2, nsrc = n * B1 / 2;  // chunks (n is a multiple of 6: even)
  const int nbk = n16 / 16, ib = 4;
  const bool prog = nbk <= 64 && nbk > 2 * ib;
  const int cpb = 8 * B1;  // chunks per 16-row block
  // rhs loads issued before the band copy (one round trip for both), with the fused iteration's
  // camera-block terms of the rows staged first (16 ib rows per side: one item per thread), which
  // would otherwise cost a round trip after the copy.  The epilogue's poses go to waves 6 / 7
  // (camera t - 384), idle since their staging
  static_assert(16 * 4 * 6 <= kChol2sThreads, "one stage_fix item per thread");
  int fa0 = -1, fa1 = -1;
  double fv0 = 0.0, fv1 = 0.0;
  if (HEAD && prog) {
    fv0 = stage_fix_val(d, o, W, S0.radius, 0, 16 * ib, t, fa0);
    fv1 = stage_fix_val(d, o, W, S0.radius, 16 * (nbk - ib), n16, t, fa1);
  }
  const int cur = S0.cur, ep = t - (NT - 128);  // epilogue: camera ep (+ 128 k) of the window
  double rz;
  {
    const int row = t < rt ? t : n16 - 1 - (t - rt);
    rz = (t < rt + rb && row < n) ? d.rhs[W.row_base + row] : 0.0;
    // (the rhs is complete: k_ba_red writes (V - R) sc)
  }
  if (prog) {  // both sides' first ib blocks in one batch
    stage_band2<7>(S2, Ab, 0, ib * cpb, (nbk - ib) * cpb, nch, t, NT, n, bw, nsrc);
  } else {
    stage_band<14>(S2, Ab, 0, nch, t, NT, n, bw, nsrc);
  }
  if (t < rt) zt[t] = rz;
  else if (t < rt + rb) zb[t - rt] = rz;
  for (int k = t + NT; k < rt + rb; k += NT) {  // (n16 > 464 only)
    const int row = k < rt ? k : n16 - 1 - (k - rt);
    double v = row < n ? d.rhs[W.row_base + row] : 0.0;
    if (k < rt) zt[k] = v; else zb[k - rt] = v;
  }
  if (t == 0) {
    *zero = 0.0;
    s_bad = 0;
    s_head_done = 0;
    s_pdone[0] = 0; s_pdone[1] = 0;
    s_linv[0] = 0; s_linv[1] = 0;
    s_lrd[0] = 0; s_lrd[1] = 0; s_prd[0] = 0; s_prd[1] = 0;
    s_hand[0] = 0; s_hand[1] = 0; s_hand[2] = 0;
    s_kdone[0] = 0; s_kdone[1] = 0;
    unsigned long long msk = 0;
    for (int b = 0; b < nbk; ++b) msk |= (unsigned long long)(!prog || b < ib || b >= nbk - ib) << (b & 63);
    s_mask = msk;
  }
  __syncthreads();
  if (HEAD) {  // the camera blocks of the rows staged so far
    if (prog) {
      if (fa0 >= 0) Ab[fa0] = Ab[fa0] + fv0;
      if (fa1 >= 0) Ab[fa1] = Ab[fa1] + fv1;
    } else {
      stage_fix(d, o, Ab, W, S0.radius, 0, n16, t, NT);
    }
    __syncthreads();
  }
  BandSide top{Ab, zt, xt, rt, bw, lane, bw, bw, 1};
  BandSide bot{Ab, zb, xb, rb, bw, lane, (n16 - 1) * B1 + bw, -1, -bw};
  top.pdone = &s_pdone[0]; bot.pdone = &s_pdone[1];
  top.zslot = (int)(zero - Ab); bot.zslot = top.zslot;
  top.kco = d.kco + (size_t)((W.row_base >> 4) + w) * 1024;
  bot.kco = top.kco + (size_t)(m >> 4) * 1024;
  top.nbk = bot.nbk = nbk; top.dir = 1; bot.dir = -1;
  if (prog) { top.mask = &s_mask; bot.mask = &s_mask; }
#ifdef LORB_CHOL_TRACE
  // dbg[512 w + ...]: chain top 0.. (3 per panel), update top 64.. (4 per panel), chain bottom
  // 128.., update bottom 160.., single events 200.., diagonal-block inverses 256..
  const unsigned long long tr0 = __builtin_amdgcn_s_memtime();
  unsigned long long* trb = d.dbg + 512 * w;
  top.trace = trb; bot.trace = trb; top.t0 = tr0; bot.t0 = tr0;
  if (t == 0) trb[252] = tr0;  // raw
  top.tslot = wv == 0 ? 0 : 64; bot.tslot = wv == 1 ? 128 : 160;
  top.bslot = 320; bot.bslot = 400;
#define TR1(k) do { if (lane == 0) trb[200 + (k)] = __builtin_amdgcn_s_memtime() - tr0; } while (0)
#else
#define TR1(k) do {} while (0)
#endif
  const int side = wv & 1;                 // 0 top, 1 bottom
  const BandSide& me = side == 0 ? top : bot;
  double* pb = side == 0 ? pbt : pbb;
  int* lrd = &s_lrd[side];
  int* prd = &s_prd[side];
  int lwant = 0, pwant = 0;
  bool bad = false;
  double zr = 0.0;
  double P[NB];
  v4d T[10];
  if (wv >= 6) {
    if (prog) {  // remaining blocks [ib, nbk - ib): wave 6 from the top, wave 7 from the bottom
      const int lo = ib, hi = nbk - ib, mid = (lo + hi) / 2;
      const int nk = side == 0 ? mid - lo : hi - mid;
      auto blk = [&](int k) { return side == 0 ? lo + k : hi - 1 - k; };
      auto put = [&](const StageBlk& R, int b) {
        R.template store<HEAD>(o, S0.radius, Ab, b, cpb, nch, lane);
        if (lane == 0) __hip_atomic_fetch_or(&s_mask, 1ull << b, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
      };
      for (int k = 0; k < nk; ++k) {
        StageBlk R;
        R.template load<HEAD>(d, W, S2, blk(k), cpb, nch, nsrc, lane);
        put(R, blk(k));
      }
    }
    TR1(8 + side);
  }
  if (HEAD && wv == 4) {  // the iteration head while the first panels factor
    const WinState S = d.sharded ? lm_head<true>(d, o, w, lane, S0, W) : lm_head<false>(d, o, w, lane, S0, W);
    if (lane == 0) s_head_done = S.done;
    if (fold && lane == 0) d.ls_fail[w] = 0;  // (the head has stored it as st.chol_fail)
  }
  // diagonal-block inverses (waves 4 / 5; on waves 6 / 7 after their staging, off the chain waves'
  // SIMDs, they measured no faster)
  if (wv == 4 || wv == 5) {
    int* pd = &s_pdone[side];
    const int nblk = (side == 0 ? m : nB) / 16;
    for (int p = 0; p < nblk; ++p) {
      while (__hip_atomic_load(pd, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) <= p) __builtin_amdgcn_s_sleep(1);
      TR1(56 + 32 * side + 2 * p);   // dbg[256 + 32 side + 2 p]
      me.linv(16 * p);
      if (lane == 0) __hip_atomic_fetch_add(&s_linv[side], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
      TR1(57 + 32 * side + 2 * p);
    }
    TR1(10 + side);
  } else if (wv < 2) {
    me.init_panel(P, zr);
    me.chain(P, zr, bad, 0, side == 0 ? m : nB, true, lrd, prd, pwant, pb);
  } else if (wv < 4) {
    me.init_tiles(T);
    me.update(T, 0, side == 0 ? m : nB, lrd, prd, lwant, pb);
  }
  // The T / B back-substitution operators (bsk_block, on the matrix cores), once a side's diagonal
  // inverses are done, on SIMDs 1 and 3 (the M phase's chain and update waves are on 0 and 2): waves
  // 5 / 7 build the top side's (alternate blocks, in the order the back-substitution needs them),
  // waves 1 / 3 the bottom side's after their hand-over to the M phase (below).  The stores drain
  // before the barrier that precedes the back-substitution.
  auto build_ops = [&](int ks, int par) {
    const BandSide& kside = ks == 0 ? top : bot;
    const int nkb = (ks == 0 ? m : nB) / 16;
    wait_ge<true>(&s_linv[ks], nkb);
    TR1(16 + 2 * ks);
    for (int b = nkb - 1 - par; b >= 0; b -= 2) kside.bsk_block(16 * b);
    __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0): the operators are in L2 before the post
    if (lane == 0) __hip_atomic_fetch_add(&s_kdone[ks], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    TR1(17 + 2 * ks);
  };
  if (wv == 5 || wv == 7) build_ops(0, wv == 7);
  // Hand-over to the M phase by flags, not barriers (the diagonal-block inverses of waves 4 / 5
  // may still be running): wave 2 posts that it has read its last L from xt, wave 3 then writes
  // the bottom side's window on M into X = xt (+ xb) and posts it, wave 1 posts zX.
  double* X = xt;  // 48 x 48 in the two exchanges (idle now), original M orientation
  if (wv == 3) {   // the bottom side's window on M, reversed back
    wait_ge<true>(&s_hand[0], 1);
#pragma unroll
    for (int I = 0; I < 3; ++I)
#pragma unroll
      for (int J = 0; J <= I; ++J)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int rho = 16 * I + (lane >> 4) + 4 * r, kap = 16 * J + (lane & 15);
          // unconditional: the upper-triangle slots are never read (no exec-mask branches)
          X[(47 - kap) * 48 + (47 - rho)] = T[tri4(I, J)][r];
          (void)kap; (void)rho;
        }
    if (lane == 0) __hip_atomic_fetch_add(&s_hand[1], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    TR1(2);
  }
  if (wv == 1) {
    if (lane < 48) zX[47 - lane] = zr;
    if (bad) s_bad = 1;
    if (lane == 0) __hip_atomic_fetch_add(&s_hand[2], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  if (wv == 1 || wv == 3) build_ops(1, wv == 3);
  if (wv == 2) {
    TR1(0);
    if (lane == 0) __hip_atomic_fetch_add(&s_hand[0], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    wait_ge<true>(&s_hand[1], 1);
    TR1(1);
  }
  if (wv == 0) wait_ge<true>(&s_hand[2], 1);
  if (wv == 2) {
    // S_M = (S_MM - L_MT L_MT^T) + (S_MM - L_MB L_MB^T) - S_MM ; rows >= m+48 leave the window
#pragma unroll
    for (int I = 0; I < 3; ++I)
#pragma unroll
      for (int J = 0; J <= I; ++J)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int rho = 16 * I + (lane >> 4) + 4 * r, kap = 16 * J + (lane & 15);
          // branch-free: above the diagonal the tiles hold values nobody reads
          T[tri4(I, J)][r] += X[rho * 48 + kap] - top.get(m + rho, m + kap);
        }
#pragma unroll
    for (int J = 0; J < 4; ++J) T[tri4(3, J)] = v4d{0.0, 0.0, 0.0, 0.0};
    TR1(14);
    BandSide topM = top;
    topM.mask = nullptr; topM.pdone = nullptr;
    {  // M's first panel column to the chain wave
      const int ci = lane & 15, ck = lane >> 4;
#pragma unroll
      for (int I = 0; I < 4; ++I)
#pragma unroll
        for (int r = 0; r < 4; ++r) pbt[(16 * I + ck + 4 * r) * 17 + ci] = T[tri4(I, 0)][r];
      if (lane == 0) __hip_atomic_fetch_add(&s_prd[0], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    TR1(15);
    topM.update(T, m, m + 48, &s_lrd[0], &s_prd[0], lwant, pbt);
  } else if (wv == 0) {
    zr = lane < 48 ? zr + zX[lane] - zt[m + lane] : 0.0;
    BandSide topM = top;
    topM.mask = nullptr; topM.pdone = nullptr;
    TR1(3);
    topM.chain(P, zr, bad, m, m + 48, false, &s_lrd[0], &s_prd[0], pwant, pbt);
    TR1(4);
    if (bad) s_bad = 1;
  }
  // (No barrier here.  Wave 0 goes from M's factor straight into the back-substitution,
  // wave 1 waits for y_M by flag, the operators are complete by their builders' flags; a failed
  // factorization (s_bad) only computes values nobody reads and is caught after the last barrier.)
  // the side's operator set and window (wave 0 top, wave 1 bottom), then ONE call site
  // of the unrolled T / B back-substitution for both waves (one copy of its code in the
  // instruction cache: the bottom side's copy missed it, 4 k cycles before its first block)
  double cf[16];
  BandSide::BsWin S{0.0};
  if (wv == 0) {
    wait_ge<true>(&s_kdone[0], 2);
    top.bsk_load(m - 16, cf);  // the first T block's operator, loaded under the M blocks
    S = BandSide::BsWin{top.bs_init(m + 32, 0)};
    TR1(5);
    top.bs_run<false>(S, m + 32, m);                   // y_M (chained triangles)
    TR1(6);
    if (lane < 48) zb[nB + 47 - lane] = zt[m + lane];  // into the reversed bottom rows
    if (lane == 0) __hip_atomic_fetch_add(&s_hand[0], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
  } else if (wv == 1) {
    wait_ge<true>(&s_kdone[1], 2);
    bot.bsk_load(nB - 16, cf);
    // the bottom window's pushes from M's 48 rows: L is final since the B phase, so its 48 entries
    // per lane are loaded before the wait; after it only y_M's broadcast reads and the FMAs remain
    // (four partial sums: a 48-long dependent FMA chain cost ~2 k cycles)
    double lb[48];
    const int brow = bot.bs_row(nB - 16);
#pragma unroll
    for (int k = 0; k < 48; ++k) {
      const bool ok = brow >= 0 && nB + k - brow <= bw;
      const double v = Ab[ok ? bot.idx(nB + k, brow) : bot.base];
      lb[k] = ok ? v : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 48; ++k) asm volatile("" : "+v"(lb[k]));  // loaded here, not sunk past the wait
    wait_ge<true>(&s_hand[0], 2);  // a long wait (the M phase): sleep, do not steal LDS cycles
    TR1(20);
    double b4[4] = {0.0, 0.0, 0.0, 0.0};
    const double2* zm2 = reinterpret_cast<const double2*>(zb + nB);
#pragma unroll
    for (int k2 = 0; k2 < 24; ++k2) {
      const double2 v = zm2[k2];
      b4[(2 * k2) & 3] = fma(lb[2 * k2], v.x, b4[(2 * k2) & 3]);
      b4[(2 * k2 + 1) & 3] = fma(lb[2 * k2 + 1], v.y, b4[(2 * k2 + 1) & 3]);
    }
    const double bzw = (brow >= 0 ? zb[brow] : 0.0) - ((b4[0] + b4[1]) + (b4[2] + b4[3]));
    S = BandSide::BsWin{bzw};
    TR1(21);
  }
  if (wv < 2) {  // y_T (wave 0) / y_B (wave 1, reversed)
    const BandSide g = wv == 0 ? top : bot;
    g.bs_run_k(S, (wv == 0 ? m : nB) - 16, 0, cf);  // one product per block
    TR1(wv == 0 ? 7 : 12);
  }
  __syncthreads();
  TR1(13);
#undef TR1
  if (s_bad) {
    if (t == 0) d.st[w].chol_fail = 1;
    return;
  }
  if (HEAD && s_head_done) return;  // the head ended the solve: no candidate
  for (int k = t; k < n; k += NT) d.ycam[W.row_base + k] = k < rt ? zt[k] : zb[n16 - 1 - k];
  for (int ci2 = ep; ep >= 0 && ci2 < W.n_poses; ci2 += 128) {
    const int c = W.pose_base + ci2;
    double xn[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const int row = 6 * ci2 + k;
      const double y = row < rt ? zt[row] : zb[n16 - 1 - row];
      const double xp = d.x_pose[cur][6 * c + k];
      const double sp = d.scale_pose[6 * c + k];
      xn[k] = xp + (-y) * sp;
      d.x_pose[cur ^ 1][6 * c + k] = xn[k];
    }
    d.rot_cand[c] = lorb::rot_val(xn);
  }
  // The candidates' linearisation states (rot_lin[cur ^ 1]: an accepted step then only flips cur) on
  // the 128 threads before those (waves 4 / 5), at the same time, from the same expression for the
  // pose: behind the candidates' pass on their threads they cost the kernel 1.8 us.
  const int el = t - (NT - 256);
  for (int ci2 = el; el >= 0 && el < 128 && ci2 < W.n_poses; ci2 += 128) {
    const int c = W.pose_base + ci2;
    double xn[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int row = 6 * ci2 + k;
      const double y = row < rt ? zt[row] : zb[n16 - 1 - row];
      const double xp = d.x_pose[cur][6 * c + k];
      const double sp = d.scale_pose[6 * c + k];
      xn[k] = xp + (-y) * sp;
    }
    d.rot_lin[rot_off(d, cur ^ 1) + c] = lorb::rot_jet(xn);
  }
#ifdef LORB_CHOL_TRACE
  if (t == 0) d.dbg[512 * w + 251] = __builtin_amdgcn_s_memtime();  // raw: epilogue issued (thread 0)
#endif
}
template <bool HEAD>
__global__ __launch_bounds__(kChol2sThreads) void k_ba_chol_2s(BaDev d, LMOpt o) { chol_2s_run<HEAD>(d, o, blockIdx.x); }

template <bool HEAD>
__global__ __launch_bounds__(kChol2sThreads) void k_ba_chol_2s_g(BaGrp g, GrpGrid G, LMOpt o) {
  unsigned lb;
  const int k = grp_member(G, g.n, blockIdx.x, lb);
  chol_2s_run<HEAD>(g.d[k], o, (int)lb);
}

}  // namespace

namespace lorb {
namespace ba {

void launch_chol(int kind, const CholShape& sh, hipStream_t s, const BaDev& d, const LMOpt& o, bool head) {
  if (kind == 2) {
    if (head)
      hipLaunchKernelGGL(k_ba_chol_2s<true>, dim3(sh.W), dim3(kChol2sThreads), sizeof(double) * (size_t)sh.max_env_w, s, d, o);
    else
      hipLaunchKernelGGL(k_ba_chol_2s<false>, dim3(sh.W), dim3(kChol2sThreads), sizeof(double) * (size_t)sh.max_env_w, s, d, o);
  } else if (kind == 1) {
    hipLaunchKernelGGL(k_ba_chol_w, dim3(sh.W), dim3(256), sizeof(double) * (size_t)sh.max_env_w, s, d);
  } else if (kind == 0) {
    const size_t lds = sizeof(double) * (size_t)sh.max_env;
    const bool in_lds = lds <= (size_t)kLdsBudget;  // else in place in global memory
    const int rows = NB + sh.max_bw;  // panel rows held in registers by wave 0
    const int rpl = rows <= 64 ? 1 : rows <= 128 ? 2 : rows <= 256 ? 4 : 8;
#define LORB_CHOL(L, R) hipLaunchKernelGGL((k_ba_chol<L, R>), dim3(sh.W), dim3(256), L ? lds : 0, s, d)
    if (in_lds) { if (rpl == 1) LORB_CHOL(true, 1); else if (rpl == 2) LORB_CHOL(true, 2); else if (rpl == 4) LORB_CHOL(true, 4); else LORB_CHOL(true, 8); }
    else { if (rpl == 1) LORB_CHOL(false, 1); else if (rpl == 2) LORB_CHOL(false, 2); else if (rpl == 4) LORB_CHOL(false, 4); else LORB_CHOL(false, 8); }
#undef LORB_CHOL
  }
}

void launch_chol_2s_g(hipStream_t s, const BaGrp& g, const GrpGrid& G, const LMOpt& o, bool head, size_t lds) {
  if (head) hipLaunchKernelGGL(k_ba_chol_2s_g<true>, dim3(G.pre[g.n]), dim3(kChol2sThreads), lds, s, g, G, o);
  else hipLaunchKernelGGL(k_ba_chol_2s_g<false>, dim3(G.pre[g.n]), dim3(kChol2sThreads), lds, s, g, G, o);
}

}  // namespace ba
}  // namespace lorb
