// lorb_ba.hip -- reprojection-error bundle adjustment on gfx950 (MI355X), FP64.
//
// Restates BA::ProjectPoseOptimization (src/bundle_adjust.cpp:158-202) and
// BA::LocalPoseOptimization (src/bundle_adjust.cpp:207-330): ceres::Solve with the default
// trust-region Levenberg-Marquardt options + DENSE_SCHUR.
//
// MI355X-first structure (device-resident LM, batched over independent windows):
//   * every LM scalar decision (accept/reject, radius, tolerances) is made ON THE DEVICE by a
//     one-workgroup-per-window kernel, so an LM iteration is a fixed sequence of launches with
//     no host round trip; it is captured once into a hipGraph and replayed.
//   * point-major Schur: one workgroup per point group linearises its observations, eliminates its
//     points and forms its camera-block partials on chip (k_ba_ls; a group spans <= 128 cameras);
//     one workgroup per band block sums the groups' partials in group order (k_ba_red); the
//     back-substitution re-evaluates the linearisation (k_ba_bs2).  Nothing is stored per
//     observation.  (Round 4's pair-major path -- per-observation tiles, one workgroup per camera
//     block pair over a CSR pair list -- was removed in round 6.)
//   * the reduced camera system is banded (cameras in reverse Cuthill-McKee order): a two-sided
//     band Cholesky with the LM head inside (k_ba_chol_2s), or the wider variants.
//   * all reductions are fixed-order trees (block partials reduced in index order): deterministic,
//     no FP64 atomics.
//
// Units: lorb_ba_dev.h holds the kernel argument structs (BaDev, BaWin, WinState, LMOpt, BaGrp,
// ...), the wave / block helpers and the iteration head lm_head; lorb_ba_chol.hip the three band
// Cholesky kernels (by far the slowest to compile) with their host launchers launch_chol /
// launch_chol_2s_g; lorb_ba_build.hip the host and device plan builders with their k_db_* kernels
// and the entry points that create, rebuild, read out and destroy a plan; lorb_ba_plan.h the plan
// struct those builders fill and this file solves; this file the LM control, point-major Schur and
// pose-only kernels, solve sequencing, groups and the remaining extern "C" entry points.  A kernel
// is launched from the unit that defines it.
//
// FP64 contraction: the BA arithmetic may fuse multiply-adds (v_fma_f64; its parity bar is 1e-5
// relative, not bit-exactness -- VERDICT r04 item 3).  The Makefile's global -ffp-contract=off stays
// for the float paths that must be bit-exact (projection, grid, unprojection, ORB, stereo: the other
// translation units).  Every BA unit therefore opens with the block below, before any include, so
// that the inline device code of lorb_ba_math.h and lorb_ba_dev.h is compiled under it too.
// Everything in these units is deterministic either way (fixed reduction orders);
// the host restatement that must round like the reference (lorb_pose_to_Tcw, cv::Rodrigues) turns
// contraction off in its own body.
#ifndef LORB_NO_CONTRACT  // A/B builds only (tools/isa_fma.py, tools/build_variant.sh nofma -DLORB_NO_CONTRACT)
#pragma clang fp contract(fast)
#endif
#include "lorb_ba_math.h"
#include "lorb_internal.h"
#include "lorb_ba_dev.h"
#include "lorb_ba_plan.h"

#include <algorithm>
#include <cmath>
#include <type_traits>

namespace {

using namespace lorb::ba;
using lorb::residual;
using lorb::residual_jac;
using lorb::residual_jac_s;
using lorb::residual_s;

// K0: start of a solve, one launch: window states, x[0] <- the initial values, and the
// per-camera rotation states of that first linearisation point (transcendentals once per
// camera; later ones come from the Cholesky's epilogue, with the candidate pose).
__device__ __forceinline__ void init_run(const BaDev& d, int W, int ctot, int n_pt, int nf, const LMOpt& o, const int i,
                                         const int stride) {
  if (i < W) {
    WinState s;
    s.radius = o.init_radius; s.decrease_factor = 2.0; s.cost = 0.0; s.x_norm = 0.0; s.gmax = 0.0;
    s.initial_cost = 0.0; s.iter = 0; s.n_success = 0; s.n_invalid = 0;
    s.done = d.win[i].n_obs_all == 0 ? 1 : 0;
    s.relin = 1; s.cur = 0; s.last_successful = 1; s.term = 0; s.chol_fail = 0; s.pad = 0;
    d.st[i] = s;
    d.ls_fail[i] = 0;
    if (d.sharded) d.wfail_part[i] = 0.0;  // point-block failures (set by k_ba_ls, cleared by k_ba_lm_end)
  }
  if (i < ctot) {
    double x[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) { x[k] = d.x_init_pose[6 * i + k]; d.x_pose[0][6 * i + k] = x[k]; }
    d.rot_lin[i] = lorb::rot_jet(x);
  }
  if (i < nf) {  // the fixed poses' rotation states, once per solve (k_ba_ls / k_ba_bs2 read them)
    double x[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) x[k] = d.fixed_pose[6 * i + k];
    d.rot_fix[i] = lorb::rot_jet(x);
    d.rotv_fix[i] = lorb::rot_val(x);
  }
  for (int k = i; k < 3 * n_pt; k += stride) d.x_pt[0][k] = d.x_init_pt[k];
}
__global__ __launch_bounds__(256) void k_ba_init(BaDev d, int W, int ctot, int n_pt, int nf, LMOpt o) {
  init_run(d, W, ctot, n_pt, nf, o, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}

// Point groups (PBlk): consecutive points of one window whose observations (contiguous, sorted
// by point) number <= kGB, processed by one 256-thread workgroup: observation-parallel phases
// (thread = observation, coalesced, no serial load chains) alternate with point phases (thread =
// point) that reduce their observations from LDS serially in observation order -- the same
// summation order as a point-serial loop.  A group holds whole points, so no point may have more than
// kGB observations: both plan builders refuse such a window (lorb_ba_build.hip: the host builder takes a
// point with up to kGB observations, the device builder up to kGB - 1); ls_group has no chunk loop.

// deterministic point-group reductions (fixed butterfly per wave, fixed wave order) over the
// kGB / 64 waves of a point-group workgroup
constexpr int kGW = kGB / 64;
static_assert(kGW >= 1 && kGW <= 16 && kGB % 64 == 0, "point groups of 64..1024 observations, whole waves");
// three block reductions behind one LDS exchange (M1: the second is a max): per-wave butterfly,
// then the waves' values in wave order
template <bool M1>
__device__ __forceinline__ void block_red3(double& a, double& b, double& c, double (*red)[kGW]) {
  a = wave_sum(a); b = M1 ? wave_max(b) : wave_sum(b); c = wave_sum(c);
  if (kGW == 1) return;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    const int w = threadIdx.x >> 6;
    red[0][w] = a; red[1][w] = b; red[2][w] = c;
  }
  __syncthreads();
  a = red[0][0]; b = red[1][0]; c = red[2][0];
#pragma unroll
  for (int k = 1; k < kGW; ++k) { a += red[0][k]; b = M1 ? fmax(b, red[1][k]) : b + red[1][k]; c += red[2][k]; }
}

// Point-block prep (k_ba_ls phase B): the point's scaled E^T E + D^2 inverted at the current
// radius.  Returns false when the 3x3 block is not invertible (Ei = 0).
__device__ __forceinline__ bool prep_point(const double (&Eu)[6], const double (&bu)[3], const double (&sp)[3],
                                           double rad, const LMOpt& o, double (&Ei)[6], double (&b)[3]) {
  double E[6];
#pragma unroll
  for (int k = 0; k < 3; ++k) b[k] = bu[k] * sp[k];
  E[0] = Eu[0] * sp[0] * sp[0]; E[1] = Eu[1] * sp[0] * sp[1]; E[2] = Eu[2] * sp[0] * sp[2];
  E[3] = Eu[3] * sp[1] * sp[1]; E[4] = Eu[4] * sp[1] * sp[2]; E[5] = Eu[5] * sp[2] * sp[2];
  E[0] += fmin(fmax(E[0], o.min_diag), o.max_diag) / rad;
  E[3] += fmin(fmax(E[3], o.min_diag), o.max_diag) / rad;
  E[5] += fmin(fmax(E[5], o.min_diag), o.max_diag) / rad;
  if (!inv3(E, Ei)) {
#pragma unroll
    for (int k = 0; k < 6; ++k) Ei[k] = 0.0;
    return false;
  }
  return true;
}
__device__ __forceinline__ void prep_fail(const BaDev& d, int win, int fold) {
  // benign race: every writer stores the same value; sharded plans reduce the flag (K5).  The
  // flag is cleared by k_ba_lm_end (and k_ba_init), not by k_ba_lm_begin: k_ba_ls sets it
  // before k_ba_lm_begin runs.  fold: the launch's other groups read st.chol_fail as the previous
  // iteration's, so the flag goes to ls_fail (the Cholesky's head moves it into st and clears it).
  if (fold) d.ls_fail[win] = 1;
  else if (d.sharded) d.wfail_part[win] = 1.0;
  else d.st[win].chol_fail = 1;
}

// K2b (sharded plans): per-window reduction of the point-group partials of one phase into the
// exchange buffers (PH 0: cost, point |x|^2 (sum) and point gradient max; PH 1: model cost
// change, candidate cost, point |step|^2), fixed lane order + butterfly.
template <int PH>
__global__ __launch_bounds__(64) void k_ba_win_reduce(BaDev d) {
  const int w = blockIdx.x;
  if (d.st[w].done) return;
  const BaWin& W = d.win[w];
  const int lane = threadIdx.x;
  double a = 0.0, b = 0.0, c = 0.0;
  if (PH == 0) group_partials<0, 1, 2, true>(d.part, W.pblk_base, W.n_pblk, lane, a, c, b);
  else group_partials<3, 4, 5, false>(d.part, W.pblk_base, W.n_pblk, lane, a, b, c);
  a = wave_sum(a); b = wave_sum(b);
  c = PH == 0 ? wave_max(c) : wave_sum(c);
  if (lane == 0) {
    if (PH == 0) { d.wlin_part[2 * w] = a; d.wlin_part[2 * w + 1] = b; d.wmax_part[w] = c; }
    else { d.wstep_part[3 * w] = a; d.wstep_part[3 * w + 1] = b; d.wstep_part[3 * w + 2] = c; }
  }
}

template <bool SH>
__device__ __forceinline__ void lm_begin_run(const BaDev& d, const LMOpt& o, const int w) {
  const WinState* Sp = d.st + w;
  const WinState S = *Sp;
  const BaWin W = d.win[w];  // issued with the state, before the done test
  if (S.done) return;
  (void)lm_head<SH>(d, o, w, threadIdx.x, S, W);
}
template <bool SH>
__global__ __launch_bounds__(64) void k_ba_lm_begin(BaDev d, LMOpt o) {
  lm_begin_run<SH>(d, o, blockIdx.x);
}

// the iteration's record (lorb_lm_iteration; S is the state the step was computed from)
__device__ __forceinline__ lorb_lm_iteration lm_rec(const WinState& S, int outcome, double mcc, double ncost,
                                                    double step_norm) {
  lorb_lm_iteration r;
  r.iteration = S.iter; r.outcome = outcome;
  r.cost = S.cost; r.model_cost_change = mcc; r.new_cost = ncost; r.radius = S.radius; r.step_norm = step_norm;
  return r;
}
__device__ __forceinline__ void lm_record(const BaDev& d, int w, const lorb_lm_iteration& r) {
  if (r.iteration < 1 || r.iteration > LORB_LM_TRACE_CAP) return;
  d.trace[(size_t)w * LORB_LM_TRACE_CAP + r.iteration - 1] = r;
}

// A window state copied field by field (the aggregate copy of a state that is modified in between
// leaves a memcpy through a private slot, which the backend then places in LDS: 16 B per thread)
__device__ __forceinline__ WinState state_copy(const WinState& s) {
  WinState r;
  r.radius = s.radius; r.decrease_factor = s.decrease_factor; r.cost = s.cost; r.x_norm = s.x_norm; r.gmax = s.gmax;
  r.initial_cost = s.initial_cost; r.iter = s.iter; r.n_success = s.n_success; r.n_invalid = s.n_invalid;
  r.done = s.done; r.relin = s.relin; r.cur = s.cur; r.last_successful = s.last_successful; r.term = s.term;
  r.chol_fail = s.chol_fail; r.pad = s.pad;
  return r;
}

// K8 decision (lane 0): step validity, tolerances, accept/reject.  No side effects: S becomes the
// state after the decision, rec the iteration's record; returns 1 if accepted
__device__ __forceinline__ int lm_decide(const LMOpt& o, WinState& S, bool valid, double mccs, double ncost,
                                         double sn2, lorb_lm_iteration& rec) {
  const double model_cost_change = -mccs;
  valid = valid && isfinite(model_cost_change) && isfinite(sn2) && model_cost_change > 0.0;
  if (!valid) {
    rec = lm_rec(S, LORB_LM_STEP_INVALID, model_cost_change, ncost, sqrt(sn2));
    if (++S.n_invalid >= o.max_invalid) {
      S.done = 1; S.term = LORB_TERM_FAILURE;
    } else {
      S.radius = S.radius / S.decrease_factor;
      S.decrease_factor *= 2.0;
      S.last_successful = 0;
      if (S.iter >= o.max_iter) { S.done = 1; S.term = LORB_TERM_NO_CONVERGENCE; }
    }
    return 0;
  }
  S.n_invalid = 0;
  const double new_cost = isfinite(ncost) ? ncost : 1.7976931348623157e308;
  const double step_norm = sqrt(sn2);
  if (step_norm <= o.ptol * (S.x_norm + o.ptol)) {
    rec = lm_rec(S, LORB_LM_STEP_PARAM_TOL, model_cost_change, new_cost, step_norm);
    S.done = 1; S.term = LORB_TERM_PARAMETER_TOL; return 0;
  }
  const double cost_change = S.cost - new_cost;
  if (fabs(cost_change) <= o.ftol * S.cost) {
    rec = lm_rec(S, LORB_LM_STEP_FUNC_TOL, model_cost_change, new_cost, step_norm);
    S.done = 1; S.term = LORB_TERM_FUNCTION_TOL; return 0;
  }
  const double rel = cost_change / model_cost_change;
  rec = lm_rec(S, rel > o.min_rel ? LORB_LM_STEP_ACCEPTED : LORB_LM_STEP_REJECTED, model_cost_change, new_cost,
               step_norm);
  if (rel > o.min_rel) {
    S.cur ^= 1;
    S.relin = 1;
    S.cost = new_cost;  // the accepted point's cost (k_ba_lm_begin recomputes it when relinearising)
    S.n_success++;
    const double tt = 2.0 * rel - 1.0;
    S.radius = S.radius / fmax(1.0 / 3.0, 1.0 - tt * tt * tt);
    S.radius = fmin(o.max_radius, S.radius);
    S.decrease_factor = 2.0;
  } else {
    S.last_successful = 0;
    S.radius = S.radius / S.decrease_factor;
    S.decrease_factor *= 2.0;
  }
  // the head of the next iteration would stop here (iteration budget spent): the solve needs no
  // final linearisation, S.cost is the cost at the final point
  if (S.iter >= o.max_iter) { S.done = 1; S.term = LORB_TERM_NO_CONVERGENCE; }
  return rel > o.min_rel;
}

// K8: per-window iteration tail: camera candidate, step validity, tolerances, accept/reject, on one
// wavefront (no workgroup barrier).  (Run instead by
// the last-finishing point group of the back-substitution -- a per-window counter behind agent-scope
// release / acquire fences -- it measured far slower: on the 8-XCD device those fences write back
// and invalidate L2, C4 step 1.076 -> 1.294 ms.)
// lm_end_eval is the tail without side effects: from the state S after the iteration's head (not
// done) to the state after the decision and the iteration's record, both valid in lane 0.
// k_ba_lm_end commits them (lm_end_run); the folded iteration evaluates the tail in the prologue of
// every workgroup of the next k_ba_ls, and the window's first group commits (ls_group).
template <bool SH>
__device__ __forceinline__ void lm_end_eval(const BaDev& d, const LMOpt& o, int w, int lane, WinState& S,
                                            const BaWin& W, lorb_lm_iteration& rec) {
  bool valid = !S.chol_fail;
  double mccs = 0.0, ncost = 0.0, sn2 = 0.0;
  if (valid) {
    const int cur = S.cur;
    // the first 64 cameras' poses are requested before the group partials (one round trip for both;
    // the partials' loop would otherwise keep them behind it)
    const int c0 = W.pose_base + lane;
    const bool has0 = lane < W.n_poses;
    const double* xp = cur ? d.x_pose[1] : d.x_pose[0];   // the iterate
    const double* xpn = cur ? d.x_pose[0] : d.x_pose[1];  // the candidate (written by k_ba_chol)
    double x0[6], xn0[6];
    bool act0 = false;
    if (has0) {
      act0 = d.cam_active[c0];
#pragma unroll
      for (int k = 0; k < 6; ++k) { x0[k] = xp[6 * c0 + k]; xn0[k] = xpn[6 * c0 + k]; }
    }
    if (!SH) group_partials<3, 4, 5, false>(d.part, W.pblk_base, W.n_pblk, lane, mccs, ncost, sn2);
    if (has0) {
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        if (act0) sn2 += (x0[k] - xn0[k]) * (x0[k] - xn0[k]);  // (the same order as the loop below)
      }
    }
    for (int c = c0 + 64; c < W.pose_base + W.n_poses; c += 64) {
      const bool active = d.cam_active[c];
      for (int k = 0; k < 6; ++k) {
        const double x = xp[6 * c + k];
        const double xn = xpn[6 * c + k];
        if (active) sn2 += (x - xn) * (x - xn);
      }
    }
    mccs = wave_sum(mccs); ncost = wave_sum(ncost); sn2 = wave_sum(sn2);
    if (SH) { mccs += d.wstep[3 * w]; ncost += d.wstep[3 * w + 1]; sn2 += d.wstep[3 * w + 2]; }
  }
  // point-block / Cholesky failures are per iteration: cleared here for the next one (k_ba_ls
  // sets them before k_ba_lm_begin runs)
  S.chol_fail = 0;
  // accepted: the candidate is the new linearisation point; its rotation states are in
  // rot_lin[cur ^ 1] already (the Cholesky's epilogue), so acceptance only flips cur
  if (lane == 0) (void)lm_decide(o, S, valid, mccs, ncost, sn2, rec);
}
template <bool SH>
__device__ __forceinline__ void lm_end_run(const BaDev& d, const LMOpt& o, int w, int lane) {
  const WinState* Sp = d.st + w;
  WinState S = *Sp;
  const BaWin W = d.win[w];  // issued with the state, before the done test
  if (S.done) return;
  lorb_lm_iteration rec;
  lm_end_eval<SH>(d, o, w, lane, S, W, rec);
  if (lane == 0) {
    if (SH) d.wfail_part[w] = 0.0;
    d.st[w] = S;
    lm_record(d, w, rec);
  }
}
template <bool SH>
__global__ __launch_bounds__(64) void k_ba_lm_end(BaDev d, LMOpt o) {
  lm_end_run<SH>(d, o, blockIdx.x, threadIdx.x);
}

// ==========================================================================================
// Point-major Schur path ("PM"; the only one since round 6).  Round 4's
// pair-major path materialised 34 doubles per observation and re-read them once per camera block
// pair a point takes part in (k (k + 1) / 2 pairs for a point seen k times).  Here one kernel per point group
// linearises its observations, eliminates its points and forms the group's contributions to the
// reduced camera system on chip, and writes ONE partial per (group, camera block) of its camera
// window; a second kernel sums the partials of each block in a fixed group order (deterministic, no
// FP64 atomics).  Nothing is stored per observation: the back-substitution re-evaluates the
// linearisation (the same expression on the same inputs: the same bits).
//
// Group window: the group's optimised observations see cameras [cmin, cmin + span) (plan order);
// its blocks (a, b) (a >= b, local to cmin) lie in the band a - b <= bwc (the window's camera-level
// half band), stored row by row: slot(a, dd = a - b).  Per local camera a the partial also holds
// the camera terms diag(Jc^T Jc) (6), Jc^T r (6) and Jc^T g (6).  The diagonal blocks carry
// Jc^T (I - Q Jps^T) Jc = U - A, the off-diagonal ones -A: band = sc (sum) sc^T, plus D^2 on the
// diagonal; rhs = (Jc^T r - Jc^T g) sc.
// ==========================================================================================

__device__ __forceinline__ void pm_slot_inv(int q, int bwc, int& a, int& dd) {
  const int T = (bwc + 1) * (bwc + 2) / 2;
  if (q < T) {
    a = (int)((sqrt(8.0 * q + 1.0) - 1.0) * 0.5);
    while ((a + 1) * (a + 2) / 2 <= q) ++a;
    while (a * (a + 1) / 2 > q) --a;
    dd = q - a * (a + 1) / 2;
  } else {
    const int r = q - T;
    a = bwc + 1 + r / (bwc + 1);
    dd = r - (r / (bwc + 1)) * (bwc + 1);
  }
}

constexpr int kLsThreads = kGB;
constexpr int kLsWaves = kLsThreads / 64;

// three sums (M1: the second a max) over an NW-wave workgroup: per-wave butterfly, then the waves'
// values in wave order (every thread must call it)
template <int NW, bool M1>
__device__ __forceinline__ void block_red3w(double& a, double& b, double& c, double (*red)[NW]) {
  a = wave_sum(a); b = M1 ? wave_max(b) : wave_sum(b); c = wave_sum(c);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    const int w = threadIdx.x >> 6;
    red[0][w] = a; red[1][w] = b; red[2][w] = c;
  }
  __syncthreads();
  a = red[0][0]; b = red[1][0]; c = red[2][0];
#pragma unroll
  for (int k = 1; k < NW; ++k) { a += red[0][k]; b = M1 ? fmax(b, red[1][k]) : b + red[1][k]; c += red[2][k]; }
}

// The linearisation of one observation at the current linearisation point (k_ba_ls and k_ba_bs2
// evaluate the same expression on the same inputs, so both see the same bits).
// Camera c's entry of d.rot_lin for the iterate x_pose[cur], as one opaque register: the index
// arithmetic stays out of pm_lin's two branches, which the compiler then lays out as it always has
// (k_ba_ls and k_ba_bs2 must keep their bits).
__device__ __forceinline__ int rot_idx(const BaDev& d, int cur, int c) {
  int cr = rot_off(d, cur) + c;
  asm volatile("" : "+v"(cr));
  return cr;
}
// (cr: rot_idx of camera c)
__device__ __forceinline__ void pm_lin(const BaDev& d, const BaWin& W, int cur, int cr, int p, int c, int fx, double2 uv,
                                       double (&r)[2], double (&Jp)[6], double (&Jc)[12]) {
  double X[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) X[k] = d.x_pt[cur][3 * p + k];
  if (c >= 0) {
    double tr[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) tr[k] = d.x_pose[cur][6 * c + 3 + k];
    residual_jac_s(d.rot_lin[cr], tr, X, W.fx, W.fy, W.cx, W.cy, uv.x, uv.y, r, Jp, Jc);
  } else {  // a fixed keyframe: its rotation state from k_ba_init (rot_jet of the same pose: the same bits)
    double tr[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) tr[k] = d.fixed_pose[6 * fx + 3 + k];
    residual_jac_s(d.rot_fix[fx], tr, X, W.fx, W.fy, W.cx, W.cy, uv.x, uv.y, r, Jp, Jc);
  }
}

// PM-K1: one point group per workgroup (observation threads t < kGB; kLsThreads threads for the
// block phase).  Phases:
//   A (observation)  residual + Jacobians in registers, Jp^T Jp / Jp^T r terms to LDS;
//   B (point)        E^T E, E^T r in observation order, Jacobi scale (iteration 0), the point-block
//                    prep (prep_point); the group's camera window (min / max camera);
//   C (observation)  Jps, Q = Jps E^-1, g = Q b; every optimised observation moves to its point's
//                    camera-ordered slot (rank among the point's cameras: no table);
//   D (block row)    thread = (slot, row i): sum over the group's points in point order of row i of
//                    Jc_h^T K Jc_l (K = I - Q_h Jps_l^T on the diagonal, -Q_h Jps_l^T off it), plus
//                    the camera terms on the diagonal; written to the group's partial.
// Cost, point gradient max and |x|^2 partials per group (the head reads them when relinearising).
// SUP (ls_run_sup): the group is one of a super-group's; phase D adds its blocks into the
// super-group's partial (its camera window at the super-group's offset) instead of writing its own.
struct LsSup {
  double* gsp;  // the super-group's partial
  int cmin;     // its first camera (plan numbering)
};
// a wave-uniform value out of a VGPR (the decided state comes through LDS)
__device__ __forceinline__ double uniform_d(double v) {
  const unsigned long long u = __double_as_longlong(v);
  const unsigned lo = __builtin_amdgcn_readfirstlane((int)(u & 0xffffffffu)), hi = __builtin_amdgcn_readfirstlane((int)(u >> 32));
  return __longlong_as_double(((unsigned long long)hi << 32) | lo);
}
// d.fold (a launch argument: the folded iteration tail, 1; 2: a plan of one window, whose state is
// requested before the group record arrives): the previous iteration has run no k_ba_lm_end.  One
// kernel serves both forms, so that the linearisation is the same machine code, hence the same bits,
// with the tail folded or not.  Wave 0 of every workgroup evaluates that tail for the group's window
// (lm_end_eval: the same loads in the same order, so every group decides the same bits) and hands the
// decided state to the group through LDS; the window's first group also commits it, to st2 (the
// launch's other groups still read st) with the iteration's record.  Nothing a workgroup reads here
// is written by this launch.
template <bool SUP>
__device__ __forceinline__ void ls_group(const BaDev& d, const LMOpt& o, const unsigned bid, const LsSup& su) {
  const int fold = SUP ? 0 : d.fold;  // (partial runs keep the k_ba_lm_end kernel)
  __shared__ double s_jc[kGB][12];   // B / C: per point Ei (0..5), bs (6..8), sp (9..11); D: Jc per slot
  __shared__ double s_qj[kGB][12];   // A / B: Jp^T Jp (6) | Jp^T r (3) per observation; D: Q | Jps per slot
  __shared__ double s_rg[kGB][4];    // D: r | g per slot
  __shared__ unsigned long long s_mask[2][kGB];  // per point: its cameras, bits a - cmin (two words: spans <= 128)
  __shared__ int s_po[kGB];
  __shared__ int s_mm[2][kLsWaves];
  __shared__ double red3[3][kLsWaves];
#ifdef LORB_LS_STAMPS
  // dbg[8 g + k]: s_memtime at the kernel's entry (k 0) and after phase A (1), B (2), C (3), D (4),
  // the partial sums (5) of group g (thread 0)
#define LS_STAMP(k) do { if (threadIdx.x == 0) d.dbg[8 * bid + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define LS_STAMP(k) do {} while (0)
#endif
  LS_STAMP(0);
#ifdef LORB_LS_STAMPS
  // where the group ran: HW_ID (hwreg 4) << 8 | XCC_ID (hwreg 20); when: the 100 MHz real-time
  // counter at the start (<< 20) | the ticks to the end (slot 7, written at LS_STAMP(5))
  const unsigned long long ls_rt0 = __builtin_amdgcn_s_memrealtime();
  if (threadIdx.x == 0)
    d.dbg[8 * bid + 6] = ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) << 8) |
                                (__builtin_amdgcn_s_getreg((31 << 11) | 20) & 255);
#endif
  // fold == 2: the window is 0, so its state and the tail's part of its layout are requested with
  // the group record, not after it (the fold then adds one dependent round trip, the tail's loads)
  WinState S0{};
  BaWin W0{};  // (pose_base, n_poses, pblk_base, n_pblk: what lm_end_eval reads)
  if (fold == 2) {
    S0 = state_copy(d.st[0]);
    W0.pose_base = d.win[0].pose_base; W0.n_poses = d.win[0].n_poses;
    W0.pblk_base = d.win[0].pblk_base; W0.n_pblk = d.win[0].n_pblk;
  }
  const PBlk g = d.pblk[bid];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const bool has = t < g.no;
  const int of = g.o0 + min(t, max(g.no - 1, 0));
  const int p_ = has ? d.obs_pt[of] : 0, c_ = has ? d.obs_cam[of] : -1;
  const int fx_ = has ? d.obs_fix[of] : 0;
  const double2 uv = has ? d.obs_uv[of] : make_double2(0.0, 0.0);
  int po0 = 0, po1 = 0;
  // the point phase's global inputs (both iterates: cur is not known yet) go out with the group's
  double Xp[2][3] = {{0, 0, 0}, {0, 0, 0}}, spp[3] = {0, 0, 0};
  if (t < g.cnt) {
    const int p = g.p0 + t;
    po0 = d.pt_obs_off[p]; po1 = d.pt_obs_off[p + 1];
#pragma unroll
    for (int k = 0; k < 3; ++k) { Xp[0][k] = d.x_pt[0][3 * p + k]; Xp[1][k] = d.x_pt[1][3 * p + k]; spp[k] = d.scale_pt[3 * p + k]; }
  }
  __shared__ WinState s_dec;
  int win = 0;
  if (fold != 2) {
    win = g.win;
    S0 = state_copy(d.st[win]);
    if (fold) {
      W0.pose_base = d.win[win].pose_base; W0.n_poses = d.win[win].n_poses;
      W0.pblk_base = d.win[win].pblk_base; W0.n_pblk = d.win[win].n_pblk;
    }
  }
  if (S0.done) return;
  const BaWin& W = d.win[win];
  int cur = S0.cur, iter = S0.iter;
  double rad = S0.radius;
  if (fold) {
    if (wv == 0) {
      WinState Sn = S0;
      lorb_lm_iteration rec;
      lm_end_eval<false>(d, o, win, lane, Sn, W0, rec);
      if (lane == 0) {
        s_dec = Sn;
        if ((int)bid == W0.pblk_base) { d.st2[win] = Sn; lm_record(d, win, rec); }
      }
    }
    __syncthreads();
    if (__builtin_amdgcn_readfirstlane(s_dec.done)) return;
    cur = __builtin_amdgcn_readfirstlane(s_dec.cur);
    iter = __builtin_amdgcn_readfirstlane(s_dec.iter);
    rad = uniform_d(s_dec.radius);
  }
  if (t < kGB) { s_mask[0][t] = 0ull; s_mask[1][t] = 0ull; }
  // A
  double r[2] = {0, 0}, Jp[6] = {0, 0, 0, 0, 0, 0}, Jc[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) Jc[k] = 0.0;
  double cost = 0.0;
  if (has) {
    pm_lin(d, W, cur, rot_idx(d, cur, c_), p_, c_, fx_, uv, r, Jp, Jc);
    cost = 0.5 * (r[0] * r[0] + r[1] * r[1]);
    double* v = s_qj[t];
    v[0] = Jp[0] * Jp[0] + Jp[3] * Jp[3]; v[1] = Jp[0] * Jp[1] + Jp[3] * Jp[4];
    v[2] = Jp[0] * Jp[2] + Jp[3] * Jp[5]; v[3] = Jp[1] * Jp[1] + Jp[4] * Jp[4];
    v[4] = Jp[1] * Jp[2] + Jp[4] * Jp[5]; v[5] = Jp[2] * Jp[2] + Jp[5] * Jp[5];
    v[6] = Jp[0] * r[0] + Jp[3] * r[1]; v[7] = Jp[1] * r[0] + Jp[4] * r[1];
    v[8] = Jp[2] * r[0] + Jp[5] * r[1];
  }
  {
    int mn = has && c_ >= 0 ? c_ : 0x7fffffff, mx = has && c_ >= 0 ? c_ : -1;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) { mn = min(mn, __shfl_xor(mn, s, 64)); mx = max(mx, __shfl_xor(mx, s, 64)); }
    if (lane == 0) { s_mm[0][wv] = mn; s_mm[1][wv] = mx; }
  }
  __syncthreads();
  LS_STAMP(1);
  int cmin = s_mm[0][0], cmax = s_mm[1][0];
#pragma unroll
  for (int k = 1; k < kLsWaves; ++k) { cmin = min(cmin, s_mm[0][k]); cmax = max(cmax, s_mm[1][k]); }
  const int span = cmax >= 0 ? cmax - cmin + 1 : 0;
  // B (point t) -- and the observations' camera bits
  double gm = 0.0, xn2 = 0.0;
  if (t < g.cnt) {
    const int p = g.p0 + t;
    double E[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0};
    for (int e = po0 - g.o0; e < po1 - g.o0; ++e) {
      const double* v = s_qj[e];
#pragma unroll
      for (int k = 0; k < 6; ++k) E[k] += v[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) b[k] += v[6 + k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) d.etb[3 * p + k] = b[k];
    double sp[3];
    if (iter == 0) {
      sp[0] = 1.0 / (1.0 + sqrt(E[0]));
      sp[1] = 1.0 / (1.0 + sqrt(E[3]));
      sp[2] = 1.0 / (1.0 + sqrt(E[5]));
#pragma unroll
      for (int k = 0; k < 3; ++k) d.scale_pt[3 * p + k] = sp[k];
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) sp[k] = spp[k];
    }
    if (po1 > po0) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double X = cur ? Xp[1][k] : Xp[0][k];
        gm = fmax(gm, fabs(X - (X + -b[k])));
        xn2 += X * X;
      }
    }
    double Ei[6], bs[3];
    if (!prep_point(E, b, sp, rad, o, Ei, bs)) prep_fail(d, win, fold);
#pragma unroll
    for (int k = 0; k < 6; ++k) { d.pinv[6 * p + k] = Ei[k]; s_jc[t][k] = Ei[k]; }
#pragma unroll
    for (int k = 0; k < 3; ++k) { s_jc[t][6 + k] = bs[k]; s_jc[t][9 + k] = sp[k]; }
    s_po[t] = po0 - g.o0;
  }
  const int lp = p_ - g.p0;
  const int a_ = c_ - cmin;
  if (has && c_ >= 0) atomicOr(&s_mask[a_ >> 6][lp], 1ull << (a_ & 63));
  __syncthreads();
  LS_STAMP(2);
  // C: Jps, Q, g (reads the point data), then the camera-ordered slot
  double Q[6], Js[6], g0 = 0.0, g1 = 0.0;
  int slot = -1;
  if (has && c_ >= 0) {
    const double* pt = s_jc[lp];
#pragma unroll
    for (int k = 0; k < 6; ++k) Js[k] = Jp[k] * pt[9 + k % 3];
#pragma unroll
    for (int rr = 0; rr < 2; ++rr)
#pragma unroll
      for (int j = 0; j < 3; ++j)
        Q[3 * rr + j] = Js[3 * rr] * s3(pt, 0, j) + Js[3 * rr + 1] * s3(pt, 1, j) + Js[3 * rr + 2] * s3(pt, 2, j);
    g0 = Q[0] * pt[6] + Q[1] * pt[7] + Q[2] * pt[8];
    g1 = Q[3] * pt[6] + Q[4] * pt[7] + Q[5] * pt[8];
    const unsigned long long m0 = s_mask[0][lp];
    slot = s_po[lp] + (a_ < 64 ? __popcll(m0 & ((1ull << a_) - 1ull))
                               : __popcll(m0) + __popcll(s_mask[1][lp] & ((1ull << (a_ - 64)) - 1ull)));
  }
  __syncthreads();
  if (slot >= 0) {
#pragma unroll
    for (int k = 0; k < 12; ++k) s_jc[slot][k] = Jc[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) { s_qj[slot][k] = Q[k]; s_qj[slot][6 + k] = Js[k]; }
    s_rg[slot][0] = r[0]; s_rg[slot][1] = r[1]; s_rg[slot][2] = g0; s_rg[slot][3] = g1;
  }
  __syncthreads();
  LS_STAMP(3);
  // D
  const int bwc = W.bwc, nsl = pm_nslots(span, bwc);
  double* gp = SUP ? su.gsp : d.gpart + W.part_base + (size_t)(bid - W.sg_base) * W.part_stride;
  const int aoff = SUP ? cmin - su.cmin : 0;  // the group's first camera in the super-group's window
  if (!SUP && t == 0) d.gspan[bid] = make_int2(span > 0 ? cmin - W.pose_base : 0, span);
  // Lane = slot (its whole 6 x 6 block: the point's loads serve 36 outputs), wave = point subset:
  // every lane of a wave walks the same points (k = wave, wave + 4, ...: a uniform loop, so the next
  // point's mask / offset are requested before this point's FMAs), a lane whose two cameras the
  // point does not share sits the point out.  The four waves' blocks are then summed in wave order
  // through LDS (the observation data is dead by then).  More than 64 slots: waves take 64-slot
  // chunks over all points instead (no point split, no cross-wave sum).
  // A group of few slots (a window's newest points: many points, 1 - 4 cameras) would leave most
  // lanes idle through a long point loop: there R = 2^lr lanes share a slot (R nsl <= 64), lane =
  // (slot, point subset), and their sums are combined by a butterfly (fixed order) first.
  const bool split = nsl <= 64;
  int lr = 0;
  if (split) while (lr < 6 && (nsl << (lr + 1)) <= 64) ++lr;
  const int nrounds = split ? 1 : (nsl + 64 * kLsWaves - 1) / (64 * kLsWaves);
  for (int rd = 0; rd < nrounds; ++rd) {
    const int q = split ? lane >> lr : 64 * (kLsWaves * rd + wv) + lane;
    const int rr = split ? lane & ((1 << lr) - 1) : 0;
    const bool act = q < nsl;
    int a = 0, dd = 0;
    if (act) pm_slot_inv(q, bwc, a, dd);
    const int b = a - dd;
    const bool dg = dd == 0;
    double acc[36], ex[18];
#pragma unroll
    for (int k = 0; k < 36; ++k) acc[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 18; ++k) ex[k] = 0.0;
    const int k0 = split ? (wv << lr) + rr : 0, kst = split ? kLsWaves << lr : 1;
    // the point loop, for group windows of <= 64 cameras (one mask word) or up to 128 (two: the
    // lane's two cameras pick their word, a rank in the high word adds the low word's count)
    auto point_loop = [&](auto wide_tag) {
      constexpr bool kWide = decltype(wide_tag)::value;
      const int wa = kWide ? a >> 6 : 0, wb = kWide ? b >> 6 : 0;
      const unsigned long long ba = act ? 1ull << (a & 63) : 0ull, bb = 1ull << (b & 63);
      unsigned long long m = s_mask[0][k0], mh = kWide ? s_mask[1][k0] : 0ull;
      int po = s_po[k0];
      for (int k = k0; k < g.cnt; k += kst) {
        const unsigned long long mc = m, mch = mh;
        const int pc = po;
        if (k + kst < g.cnt) {  // the next point's
          m = s_mask[0][k + kst]; po = s_po[k + kst];
          if (kWide) mh = s_mask[1][k + kst];
        }
        const unsigned long long ma = kWide && wa ? mch : mc, mb = kWide && wb ? mch : mc;
        if ((ma & ba) && (mb & bb)) {
          const int lo = kWide ? __popcll(mc) : 0;
          const int eh = pc + (kWide && wa ? lo : 0) + __popcll(ma & (ba - 1ull));
          const int el = pc + (kWide && wb ? lo : 0) + __popcll(mb & (bb - 1ull));
          const double* Qh = s_qj[eh];
          const double* Jl = s_qj[el] + 6;
          const double* Ch = s_jc[eh];
          const double* Cl = s_jc[el];
          double k00 = -(Qh[0] * Jl[0] + Qh[1] * Jl[1] + Qh[2] * Jl[2]);
          double k01 = -(Qh[0] * Jl[3] + Qh[1] * Jl[4] + Qh[2] * Jl[5]);
          double k10 = -(Qh[3] * Jl[0] + Qh[4] * Jl[1] + Qh[5] * Jl[2]);
          double k11 = -(Qh[3] * Jl[3] + Qh[4] * Jl[4] + Qh[5] * Jl[5]);
          if (dg) { k00 += 1.0; k11 += 1.0; }
          double cl[12], ch[12];
#pragma unroll
          for (int j = 0; j < 12; ++j) { cl[j] = Cl[j]; ch[j] = Ch[j]; }
#pragma unroll
          for (int i = 0; i < 6; ++i) {
            const double z0 = ch[i] * k00 + ch[6 + i] * k10, z1 = ch[i] * k01 + ch[6 + i] * k11;
#pragma unroll
            for (int j = 0; j < 6; ++j) acc[6 * i + j] = fma(z0, cl[j], fma(z1, cl[6 + j], acc[6 * i + j]));
          }
          if (dg) {
            const double* rg = s_rg[eh];
            const double g0r = rg[0], g1r = rg[1], g2r = rg[2], g3r = rg[3];
#pragma unroll
            for (int i = 0; i < 6; ++i) {
              ex[i] = fma(ch[i], ch[i], fma(ch[6 + i], ch[6 + i], ex[i]));
              ex[6 + i] = fma(ch[i], g0r, fma(ch[6 + i], g1r, ex[6 + i]));
              ex[12 + i] = fma(ch[i], g2r, fma(ch[6 + i], g3r, ex[12 + i]));
            }
          }
        }
      }
    };
    if (k0 < g.cnt) {
      if (span > 64) point_loop(std::true_type{});
      else point_loop(std::false_type{});
    }
    for (int m = 1; m < (1 << lr); m <<= 1) {  // the slot's R subsets (lr = 0 unless split)
#pragma unroll
      for (int k = 0; k < 36; ++k) acc[k] += __shfl_xor(acc[k], m, 64);
#pragma unroll
      for (int k = 0; k < 18; ++k) ex[k] += __shfl_xor(ex[k], m, 64);
    }
    const bool own = act && rr == 0;  // the slot's lane after the butterfly
    if (split) {
      // ((w0 + w1) + w2) + w3 through 64 x 36 + 64 x 18 buffers over the dead observation data
      static_assert(64 * 36 <= kGB * 12 && 64 * 18 <= kGB * 12, "reduction buffers");
      __syncthreads();
#pragma unroll
      for (int w = 0; w < kLsWaves; ++w) {
        if (wv == w && own) {
          double* bl = &s_jc[0][0] + 36 * q;
          double* bx = &s_qj[0][0] + 18 * q;
#pragma unroll
          for (int k = 0; k < 36; ++k) { if (w > 0) acc[k] += bl[k]; if (w + 1 < kLsWaves) bl[k] = acc[k]; }
          if (dg) {
#pragma unroll
            for (int k = 0; k < 18; ++k) { if (w > 0) ex[k] += bx[k]; if (w + 1 < kLsWaves) bx[k] = ex[k]; }
          }
        }
        if (w + 1 < kLsWaves) __syncthreads();
      }
    }
    if (own && (!split || wv == kLsWaves - 1)) {
      if (SUP) {  // added in group order into the super-group's partial (zeroed by ls_run_sup)
        double* out = gp + 36 * pm_slot(a + aoff, dd, bwc);
#pragma unroll
        for (int k = 0; k < 36; ++k) out[k] = out[k] + acc[k];
        if (dg) {
          double* gc = gp + W.part_cam + 18 * (a + aoff);
#pragma unroll
          for (int k = 0; k < 18; ++k) gc[k] = gc[k] + ex[k];
        }
      } else {
        double* out = gp + 36 * q;
#pragma unroll
        for (int k = 0; k < 36; ++k) out[k] = acc[k];
        if (dg) {
          double* gc = gp + W.part_cam + 18 * a;
#pragma unroll
          for (int k = 0; k < 18; ++k) gc[k] = ex[k];
        }
      }
    }
  }
  LS_STAMP(4);
  block_red3w<kLsWaves, true>(cost, gm, xn2, red3);
  if (t == 0) { double* P = d.part + 8 * bid; P[0] = cost; P[1] = gm; P[2] = xn2; }
  LS_STAMP(5);
#ifdef LORB_LS_STAMPS
  if (t == 0) d.dbg[8 * bid + 7] = (ls_rt0 << 20) | ((__builtin_amdgcn_s_memrealtime() - ls_rt0) & 0xfffff);
#endif
#undef LS_STAMP
}
__device__ __forceinline__ void ls_run(const BaDev& d, const LMOpt& o, const unsigned bid) {
  if ((int)bid >= d.live[0]) return;
  ls_group<false>(d, o, bid, LsSup{nullptr, 0});
}
__global__ __launch_bounds__(kLsThreads) void k_ba_ls(BaDev d, LMOpt o) { ls_run(d, o, blockIdx.x); }

// Super-group sid: its point groups one after another in one workgroup, their camera-block sums
// added in group order into ONE partial over the union of their camera windows (a window with more
// point groups than two workgroups per CU take in one round: VERDICT r05 item 2, the partials' HBM
// round trip).  The union window comes from the super-group's observations (one pass); its region
// of the partial is zeroed first.
__device__ __forceinline__ void ls_run_sup(const BaDev& d, const LMOpt& o, const unsigned sid) {
  __shared__ int s_r[2][kLsWaves];
  if ((int)sid >= d.live[2]) return;
  const int4 sg = d.sgrp[sid];
  const WinState& S = d.st[sg.x];
  if (S.done) return;
  const BaWin& W = d.win[sg.x];
  const PBlk gf = d.pblk[sg.y], gl = d.pblk[sg.y + sg.z - 1];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  int mn = 0x7fffffff, mx = -1;
  for (int e = gf.o0 + t; e < gl.o0 + gl.no; e += kLsThreads) {
    const int c = d.obs_cam[e];
    if (c >= 0) { mn = min(mn, c); mx = max(mx, c); }
  }
#pragma unroll
  for (int k = 32; k > 0; k >>= 1) { mn = min(mn, __shfl_xor(mn, k, 64)); mx = max(mx, __shfl_xor(mx, k, 64)); }
  if (lane == 0) { s_r[0][wv] = mn; s_r[1][wv] = mx; }
  __syncthreads();
  int cmin = s_r[0][0], cmax = s_r[1][0];
#pragma unroll
  for (int k = 1; k < kLsWaves; ++k) { cmin = min(cmin, s_r[0][k]); cmax = max(cmax, s_r[1][k]); }
  const int span = cmax >= 0 ? cmax - cmin + 1 : 0;
  double* gsp = d.gpart + W.part_base + (size_t)(sid - W.sg_base) * W.part_stride;
  const int nb = 36 * pm_nslots(span, W.bwc), nc = 18 * span;
  for (int i = t; i < nb + nc; i += kLsThreads) gsp[i < nb ? i : W.part_cam + (i - nb)] = 0.0;
  if (t == 0) d.gspan[sid] = make_int2(span > 0 ? cmin - W.pose_base : 0, span);
  __syncthreads();
  for (int k = 0; k < sg.z; ++k) ls_group<true>(d, o, sg.y + k, LsSup{gsp, cmin});
}
__global__ __launch_bounds__(kLsThreads) __attribute__((amdgpu_waves_per_eu(2))) void k_ba_ls_sup(BaDev d, LMOpt o) {
  ls_run_sup(d, o, blockIdx.x);
}

// PM-K2: one workgroup per camera block (h, l) of a window: the partials of the window's groups
// whose camera window holds the block, summed in group order.  Thread = (entry e, subset s); the
// candidate groups of each 256-group chunk are compacted in order, subset s takes every nsub-th.
// MODE 0: the camera terms of the diagonal blocks only (U diag, V: the iteration head's inputs,
//         before k_ba_lm_begin fixes the iteration-0 Jacobi scale);
// MODE 1: the band with D^2 on the diagonal (rank 0) and the rhs (V - R) sc (round 4's pair-major
//         result, for the Cholesky without a head);
// MODE 2: the fused iteration: band without D^2 (k_ba_chol_2s<true> adds it), rhs, U diag and V.
// RT threads per block (256 or 1024: red_threads() picks per plan -- 1024 when a block has many
// candidate groups, or the grid leaves CUs idle; 256 when many blocks share the GPU)
template <int MODE, int RT>
__device__ __forceinline__ void red_run(const BaDev& d, const LMOpt& o, const unsigned bid) {
  constexpr int kRt = RT, kRw = kRt / 64;
  constexpr int kRc = 1024 / kRt;  // groups per thread per chunk: 1024 groups' windows requested at once
  __shared__ int s_cand[kRt * kRc];
  __shared__ int s_a[kRt * kRc];
  __shared__ int s_wc[kRc][kRw];
  __shared__ double s_acc[1024];
  __shared__ double s_tot[54];
  if ((int)bid >= d.live[1]) return;
  const BlockPair bp = d.bp[bid];
  const bool diag = bp.ch == bp.cl;
  if (MODE == 0 && !diag) return;
  const WinState& S = (d.fold ? d.st2 : d.st)[bp.win];  // (fold: the state k_ba_ls decided)
  const BaWin& W = d.win[bp.win];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  // the finalisation's scales (and MODE 1's camera diagonal) go out with the state
  const int fi = t < 36 ? t / 6 : (t < 42 ? t - 36 : 0), fj = t < 36 ? t % 6 : 0;
  double sci = 1.0, scj = 1.0, udg = 0.0;
  if (MODE != 0) {
    sci = d.scale_pose[6 * bp.ch + fi];
    scj = d.scale_pose[6 * bp.cl + fj];
    if (MODE == 1 && diag) udg = d.U[21 * bp.ch + u21(fi, fi)];
  }
  // (fold: st done -- the head ended the solve earlier -- leaves st2 stale; both requested at once)
  if (S.done | d.st[bp.win].done) return;
  const int h = bp.ch - W.pose_base, l = bp.cl - W.pose_base, dd = h - l;
  // entries: [0, 36) the block, [36, 54) the camera terms (U diag, V, R); MODE 0: U diag, V only
  const int e0 = MODE == 0 ? 36 : 0, ne = MODE == 0 ? 12 : (diag ? 54 : 36);
  // The sum's shape does not depend on the width: candidate j of a chunk belongs to subset j mod NS
  // (NS = 1024 / ne, the subsets a 1024-thread block runs one per thread), each subset sums its
  // candidates in order, and the subsets are combined in a fixed tree -- so the 256-, 512- and
  // 1024-thread kernels give the same bits (a window solved alone or batched with others takes the
  // same band).  A narrower block runs up to kSp subsets per thread.
  const int NS = 1024 / ne;
  const int nsub = kRt / ne, e = t % ne, sub = t / ne;
  constexpr int kSp = RT >= 1024 ? 1 : RT >= 512 ? 3 : 5;  // ceil(NS / nsub) for ne in {12, 36, 54}
  double acc[kSp];
#pragma unroll
  for (int q = 0; q < kSp; ++q) acc[q] = 0.0;
  const int g0 = W.sg_base, ng = W.n_sg;
  for (int c0 = 0; c0 < ng; c0 += kRt * kRc) {
    int2 gs[kRc];
#pragma unroll
    for (int u = 0; u < kRc; ++u) {
      const int gi = c0 + kRt * u + t;
      gs[u] = gi < ng ? d.gspan[g0 + gi] : make_int2(0, 0);
    }
    unsigned long long bal[kRc];
#pragma unroll
    for (int u = 0; u < kRc; ++u) {
      const bool cand = gs[u].y > 0 && gs[u].x <= l && h < gs[u].x + gs[u].y;
      bal[u] = __ballot(cand);
      if (lane == 0) s_wc[u][wv] = __popcll(bal[u]);
    }
    __syncthreads();
    // candidates in group order: sub-chunk u, then wave, then lane
    int pre = 0, nc = 0;
#pragma unroll
    for (int u = 0; u < kRc; ++u)
#pragma unroll
      for (int k = 0; k < kRw; ++k) nc += s_wc[u][k];
#pragma unroll
    for (int u = 0; u < kRc; ++u) {
      int pu = pre;
#pragma unroll
      for (int k = 0; k < kRw; ++k) pu += k < wv ? s_wc[u][k] : 0;
      if ((bal[u] >> lane) & 1ull) {
        const int j = pu + __popcll(bal[u] & ((1ull << lane) - 1ull));
        s_cand[j] = c0 + kRt * u + t;
        s_a[j] = h - gs[u].x;
      }
#pragma unroll
      for (int k = 0; k < kRw; ++k) pre += s_wc[u][k];
    }
    __syncthreads();
    if (sub < nsub) {
      const int ee = e0 + e;
      auto at = [&](int j) -> const double* {
        const double* gp = d.gpart + W.part_base + (size_t)s_cand[j] * W.part_stride;
        const int a = s_a[j];
        return ee < 36 ? gp + 36 * pm_slot(a, dd, W.bwc) + ee : gp + W.part_cam + 18 * a + (ee - 36);
      };
      // kRu candidates' loads in flight before they are added (in candidate order: the same sum)
      // (a short last batch adds exact zeros for its missing candidates: the same sum)
      // the thread's subsets advance together, kRu candidates each per round (kSp x kRu loads in
      // flight); every subset still adds its candidates in order
      constexpr int kRu = RT >= 1024 ? 8 : RT >= 512 ? 4 : 2;
      for (int b0 = 0;; b0 += kRu) {
        double v[kSp][kRu];
        bool more = false;
#pragma unroll
        for (int q = 0; q < kSp; ++q) {
          const int s0 = sub + q * nsub;
#pragma unroll
          for (int u = 0; u < kRu; ++u) {
            const int j = s0 + (b0 + u) * NS;
            v[q][u] = s0 < NS && j < nc ? *at(j) : 0.0;
          }
          more |= s0 < NS && s0 + (b0 + kRu) * NS < nc;
        }
#pragma unroll
        for (int q = 0; q < kSp; ++q)
#pragma unroll
          for (int u = 0; u < kRu; ++u) acc[q] += v[q][u];
        if (!more) break;
      }
    }
    __syncthreads();
  }
  if (sub < nsub) {
#pragma unroll
    for (int q = 0; q < kSp; ++q) {
      const int s0 = sub + q * nsub;
      if (s0 < NS) s_acc[e + s0 * ne] = acc[q];
    }
  }
  __syncthreads();
  if (t < ne) {  // the subsets' sums: four interleaved partial sums, then their pairs
    double v4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int s = 0; s < NS; ++s) v4[s & 3] += s_acc[t + s * ne];
    s_tot[t] = (v4[0] + v4[1]) + (v4[2] + v4[3]);
  }
  __syncthreads();
  const int c = bp.ch;
  if (MODE == 0) {
    if (t < 6) d.U_part[21 * c + u21(t, t)] = s_tot[t];
    else if (t < 12) d.V_part[6 * c + t - 6] = s_tot[t];
    return;
  }
  double* A = d.env_part + W.env_base;
  if (t < 36) {
    const int i = fi, j = fj;
    if (!diag || j <= i) {
      double v = s_tot[t] * sci * scj;
      if (MODE == 1 && diag && i == j && d.rank0) {
        const double u = udg * sci * sci;
        v += fmin(fmax(u, o.min_diag), o.max_diag) / S.radius;
      }
      band(A, W.bw, 6 * h + i, 6 * l + j) = v;
    }
  } else if (diag && t < 42) {
    const int i = fi;
    d.rhs_part[W.row_base + 6 * h + i] = (s_tot[42 + i] - s_tot[48 + i]) * sci;
    if (MODE == 2) { d.U_part[21 * c + u21(i, i)] = s_tot[36 + i]; d.V_part[6 * c + i] = s_tot[42 + i]; }
  }
}
template <int MODE, int RT>
__global__ __launch_bounds__(RT) void k_ba_red(BaDev d, LMOpt o) { red_run<MODE, RT>(d, o, blockIdx.x); }

// PM-K3: point-group back-substitution with the linearisation re-evaluated
// in registers instead of read back: b_p -= sum_e Jps_e^T (Jc_e y_c(e)), the point step and
// candidate, then the model cost change and the candidate cost per observation.
__device__ __forceinline__ void bs2_run(const BaDev& d, const unsigned bid) {
  __shared__ double sh[kGB][3], sst[kGB][3], sxn[kGB][3], ssp[kGB][3];
  __shared__ double red3[3][kGW];
  if ((int)bid >= d.live[0]) return;
  const PBlk g = d.pblk[bid];
  const int t = threadIdx.x;
  const bool has = t < g.no;
  const int of = g.o0 + min(t, max(g.no - 1, 0));
  const int p_ = has ? d.obs_pt[of] : 0, c_ = has ? d.obs_cam[of] : -1;
  const int fx_ = has ? d.obs_fix[of] : 0;
  const double2 uv = has ? d.obs_uv[of] : make_double2(0.0, 0.0);
  double b[3] = {0, 0, 0}, sp[3] = {0, 0, 0}, Xa[3] = {0, 0, 0}, Xb[3] = {0, 0, 0};
  double Ei[6] = {0, 0, 0, 0, 0, 0};
  int po0 = 0, po1 = 0;
  if (t < g.cnt) {
    const int p = g.p0 + t;
    po0 = d.pt_obs_off[p]; po1 = d.pt_obs_off[p + 1];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      sp[k] = d.scale_pt[3 * p + k];
      b[k] = d.etb[3 * p + k] * sp[k];
      Xa[k] = d.x_pt[0][3 * p + k];
      Xb[k] = d.x_pt[1][3 * p + k];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) Ei[k] = d.pinv[6 * p + k];
  }
  const WinState& S = d.st[g.win];
  if (S.done || S.chol_fail) return;
  const BaWin& W = d.win[g.win];
  const int cur = S.cur;
  if (t < g.cnt) {
#pragma unroll
    for (int k = 0; k < 3; ++k) ssp[t][k] = sp[k];
  }
  // every camera-indexed input (the step y, the Jacobi scale, the candidate pose) goes out with the
  // linearisation's: one dependent round trip after the observation's indices
  double ys[6] = {0, 0, 0, 0, 0, 0}, tc[3] = {0, 0, 0};
  lorb::RotVal Rc{};
  if (has && c_ >= 0) {
    const double* y = d.ycam + W.row_base + 6 * (c_ - W.pose_base);
#pragma unroll
    for (int i = 0; i < 6; ++i) ys[i] = y[i] * d.scale_pose[6 * c_ + i];
    Rc = d.rot_cand[c_];
#pragma unroll
    for (int k = 0; k < 3; ++k) tc[k] = d.x_pose[cur ^ 1][6 * c_ + 3 + k];
  }
  double r[2] = {0, 0}, Jp[6] = {0, 0, 0, 0, 0, 0}, Jc[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) Jc[k] = 0.0;
  if (has) pm_lin(d, W, cur, rot_idx(d, cur, c_), p_, c_, fx_, uv, r, Jp, Jc);
  const int lp = p_ - g.p0;
  __syncthreads();
  // W^T y = Jps^T (Jcs y): this observation's push into its point's rhs
  double ya0 = 0.0, ya1 = 0.0;
  if (has) {
    if (c_ >= 0) {
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        ya0 += Jc[i] * ys[i];
        ya1 += Jc[6 + i] * ys[i];
      }
#pragma unroll
      for (int j = 0; j < 3; ++j) sh[t][j] = (Jp[j] * ssp[lp][j]) * ya0 + (Jp[3 + j] * ssp[lp][j]) * ya1;
    } else {
      sh[t][0] = sh[t][1] = sh[t][2] = 0.0;
    }
  }
  __syncthreads();
  double sn2 = 0.0;
  if (t < g.cnt) {
    const int p = g.p0 + t;
    for (int e = po0 - g.o0; e < po1 - g.o0; ++e) {
#pragma unroll
      for (int j = 0; j < 3; ++j) b[j] -= sh[e][j];
    }
    double X[3], step[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) X[k] = cur ? Xb[k] : Xa[k];
#pragma unroll
    for (int j = 0; j < 3; ++j)
      step[j] = -(s3(Ei, j, 0) * b[0] + s3(Ei, j, 1) * b[1] + s3(Ei, j, 2) * b[2]);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double xn = X[j] + step[j] * sp[j];
      d.x_pt[cur ^ 1][3 * p + j] = xn;
      sxn[t][j] = xn;
      sst[t][j] = step[j] * sp[j];
      if (po1 > po0) sn2 += (X[j] - xn) * (X[j] - xn);
    }
  }
  __syncthreads();
  double mcc = 0.0, ncost = 0.0;
  if (has) {
    const double Xn[3] = {sxn[lp][0], sxn[lp][1], sxn[lp][2]};
    double m0 = 0.0, m1 = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      m0 += Jp[j] * sst[lp][j];
      m1 += Jp[3 + j] * sst[lp][j];
    }
    double rn[2];
    if (c_ >= 0) {
      m0 -= ya0;
      m1 -= ya1;
      residual_s(Rc, tc, Xn, W.fx, W.fy, W.cx, W.cy, uv.x, uv.y, rn);
    } else {
      double tr[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) tr[k] = d.fixed_pose[6 * fx_ + 3 + k];
      residual_s(d.rotv_fix[fx_], tr, Xn, W.fx, W.fy, W.cx, W.cy, uv.x, uv.y, rn);
    }
    mcc = m0 * (r[0] + m0 / 2.0) + m1 * (r[1] + m1 / 2.0);
    ncost = 0.5 * (rn[0] * rn[0] + rn[1] * rn[1]);
  }
  block_red3<false>(mcc, ncost, sn2, red3);
  if (t == 0) {
    double* P = d.part + 8 * bid;
    P[3] = mcc; P[4] = ncost; P[5] = sn2;
  }
}
__global__ __launch_bounds__(kGB) void k_ba_bs2(BaDev d) { bs2_run(d, blockIdx.x); }

__global__ __launch_bounds__(256) void k_ba_init_g(BaGrp g, GrpGrid G, GrpInit a, LMOpt o) {
  unsigned lb;
  const int k = grp_member(G, g.n, blockIdx.x, lb);
  init_run(g.d[k], a.W[k], a.ctot[k], a.n_pt[k], a.nf[k], o, (int)(lb * 256 + threadIdx.x),
           (G.pre[k + 1] - G.pre[k]) * 256);
}
__global__ __launch_bounds__(kLsThreads) void k_ba_ls_g(BaGrp g, GrpGrid G, LMOpt o) {
  unsigned lb;
  const int k = grp_member(G, g.n, blockIdx.x, lb);
  ls_run(g.d[k], o, lb);
}
template <int MODE, int RT>
__global__ __launch_bounds__(RT) void k_ba_red_g(BaGrp g, GrpGrid G, LMOpt o) {
  unsigned lb;
  const int k = grp_member(G, g.n, blockIdx.x, lb);
  red_run<MODE, RT>(g.d[k], o, lb);
}
__global__ __launch_bounds__(64) void k_ba_lm_begin_g(BaGrp g, GrpGrid G, LMOpt o) {
  unsigned lb;
  const int k = grp_member(G, g.n, blockIdx.x, lb);
  lm_begin_run<false>(g.d[k], o, (int)lb);
}
__global__ __launch_bounds__(kGB) void k_ba_bs2_g(BaGrp g, GrpGrid G) {
  unsigned lb;
  const int k = grp_member(G, g.n, blockIdx.x, lb);
  bs2_run(g.d[k], lb);
}
__global__ __launch_bounds__(64) void k_ba_lm_end_g(BaGrp g, GrpGrid G, LMOpt o) {
  unsigned lb;
  const int k = grp_member(G, g.n, blockIdx.x, lb);
  lm_end_run<false>(g.d[k], o, (int)lb, threadIdx.x);
}

// ------------------------------------------------------------------------------------------
// pose-only LM (BA::ProjectPoseOptimization), one workgroup per frame, whole solve in-kernel.
// kPoW wavefronts per frame (a12 is the per-frame tracking call: a few hundred residuals): threads
// stride the frame's residuals (the first kPoC per thread held in registers for the whole solve);
// the 28 normal-equation sums are one reduce-scatter per wave (wave_sum_all) plus the waves' sums in
// wave order through LDS, the candidate cost a butterfly plus the same; every thread then carries
// the frame's LM state and solves the 6 x 6 system redundantly (identical bits everywhere, so the
// control flow is uniform).  Two barriers per iteration; the LDS exchange is double-buffered.
constexpr int kPoW = 4, kPoThreads = 64 * kPoW;
constexpr int kPoRegRes = 2 * kPoThreads;  // residuals per frame held in registers (kPoC per thread)
// a small batch's residual offsets as a kernel argument: the residual loads need no round trip first
constexpr int kPoArgF = 16;
struct PoOff { int n; int off[kPoArgF + 1]; };
// The solve of one frame by one kPoThreads workgroup: residuals [0, nres), residual r fetched by
// load(r, X, uv) (as doubles).  k_ba_pose_only reads them from the batch's arrays, k_track_tail from
// the slots its own compaction listed.  pose_init: 6 floats; pose_out: 6 doubles; sum: one record.
// An empty problem leaves the pose as given and a zeroed summary.
template <class Load>
__device__ __forceinline__ void po_run(int nres, double fx, double fyv, double cx, double cy,
                                       const float* pose_init, const LMOpt& o, Load load,
                                       double* __restrict__ pose_out, lorb_ba_summary* __restrict__ sum) {
  __shared__ double s_nv[2][kPoW][28];
  __shared__ double s_cv[2][kPoW];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int r0 = 0, r1 = nres;
  double xs[6], xn[6], sc[6], JtJ[21], Jtr[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) { xs[k] = (double)pose_init[k]; xn[k] = xs[k]; sc[k] = 1.0; }
  if (r1 == r0) {
    if (t < 6) pose_out[t] = xs[t];
    if (t == 0) { lorb_ba_summary z = {}; *sum = z; }
    return;
  }
  double radius = o.init_radius, df = 2.0;
  int iter = 0, n_success = 0, n_invalid = 0, term = LORB_TERM_NO_CONVERGENCE, last_successful = 1;
  double initial_cost = 0.0, cost = 0.0, gmax = 0.0, xnorm = 0.0;
  bool relin = true;
  int buf = 0;
  // the thread's first kPoC residuals (r0 + t + kPoThreads q) stay in registers for the whole solve;
  // a frame with more reads the rest from memory in each pass (same per-thread order)
  constexpr int kPoC = kPoRegRes / kPoThreads;
  double cX[kPoC][3], cuv[kPoC][2];
#pragma unroll
  for (int q = 0; q < kPoC; ++q) {
    load(min(r0 + t + kPoThreads * q, r1 - 1), cX[q], cuv[q]);
  }
  for (;;) {
    if (relin) {
      double v[32];  // 21 JtJ + 6 Jtr + cost (+ wave_sum_all's padding)
#pragma unroll
      for (int k = 0; k < 28; ++k) v[k] = 0.0;
      const lorb::RotJet R = lorb::rot_jet(xs);  // one frame: rotation state hoisted
      auto acc = [&](const double (&X)[3], double u, double w) {
        double rr[2], Jp[6], Jc[12];
        residual_jac_s(R, xs + 3, X, fx, fyv, cx, cy, u, w, rr, Jp, Jc);
        int q = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a) {
          v[21 + a] = fma(Jc[a], rr[0], fma(Jc[6 + a], rr[1], v[21 + a]));
#pragma unroll
          for (int b = a; b < 6; ++b) { v[q] = fma(Jc[a], Jc[b], fma(Jc[6 + a], Jc[6 + b], v[q])); ++q; }
        }
        v[27] += 0.5 * (rr[0] * rr[0] + rr[1] * rr[1]);
      };
#pragma unroll
      for (int q = 0; q < kPoC; ++q)
        if (r0 + t + kPoThreads * q < r1) acc(cX[q], cuv[q][0], cuv[q][1]);
      for (int r = r0 + t + kPoThreads * kPoC; r < r1; r += kPoThreads) {
        double X[3], uv[2];
        load(r, X, uv);
        acc(X, uv[0], uv[1]);
      }
      wave_sum_all<28>(v);
      if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 28; ++k) s_nv[buf][wv][k] = v[k];
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < 28; ++k) {
        double a = s_nv[buf][0][k];
#pragma unroll
        for (int w = 1; w < kPoW; ++w) a += s_nv[buf][w][k];
        v[k] = a;
      }
      buf ^= 1;
#pragma unroll
      for (int k = 0; k < 21; ++k) JtJ[k] = v[k];
#pragma unroll
      for (int k = 0; k < 6; ++k) Jtr[k] = v[21 + k];
      cost = v[27];
      double gm = 0.0, xn2 = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) { gm = fmax(gm, fabs(xs[k] - (xs[k] + -Jtr[k]))); xn2 += xs[k] * xs[k]; }
      gmax = gm;
      xnorm = sqrt(xn2);
      if (iter == 0) {
        initial_cost = cost;
        const int dg[6] = {0, 6, 11, 15, 18, 20};
#pragma unroll
        for (int k = 0; k < 6; ++k) sc[k] = o.jacobi ? 1.0 / (1.0 + sqrt(JtJ[dg[k]])) : 1.0;
      }
      last_successful = 1;
      relin = false;
    }
    if (iter >= o.max_iter) { term = LORB_TERM_NO_CONVERGENCE; break; }
    if (last_successful && gmax <= o.gtol) { term = LORB_TERM_GRADIENT_TOL; break; }
    if (radius <= o.min_radius) { term = LORB_TERM_MIN_RADIUS; break; }
    iter++;
    // (Js^T Js + D^2) y = Js^T r, D^2 = clamp(diag)/radius ; dense 6x6 Cholesky
    double A[36], y[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
      for (int b = 0; b < 6; ++b) A[6 * a + b] = JtJ[u21(a, b)] * sc[a] * sc[b];
      y[a] = Jtr[a] * sc[a];
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) A[7 * a] += fmin(fmax(A[7 * a], o.min_diag), o.max_diag) / radius;
    // the six pivots' reciprocal square roots once (v_rsq_f64 + two Newton steps, as k_ba_chol:
    // no IEEE sqrt / division on the chain); the column and both triangular solves multiply by them
    bool ok = true;
    double il[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      double dd = A[7 * j];
#pragma unroll
      for (int k = 0; k < j; ++k) dd -= A[6 * j + k] * A[6 * j + k];
      ok = ok && dd > 0.0;
      il[j] = rsqrt_refined(dd);
#pragma unroll
      for (int i = j + 1; i < 6; ++i) {
        double sv = A[6 * i + j];
#pragma unroll
        for (int k = 0; k < j; ++k) sv -= A[6 * i + k] * A[6 * j + k];
        A[6 * i + j] = sv * il[j];
      }
    }
    double mcc = -1.0;
    if (ok) {
#pragma unroll
      for (int i = 0; i < 6; ++i) { double sv = y[i]; for (int k = 0; k < i; ++k) sv -= A[6 * i + k] * y[k]; y[i] = sv * il[i]; }
#pragma unroll
      for (int i = 5; i >= 0; --i) { double sv = y[i]; for (int k = i + 1; k < 6; ++k) sv -= A[6 * k + i] * y[k]; y[i] = sv * il[i]; }
      // model cost change = -(step.Js^T r + 0.5 step^T Js^T Js step), step = -y
      // on the unscaled step z = sc (-y): lin = z . J^T r, quad = z^T (J^T J z) -- six independent
      // row products, then two dot products (short dependent chains)
      double z[6], w[6];
#pragma unroll
      for (int a = 0; a < 6; ++a) z[a] = sc[a] * -y[a];
#pragma unroll
      for (int a = 0; a < 6; ++a) {
        w[a] = 0.0;
#pragma unroll
        for (int b = 0; b < 6; ++b) w[a] = fma(JtJ[u21(a, b)], z[b], w[a]);
      }
      double lin = 0.0, quad = 0.0;
#pragma unroll
      for (int a = 0; a < 6; ++a) { lin = fma(z[a], Jtr[a], lin); quad = fma(z[a], w[a], quad); }
      mcc = -(lin + 0.5 * quad);
#pragma unroll
      for (int a = 0; a < 6; ++a) xn[a] = xs[a] + (-y[a]) * sc[a];
      ok = isfinite(mcc) && mcc > 0.0;
    }
    if (!ok) {
      if (++n_invalid >= o.max_invalid) { term = LORB_TERM_FAILURE; break; }
      radius /= df; df *= 2.0; last_successful = 0;
      continue;
    }
    n_invalid = 0;
    // candidate cost
    double cv = 0.0;
    {
      const lorb::RotVal R = lorb::rot_val(xn);
#pragma unroll
      for (int q = 0; q < kPoC; ++q)
        if (r0 + t + kPoThreads * q < r1) {
          double rr[2];
          residual_s(R, xn + 3, cX[q], fx, fyv, cx, cy, cuv[q][0], cuv[q][1], rr);
          cv += 0.5 * (rr[0] * rr[0] + rr[1] * rr[1]);
        }
      for (int r = r0 + t + kPoThreads * kPoC; r < r1; r += kPoThreads) {
        double X[3], uv[2], rr[2];
        load(r, X, uv);
        residual_s(R, xn + 3, X, fx, fyv, cx, cy, uv[0], uv[1], rr);
        cv += 0.5 * (rr[0] * rr[0] + rr[1] * rr[1]);
      }
    }
    cv = wave_sum(cv);
    if (lane == 0) s_cv[buf][wv] = cv;
    __syncthreads();
    cv = s_cv[buf][0];
#pragma unroll
    for (int w = 1; w < kPoW; ++w) cv += s_cv[buf][w];
    buf ^= 1;
    const double new_cost = isfinite(cv) ? cv : 1.7976931348623157e308;
    double sn2 = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) sn2 += (xs[k] - xn[k]) * (xs[k] - xn[k]);
    if (sqrt(sn2) <= o.ptol * (xnorm + o.ptol)) { term = LORB_TERM_PARAMETER_TOL; break; }
    const double cc = cost - new_cost;
    if (fabs(cc) <= o.ftol * cost) { term = LORB_TERM_FUNCTION_TOL; break; }
    const double rel = cc / mcc;
    if (rel > o.min_rel) {
#pragma unroll
      for (int k = 0; k < 6; ++k) xs[k] = xn[k];
      relin = true;
      n_success++;
      const double tt = 2.0 * rel - 1.0;
      radius = fmin(o.max_radius, radius / fmax(1.0 / 3.0, 1.0 - tt * tt * tt));
      df = 2.0;
    } else {
      last_successful = 0;
      radius /= df;
      df *= 2.0;
    }
  }
#pragma unroll
  for (int k = 0; k < 6; ++k)
    if (t == k) pose_out[k] = xs[k];
  if (t == 0) {
    lorb_ba_summary sm;
    sm.iterations = iter; sm.successful_steps = n_success; sm.termination = term; sm.pad_ = 0;
    sm.initial_cost = initial_cost; sm.final_cost = cost;
    *sum = sm;
  }
}
__global__ __launch_bounds__(kPoThreads) void k_ba_pose_only(PoOff aoff, const int32_t* __restrict__ res_off,
                                                             const float* __restrict__ intr,
                                                             const float* __restrict__ pose_init,
                                                             const float* __restrict__ pts3d,
                                                             const float* __restrict__ obs2d, LMOpt o,
                                                             double* __restrict__ pose_out,
                                                             lorb_ba_summary* __restrict__ sums) {
  const int f = blockIdx.x;
  const int r0 = aoff.n ? aoff.off[f] : res_off[f], r1 = aoff.n ? aoff.off[f + 1] : res_off[f + 1];
  const float* P = pts3d + 3 * (size_t)r0;
  const float* U = obs2d + 2 * (size_t)r0;
  po_run(r1 - r0, intr[4 * f], intr[4 * f + 1], intr[4 * f + 2], intr[4 * f + 3], pose_init + 6 * f, o,
         [&](int r, double (&X)[3], double (&uv)[2]) {
#pragma unroll
           for (int k = 0; k < 3; ++k) X[k] = P[3 * r + k];
           uv[0] = U[2 * r]; uv[1] = U[2 * r + 1];
         },
         pose_out + 6 * f, sums + f);
}

// The residual slots of a tracking chain's tail (k_track_tail, k_local_tail): slot j holds a map
// point after the matching if code[j] >= 0 (the point pt_pos[code[j]]) or, where `keep` is set, if
// the code is UNCHANGED and slot_state[j] is not EMPTY (the point slot_pos[j]).
struct TailSlots {
  int nk;
  const int* code;
  bool keep;
  const uint8_t* slot_state;  // null: all EMPTY
  const float *slot_pos, *pt_pos, *x, *y;
  float* list;      // 5 floats per slot: the residuals past the LM's register-resident ones
  int* copy_to;     // non-null: the codes are also stored here
  int* assign_out;  // non-null: and here (the mapped result block)
};
// The tail body, one kPoThreads workgroup: the slots holding a map point compacted in ascending
// slot order by a workgroup scan (src/bundle_adjust.cpp:173-186 walks the slots in order), their
// count stored at *n_res, then the pose-only LM over them (over none unless `solve`: the empty
// problem, which leaves pose_init widened and a zeroed summary).  The first kPoRegRes residuals are
// listed by slot in LDS and each thread loads its own straight into the registers the LM keeps them
// in; later ones go through a list in global memory written before the barrier that ends the
// compaction.
__device__ __forceinline__ void tail_run(const TailSlots& s, bool solve, double fx, double fyv, double cx, double cy,
                                         const float* pose_init, const LMOpt& o, int* __restrict__ n_res,
                                         double* __restrict__ pose_out, lorb_ba_summary* __restrict__ sum) {
  __shared__ int s_slot[kPoRegRes];
  __shared__ int wsum[kPoW];
  const int t = threadIdx.x;
  int nres = 0;
  for (int c0 = 0; c0 < s.nk; c0 += kPoThreads) {
    const int j = c0 + t;
    int cd = LORB_ASSIGN_NULL;
    bool has = false;
    if (j < s.nk) {
      cd = s.code[j];
      has = cd >= 0 || (s.keep && cd == LORB_ASSIGN_UNCHANGED && s.slot_state && s.slot_state[j] != LORB_SLOT_EMPTY);
      if (s.copy_to) s.copy_to[j] = cd;
      if (s.assign_out) s.assign_out[j] = cd;
    }
    int tot;
    const int r = nres + lorb::block_excl_scan<kPoThreads>(has ? 1 : 0, wsum, &tot);
    if (has) {
      if (r < kPoRegRes) {
        s_slot[r] = j;
      } else {
        const float* X = cd >= 0 ? s.pt_pos + 3 * (size_t)cd : s.slot_pos + 3 * (size_t)j;
        float* L = s.list + 5 * (size_t)r;
        L[0] = X[0]; L[1] = X[1]; L[2] = X[2]; L[3] = s.x[j]; L[4] = s.y[j];
      }
    }
    nres += tot;
  }
  __syncthreads();  // s_slot and the list are complete (the scan's barriers order the loop itself)
  if (t == 0) *n_res = nres;
  po_run(solve ? nres : 0, fx, fyv, cx, cy, pose_init, o,
         [&](int r, double (&X)[3], double (&uv)[2]) {
           if (r < kPoRegRes) {
             const int j = s_slot[r], cd = s.code[j];
             const float* Xp = cd >= 0 ? s.pt_pos + 3 * (size_t)cd : s.slot_pos + 3 * (size_t)j;
#pragma unroll
             for (int k = 0; k < 3; ++k) X[k] = Xp[k];
             uv[0] = s.x[j]; uv[1] = s.y[j];
           } else {
             const float* L = s.list + 5 * (size_t)r;
#pragma unroll
             for (int k = 0; k < 3; ++k) X[k] = L[k];
             uv[0] = L[3]; uv[1] = L[4];
           }
         },
         pose_out, sum);
}

// The tail of the motion-tracking chain (VisualOdometry::EstimatePoseMotion after its matcher
// calls), one workgroup: which pass counts (pass 1 unless it found <= min_matches, then the retry,
// which must itself find more), the final assign codes, and tail_run over the slots holding a map
// point afterwards (the retry starts from emptied slots: only its own matches count).
// (the body, shared with k_track_frames_tail; returns whether the retry ran)
__device__ __forceinline__ bool track_tail_run(const lorb::TrackTail& a, const LMOpt& o) {
  const int nm1 = *a.nm1;
  const bool retry = nm1 <= a.min_matches;
  const int nm2 = retry ? *a.nm2 : -1;
  const int pass = !retry ? 1 : (nm2 > a.min_matches ? 2 : 0);
  if (threadIdx.x == 0) { a.rec->pass = pass; a.rec->nmatches_first = nm1; a.rec->nmatches_retry = nm2; }
  const TailSlots s = {a.nk, retry ? a.assign2 : a.assign, !retry, a.slot_state, a.slot_pos, a.last_pos, a.x, a.y,
                       a.list, retry ? a.assign : nullptr, a.assign_out};
  tail_run(s, pass != 0, a.fx, a.fy_eff, a.cx, a.cy, a.pose_init, o, &a.rec->n_residuals, a.rec->pose, &a.rec->summary);
  return retry;
}
__global__ __launch_bounds__(kPoThreads) void k_track_tail(lorb::TrackTail a, LMOpt o) { track_tail_run(a, o); }

// The tail of lorb_track_motion_frames_dev: k_track_tail with the keypoint count read from device
// memory (a.nk is the bound on entry), then the codes that count -- a.assign after the body -- applied
// to the current frame's slots: code i >= 0 copies last slot i (state, pos, desc); NULL empties the
// slot; UNCHANGED keeps a given slot when pass 1 stood and empties it otherwise (the retry starts from
// emptied slots, src/visual_odometry.cpp:128; slots not given are all EMPTY whatever the array holds).
// The apply runs after the LM: the solve has read slot_pos (the kept slots' points) by then, and the
// few dozen bytes per slot are not worth a launch of their own.
// (the body, shared with k_track_frames_tail_pose and k_track_frames_tail_refer; kGids: the latter's,
// which writes each slot's id beside the slot)
template <bool kGids = false>
__device__ __forceinline__ void track_frames_tail_run(lorb::TrackTail& a, const lorb::FramesTail& f, const LMOpt& o,
                                                      const lorb::ReferGids* g = nullptr) {
  int n_last;
  if (!lorb::frame_counts(f.dc, &n_last, &a.nk)) return;
  const bool retry = track_tail_run(a, o);
  __syncthreads();  // every thread's codes are in a.assign, every read of the entry slots is done
  const bool keep = !retry && f.given;
  const uint4* ld = reinterpret_cast<const uint4*>(f.last.desc);
  uint4* cd = reinterpret_cast<uint4*>(f.cur.desc);
  for (int j = threadIdx.x; j < a.nk; j += kPoThreads) {
    const int c = a.assign[j];
    if (c >= 0) {
      f.cur.state[j] = f.last.state[c];
#pragma unroll
      for (int k = 0; k < 3; ++k) f.cur.pos[3 * (size_t)j + k] = f.last.pos[3 * (size_t)c + k];
      cd[2 * (size_t)j] = ld[2 * (size_t)c];
      cd[2 * (size_t)j + 1] = ld[2 * (size_t)c + 1];
    } else if (c == LORB_ASSIGN_NULL || !keep) {
      f.cur.state[j] = LORB_SLOT_EMPTY;
    }
    if constexpr (kGids) {
      if (g->cur_gid) g->cur_gid[j] = lorb::motion_entry_id(g->cur_gid[j], c, keep, g->refer_gid, g->n_max_refer);
    }
  }
}
__global__ __launch_bounds__(kPoThreads) void k_track_frames_tail(lorb::TrackTail a, lorb::FramesTail f, LMOpt o) {
  track_frames_tail_run(a, f, o);
}
// The tail of lorb_track_motion_frames_pose_dev: the LM starts from the pose the chain's first kernel
// left in its MotionPose block (f.dc.last is that block's n_last: -1 on status 1, and the kernel returns).
__global__ __launch_bounds__(kPoThreads) void k_track_frames_tail_pose(lorb::TrackTail a, lorb::FramesTail f,
                                                                       const lorb::MotionPose* __restrict__ pose, LMOpt o) {
#pragma unroll
  for (int k = 0; k < 6; ++k) a.pose_init[k] = pose->pose_init[k];
  track_frames_tail_run(a, f, o);
}
// The tail of lorb_track_motion_refer_pose_dev (the "last" frame is the refer frame): the same, and the
// codes that count applied to the slots' ids as they are to the slots -- motion_entry_id with the refer
// frame's ids as the source, an UNCHANGED slot keeping the id the call's first kernel left when pass 1
// stood.  A skipped attempt returns with the body (n_last = -1) and writes no id.
__global__ __launch_bounds__(kPoThreads) void k_track_frames_tail_refer(lorb::TrackTail a, lorb::FramesTail f,
                                                                        const lorb::MotionPose* __restrict__ pose,
                                                                        lorb::ReferGids g, LMOpt o) {
#pragma unroll
  for (int k = 0; k < 6; ++k) a.pose_init[k] = pose->pose_init[k];
  track_frames_tail_run<true>(a, f, o, &g);
}

// The tail of the local-map tracking chain (VisualOdometry::EstimatePoseLocal after its matcher
// call, src/visual_odometry.cpp:204-209), one workgroup: nToMatch counted from a8's flags (an
// integer sum), the nMatches <= min_matches gate, and tail_run over the slots holding a map point
// after a5 (a slot a5 left alone keeps the point stage 1 gave it).
// (the body, shared with k_local_frames_tail; pose_init: the a12 start, wherever it lives)
__device__ __forceinline__ void local_tail_run(const lorb::LocalTail& a, const float* pose_init, const LMOpt& o) {
  __shared__ int wcnt[kPoW];
  const int nm = *a.nm;
  int c = 0;
  for (int m = threadIdx.x; m < a.np; m += kPoThreads) c += a.in_view[m] != 0;
  int n_in_view;
  lorb::block_excl_scan<kPoThreads>(c, wcnt, &n_in_view);
  const bool ok = nm > a.min_matches;
  if (threadIdx.x == 0) { a.rec->ok = ok; a.rec->nmatches = nm; a.rec->n_in_view = n_in_view; }
  const TailSlots s = {a.nk, a.assign, true, a.slot_state, a.slot_pos, a.pt_pos, a.x, a.y, a.list, nullptr, a.assign_out};
  tail_run(s, ok, a.fx, a.fy_eff, a.cx, a.cy, pose_init, o, &a.rec->n_residuals, a.rec->pose, &a.rec->summary);
}
__global__ __launch_bounds__(kPoThreads) void k_local_tail(lorb::LocalTail a, LMOpt o) { local_tail_run(a, a.pose_init, o); }

// The tail of lorb_track_local_frames_dev: k_local_tail with both counts read from device memory
// (a.nk / a.np are the bounds on entry) and the LM started from the pose k_local_head handed over;
// then Frame::SetPose of the result rounded to float (the hand-over's own function: with ok == 0 the
// pose is pose_in widened, so Tcw has the bits of Tcw_in), and a5's codes applied to the frame's
// slots -- code k >= 0 gives the slot point k of the table (state from its lock flag, pos, desc, id);
// UNCHANGED slots stay -- whether or not the gate passed (src/visual_odometry.cpp:204-205 keeps the
// matcher's writes).  The apply runs after the LM for the reason k_track_frames_tail gives.
__global__ __launch_bounds__(kPoThreads) void k_local_frames_tail(lorb::LocalTail a, lorb::LocalFramesTail f, LMOpt o) {
  if (!lorb::frame_counts(f.dc, &a.np, &a.nk)) return;
  local_tail_run(a, f.pose->pose_in, o);
  __syncthreads();  // the record's pose is written, every read of the entry slots is done
  if (threadIdx.x == 0) {
    float p[6];
    for (int k = 0; k < 6; ++k) p[k] = (float)a.rec->pose[k];
    lorb::pose_to_Tcw(p, p + 3, f.rec->Tcw);
  }
  const uint4* pd = reinterpret_cast<const uint4*>(f.pt_desc);
  uint4* cd = reinterpret_cast<uint4*>(f.cur.desc);
  for (int j = threadIdx.x; j < a.nk; j += kPoThreads) {
    const int c = a.assign[j];
    if (c >= 0) {
      f.cur.state[j] = f.pt_locked[c] ? LORB_SLOT_LOCKED : LORB_SLOT_FREE;
#pragma unroll
      for (int k = 0; k < 3; ++k) f.cur.pos[3 * (size_t)j + k] = a.pt_pos[3 * (size_t)c + k];
      cd[2 * (size_t)j] = pd[2 * (size_t)c];
      cd[2 * (size_t)j + 1] = pd[2 * (size_t)c + 1];
      f.slot_id[j] = c;
    }
  }
}

LMOpt to_dev_opt(const lorb_lm_options* o) {
  LMOpt d;
  d.max_iter = o->max_num_iterations; d.max_invalid = o->max_num_consecutive_invalid_steps;
  d.jacobi = o->jacobi_scaling; d.ftol = o->function_tolerance; d.gtol = o->gradient_tolerance;
  d.ptol = o->parameter_tolerance; d.init_radius = o->initial_trust_region_radius;
  d.max_radius = o->max_trust_region_radius; d.min_radius = o->min_trust_region_radius;
  d.min_rel = o->min_relative_decrease; d.min_diag = o->min_lm_diagonal; d.max_diag = o->max_lm_diagonal;
  return d;
}
// field by field (LMOpt has padding after its ints: a memcmp would see whatever those bytes hold)
bool same_opt(const LMOpt& a, const LMOpt& b) {
  return a.max_iter == b.max_iter && a.max_invalid == b.max_invalid && a.jacobi == b.jacobi && a.ftol == b.ftol &&
         a.gtol == b.gtol && a.ptol == b.ptol && a.init_radius == b.init_radius && a.max_radius == b.max_radius &&
         a.min_radius == b.min_radius && a.min_rel == b.min_rel && a.min_diag == b.min_diag && a.max_diag == b.max_diag;
}

// LORB_NO_GRAPH=1: eager launches instead of a captured graph; LORB_NO_FUSE=1: no fused iteration
// (and no plan group run as one set of launches).  Read once.
bool no_graph() { static const bool v = env_flag("LORB_NO_GRAPH"); return v; }
bool no_fuse() { static const bool v = env_flag("LORB_NO_FUSE"); return v; }

// Cholesky kernel for the plan's band: 2 k_ba_chol_2s, 1 k_ba_chol_w, 0 k_ba_chol, -1 none
int chol_kind_of(const lorb_ba_plan* P) {
  static const bool force_old = [] { const char* e = getenv("LORB_CHOL"); return e && e[0] == 'o'; }();
  static const bool no_2s = [] { const char* e = getenv("LORB_CHOL"); return e && e[0] == 'w'; }();
  if (!P->Ctot) return -1;
  const bool chol_w = !force_old && P->max_bw <= 48 && sizeof(double) * (size_t)P->max_env_w <= (size_t)kLdsBudget;
  // two-sided: its back-substitution uses the full inverse of each 16 x 16 diagonal block, which
  // the band storage holds only for bw >= 15
  const bool chol_2s = chol_w && !no_2s && P->min_n16 >= 128 && P->min_bw >= 15;
  return chol_2s ? 2 : chol_w ? 1 : 0;
}

// doubles of exchange 2 (reduced camera system, rhs, failure flags)
size_t x2_count(const lorb_ba_plan* P) {
  return P->devb ? P->x2_off + (size_t)P->env_total : (size_t)P->env_total + P->n_total + P->W;
}

// k_ba_red's width: 1024 threads when a block has many candidate groups (a window's groups x the
// cameras a group spans / the window's cameras >= 128: the shared window) or the grid leaves CUs
// idle (<= 256 blocks: C3); 512 up to 1024 blocks (C4's 372: 9.8 -> 7.8 us); 256 when many blocks
// share the GPU (several C4 windows per plan)
int red_threads(const lorb_ba_plan* P) {
  const double W = std::max(P->W, 1), cams = std::max((double)P->Ctot / W, 1.0);
  const double cand = (double)P->n_pblk / W * ((P->max_bw + 1) / 6.0) / cams;
  if (P->grid_bp <= 256 || cand >= 128.0) return 1024;
  return P->grid_bp <= 1024 ? 512 : 256;
}
// the same rule over a plan group's k_ba_red_g, a launch of nb blocks: 1024 where a member that shares
// the GPU (> 256 blocks of its own) has that many candidates (the sums do not depend on the width;
// for n = 1 this is red_threads(plans[0]))
int red_threads(lorb_ba_plan* const* plans, int n, int nb) {
  bool wide = nb <= 256;
  for (int k = 0; k < n; ++k) wide = wide || (red_threads(plans[k]) == 1024 && plans[k]->grid_bp > 256);
  return wide ? 1024 : nb <= 1024 ? 512 : 256;
}

// k_ba_init's blocks for one plan
int init_blocks(const lorb_ba_plan* P) {
  const int n = std::max(std::max(std::max(P->W, P->Ctot), P->NF), std::min(3 * P->pt_launch, 256 * 1024));
  return lorb::ceil_div(std::max(n, 1), 256);
}

// LORB_NO_FOLD=1 (read at every solve): every iteration ends with the k_ba_lm_end kernel.  Else the
// fused iterations of an unsharded plan on the two-sided Cholesky without partial runs fold the
// previous iteration's tail into their k_ba_ls -- unless a window has cameras and no point group (no
// workgroup of k_ba_ls would commit its state).  The fold trades a launch for one more dependent round
// trip and a redundant evaluation in every workgroup: it pays where k_ba_ls is one round of
// workgroups (two per CU: the C4 window's 346), and costs where the launch fills the GPU several
// times over (8 C4 windows in one plan or in concurrent groups: -1.7 % / -2.8 %, profiles/r11/), so
// launches of more than kFoldMaxGroups workgroups keep the kernel.  The plans of one set of
// launches (a plan; the members of a fused group) fold together or not at all.
constexpr int kFoldMaxGroups = 512;
bool fold_of(lorb_ba_plan* const* plans, size_t n) {
  int groups = 0;
  for (size_t k = 0; k < n; ++k) {
    const lorb_ba_plan* P = plans[k];
    if (env_flag("LORB_NO_FOLD") || no_fuse() || P->comm || P->has_super || chol_kind_of(P) != 2) return false;
    for (const BaWin& w : P->hwin)
      if (w.n_poses > 0 && w.n_pblk == 0) return false;
    if (P->grid_pblk <= 0) return false;
    groups += P->grid_pblk;
  }
  return groups <= kFoldMaxGroups;
}
bool fold_of(lorb_ba_plan* P) { return fold_of(&P, 1); }

// the launch shape of a solve of P's fields as they are, folding or not
lorb_ba_plan::GraphKey graph_key(const lorb_ba_plan* P, bool fold) {
  lorb_ba_plan::GraphKey k;
  k.kind = chol_kind_of(P);
  k.lds = k.kind >= 1 ? P->max_env_w : P->max_env + 1000000 * P->max_bw;
  k.memset_env = sizeof(double) * (size_t)P->max_env > (size_t)kLdsBudget;
  k.env_total = k.memset_env ? P->env_total : 0;
  k.grid_pblk = P->grid_pblk; k.grid_bp = P->grid_bp; k.pt_launch = P->pt_launch;
  k.x2_n = P->comm ? (int)x2_count(P) : 0;  // the captured all-reduce's count
  k.red_wide = red_threads(P);
  k.sup = P->has_super ? 1 : 0;
  k.grid_sg = P->grid_sg;
  k.fold = fold ? 1 : 0;
  return k;
}

// The band's structural zeros (set at plan creation) persist under the LDS Cholesky, which never
// writes env (k_ba_red rewrites every stored entry of every block each iteration); the in-place
// global variant needs them restored.
int restore_band(const lorb_ba_plan* P, hipStream_t s) {
  const bool chol_in_lds = sizeof(double) * (size_t)P->max_env <= (size_t)kLdsBudget;
  if (P->env_total && !chol_in_lds && !P->comm) LORB_HIP(P->ctx, hipMemsetAsync(P->dev.env, 0, sizeof(double) * P->env_total, s));
  return LORB_OK;
}

// The exchanges of a sharded plan.  1: camera blocks + cost / |x|^2 (sum over n = 27 Ctot + 2 W
// doubles), gradient max (max).  A fused iteration sums exchanges 1 and 2 at once, n = P->fx_n: the
// contiguous [U | V | cost, |x|^2 | pad | band | rhs | failure flags] (the band's camera blocks and the
// rhs carry -a / -r only: the Cholesky adds the global U sc sc^T + D^2 and V sc as it stages them).
int exchange_1(const lorb_ba_plan* P, hipStream_t s, size_t n) {
  hipLaunchKernelGGL(k_ba_win_reduce<0>, dim3(P->W), dim3(64), 0, s, P->dev);
  lorb::KernelTimer kt(P->ctx, LORB_K_ALLREDUCE);
  LORB_TRY(lorb::comm_allreduce(P->comm, P->dev.U_part, P->dev.U, n, LORB_OP_SUM));
  return lorb::comm_allreduce(P->comm, P->dev.wmax_part, P->dev.wmax, (size_t)P->W, LORB_OP_MAX);
}
// 2: reduced camera system, rhs, point-block failure flags
int exchange_2(const lorb_ba_plan* P) {
  lorb::KernelTimer kt(P->ctx, LORB_K_ALLREDUCE);
  return lorb::comm_allreduce(P->comm, P->x2_send, P->x2_recv, x2_count(P), LORB_OP_SUM);
}
// 3: model cost change, candidate cost, point |step|^2
int exchange_3(const lorb_ba_plan* P, hipStream_t s) {
  hipLaunchKernelGGL(k_ba_win_reduce<1>, dim3(P->W), dim3(64), 0, s, P->dev);
  lorb::KernelTimer kt(P->ctx, LORB_K_ALLREDUCE);
  return lorb::comm_allreduce(P->comm, P->dev.wstep_part, P->dev.wstep, 3 * (size_t)P->W, LORB_OP_SUM);
}

// block prefix of one group launch: f(P) workgroups per member
template <typename F>
GrpGrid grp_grid(lorb_ba_plan* const* plans, int n, F f) {
  GrpGrid g{};
  for (int k = 0; k < n; ++k) g.pre[k + 1] = g.pre[k] + f(plans[k]);
  for (int k = n + 1; k <= kGrpMax; ++k) g.pre[k] = g.pre[n];
  return g;
}

// What enqueue_solve launches on: one plan (its own kernels on the grids its fields give), or the
// members of a fused group (the k_ba_*_g kernels, a block range per member; group_fused: never
// sharded, always the two-sided Cholesky, no partial runs).  A plan is not a group of one.
struct LmTarget {
  lorb_ba_plan* const* plans;
  int n;
  bool grouped, fold;  // fold: this solve folds (fold_of)
  lorb_ctx* ctx;
  hipStream_t s;
  // the kernels' argument (the plan's / the group's); [1]: fold set, for the k_ba_ls, k_ba_red<2> and
  // Cholesky of a folding iteration
  BaDev d[2]{};
  BaGrp g[2]{};
  LmTarget(lorb_ba_plan* const* plans_, int n_, bool grouped_, bool fold_)
      : plans(plans_), n(n_), grouped(grouped_), fold(fold_), ctx(plans_[0]->ctx), s(ctx->stream) {
    bool one_win = true;
    for (int k = 0; k < n; ++k) one_win = one_win && plans[k]->W == 1;
    d[0] = d[1] = plans[0]->dev;
    d[1].fold = one_win ? 2 : 1;
    if (!grouped) return;
    g[0].n = g[1].n = n;
    for (int k = 0; k < n; ++k) {
      g[0].d[k] = g[1].d[k] = plans[k]->dev;
      g[1].d[k].fold = d[1].fold;
    }
  }
  // one stage: the plan's kernel on its grid (a field of the plan), or the group's on every member's
  template <typename KP, typename KG, typename... A>
  void launch(KP plan_kernel, KG group_kernel, int lorb_ba_plan::*grid, int block, bool folding, const A&... a) const {
    if (!grouped) {
      const int nb = plans[0]->*grid;
      if (nb) hipLaunchKernelGGL(plan_kernel, dim3(nb), dim3(block), 0, s, d[folding], a...);
      return;
    }
    const GrpGrid gg = grp_grid(plans, n, [&](const lorb_ba_plan* P) { return P->*grid; });
    if (gg.pre[n]) hipLaunchKernelGGL(group_kernel, dim3(gg.pre[n]), dim3(block), 0, s, g[folding], gg, a...);
  }
  void init(const LMOpt& o) const {
    const lorb_ba_plan* P = plans[0];
    if (!grouped) {
      hipLaunchKernelGGL(k_ba_init, dim3(init_blocks(P)), dim3(256), 0, s, d[0], P->W, P->Ctot, P->pt_launch, P->NF, o);
      return;
    }
    GrpInit a{};
    for (int k = 0; k < n; ++k) {
      P = plans[k];
      a.W[k] = P->W; a.ctot[k] = P->Ctot; a.n_pt[k] = P->pt_launch; a.nf[k] = P->NF;
    }
    const GrpGrid gg = grp_grid(plans, n, init_blocks);
    hipLaunchKernelGGL(k_ba_init_g, dim3(gg.pre[n]), dim3(256), 0, s, g[0], gg, a, o);
  }
  // k_ba_red in its mode's and width's instance, if there are block pairs
  template <int MODE>
  void red(bool folding, const LMOpt& o) const {
    int nb = 0;
    for (int k = 0; k < n; ++k) nb += plans[k]->grid_bp;
    if (!nb) return;
    lorb::KernelTimer kt(ctx, LORB_K_BA_SCHUR);
    const int rt = red_threads(plans, n, nb);
    if (rt == 1024) launch(k_ba_red<MODE, 1024>, k_ba_red_g<MODE, 1024>, &lorb_ba_plan::grid_bp, 1024, folding, o);
    else if (rt == 512) launch(k_ba_red<MODE, 512>, k_ba_red_g<MODE, 512>, &lorb_ba_plan::grid_bp, 512, folding, o);
    else launch(k_ba_red<MODE, 256>, k_ba_red_g<MODE, 256>, &lorb_ba_plan::grid_bp, 256, folding, o);
  }
  void chol(int kind, bool folding, const LMOpt& o, bool head) const {
    lorb::KernelTimer kt(ctx, LORB_K_BA_CHOLESKY);
    const lorb_ba_plan* P = plans[0];
    if (!grouped) return launch_chol(kind, CholShape{P->W, P->max_env, P->max_env_w, P->max_bw}, s, d[folding], o, head);
    size_t lds = 0;
    for (int k = 0; k < n; ++k) lds = std::max(lds, sizeof(double) * (size_t)plans[k]->max_env_w);
    launch_chol_2s_g(s, g[folding], grp_grid(plans, n, [](const lorb_ba_plan* Q) { return Q->W; }), o, head, lds);
  }
};

// The whole LM solve on the ctx stream, for a plan and for a fused group: x <- initial values, then
// max_iter iterations (k_ba_lm_end closes the solve when the budget is spent: no final linearisation).
// First iteration: k_ba_ls -> k_ba_red<0> (camera terms) -> k_ba_lm_begin -> k_ba_red<1> -> Cholesky
// -> k_ba_bs2 -> k_ba_lm_end.  Later iterations on the two-sided Cholesky run fused (LORB_NO_FUSE:
// none does): k_ba_red<2> writes the band, rhs and camera terms at once (the Jacobi scale is
// iteration 0's) and the head runs inside the Cholesky (k_ba_lm_begin's work), so k_ba_ls ->
// k_ba_red<2> -> k_ba_chol_2s<true> -> k_ba_bs2 -> k_ba_lm_end: five launches.
// A folding solve drops k_ba_lm_end from every iteration but the last (fold_out: a fused iteration
// follows and runs the tail in its k_ba_ls, fold_in), four launches: the decided state goes to st2,
// which k_ba_red<2> and the Cholesky's head read (those three get the argument with fold set).
// No iterations: one linearisation (cost, termination), the head of a first iteration.
int enqueue_solve(const LmTarget& t, const LMOpt& o) {
  using P = lorb_ba_plan;
  const P* X = !t.grouped && t.plans[0]->comm ? t.plans[0] : nullptr;  // the sharded plan
  const bool sup = !t.grouped && t.plans[0]->has_super;  // k_ba_ls per partial run
  const int kind = chol_kind_of(t.plans[0]);  // (-1: no cameras; a group: 2 for every member)
  t.init(o);
  LORB_CHECK_LAUNCH(t.ctx);
  for (int it = 0; it < std::max(o.max_iter, 1); ++it) {
    const bool fused = it > 0 && kind == 2 && !no_fuse();
    const bool fold_in = t.fold && fused, fold_out = t.fold && it + 1 < o.max_iter;
    {  // (fold_in: the previous iteration's tail in the prologue, ls_group)
      lorb::KernelTimer kt(t.ctx, LORB_K_BA_LINEARIZE);
      t.launch(sup ? k_ba_ls_sup : k_ba_ls, k_ba_ls_g, sup ? &P::grid_sg : &P::grid_pblk, kLsThreads, fold_in, o);
    }
    if (!fused) {  // the head as kernels: the group partials' camera terms, exchange 1, k_ba_lm_begin
      t.red<0>(false, o);
      if (X) LORB_TRY(exchange_1(X, t.s, (size_t)X->Ctot * 27 + 2 * X->W));
      t.launch(X ? k_ba_lm_begin<true> : k_ba_lm_begin<false>, k_ba_lm_begin_g, &P::W, 64, false, o);
      if (o.max_iter <= 0) break;
    }
    for (int k = 0; k < t.n; ++k) LORB_TRY(restore_band(t.plans[k], t.s));  // (a memset, or nothing)
    if (fused) t.red<2>(fold_in, o);
    else t.red<1>(false, o);
    if (X) LORB_TRY(fused ? exchange_1(X, t.s, X->fx_n) : exchange_2(X));
    if (kind >= 0) t.chol(kind, fold_in, o, fused);
    t.launch(k_ba_bs2, k_ba_bs2_g, &P::grid_pblk, kGB, false);
    if (X) LORB_TRY(exchange_3(X, t.s));
    if (!fold_out) t.launch(X ? k_ba_lm_end<true> : k_ba_lm_end<false>, k_ba_lm_end_g, &P::W, 64, false, o);
    for (int k = 0; k < t.n; ++k) t.plans[k]->chol_kind = kind;
    LORB_CHECK_LAUNCH(t.ctx);
  }
  return LORB_OK;
}

int plan_solve(lorb_ba_plan* P, const lorb_lm_options* opt) {
  lorb_ctx* ctx = P->ctx;
  LMOpt o = to_dev_opt(opt);
  P->fold = fold_of(P);
  // per-kernel events cannot live inside a graph, and neither can a host-transport exchange
  const bool timing = ctx->ktime || no_graph() || (P->comm && !P->comm->rccl);
  const lorb_ba_plan::GraphKey key = graph_key(P, P->fold);
  P->skey = key;
  const auto enqueue = [&] { return enqueue_solve(LmTarget(&P, 1, false, P->fold), o); };
  if (timing) return enqueue();
  const bool same = key == P->gkey && same_opt(P->graph_opt, o);
  return P->cache.replay_or_capture(ctx, same, enqueue, [&] { P->gkey = key; P->graph_opt = o; });
}

int plan_read(lorb_ba_plan* P, double* const* pose_out, double* const* point_out,
              lorb_ba_summary* sums) {
  lorb_ctx* ctx = P->ctx;
  std::vector<WinState> st(P->W);
  std::vector<std::vector<double>> hp(P->W);  // poses in plan camera order
  LORB_HIP(ctx, hipMemcpyAsync(st.data(), P->d_state, sizeof(WinState) * P->W, hipMemcpyDeviceToHost, ctx->stream));
  LORB_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int w = 0; w < P->W; ++w) {
    const BaWin& bw = P->hwin[w];
    const int cur = st[w].cur;
    if (pose_out && pose_out[w] && bw.n_poses) {
      hp[w].resize(6 * (size_t)bw.n_poses);
      LORB_HIP(ctx, hipMemcpyAsync(hp[w].data(), P->dev.x_pose[cur] + 6 * bw.pose_base, sizeof(double) * 6 * bw.n_poses, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (point_out && point_out[w] && bw.n_points)
      LORB_HIP(ctx, hipMemcpyAsync(point_out[w], P->dev.x_pt[cur] + 3 * bw.point_base, sizeof(double) * 3 * bw.n_points, hipMemcpyDeviceToHost, ctx->stream));
    if (sums) {
      lorb_ba_summary s{};
      s.iterations = st[w].iter; s.successful_steps = st[w].n_success; s.termination = st[w].term;
      s.initial_cost = st[w].initial_cost; s.final_cost = st[w].cost;
      if (bw.n_obs_all == 0) { s.iterations = 0; s.termination = LORB_TERM_FUNCTION_TOL; }
      sums[w] = s;
    }
  }
  LORB_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int w = 0; w < P->W; ++w) {  // back to the caller's pose order
    if (hp[w].empty()) continue;
    const std::vector<int>& map = P->cam_map[w];
    for (int c = 0; c < P->hwin[w].n_poses; ++c)
      for (int q = 0; q < 6; ++q)
        pose_out[w][6 * (size_t)c + q] = hp[w][6 * (size_t)(map.empty() ? c : map[c]) + q];
  }
  return LORB_OK;
}

}  // namespace

namespace lorb {
// plan_solve's host-side choices on the plan's fields as they are now against the last solve's
bool ba_plan_solve_key_same(lorb_ba_plan* P) {
  return graph_key(P, fold_of(P)) == P->skey;
}
}  // namespace lorb

// A plan group (lorb_ba_group_*): member plans (not owned) on one context, solved by one set of
// launches (k_ba_*_g) captured in one graph.  The graph holds the members' BaDev and launch shapes:
// it is re-captured when a member's buffers moved (lorb_ba_plan::gen), its launch shape changed or
// the options differ.
struct lorb_ba_group {
  lorb_ctx* ctx = nullptr;
  std::vector<lorb_ba_plan*> plans;
  GraphCache cache{"group graph"};  // cache.captures: graph captures so far
  LMOpt graph_opt{};
  std::vector<unsigned> gens;
  std::vector<lorb_ba_plan::GraphKey> keys;
  int n_fused = 0;  // solves run as one set of launches
};

namespace {

// a group runs as one set of launches when every member is an unsharded plan on the two-sided
// Cholesky (the fused iteration); otherwise its members are solved one after another, each by its
// own path (the same bits either way)
bool group_fused(const lorb_ba_group* G) {
  if (no_fuse() || G->plans.size() > (size_t)kGrpMax) return false;
  for (const lorb_ba_plan* P : G->plans)
    if (P->W == 0 || P->comm || P->has_super || chol_kind_of(P) != 2) return false;
  return true;
}

int group_solve(lorb_ba_group* G, const lorb_lm_options* opt) {
  lorb_ctx* ctx = G->ctx;
  if (!group_fused(G)) {
    for (lorb_ba_plan* P : G->plans)
      if (P->W > 0) LORB_TRY(plan_solve(P, opt));
    return LORB_OK;
  }
  const LMOpt o = to_dev_opt(opt);
  const bool fold = fold_of(G->plans.data(), G->plans.size());
  for (lorb_ba_plan* P : G->plans) P->fold = fold;  // (part of the members' graph keys)
  const auto enqueue = [&] { return enqueue_solve(LmTarget(G->plans.data(), (int)G->plans.size(), true, fold), o); };
  if (no_graph() || ctx->ktime) {  // per-kernel timing: eager launches (events cannot live in a graph)
    LORB_TRY(enqueue());
    G->n_fused++;
    return LORB_OK;
  }
  bool same = same_opt(G->graph_opt, o) && G->gens.size() == G->plans.size();
  for (size_t k = 0; k < G->plans.size() && same; ++k)
    same = G->gens[k] == G->plans[k]->gen && G->keys[k] == graph_key(G->plans[k], fold);
  LORB_TRY(G->cache.replay_or_capture(ctx, same, enqueue, [&] {
    G->graph_opt = o;
    G->gens.clear(); G->keys.clear();
    for (const lorb_ba_plan* P : G->plans) { G->gens.push_back(P->gen); G->keys.push_back(graph_key(P, fold)); }
  }));
  G->n_fused++;
  return LORB_OK;
}

}  // namespace

namespace lorb {
int launch_local_tail(lorb_ctx* ctx, const LocalTail& t, const lorb_lm_options* opt) {
  hipLaunchKernelGGL(k_local_tail, dim3(1), dim3(kPoThreads), 0, ctx->stream, t, to_dev_opt(opt));
  LORB_CHECK_LAUNCH(ctx);
  return LORB_OK;
}
int launch_local_frames_tail(lorb_ctx* ctx, const LocalTail& t, const LocalFramesTail& f, const lorb_lm_options* opt) {
  hipLaunchKernelGGL(k_local_frames_tail, dim3(1), dim3(kPoThreads), 0, ctx->stream, t, f, to_dev_opt(opt));
  LORB_CHECK_LAUNCH(ctx);
  return LORB_OK;
}
int launch_track_tail(lorb_ctx* ctx, const TrackTail& t, const lorb_lm_options* opt) {
  hipLaunchKernelGGL(k_track_tail, dim3(1), dim3(kPoThreads), 0, ctx->stream, t, to_dev_opt(opt));
  LORB_CHECK_LAUNCH(ctx);
  return LORB_OK;
}
int launch_track_frames_tail(lorb_ctx* ctx, const TrackTail& t, const FramesTail& f, const lorb_lm_options* opt) {
  hipLaunchKernelGGL(k_track_frames_tail, dim3(1), dim3(kPoThreads), 0, ctx->stream, t, f, to_dev_opt(opt));
  LORB_CHECK_LAUNCH(ctx);
  return LORB_OK;
}
int launch_track_frames_tail_pose(lorb_ctx* ctx, const TrackTail& t, const FramesTail& f, const MotionPose* pose,
                                  const lorb_lm_options* opt) {
  hipLaunchKernelGGL(k_track_frames_tail_pose, dim3(1), dim3(kPoThreads), 0, ctx->stream, t, f, pose, to_dev_opt(opt));
  LORB_CHECK_LAUNCH(ctx);
  return LORB_OK;
}
int launch_track_frames_tail_refer(lorb_ctx* ctx, const TrackTail& t, const FramesTail& f, const MotionPose* pose,
                                   const ReferGids& g, const lorb_lm_options* opt) {
  hipLaunchKernelGGL(k_track_frames_tail_refer, dim3(1), dim3(kPoThreads), 0, ctx->stream, t, f, pose, g, to_dev_opt(opt));
  LORB_CHECK_LAUNCH(ctx);
  return LORB_OK;
}
}  // namespace lorb

extern "C" {

int lorb_ba_plan_solve(lorb_ba_plan* plan, const lorb_lm_options* opt) {
  if (!plan || !opt) return LORB_E_INVALID;
  if (plan->W == 0) return LORB_OK;
  return plan_solve(plan, opt);
}

int lorb_ba_plan_read(lorb_ba_plan* plan, double* const* pose_out, double* const* point_out,
                      lorb_ba_summary* summaries) {
  if (!plan) return LORB_E_INVALID;
  if (plan->W == 0) return LORB_OK;
  return plan_read(plan, pose_out, point_out, summaries);
}

int lorb_ba_plan_trace(lorb_ba_plan* plan, int32_t window, lorb_lm_iteration* out, int32_t cap, int32_t* n_out) {
  if (!plan || !n_out || cap < 0 || (cap > 0 && !out)) return LORB_E_INVALID;
  *n_out = 0;
  if (window < 0 || window >= std::max(plan->W, 0)) return plan->W == 0 ? LORB_OK : LORB_E_INVALID;
  lorb_ctx* ctx = plan->ctx;
  WinState st;
  LORB_HIP(ctx, hipMemcpyAsync(&st, plan->d_state + window, sizeof(WinState), hipMemcpyDeviceToHost, ctx->stream));
  LORB_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const int n = std::min(std::min(st.iter, (int)LORB_LM_TRACE_CAP), (int)cap);
  if (n > 0) {
    LORB_HIP(ctx, hipMemcpyAsync(out, plan->dev.trace + (size_t)window * LORB_LM_TRACE_CAP, sizeof(lorb_lm_iteration) * n,
                                 hipMemcpyDeviceToHost, ctx->stream));
    LORB_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  *n_out = std::max(n, 0);
  return LORB_OK;
}

// diagnostic: copy BaDev::dbg -- the two-sided Cholesky's event trace of window 0 (LORB_CHOL_TRACE
// builds, 512 entries) or k_ba_ls's phase stamps, 8 per point group of a host-built plan (LORB_LS_STAMPS builds)
int lorb_ba_plan_debug_stamps(lorb_ba_plan* plan, unsigned long long* out8) {
  if (!plan || !out8) return LORB_E_INVALID;
  const size_t nst = dbg_words(1, (size_t)std::max(plan->n_pblk, plan->W));
  LORB_HIP(plan->ctx, hipMemcpyAsync(out8, plan->dev.dbg, nst * sizeof(unsigned long long), hipMemcpyDeviceToHost, plan->ctx->stream));
  LORB_HIP(plan->ctx, hipStreamSynchronize(plan->ctx->stream));
  return LORB_OK;
}

int lorb_ba_plan_info(lorb_ba_plan* plan, int32_t* info, int32_t n) {
  if (!plan || !info || n < 0) return LORB_E_INVALID;
  int bw = 0;
  for (const BaWin& w : plan->hwin) bw = std::max(bw, w.bw);
  int reordered = 0;
  for (const auto& m : plan->cam_map)
    for (size_t c = 0; c < m.size(); ++c) reordered |= m[c] != (int)c;
  int runs = 0;
  for (const BaWin& w : plan->hwin) runs += w.n_sg;
  const int32_t v[12] = {bw, plan->chol_kind, plan->n_bp, plan->n_pblk, plan->K, plan->Ptot, plan->Ctot, reordered,
                         1, red_threads(plan), plan->has_super ? runs : 0, plan->cache.kernel_nodes};
  for (int i = 0; i < n && i < 12; ++i) info[i] = v[i];
  return LORB_OK;
}

int lorb_ba_group_create(lorb_ctx* ctx, int32_t n_plans, lorb_ba_plan* const* plans, lorb_ba_group** out) {
  if (!ctx || !out || n_plans < 1 || !plans) return LORB_E_INVALID;
  *out = nullptr;
  for (int k = 0; k < n_plans; ++k) {
    if (!plans[k]) return lorb::set_error(ctx, LORB_E_INVALID, "lorb_ba_group_create: plan %d is null", k);
    if (plans[k]->ctx != ctx)
      return lorb::set_error(ctx, LORB_E_INVALID, "lorb_ba_group_create: plan %d belongs to another context", k);
    for (int j = 0; j < k; ++j)
      if (plans[j] == plans[k]) return lorb::set_error(ctx, LORB_E_INVALID, "lorb_ba_group_create: plan %d appears twice", k);
  }
  lorb_ba_group* G = new (std::nothrow) lorb_ba_group();
  if (!G) return LORB_E_NOMEM;
  G->ctx = ctx;
  G->plans.assign(plans, plans + n_plans);
  *out = G;
  return LORB_OK;
}

int lorb_ba_group_solve(lorb_ba_group* group, const lorb_lm_options* opt) {
  if (!group || !opt) return LORB_E_INVALID;
  return group_solve(group, opt);
}

int lorb_ba_group_info(lorb_ba_group* group, int32_t* info, int32_t n) {
  if (!group || !info || n < 0) return LORB_E_INVALID;
  const int32_t v[4] = {(int32_t)group->plans.size(), group->n_fused, group->cache.captures, group->cache.kernel_nodes};
  for (int i = 0; i < n && i < 4; ++i) info[i] = v[i];
  return LORB_OK;
}

int lorb_ba_group_destroy(lorb_ba_group* group) {
  if (!group) return LORB_OK;
  (void)hipStreamSynchronize(group->ctx->stream);
  delete group;
  return LORB_OK;
}

int lorb_ba_local(lorb_ctx* ctx, int32_t n_windows, const lorb_ba_window* windows,
                  const lorb_lm_options* opt, double* const* pose_out, double* const* point_out,
                  lorb_ba_summary* summaries) {
  if (!ctx || !opt) return LORB_E_INVALID;
  lorb_ba_plan* P = nullptr;
  LORB_TRY(lorb_ba_plan_create(ctx, n_windows, windows, &P));
  int rc = lorb_ba_plan_solve(P, opt);
  if (rc == LORB_OK) rc = lorb_ba_plan_read(P, pose_out, point_out, summaries);
  lorb_ba_plan_destroy(P);
  return rc;
}

int lorb_ba_pose_only(lorb_ctx* ctx, const lorb_pose_problem_batch* prob,
                      const lorb_lm_options* opt, double* pose_out, float* Tcw_out,
                      lorb_ba_summary* summaries) {
  if (!ctx || !prob || !opt || !pose_out) return LORB_E_INVALID;
  const int nf = prob->n_frames;
  if (nf <= 0) return LORB_OK;
  const int nr = prob->res_off[nf];
  // every input in one pinned staging, poses and summaries stored straight into pinned memory.  A
  // batch whose frames all fit the kernel's register-resident residuals reads each input once: the
  // kernel then reads the mapped staging directly (no pull launch); larger frames re-read theirs
  // every pass, from HBM after a pull.
  int max_res = 0;
  for (int f = 0; f < nf; ++f) max_res = std::max(max_res, prob->res_off[f + 1] - prob->res_off[f]);
  lorb::InPack in(ctx);
  const int i_roff = in.add_t(prob->res_off, (size_t)nf + 1), i_intr = in.add_t(prob->intr, (size_t)nf * 4),
            i_pinit = in.add_t(prob->pose_init, (size_t)nf * 6), i_pts = in.add_t(prob->pts3d, (size_t)nr * 3),
            i_obs = in.add_t(prob->obs2d, (size_t)nr * 2);
  LORB_TRY(in.commit(max_res <= kPoRegRes));
  lorb::OutPack out(ctx);
  const int o_pose = out.add(sizeof(double) * 6 * nf), o_sum = out.add(sizeof(lorb_ba_summary) * nf);
  LORB_TRY(out.alloc(true));  // the kernel stores poses and summaries into the mapped block
  PoOff aoff{};
  if (nf <= kPoArgF) {
    aoff.n = nf;
    for (int f = 0; f <= nf; ++f) aoff.off[f] = prob->res_off[f];
  }
  hipLaunchKernelGGL(k_ba_pose_only, dim3(nf), dim3(kPoThreads), 0, ctx->stream, aoff, in.dev<int32_t>(i_roff), in.dev<float>(i_intr),
                     in.dev<float>(i_pinit), in.dev<float>(i_pts), in.dev<float>(i_obs), to_dev_opt(opt),
                     out.dev<double>(o_pose), out.dev<lorb_ba_summary>(o_sum));
  LORB_CHECK_LAUNCH(ctx);
  LORB_TRY(out.fetch());
  memcpy(pose_out, out.host<double>(o_pose), sizeof(double) * 6 * nf);
  if (summaries) memcpy(summaries, out.host<lorb_ba_summary>(o_sum), sizeof(lorb_ba_summary) * nf);
  if (Tcw_out)
    for (int f = 0; f < nf; ++f) {
      const float R[3] = {(float)pose_out[6 * f], (float)pose_out[6 * f + 1], (float)pose_out[6 * f + 2]};
      const float T[3] = {(float)pose_out[6 * f + 3], (float)pose_out[6 * f + 4], (float)pose_out[6 * f + 5]};
      lorb_pose_to_Tcw(R, T, Tcw_out + 16 * f);
    }
  return LORB_OK;
}

int lorb_ba_pose_only_dev(lorb_ctx* ctx, const lorb_pose_problem_batch* d_prob, const lorb_lm_options* opt,
                          double* d_pose_out, lorb_ba_summary* d_summaries) {
  if (!ctx || !d_prob || !opt) return LORB_E_INVALID;
  const int nf = d_prob->n_frames;
  if (nf <= 0) return LORB_OK;
  if (!d_prob->res_off || !d_prob->intr || !d_prob->pose_init || !d_pose_out || !d_summaries)
    return lorb::set_error(ctx, LORB_E_INVALID, "null array");
  // the offsets live on the device: the kernel reads them from memory (aoff.n == 0)
  PoOff aoff{};
  hipLaunchKernelGGL(k_ba_pose_only, dim3(nf), dim3(kPoThreads), 0, ctx->stream, aoff, d_prob->res_off, d_prob->intr,
                     d_prob->pose_init, d_prob->pts3d, d_prob->obs2d, to_dev_opt(opt), d_pose_out, d_summaries);
  LORB_CHECK_LAUNCH(ctx);
  return LORB_OK;
}

// cv::Rodrigues (vector -> matrix, double internally) + Frame::UpdatePoseMat write-back
// (lorb::pose_to_Tcw turns contraction off in its own body: the file-scope pragma must not reach this
// restatement, which rounds like the reference's un-contracted host build whatever -march the
// library is built with)
void lorb_pose_to_Tcw(const float rvec[3], const float tvec[3], float T[16]) { lorb::pose_to_Tcw(rvec, tvec, T); }

// cv::Rodrigues (matrix -> vector) + Frame::UpdatePoseVector's translation (lorb::Tcw_to_rvec, which
// turns contraction off in its own body for the same reason)
int lorb_Tcw_to_pose(const float Tcw[16], float R[3], float T[3]) {
  if (!Tcw || !R || !T) return LORB_E_INVALID;
  lorb::Tcw_to_rvec(Tcw, R);
  T[0] = Tcw[3]; T[1] = Tcw[7]; T[2] = Tcw[11];
  return LORB_OK;
}

// Frame::SetPose(Tcw): the host's way to make a frame's first block (lorb::inv4_lu32f is float only and
// lives in lorb_window.hip, compiled -ffp-contract=off)
int lorb_frame_pose_from_Tcw(const float Tcw[16], lorb_frame_pose* out) {
  if (!Tcw || !out) return LORB_E_INVALID;
  memcpy(out->Tcw, Tcw, sizeof(out->Tcw));
  lorb::inv4_lu32f(Tcw, out->Twc);
  lorb::Tcw_to_rvec(Tcw, out->pose);
  out->pose[3] = Tcw[3]; out->pose[4] = Tcw[7]; out->pose[5] = Tcw[11];
  out->status = 0;
  return LORB_OK;
}

}  // extern "C"
