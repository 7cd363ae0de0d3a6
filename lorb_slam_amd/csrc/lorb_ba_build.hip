// lorb_ba_build.hip -- construction of bundle-adjustment plans (lorb_ba_plan.h): the host builder
// (build_plan: windows given as host arrays), the device builder (dev_build: one window whose
// observation arrays live in HBM, rebuilt every LocalMapping step) with its k_db_* kernels, and the
// entry points that create, rebuild, read out and destroy a plan.  Nothing here runs during a solve
// (lorb_ba.hip).  FP64 contraction as in every BA unit (see there): the block below, before any include.
#ifndef LORB_NO_CONTRACT  // A/B builds only (tools/isa_fma.py, tools/build_variant.sh nofma -DLORB_NO_CONTRACT)
#pragma clang fp contract(fast)
#endif
#include "lorb_ba_math.h"
#include "lorb_internal.h"
#include "lorb_ba_dev.h"
#include "lorb_ba_plan.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <map>

// ------------------------------------------------------------------------------------------
// device plan construction state (lorb_ba_plan_create_dev; see "Device-resident plan construction")
struct lorb_ba_devbuild {
  int K_cap = 0, P_cap = 0, C = 0, F = 0, Wd = 0;
  int* key_out = nullptr; int* val_out = nullptr;  // point-sorted: point, observation slot
  // build scratch, one allocation: pt_cnt (P_cap + 1) | hdr (8) | cov (C * C) | cam_cnt (C) | bits
  // (C * Wd u64, camera x point); cleared by the build before (k_db_gather), else by one memset
  int* scr = nullptr; size_t scr_bytes = 0;
  int* pt_cnt = nullptr;      // P_cap + 1
  int* hdr = nullptr;         // [0] valid obs, [1] max obs per point, [2] error flags, [3] points
  int* cov = nullptr;         // C * C
  int* cam_cnt = nullptr;     // C
  unsigned long long* bits = nullptr;
  int* perm = nullptr;        // C: input camera -> plan camera
  int pblk_cap = 0, part_cap = 0, gspan_cap = 0, sgrp_cap = 0;
  size_t gpart_cap = 0;  // doubles of BaDev::gpart (the point groups' partials)
  int* pinned = nullptr; size_t pinned_n = 0;  // the readback's landing buffer (pinned host memory)
  bool dirty = true;  // the build scratch needs a clearing fill (first build, or after a failed one)
  bool sorted_hint = false;  // the caller's slots are sorted by point: try k_db_sorted first
  std::vector<double> h_red;                     // sharded: the build's host all-reduce
  // per-build structure uploaded in one copy: [BaWin | live (3) | perm (C) | gcam (C) | adj (C * C bytes) |
  // bp (up_bp_cap)]
  unsigned char* up_dev = nullptr; unsigned char* up_host = nullptr; int up_bp_cap = 0;
  const unsigned char* up_host_dev = nullptr;  // up_host as the device reads it (pinned, mapped)
  size_t off_live = 0, off_perm = 0, off_gcam = 0, off_adj = 0, off_bp = 0, up_bytes = 0;
  // Speculation on the plan's structure (dev_spec_issue / dev_spec_verify): a completed build keeps
  // what its host phase derived from the adjacency pattern -- last_adj and last_map (below), the
  // (ch, cl) block list (last_bps), the band (hwin[0].bw) and the groups per partial run (spec_sf) --
  // and the upload block keeps the parts that do not depend on counts (perm, the block list's
  // (ch, cl), BaWin's band and layout constants, the adjacency as bytes).  spec_ok: all of that
  // describes the plan as the device holds it.  spec_pending: a speculative gather is queued and
  // not yet verified.  spec_out: the words k_db_spec leaves for k_db_gather<true> (see DbSpec).
  bool spec_ok = false, spec_pending = false;
  int spec_sf = 1;
  int* spec_out = nullptr;
  // camera_order is a function of the adjacency pattern alone: a build whose pattern equals the
  // previous one's (a sliding window usually keeps its banded pattern) reuses that order
  std::vector<char> last_adj;
  std::vector<int> h_copy;  // host copy of the build's readback
  std::vector<int> last_map;
  std::vector<lorb::ba::BlockPair> last_bps;  // the last completed build's block list
  // a build issued (dev_build_issue: phase 1 and the readback queued) and not yet finished
  hipEvent_t rb_ev = nullptr;
  bool rb_pending = false, rb_sorted = false, rb_fuse = false;
  ~lorb_ba_devbuild() {  // owns the event and the pinned blocks (the device allocations are in the plan's `allocs`)
    if (rb_ev) (void)hipEventDestroy(rb_ev);
    if (pinned) (void)hipHostFree(pinned);
    if (up_host) (void)hipHostFree(up_host);
  }
};

namespace {

using namespace lorb::ba;

// the diagnostics a plan prints when it is destroyed (LORB_HOST_PHASE, LORB_PM_SPANS and, in
// LORB_LS_STAMPS builds, LORB_LS_PRINT); nothing unless one of them is enabled
void print_diagnostics(const lorb_ba_plan& p) {
  if (p.hp_n)
    fprintf(stderr, "lorb_ba_plan: host phase %.2f us per device build (%d builds): checks %.2f order %.2f blocks %.2f "
            "buffers %.2f staging %.2f launch %.2f\n", p.hp_us / p.hp_n, p.hp_n, p.hp_sec[0] / p.hp_n, p.hp_sec[1] / p.hp_n,
            p.hp_sec[2] / p.hp_n, p.hp_sec[3] / p.hp_n, p.hp_sec[4] / p.hp_n, p.hp_sec[5] / p.hp_n);
  // LORB_PM_SPANS=1 (diagnostics): the point groups' camera spans of the last linearisation
  if (p.dev.gspan && p.n_pblk > 0 && getenv("LORB_PM_SPANS")) {
    std::vector<int2> gs(p.n_pblk);
    if (hipStreamSynchronize(p.ctx->stream) == hipSuccess &&
        hipMemcpy(gs.data(), p.dev.gspan, sizeof(int2) * p.n_pblk, hipMemcpyDeviceToHost) == hipSuccess) {
      std::vector<int> sp;
      for (const int2& g : gs) if (g.y > 0) sp.push_back(g.y);
      std::sort(sp.begin(), sp.end());
      if (!sp.empty())
        fprintf(stderr, "lorb_ba_plan: %d point groups (%zu live), %d observations; camera span p50 %d p90 %d max %d\n",
                p.n_pblk, sp.size(), p.K, sp[sp.size() / 2], sp[sp.size() * 9 / 10], sp.back());
    }
  }
#ifdef LORB_LS_STAMPS
  // LORB_LS_PRINT=1: the last k_ba_ls launch's phase cycles (medians over the point groups)
  if (p.dev.dbg && p.n_pblk > 0 && getenv("LORB_LS_PRINT")) {
    std::vector<unsigned long long> st((size_t)p.n_pblk * 8);
    if (hipStreamSynchronize(p.ctx->stream) == hipSuccess &&
        hipMemcpy(st.data(), p.dev.dbg, sizeof(unsigned long long) * st.size(), hipMemcpyDeviceToHost) == hipSuccess) {
      fprintf(stderr, "lorb_ba_plan: k_ba_ls phase cycles (median, p90):");
      for (int k = 0; k < 5; ++k) {
        std::vector<long long> v;
        for (int g = 0; g < p.n_pblk; ++g)
          if (st[8 * g]) v.push_back((long long)(st[8 * g + k + 1] - st[8 * g + k]));
        std::sort(v.begin(), v.end());
        if (!v.empty()) fprintf(stderr, " %c %lld %lld", "ABCDE"[k], v[v.size() / 2], v[v.size() * 9 / 10]);
      }
      fprintf(stderr, "\n");
      // per XCC (s_memtime is per XCC): first start -> last end, and groups that shared a CU with
      // an earlier one (same XCC / SE / SH / CU) -- started after it ended (serial) or not (co-resident)
      std::map<unsigned long long, std::vector<int>> by_cu;
      unsigned long long r0 = ~0ull, r1 = 0;
      std::vector<long long> dur;
      for (int g = 0; g < p.n_pblk; ++g) {
        if (!st[8 * g]) continue;
        const unsigned long long a = st[8 * g + 7] >> 20, b = a + (st[8 * g + 7] & 0xfffff);
        r0 = std::min(r0, a); r1 = std::max(r1, b);
        dur.push_back((long long)(b - a));
        by_cu[st[8 * g + 6] & 0xff00ffull].push_back(g);  // XCC | CU / SH / SE of HW_ID
      }
      std::sort(dur.begin(), dur.end());
      int shared = 0;
      long long pair_max = 0;
      for (auto& c : by_cu) {
        if (c.second.size() < 2) continue;
        ++shared;
        unsigned long long a = ~0ull, b = 0;
        for (int g : c.second) { a = std::min(a, st[8 * g + 7] >> 20); b = std::max(b, (st[8 * g + 7] >> 20) + (st[8 * g + 7] & 0xfffff)); }
        pair_max = std::max(pair_max, (long long)(b - a));
      }
      if (!dur.empty())
        fprintf(stderr, "lorb_ba_plan: k_ba_ls real time (us): first start -> last end %.2f; group p50 %.2f p90 %.2f max %.2f; "
                "%zu CUs, %d with > 1 group (their span max %.2f)\n", (r1 - r0) * 0.01, dur[dur.size() / 2] * 0.01,
                dur[dur.size() * 9 / 10] * 0.01, dur.back() * 0.01, by_cu.size(), shared, pair_max * 0.01);
      // the slowest groups: phases, points / observations, camera span
      std::vector<PBlk> pb(p.n_pblk);
      std::vector<int2> gs(p.n_pblk);
      if (hipMemcpy(pb.data(), p.dev.pblk, sizeof(PBlk) * p.n_pblk, hipMemcpyDeviceToHost) == hipSuccess &&
          hipMemcpy(gs.data(), p.dev.gspan, sizeof(int2) * p.n_pblk, hipMemcpyDeviceToHost) == hipSuccess) {
        std::vector<int> ord;
        for (int g = 0; g < p.n_pblk; ++g) if (st[8 * g]) ord.push_back(g);
        std::sort(ord.begin(), ord.end(), [&](int a, int b) { return (st[8 * a + 7] & 0xfffff) > (st[8 * b + 7] & 0xfffff); });
        for (size_t i = 0; i < ord.size() && i < 6; ++i) {
          const int g = ord[i];
          fprintf(stderr, "  group %d: %.2f us, points %d obs %d span %d, phases", g, (st[8 * g + 7] & 0xfffff) * 0.01,
                  pb[g].cnt, pb[g].no, gs[g].y);
          for (int k = 0; k < 5; ++k) fprintf(stderr, " %lld", (long long)(st[8 * g + k + 1] - st[8 * g + k]));
          fprintf(stderr, "\n");
        }
      }
    }
  }
#endif
}

template <typename T>
int dalloc(lorb_ba_plan* P, size_t n, T** out) {
  void* p = nullptr;
  LORB_HIP(P->ctx, hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)));
  P->allocs.push_back(p);
  *out = static_cast<T*>(p);
  return LORB_OK;
}
template <typename T>
int dupload(lorb_ba_plan* P, const std::vector<T>& v, T** out) {
  LORB_TRY(dalloc(P, v.size(), out));
  if (!v.empty())
    LORB_HIP(P->ctx, hipMemcpyAsync(*out, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, P->ctx->stream));
  return LORB_OK;
}
template <typename T>  // (BaDev's read-only arrays)
int dalloc(lorb_ba_plan* P, size_t n, const T** out) { return dalloc(P, n, const_cast<T**>(out)); }
template <typename T>
int dupload(lorb_ba_plan* P, const std::vector<T>& v, const T** out) { return dupload(P, v, const_cast<T**>(out)); }
// frees a plan allocation once the stream is idle and forgets it in `allocs`
int dfree(lorb_ba_plan* P, const void* ptr) {
  LORB_HIP(P->ctx, hipStreamSynchronize(P->ctx->stream));
  LORB_HIP(P->ctx, hipFree(const_cast<void*>(ptr)));
  auto it = std::find(P->allocs.begin(), P->allocs.end(), ptr);
  if (it != P->allocs.end()) P->allocs.erase(it);
  return LORB_OK;
}

// Camera-level half band of S for a labelling (pos[c] = new index of camera c): max over cameras of
// pos(c) - min(pos(n)) over the cameras n it shares a point with (itself included).
int camera_band(int C, const std::vector<char>& adj, const std::vector<int>& pos) {
  int b = 0;
  for (int c = 0; c < C; ++c) {
    int lo = pos[c];
    for (int n = 0; n < C; ++n)
      if (adj[(size_t)c * C + n]) lo = std::min(lo, pos[n]);
    b = std::max(b, pos[c] - lo);
  }
  return b;
}

// Reverse Cuthill-McKee over the window's camera covisibility graph (adj: C x C, symmetric).  The
// reference orders a LocalPoseOptimization window as [current] + GetCovisibleFrames() sorted by
// ascending covisibility weight (src/bundle_adjust.cpp:210-220, src/frame.cpp:754-774), which
// scatters the non-zero blocks of S over the whole matrix; RCM restores a narrow band, so the
// banded Cholesky applies.  Deterministic: BFS from the lowest-degree unvisited camera (lowest
// index on ties), neighbours in (degree, index) order, then reversed.  Returns old -> new; the
// identity when RCM does not narrow the band.
std::vector<int> camera_order(int C, const std::vector<char>& adj) {
  std::vector<int> id(C), deg(C, 0);
  for (int c = 0; c < C; ++c) {
    id[c] = c;
    for (int n = 0; n < C; ++n) deg[c] += (n != c) && adj[(size_t)c * C + n];
  }
  static const bool off = env_flag("LORB_NO_RCM");
  if (off || C < 3) return id;
  std::vector<int> order;
  std::vector<char> seen(C, 0);
  order.reserve(C);
  while ((int)order.size() < C) {
    int s = -1;
    for (int c = 0; c < C; ++c)
      if (!seen[c] && (s < 0 || deg[c] < deg[s])) s = c;
    size_t head = order.size();
    order.push_back(s);
    seen[s] = 1;
    while (head < order.size()) {
      const int u = order[head++];
      std::vector<int> nb;
      for (int n = 0; n < C; ++n)
        if (n != u && adj[(size_t)u * C + n] && !seen[n]) nb.push_back(n);
      std::sort(nb.begin(), nb.end(), [&](int a, int b) { return deg[a] != deg[b] ? deg[a] < deg[b] : a < b; });
      for (int n : nb) { seen[n] = 1; order.push_back(n); }
    }
  }
  std::reverse(order.begin(), order.end());
  std::vector<int> pos(C);
  for (int i = 0; i < C; ++i) pos[order[i]] = i;
  return camera_band(C, adj, pos) < camera_band(C, adj, id) ? pos : id;
}

// Point groups and their partials.  A group's camera window [cmin, cmin + span) is held by
// k_ba_ls as two 64-bit words per point, so a group spans at most kPmSpan cameras: device-built
// plans (one window of C cameras) take C <= kPmSpan; host-built plans cut a group where the next
// point would widen it past kPmSpan (any C, as long as no single point's cameras lie more than
// kPmSpan apart in the plan's camera order).
constexpr int kPmSpan = 128;
// the partial budget of one plan: a group's partial holds the camera blocks of a
// window of `span_max` cameras; far above every workload here (C4: 5 MB, the shared window: 0.3 GB)
constexpr size_t kPartBudgetBytes = (size_t)16 << 30;
// a window's partial layout: camera half band, the slots of a group window of span_max cameras, the
// camera terms after them; its groups' partials from `total` on (advanced)
void pm_layout(BaWin& bw, int span_max, long long& total) {
  bw.bwc = bw.n > 0 ? std::max(bw.bw - 5, 0) / 6 : 0;
  span_max = std::max(std::min(span_max, bw.n_poses), 0);
  bw.part_cam = 36 * pm_nslots(span_max, bw.bwc);
  bw.part_stride = bw.part_cam + 18 * span_max;
  bw.part_base = total;
  total += (long long)bw.n_sg * bw.part_stride;
}
// Partial runs: F consecutive point groups per k_ba_ls workgroup, one partial per run, when a window
// has more point groups than one round of two workgroups per CU takes (F = 1 otherwise: C3 / C4
// windows, alone or batched -- F depends on the window only, so a window's bits do not depend on its
// plan's other windows).  LORB_SG_F=k forces k (tests).
int sg_factor(int n_pblk) {
  const char* e = getenv("LORB_SG_F");
  if (e && atoi(e) >= 1) return n_pblk > 1 ? atoi(e) : 1;
  return n_pblk > 512 ? (n_pblk + 479) / 480 : 1;
}
int part_budget_check(lorb_ctx* ctx, long long total) {
  if ((size_t)std::max(total, 1ll) * sizeof(double) > kPartBudgetBytes)
    return lorb::set_error(ctx, LORB_E_NOMEM, "point-group partials need %.1f GB (> %.0f GB budget)",
                           (double)total * sizeof(double) / 1e9, (double)kPartBudgetBytes / 1e9);
  return LORB_OK;
}

// uniform band of S from each camera's first coupled camera: bw = max_i (i - first_nonzero_col(i));
// exact for Cholesky (no fill outside the envelope, and the zero padding never changes a value)
int band_of(const std::vector<int>& fc) {
  int bw = 0;
  for (int c = 0; c < (int)fc.size(); ++c) bw = std::max(bw, 6 * c + 5 - 6 * fc[c]);
  return bw;
}

// The exchange buffers of a plan of C cameras and W windows (see BaDev): [lin | pad | solve] in one
// block (the sharded fused iteration all-reduces both at once; solve, of solve_n doubles, starts
// 256-byte aligned), the gradient maxima and the step sums.  Over more than one rank the *_part
// twins are this rank's partial sums (zeroed here), all-reduced into the global buffers; otherwise
// the exchanges are the identity: the partials alias the global buffers and the collectives run in
// place.  The caller places env / rhs / wfail in *sol (global) and *sol_part, in its own order.
int alloc_exchange(lorb_ba_plan* P, size_t C, size_t W, size_t solve_n, double** sol, double** sol_part) {
  BaDev& d = P->dev;
  const lorb_comm* comm = P->comm;
  const size_t lin_pad = (C * 27 + 2 * W + 31) & ~(size_t)31;
  P->fx_n = lin_pad + solve_n;
  double *lin, *mx, *stp;
  LORB_TRY(dalloc(P, P->fx_n, &lin)); LORB_TRY(dalloc(P, W, &mx)); LORB_TRY(dalloc(P, 3 * W, &stp));
  double *linp = lin, *mxp = mx, *stpp = stp;
  if (comm && comm->nranks > 1) {
    LORB_TRY(dalloc(P, P->fx_n, &linp)); LORB_TRY(dalloc(P, W, &mxp)); LORB_TRY(dalloc(P, 3 * W, &stpp));
    LORB_HIP(P->ctx, hipMemsetAsync(linp, 0, sizeof(double) * P->fx_n, P->ctx->stream));
  }
  d.U = lin; d.V = lin + C * 21; d.wlin = lin + C * 27; d.wmax = mx; d.wstep = stp;
  d.U_part = linp; d.V_part = linp + C * 21; d.wlin_part = linp + C * 27; d.wmax_part = mxp; d.wstep_part = stpp;
  *sol = lin + lin_pad; *sol_part = linp + lin_pad;
  P->x2_send = *sol_part; P->x2_recv = *sol;
  d.sharded = comm ? 1 : 0;
  d.rank0 = comm ? (comm->rank == 0) : 1;
  return LORB_OK;
}

// per point of a window, the optimised cameras of its observations (build_plan's main pass rejects
// the observations skipped here)
std::vector<std::vector<int>> point_cameras(const lorb_ba_window& in) {
  std::vector<std::vector<int>> pf(std::max(in.n_points, 0));
  for (int k = 0; k < in.n_obs; ++k) {
    const int p = in.obs_point[k], f = in.obs_frame[k];
    if (p >= 0 && p < in.n_points && f >= 0 && f < in.n_poses) pf[p].push_back(f);
  }
  return pf;
}

int build_plan(lorb_ctx* ctx, int nw, const lorb_ba_window* win_in, lorb_ba_plan* P) {
  // camera relabelling per window (RCM), applied to copies of the pose / observation arrays; the
  // covisibility graph of a sharded window is all-reduced so every rank picks the same order
  P->cam_map.assign(nw, {});
  std::vector<lorb_ba_window> wins(win_in, win_in + nw);
  std::vector<std::vector<int>> frame_buf(nw);
  std::vector<std::vector<float>> pose_buf(nw);
  for (int w = 0; w < nw; ++w) {
    const lorb_ba_window& in = win_in[w];
    const int C = std::max(in.n_poses, 0);
    std::vector<char> adj((size_t)C * C, 0);
    for (auto& v : point_cameras(in))
      for (int a : v)
        for (int b : v) adj[(size_t)a * C + b] = 1;
    if (P->comm && C > 0) {
      std::vector<double> h(adj.begin(), adj.end());
      LORB_TRY(lorb::comm_allreduce_host(P->comm, h.data(), h.size(), LORB_OP_MAX));
      for (size_t i = 0; i < h.size(); ++i) adj[i] = h[i] > 0.0;
    }
    std::vector<int> map = camera_order(C, adj);
    bool ident = true;
    for (int c = 0; c < C; ++c) ident &= map[c] == c;
    P->cam_map[w] = map;
    if (ident) continue;
    frame_buf[w].assign(in.obs_frame, in.obs_frame + std::max(in.n_obs, 0));
    for (int& f : frame_buf[w])
      if (f >= 0 && f < C) f = map[f];
    pose_buf[w].resize(6 * (size_t)C);
    for (int c = 0; c < C; ++c)
      for (int q = 0; q < 6; ++q) pose_buf[w][6 * (size_t)map[c] + q] = in.pose_init[6 * (size_t)c + q];
    wins[w].obs_frame = frame_buf[w].data();
    wins[w].pose_init = pose_buf[w].data();
  }
  const lorb_ba_window* win = wins.data();
  P->ctx = ctx;
  P->W = nw;
  lorb_comm* comm = P->comm;
  // sharded: band structure, camera activity and observation counts are global -- reduce the
  // per-window first-coupled camera (min), per-camera and per-window observation counts (sum)
  std::vector<std::vector<int>> g_fc(nw);
  std::vector<std::vector<int>> g_cam_obs(nw);
  std::vector<int> g_obs(nw, 0);
  if (comm) {
    size_t nfc = 0;
    for (int w = 0; w < nw; ++w) nfc += (size_t)std::max(win[w].n_poses, 0);
    std::vector<double> hmin(nfc), hsum(nfc + nw);
    size_t o = 0;
    for (int w = 0; w < nw; ++w) {
      const lorb_ba_window& in = win[w];
      std::vector<int> fc(std::max(in.n_poses, 0)), cobs(std::max(in.n_poses, 0), 0);
      for (int c = 0; c < in.n_poses; ++c) fc[c] = c;
      for (auto& v : point_cameras(in))
        for (int a : v) {
          cobs[a]++;
          for (int b : v) fc[a] = std::min(fc[a], b);
        }
      for (int c = 0; c < in.n_poses; ++c) { hmin[o + c] = fc[c]; hsum[o + c] = cobs[c]; }
      hsum[nfc + w] = in.n_obs;
      o += in.n_poses;
    }
    LORB_TRY(lorb::comm_allreduce_host(comm, hmin.data(), hmin.size(), LORB_OP_MIN));
    LORB_TRY(lorb::comm_allreduce_host(comm, hsum.data(), hsum.size(), LORB_OP_SUM));
    o = 0;
    for (int w = 0; w < nw; ++w) {
      g_fc[w].resize(win[w].n_poses); g_cam_obs[w].resize(win[w].n_poses);
      for (int c = 0; c < win[w].n_poses; ++c) { g_fc[w][c] = (int)hmin[o + c]; g_cam_obs[w][c] = (int)hsum[o + c]; }
      g_obs[w] = (int)hsum[nfc + w];
      o += win[w].n_poses;
    }
  }
  std::vector<int> cam_active;
  std::vector<int> pt_obs_off(1, 0), obs_cam, obs_fix, obs_pt;
  std::vector<double2> obs_uv;
  std::vector<double> fixed, xpose, xpt;
  std::vector<PBlk> pblk;
  std::vector<int2> gcam;   // per point group: first / last optimised camera (plan numbering)
  std::vector<int4> sgrp;   // partial runs
  std::vector<BlockPair> bps;
  int pose_base = 0, point_base = 0, fix_base = 0, env_base = 0, row_base = 0, n_pairs = 0;
  long long part_total = 0;
  for (int w = 0; w < nw; ++w) {
    const lorb_ba_window& in = win[w];
    if (in.n_poses < 0 || in.n_points < 0 || in.n_obs < 0 || in.n_fixed < 0)
      return lorb::set_error(ctx, LORB_E_INVALID, "window %d: negative sizes", w);
    BaWin bw{};
    bw.pose_base = pose_base; bw.n_poses = in.n_poses;
    bw.point_base = point_base; bw.n_points = in.n_points;
    bw.fx = in.fx; bw.fy = in.fy; bw.cx = in.cx; bw.cy = in.cy;
    bw.obs_base = (int)obs_cam.size(); bw.n_obs = in.n_obs;
    bw.n_obs_all = comm ? g_obs[w] : in.n_obs;
    // obs sorted by point (stable)
    std::vector<int> cnt(in.n_points + 1, 0);
    for (int k = 0; k < in.n_obs; ++k) {
      const int p = in.obs_point[k], f = in.obs_frame[k];
      if (p < 0 || p >= in.n_points) return lorb::set_error(ctx, LORB_E_INVALID, "window %d obs %d: bad point %d", w, k, p);
      if (f >= in.n_poses || f < -in.n_fixed) return lorb::set_error(ctx, LORB_E_INVALID, "window %d obs %d: bad frame %d", w, k, f);
      cnt[p + 1]++;
    }
    for (int p = 0; p < in.n_points; ++p) cnt[p + 1] += cnt[p];
    std::vector<int> order(in.n_obs), fill(in.n_points, 0);
    for (int k = 0; k < in.n_obs; ++k) { const int p = in.obs_point[k]; order[cnt[p] + fill[p]++] = k; }
    const int ob0 = (int)obs_cam.size();
    for (int p = 0; p < in.n_points; ++p) pt_obs_off.push_back(ob0 + cnt[p + 1]);
    for (int e = 0; e < in.n_obs; ++e) {
      const int k = order[e], f = in.obs_frame[k];
      obs_cam.push_back(f >= 0 ? pose_base + f : -1);
      obs_pt.push_back(point_base + in.obs_point[k]);
      obs_fix.push_back(f >= 0 ? -1 : fix_base + (-1 - f));
      obs_uv.push_back(make_double2(in.obs_uv[2 * k], in.obs_uv[2 * k + 1]));
    }
    for (int i = 0; i < 6 * in.n_fixed; ++i) fixed.push_back(in.fixed_pose[i]);
    for (int i = 0; i < 6 * in.n_poses; ++i) xpose.push_back(in.pose_init[i]);
    for (int i = 0; i < 3 * in.n_points; ++i) xpt.push_back(in.point_init[i]);
    // camera activity: observed by this rank (sharded: by some rank)
    {
      std::vector<int> n_cam(in.n_poses, 0);
      for (int e = 0; e < in.n_obs; ++e) { const int c = obs_cam[ob0 + e]; if (c >= 0) n_cam[c - pose_base]++; }
      for (int c = 0; c < in.n_poses; ++c) cam_active.push_back(comm ? (g_cam_obs[w][c] > 0) : n_cam[c] > 0);
    }
    // camera blocks (ch, cl), ch >= cl, that some point couples, with their observation-pair counts
    // (every diagonal block exists); the first coupled camera of each row for the band
    std::map<std::pair<int, int>, int> bmap;
    for (int c = 0; c < in.n_poses; ++c) bmap[{c, c}];
    std::vector<int> fc(in.n_poses);
    for (int c = 0; c < in.n_poses; ++c) fc[c] = c;
    for (int p = 0; p < in.n_points; ++p) {
      const int e0 = ob0 + cnt[p], e1 = ob0 + cnt[p + 1];
      for (int a = e0; a < e1; ++a) {
        const int ca = obs_cam[a];
        if (ca < 0) continue;
        for (int b = e0; b < e1; ++b) {
          const int cb = obs_cam[b];
          if (cb < 0 || cb > ca) continue;
          // the reference keys a point's observations by Frame* (include/map_point.h:83): one per
          // camera (k_ba_ls places a point's observations by camera rank)
          if (cb == ca && a != b)
            return lorb::set_error(ctx, LORB_E_INVALID, "window %d: a point observed twice by one camera", w);
          bmap[{ca - pose_base, cb - pose_base}]++;
          fc[ca - pose_base] = std::min(fc[ca - pose_base], cb - pose_base);
        }
      }
    }
    for (auto& kv : bmap) {
      bps.push_back(BlockPair{w, pose_base + kv.first.first, pose_base + kv.first.second, n_pairs, kv.second});
      n_pairs += kv.second;
    }
    const int n = 6 * in.n_poses;
    if (comm)
      for (int c = 0; c < in.n_poses; ++c) fc[c] = std::min(fc[c], g_fc[w][c]);
    const int bwid = band_of(fc);
    bw.env_base = env_base; bw.env_size = n * (bwid + 1); bw.n = n; bw.row_base = row_base; bw.bw = bwid;
    P->max_env = std::max(P->max_env, bw.env_size + 2 * n);
    P->max_bw = std::max(P->max_bw, bwid);
    if (n > 0) P->min_bw = std::min(P->min_bw, bwid);
    {
      const int n16 = (n + 15) & ~15;
      P->max_env_w = std::max(P->max_env_w, chol_lds_words(n16, bwid));
      if (n16 > 0) P->min_n16 = std::min(P->min_n16, n16);
    }
    env_base += bw.env_size; row_base += n;
    // point groups: consecutive points with <= kGB observations (and <= kGB points) in total whose
    // optimised cameras span <= kPmSpan (k_ba_ls's camera masks); the widest group sizes the partials
    bw.pblk_base = (int)pblk.size();
    int span_max = 0;
    for (int p = 0; p < in.n_points;) {
      PBlk g{w, point_base + p, 0, ob0 + cnt[p], 0};
      int gmin = INT32_MAX, gmax = -1;
      while (p < in.n_points && g.cnt < kGB) {
        const int k = cnt[p + 1] - cnt[p];
        int pmin = INT32_MAX, pmax = -1;
        for (int e = ob0 + cnt[p]; e < ob0 + cnt[p + 1]; ++e)
          if (obs_cam[e] >= 0) { pmin = std::min(pmin, obs_cam[e]); pmax = std::max(pmax, obs_cam[e]); }
        if (k > kGB)
          return lorb::set_error(ctx, LORB_E_UNSUPPORTED, "window %d: point %d has %d observations (a point group holds %d)",
                                 w, p, k, kGB);
        if (pmax - pmin >= kPmSpan)
          return lorb::set_error(ctx, LORB_E_UNSUPPORTED, "window %d: point %d is seen by cameras %d apart (at most %d)",
                                 w, p, pmax - pmin, kPmSpan - 1);
        const int nmin = std::min(gmin, pmin), nmax = std::max(gmax, pmax);
        if (g.cnt > 0 && (g.no + k > kGB || (nmax >= 0 && nmax - nmin >= kPmSpan))) break;
        g.cnt++; g.no += k; ++p;
        gmin = nmin; gmax = nmax;
      }
      if (gmax >= 0) span_max = std::max(span_max, gmax - gmin + 1);
      pblk.push_back(g);
      gcam.push_back(make_int2(gmin, gmax));
    }
    bw.n_pblk = (int)pblk.size() - bw.pblk_base;
    {  // partial runs (super-groups) and the widest run's camera window
      const int F = sg_factor(bw.n_pblk);
      bw.sg_base = (int)sgrp.size();
      if (F > 1) span_max = 0;
      for (int g = 0; g < bw.n_pblk; g += F) {
        const int ng = std::min(F, bw.n_pblk - g);
        sgrp.push_back(make_int4(w, bw.pblk_base + g, ng, 0));
        int umin = INT32_MAX, umax = -1;
        for (int k = 0; k < ng; ++k) {
          const int2 c = gcam[bw.pblk_base + g + k];
          if (c.y >= 0) { umin = std::min(umin, c.x); umax = std::max(umax, c.y); }
        }
        if (F > 1 && umax >= 0) span_max = std::max(span_max, umax - umin + 1);
      }
      bw.n_sg = (int)sgrp.size() - bw.sg_base;
      P->has_super = P->has_super || F > 1;
    }
    pm_layout(bw, span_max, part_total);
    P->hwin.push_back(bw);
    pose_base += in.n_poses; point_base += in.n_points; fix_base += in.n_fixed;
  }
  P->Ctot = pose_base; P->Ptot = point_base; P->K = (int)obs_cam.size(); P->NF = fix_base;
  LORB_TRY(part_budget_check(ctx, part_total));
  P->n_pblk = (int)pblk.size(); P->n_bp = (int)bps.size(); P->n_pairs = n_pairs;
  P->env_total = env_base; P->n_total = row_base;
  P->grid_pblk = P->n_pblk; P->grid_bp = P->n_bp; P->pt_launch = P->Ptot;
  P->grid_sg = (int)sgrp.size();
  BaDev& d = P->dev;
  LORB_TRY(dupload(P, P->hwin, &d.win));
  LORB_TRY(dupload(P, std::vector<int>{P->n_pblk, P->n_bp, (int)sgrp.size()}, &P->live)); d.live = P->live;
  LORB_TRY(dupload(P, sgrp.empty() ? std::vector<int4>{make_int4(0, 0, 0, 0)} : sgrp, &d.sgrp));
  LORB_TRY(dupload(P, pblk, &d.pblk));
  LORB_TRY(dupload(P, obs_pt, &d.obs_pt));
  LORB_TRY(dupload(P, bps, &d.bp));
  LORB_TRY(dupload(P, pt_obs_off, &d.pt_obs_off));
  LORB_TRY(dupload(P, obs_cam, &d.obs_cam));
  LORB_TRY(dupload(P, obs_fix, &d.obs_fix));
  LORB_TRY(dupload(P, obs_uv, &d.obs_uv));
  LORB_TRY(dupload(P, fixed, &d.fixed_pose));
  LORB_TRY(dupload(P, xpose, &d.x_init_pose));
  LORB_TRY(dupload(P, xpt, &d.x_init_pt));
  LORB_TRY(dupload(P, xpose, &d.x_pose[0]));
  LORB_TRY(dupload(P, xpose, &d.x_pose[1]));
  LORB_TRY(dupload(P, xpt, &d.x_pt[0]));
  LORB_TRY(dupload(P, xpt, &d.x_pt[1]));
  const size_t C = P->Ctot, Pn = P->Ptot;
  LORB_TRY(dalloc(P, C * 6, &d.scale_pose)); LORB_TRY(dalloc(P, Pn * 3, &d.scale_pt));
  LORB_TRY(dalloc(P, Pn * 3, &d.etb)); LORB_TRY(dalloc(P, Pn * 6, &d.pinv));
  LORB_TRY(dupload(P, cam_active, &d.cam_active));
  // the solve block is env | rhs | wfail (exchange 2 of a sharded plan: all of it)
  double *sol, *solp;
  LORB_TRY(alloc_exchange(P, C, (size_t)nw, (size_t)P->env_total + P->n_total + nw, &sol, &solp));
  d.env = sol; d.rhs = sol + P->env_total; d.wfail = sol + P->env_total + P->n_total;
  d.env_part = solp; d.rhs_part = solp + P->env_total; d.wfail_part = solp + P->env_total + P->n_total;
  LORB_TRY(dalloc(P, 2 * (size_t)P->Ctot, &d.rot_lin)); d.rot_stride = P->Ctot;
  LORB_TRY(dalloc(P, (size_t)P->Ctot, &d.rot_cand));
  LORB_TRY(dalloc(P, (size_t)std::max(P->NF, 1), &d.rot_fix));
  LORB_TRY(dalloc(P, (size_t)std::max(P->NF, 1), &d.rotv_fix));
  if (P->env_total) LORB_HIP(ctx, hipMemsetAsync(d.env, 0, sizeof(double) * P->env_total, ctx->stream));
  LORB_TRY(dalloc(P, (size_t)P->n_total, &d.ycam)); LORB_TRY(dalloc(P, (size_t)P->n_pblk * 8, &d.part));
  LORB_TRY(dalloc(P, dbg_words((size_t)nw, (size_t)std::max(P->n_pblk, nw)), &d.dbg));
  LORB_TRY(dalloc(P, ((size_t)P->n_total / 16 + nw + 1) * 1024, &d.kco));
  LORB_TRY(dalloc(P, (size_t)nw, &P->d_state)); d.st = P->d_state;
  LORB_TRY(dalloc(P, (size_t)nw, &d.st2)); LORB_TRY(dalloc(P, (size_t)nw, &d.ls_fail));
  LORB_TRY(dalloc(P, (size_t)nw * LORB_LM_TRACE_CAP, &d.trace));
  LORB_TRY(dalloc(P, (size_t)std::max(part_total, 1ll), &d.gpart));
  LORB_TRY(dalloc(P, (size_t)std::max(P->grid_sg, 1), &d.gspan));
  LORB_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return LORB_OK;
}

// ==========================================================================================
// Device-resident plan construction: the plan of ONE window built from
// observation arrays that already live in HBM (the LocalMapping step appends the new keyframe's
// matches on the device).  The host keeps only the camera-level decisions: one small readback
// (observation / point counts, per-camera counts and the C x C covisibility counts) per build, then
// the camera order (RCM), the (camera, camera) block list, band and kernel choice.  Everything
// per observation, per point and per pair is built by kernels:
//   k_db_keys    validity of the observation slots, per-point counts, camera x point bitsets
//                (a camera seen twice by one point is the bit already set)
//   k_db_scan1   point offsets (one workgroup: exclusive scan, total, largest count)
//   k_db_scatter counting sort by point: slot order within a point restored by k_db_segsort
//                (stable: the caller's order within a point, as a stable radix sort gives it)
//   k_db_cov     covisibility counts of camera pairs = popcount(bits_a & bits_b), per-camera counts
//   k_db_gather  point-sorted observation records (RCM camera labels), initial values (float ->
//                double, camera relabelling), point groups of <= kGB observations (weights k + 1,
//                fixed-size bins), and the zeros the next build starts from
// ==========================================================================================

// (the build scratch pt_cnt | hdr | cov | cam_cnt | bits and the words of hdr: see lorb_ba_devbuild)
__global__ __launch_bounds__(256) void k_db_keys(lorb_ba_window_dev w, int C, int F, int Wd,
                                                 int* __restrict__ pt_cnt, int* __restrict__ hdr,
                                                 unsigned long long* __restrict__ bits) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  const int n_obs_in = *w.d_n_obs, n_pt_in = *w.d_n_points;
  // live counts beyond the capacities are an error (flag 8); clamped, so nothing is touched past
  // the plan's allocations
  const int n_obs = min(n_obs_in, w.max_obs), n_pt = min(n_pt_in, w.max_points);
  if (k == 0) {
    hdr[3] = n_pt;
    if (n_obs_in > w.max_obs || n_pt_in > w.max_points || n_obs_in < 0 || n_pt_in < 0) atomicOr(&hdr[2], 8);
  }
  if (k >= n_obs) return;
  const int q = w.d_obs_point[k], f = w.d_obs_frame[k];
  if (f >= -F && f < C) {
    if (q < 0 || q >= n_pt) {
      atomicOr(&hdr[2], 1);
    } else {
      atomicAdd(&pt_cnt[q], 1);
      if (f >= 0) {
        const unsigned long long m = 1ull << (q & 63);
        if (atomicOr(&bits[(size_t)f * Wd + (q >> 6)], m) & m) atomicOr(&hdr[2], 4);
      }
    }
  } else if (f >= C) {
    atomicOr(&hdr[2], 2);
  }
}

// The build's first phase when the observation slots are already sorted by point (the LocalMapping
// map keeps them so; the drop-in's windows are gathered point by point): no counting sort.  One
// thread per slot i <= n_obs: validity, the camera x point bits (a bit already set: a point seen
// twice by one camera); the point offsets from the run boundaries (slot i is the first slot of the
// points (op[i - 1], op[i]], so points without observations get the next point's, and slot n_obs
// closes the points after the last one); the run length of the point starting at i (its largest
// over points).  A slot out of order or unused (frame < -n_fixed) sets flag 16: the host then runs
// the general phase instead.
// The camera x point bits of a workgroup's slots (consecutive points: a few 64-point words) are
// OR-ed in LDS and flushed with one non-returning atomic per (camera, word); a point seen twice by
// one camera is found by the thread that starts the point's run, among the run's frames (the run
// ends at the next run start of the wave's ballot, or by a scan for the wave's last run).  The
// largest run and the error bits are reduced per workgroup before their one atomic each.
// FUSE (C * C ints fit the LDS): the covisibility counts come from the runs too -- the run's start
// thread adds each camera pair of its point (lower triangle: row = the larger camera; the host
// mirrors it after the readback) and each camera's count into LDS tables, flushed with one atomic
// per non-zero entry -- so k_db_cov does not run; and the workgroup's
// histogram of optimised observations by input camera goes to hist[f * NB + block] (NB = 256-slot
// blocks of the live slots, the blocks k_db_gather<true> places), so the placement needs no
// histogram pass of its own.
constexpr int kDbWords = 4;  // 64-point words per workgroup held in LDS (more: global atomics)
constexpr int kDbFuseLds = 64 * 1024;  // LDS bytes the FUSE tables may take
template <bool FUSE>
__global__ __launch_bounds__(256) void k_db_sorted(lorb_ba_window_dev w, int C, int F, int Wd, int* __restrict__ pt_off,
                                                   int* __restrict__ hdr, unsigned long long* __restrict__ bits,
                                                   int* __restrict__ cov, int* __restrict__ cam_cnt) {
  extern __shared__ unsigned long long s_bits[];  // C * kDbWords; FUSE: then cov C * C | cam C (ints)
  int* s_cov = reinterpret_cast<int*>(s_bits + C * kDbWords);
  int* s_cam = s_cov + C * C;
  __shared__ int s_cnt, s_err;
  const int t = threadIdx.x, lane = t & 63;
  const int i = blockIdx.x * 256 + t;
  const int n_obs_in = *w.d_n_obs, n_pt_in = *w.d_n_points;
  const int n_obs = max(min(n_obs_in, w.max_obs), 0), n_pt = max(min(n_pt_in, w.max_points), 0);
  const int* __restrict__ op = w.d_obs_point;
  const int* __restrict__ of = w.d_obs_frame;
  for (int k = t; k < C * kDbWords; k += 256) s_bits[k] = 0ull;
  if (FUSE)
    for (int k = t; k < C * C + C; k += 256) s_cov[k] = 0;
  if (t == 0) { s_cnt = 0; s_err = 0; }
  const int i0 = blockIdx.x * 256;
  const int w0 = i0 < n_obs ? max(op[i0], 0) >> 6 : 0;  // the workgroup's first word
  int err = 0, cnt = 0;
  if (i == 0) {
    hdr[3] = n_pt;
    hdr[0] = n_obs;
    if (n_obs_in > w.max_obs || n_pt_in > w.max_points || n_obs_in < 0 || n_pt_in < 0) err |= 8;
  }
  const int prev = (i > 0 && i <= n_obs) ? op[i - 1] : -1;
  const int q = i < n_obs ? op[i] : n_pt;
  const int f = i < n_obs ? of[i] : -1;
  const bool bound = i <= n_obs && (i == n_obs || prev != q);  // a run starts (or the slots end) here
  const unsigned long long bal = __ballot(bound);
  __syncthreads();
  if (i < n_obs) {
    if (f < -F) err |= 16;
    else if (f >= C) err |= 2;
    else if (q < 0 || q >= n_pt) err |= 1;
    else if (f >= 0) {
      const unsigned long long m = 1ull << (q & 63);
      const int wl = (q >> 6) - w0;
      if (wl >= 0 && wl < kDbWords) atomicOr(&s_bits[f * kDbWords + wl], m);
      else __hip_atomic_fetch_or(&bits[(size_t)f * Wd + (q >> 6)], m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if (i <= n_obs) {
    if (prev > q) err |= 16;
    else if (prev != q) {
      const int p1 = min(q, n_pt);
      for (int p = max(prev + 1, 0); p <= p1; ++p) pt_off[p] = i;
      if (i < n_obs) {
        // run end: the next boundary of this wave, else scanned past the wave
        const unsigned long long above = lane < 63 ? bal & (~0ull << (lane + 1)) : 0ull;
        int e;
        if (above) {
          e = i - lane + __builtin_ctzll(above);
        } else {  // the slots past the wave in batches of 8 (one round trip per batch, not per slot)
          e = i - lane + 64;
          for (bool more = true; more;) {
            bool eq[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) eq[u] = e + u < n_obs && op[e + u] == q;
            int run = 0;
#pragma unroll
            for (int u = 7; u >= 0; --u) run = eq[u] ? run + 1 : 0;  // leading matches
            e += run;
            more = run == 8;
          }
          e = min(max(e, i + 1), n_obs);
        }
        cnt = e - i;
        // duplicate cameras within the run (optimised cameras only, as the bitset flags them)
        constexpr int kR = 16;
        int fr[kR];
#pragma unroll
        for (int k = 0; k < kR; ++k) fr[k] = k < cnt ? of[i + k] : -1 - k;
#pragma unroll
        for (int a = 1; a < kR; ++a)
#pragma unroll
          for (int b = 0; b < a; ++b)
            if (fr[a] >= 0 && fr[a] == fr[b]) err |= 4;
        for (int a = kR; a < cnt; ++a) {  // long runs: the rest against everything before it
          const int fa = of[i + a];
          if (fa < 0) continue;
          for (int b = 0; b < a; ++b)
            if (of[i + b] == fa) err |= 4;
        }
        if (FUSE && q >= 0 && q < n_pt) {  // the point's camera pairs and camera counts
#pragma unroll
          for (int a = 0; a < kR; ++a) {
            if (fr[a] < 0 || fr[a] >= C) continue;
            atomicAdd(&s_cam[fr[a]], 1);
#pragma unroll
            for (int b = 0; b < a; ++b)
              if (fr[b] >= 0 && fr[b] < C && fr[b] != fr[a])
                atomicAdd(&s_cov[max(fr[a], fr[b]) * C + min(fr[a], fr[b])], 1);
          }
          for (int a = kR; a < cnt; ++a) {
            const int fa = of[i + a];
            if (fa < 0 || fa >= C) continue;
            atomicAdd(&s_cam[fa], 1);
            for (int b = 0; b < a; ++b) {
              const int fb = of[i + b];
              if (fb >= 0 && fb < C && fb != fa) atomicAdd(&s_cov[max(fa, fb) * C + min(fa, fb)], 1);
            }
          }
        }
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt = max(cnt, __shfl_xor(cnt, o, 64));
  if (lane == 0 && cnt) atomicMax(&s_cnt, cnt);
  if (err) atomicOr(&s_err, err);
  __syncthreads();
  for (int k = t; k < C * kDbWords; k += 256) {
    const unsigned long long v = s_bits[k];
    const int wd = w0 + k % kDbWords;
    if (v && wd < Wd)
      __hip_atomic_fetch_or(&bits[(size_t)(k / kDbWords) * Wd + wd], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (FUSE) {
    for (int k = t; k < C * C + C; k += 256) {
      const int v = s_cov[k];  // (cam_cnt follows cov in LDS and in the scratch)
      if (v) __hip_atomic_fetch_add(k < C * C ? &cov[k] : &cam_cnt[k - C * C], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if (t == 0) {
    if (s_cnt > __hip_atomic_load(&hdr[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&hdr[1], s_cnt);
    if (s_err) atomicOr(&hdr[2], s_err);
  }
}

// One workgroup: out[0 .. n) = exclusive prefix sums of in[0 .. n) (n_dev: n = *n_dev + 1, the
// live points and one past them).  hdr (optional): hdr[0] = total, hdr[1] = max(in).
__global__ __launch_bounds__(1024) void k_db_scan1(const int* __restrict__ in, int* __restrict__ out, int n,
                                                   const int* __restrict__ n_dev, int* __restrict__ hdr) {
  __shared__ int wsum[16];
  __shared__ int s_tile[lorb::kScanTileLds];
  if (n_dev) n = min(n, *n_dev + 1);
  int mx = 0;
  const int tot = lorb::wg_excl_scan(in, out, n, s_tile, wsum, &mx);
  if (hdr) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o, 64));
    if ((threadIdx.x & 63) == 0 && mx) atomicMax(&hdr[1], mx);
    if (threadIdx.x == 0) hdr[0] = tot;
  }
}

// counting sort by point: slot k goes to the end of its point's free range (the counts run down
// to zero, which leaves pt_cnt cleared); k_db_segsort restores the slot order within a point
__global__ __launch_bounds__(256) void k_db_scatter(lorb_ba_window_dev w, int C, int F,
                                                    const int* __restrict__ pt_off, int* __restrict__ pt_cnt,
                                                    int* __restrict__ val) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  const int n_obs = min(*w.d_n_obs, w.max_obs), n_pt = min(*w.d_n_points, w.max_points);
  if (k >= n_obs) return;
  const int q = w.d_obs_point[k], f = w.d_obs_frame[k];
  if (f < -F || f >= C || q < 0 || q >= n_pt) return;
  val[pt_off[q] + atomicSub(&pt_cnt[q], 1) - 1] = k;
}

// one thread per point: its slots ascending.  Points have a few observations (up to kGB - 1):
// up to 16 sort in registers (odd-even transposition network), longer ones by insertion in place.
__global__ __launch_bounds__(256) void k_db_segsort(lorb_ba_window_dev w, const int* __restrict__ pt_off,
                                                    int* __restrict__ val, int* __restrict__ key) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= min(*w.d_n_points, w.max_points)) return;
  const int a0 = pt_off[p], a1 = pt_off[p + 1], m = a1 - a0;
  if (m <= 16) {
    int v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = i < m ? val[a0 + i] : 0x7fffffff;
#pragma unroll
    for (int r = 0; r < 16; ++r)
#pragma unroll
      for (int i = r & 1; i + 1 < 16; i += 2) {
        const int lo = min(v[i], v[i + 1]), hi = max(v[i], v[i + 1]);
        v[i] = lo; v[i + 1] = hi;
      }
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (i < m) { val[a0 + i] = v[i]; key[a0 + i] = p; }
  } else {
    for (int i = a0 + 1; i < a1; ++i) {
      const int x = val[i];
      int j = i - 1;
      while (j >= a0 && val[j] > x) { val[j + 1] = val[j]; --j; }
      val[j + 1] = x;
    }
    for (int i = a0; i < a1; ++i) key[i] = p;
  }
}

// one wavefront per camera pair (a <= b): covisibility = popcount of the AND of their point bitsets
__global__ __launch_bounds__(256) void k_db_cov(int C, int Wd, const unsigned long long* __restrict__ bits,
                                                int* __restrict__ cov, int* __restrict__ cam_cnt) {
  const int pr = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (pr >= C * (C + 1) / 2) return;
  int a = 0, r = pr;  // pr -> (a, b), a <= b, row a holds C - a pairs
  while (r >= C - a) { r -= C - a; ++a; }
  const int b = a + r;
  const unsigned long long* x = bits + (size_t)a * Wd;
  const unsigned long long* y = bits + (size_t)b * Wd;
  int c = 0;
  for (int i = lane; i < Wd; i += 64) c += __popcll(x[i] & y[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if (lane == 0) {
    if (a == b) {
      cam_cnt[a] = c;
      cov[a * C + a] = 0;
    } else {
      cov[a * C + b] = c;
      cov[b * C + a] = c;
    }
  }
}

// The work of a build that only needs the pre-readback results and the upload, in one launch:
//  * point-sorted structure arrays; per 256-observation block (blocks < NB) the plan-camera
//    histogram (camera-major hist[c * NB + block], fixed-camera observations not counted);
//  * initial values (float -> double, camera relabelling) and camera activity (k_db_init);
//  * point groups: group g = points [start(g), start(g + 1)), start(g) = the first point p with
//    off[p] + p >= g S (weights k_p + 1, so a group holds <= kGB observations and points; trailing
//    groups can be empty);
//  * zeros: this rank's band, and the build scratch the next build accumulates into (camera x point
//    bitsets, header max / error words, cov / cam_cnt; pt_cnt is left zero by k_db_scatter), so the
//    next build needs no clearing fill.
struct DbFused {
  int C, F, P, G, S, env_n, bits_n;
  int sorted;        // the slots were sorted by point (k_db_sorted): slot e is sorted position e
  unsigned long long* bits;
  int* hdr;
  int* cov;          // cov | cam_cnt (C * C + C ints): zeroed for the next build's k_db_sorted<true>
  int cov_n;
  // the upload is not copied before the launch -- the workgroups copy it from the mapped pinned
  // staging (src -> dst, words), and read perm / gcam from `cams` (kernel arguments), not from the copy
  const int* up_src;
  int* up_dst;
  int up_words;
  int sgf = 1, nsg = 0;  // partial runs: groups per run, runs
  int4* sgrp = nullptr;
};
struct DbCams {  // kernel arguments: device plans hold <= kPmSpan cameras
  int perm[kPmSpan], gcam[kPmSpan];
};
// Point groups: group g = points [start(g), start(g + 1)), start(g) = the smallest p with
// off[p] + p >= g S (P if none), found by one wavefront, 32-ary: each half-wave probes 32 points spread over its
// range per step (one memory round trip) and keeps the gap where the predicate turns true, so a
// 10 k-point window takes 3 round trips instead of 14 dependent loads.  Lanes 0-31 find the start
// of bound b0, lanes 32-63 that of b1.
__device__ __forceinline__ void group_bounds(const int* __restrict__ off, int P, long long b0, long long b1, int lane,
                                             int& s0, int& s1) {
  const int half = lane >> 5, j = lane & 31;
  const long long bound = half ? b1 : b0;
  int lo = 0, hi = P;  // the answer is in [lo, hi] (hi = P: none below P)
  while (__ballot(hi > lo)) {
    const int n = hi - lo;
    bool pr = false;
    if (n > 0) {
      const int q = lo + (int)(((long long)n * (j + 1)) / 33);  // < hi
      pr = (long long)off[q] + q >= bound;
    }
    const unsigned long long bal = __ballot(pr);
    const unsigned msk = half ? (unsigned)(bal >> 32) : (unsigned)bal;
    if (n > 0) {
      if (msk) {
        const int f = __builtin_ctz(msk);
        hi = lo + (int)(((long long)n * (f + 1)) / 33);
        if (f > 0) lo = lo + (int)(((long long)n * f) / 33) + 1;
      } else {
        lo = lo + (int)(((long long)n * 32) / 33) + 1;
      }
    }
  }
  s0 = __shfl(lo, 0, 64);
  s1 = __shfl(lo, 32, 64);
}
// The speculative build (dev_spec_issue): the host has not seen phase 1's readback yet and assumes the
// last build's adjacency pattern, hence its camera order, (ch, cl) block list, band and groups per
// partial run.  One workgroup, queued behind the readback copy, takes the counts from the scratch
// where phase 1 left them, checks that a plan built on the assumption stays inside the buffers as
// allocated, and writes the count-dependent words of the upload block (the rest of it is the last
// build's): BaWin's n_points / n_obs / n_obs_all / n_pblk / n_sg, live[], every block's pair count and
// offset, the cameras' activity.  out[0] is the validity word: no error or out-of-order bit, the counts
// within the capacities, every point within a point group, the point groups, their partials and the
// partial-run factor as allocated / assumed, and the adjacency pattern of cov / cam_cnt equal to the
// assumed one (cov holds the lower triangle: k_db_sorted<true>).  When it is 0 the plan left behind is
// empty -- no points, observations, groups, blocks or runs -- so k_ba_init marks the window done and
// every kernel of the LM graph exits: nothing is indexed with an unchecked count.  The word protects
// the speculative solve only; the host decides hit or miss from the readback (dev_spec_verify).
struct DbSpec {
  int C, P_cap, K_cap, pblk_cap, nbp, sf, sg_force, part_stride;  // sg_force: LORB_SG_F (0: sg_factor's rule)
  long long gpart_cap;
  const int* hdr; const int* cov; const int* cam_cnt;
  const unsigned char* adj;  // the assumed pattern, C x C
  BaWin* win; int* live; BlockPair* bp; int* cam_active;
  int* out;  // [0] valid, [1] K, [2] points, [3] point groups, [4] S (group size bound), [5] partial runs
};
__global__ __launch_bounds__(1024) void k_db_spec(DbSpec s, DbCams cams) {
  __shared__ int s_inv[kPmSpan];
  __shared__ int s_sum[1024];
  __shared__ int s_bad;
  const int t = threadIdx.x, C = s.C;
  if (t == 0) s_bad = 0;
  if (t < C) s_inv[cams.perm[t]] = t;
  __syncthreads();
  int K = s.hdr[0], Pn = s.hdr[3];
  const int maxk = s.hdr[1], err = s.hdr[2];
  bool ok = err == 0 && K >= 0 && K <= s.K_cap && Pn >= 0 && Pn <= s.P_cap && maxk >= 0 && maxk <= kGB - 1;
  int S = 1, G = 0, NSG = 0;
  if (ok) {  // db_layout's point groups and partial runs
    S = kGB - maxk;
    G = Pn > 0 ? (int)(((long long)K + Pn - 1) / S) + 1 : 0;
    const int SF = s.sg_force ? (G > 1 ? s.sg_force : 1) : (G > 512 ? (G + 479) / 480 : 1);
    NSG = G > 0 ? (G + SF - 1) / SF : 0;
    ok = G <= s.pblk_cap && SF == s.sf && (long long)NSG * s.part_stride <= s.gpart_cap;
  }
  bool bad = false;
  for (int k = t; k < C * C; k += 1024) {
    const int i = k / C, j = k - i * C;
    if (j <= i) bad |= ((i == j ? s.cam_cnt[i] : s.cov[k]) > 0) != (s.adj[k] != 0);
  }
  if (bad) s_bad = 1;
  __syncthreads();
  ok = ok && !s_bad;
  if (!ok) { K = 0; Pn = 0; G = 0; NSG = 0; S = 1; }
  if (t == 0) {
    s.out[0] = ok; s.out[1] = K; s.out[2] = Pn; s.out[3] = G; s.out[4] = S; s.out[5] = NSG;
    s.win->n_points = Pn; s.win->n_obs = K; s.win->n_obs_all = K; s.win->n_pblk = G; s.win->n_sg = NSG;
    s.live[0] = G; s.live[1] = ok ? s.nbp : 0; s.live[2] = NSG;
  }
  if (!ok) return;
  if (t < C) s.cam_active[cams.perm[t]] = s.cam_cnt[t] > 0;
  // every block's pairs (db_blocks) and their running offset: thread t takes `per` consecutive blocks
  const int per = (s.nbp + 1023) / 1024, b0 = min(t * per, s.nbp), b1 = min(b0 + per, s.nbp);
  int sum = 0;
  for (int k = b0; k < b1; ++k) {
    const int a = s_inv[s.bp[k].ch], b = s_inv[s.bp[k].cl];
    sum += a == b ? s.cam_cnt[a] : s.cov[max(a, b) * C + min(a, b)];
  }
  s_sum[t] = sum;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {  // inclusive scan of the threads' sums
    const int v = t >= o ? s_sum[t - o] : 0;
    __syncthreads();
    s_sum[t] += v;
    __syncthreads();
  }
  int off = s_sum[t] - sum;
  for (int k = b0; k < b1; ++k) {
    const int a = s_inv[s.bp[k].ch], b = s_inv[s.bp[k].cl];
    const int cnt = a == b ? s.cam_cnt[a] : s.cov[max(a, b) * C + min(a, b)];
    s.bp[k].off = off; s.bp[k].cnt = cnt;
    off += cnt;
  }
}

// SPEC: the speculative build's gather, behind k_db_spec: the counts come from `spec` (DbSpec::out,
// zeros when the assumption failed), nothing is uploaded (the upload block holds the last build's
// structure and k_db_spec's words) and the cameras' activity is k_db_spec's.  Every loop is
// grid-stride, so the launch grid (predicted from the last counts) only bounds the parallelism.
template <bool SPEC>
__global__ __launch_bounds__(256) void k_db_gather(lorb_ba_window_dev w, BaDev d, int K, const int* __restrict__ key,
                                                   const int* __restrict__ val, DbFused f, DbCams cams,
                                                   const int* __restrict__ spec) {
  const int gt = blockIdx.x * 256 + threadIdx.x, gs = gridDim.x * 256;
  if (SPEC) { K = spec[1]; f.P = spec[2]; f.G = spec[3]; f.S = spec[4]; f.nsg = spec[5]; }
  // the upload, from the mapped staging (PCIe reads, no copy launch before this kernel)
  for (int i = gt; i < f.up_words; i += gs) f.up_dst[i] = f.up_src[i];
  const int* __restrict__ perm = cams.perm;
  const int* __restrict__ gcam = cams.gcam;
  {  // initial values and camera activity
    const int m = max(max(6 * f.C, 6 * f.F), 3 * f.P);
    for (int i = gt; i < m; i += gs) {
      if (i < 6 * f.C) {
        const int c = i / 6, q = i - 6 * c;
        d.x_init_pose[6 * perm[c] + q] = (double)w.d_pose_init[i];
        if (!SPEC && q == 0) const_cast<int*>(d.cam_active)[perm[c]] = gcam[c] > 0;
      }
      if (i < 6 * f.F) const_cast<double*>(d.fixed_pose)[i] = (double)w.d_fixed_pose[i];
      if (i < 3 * f.P) d.x_init_pt[i] = (double)w.d_point_init[i];
    }
  }
  for (int g = gt >> 6; g < f.G; g += gs >> 6) {  // point groups, one wavefront each
    int s0, s1;
    group_bounds(d.pt_obs_off, f.P, (long long)g * f.S, (long long)(g + 1) * f.S, threadIdx.x & 63, s0, s1);
    if ((threadIdx.x & 63) == 0) {
      PBlk b;
      b.win = 0; b.p0 = s0; b.cnt = s1 - s0; b.o0 = d.pt_obs_off[s0]; b.no = d.pt_obs_off[s1] - d.pt_obs_off[s0];
      const_cast<PBlk*>(d.pblk)[g] = b;
    }
  }
  for (int i = gt; i < f.nsg; i += gs) f.sgrp[i] = make_int4(0, i * f.sgf, min(f.sgf, f.G - i * f.sgf), 0);
  for (int i = gt; i < f.env_n; i += gs) d.env_part[i] = 0.0;
  for (int i = gt; i < f.bits_n; i += gs) f.bits[i] = 0ull;
  for (int i = gt; i < f.cov_n; i += gs) f.cov[i] = 0;
  if (gt == 0) { f.hdr[1] = 0; f.hdr[2] = 0; }
  // the point-sorted observation records
  for (int e = gt; e < K; e += gs) {
    const int k = f.sorted ? e : val[e];
    const int fr = w.d_obs_frame[k];
    const_cast<int*>(d.obs_pt)[e] = f.sorted ? w.d_obs_point[e] : key[e];
    const_cast<int*>(d.obs_cam)[e] = fr >= 0 ? perm[fr] : -1;
    const_cast<int*>(d.obs_fix)[e] = fr >= 0 ? -1 : -1 - fr;
    const_cast<double2*>(d.obs_uv)[e] = make_double2(w.d_obs_uv[2 * k], w.d_obs_uv[2 * k + 1]);
  }
}

// plan camera order -> caller order, as float (Frame::SetPose / MapPoint::SetWorldPos write-back).
// ring (the LocalMapping map's keyframe ring of R slots): caller pose c goes to slot (t0 + c) mod R.
__global__ __launch_bounds__(256) void k_db_result(BaDev d, int C, int P, const int* __restrict__ perm,
                                                   float* __restrict__ pose_out, float* __restrict__ pt_out,
                                                   float* __restrict__ ring, int R, int t0) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int cur = d.st[0].cur;
  if ((pose_out || ring) && i < 6 * C) {
    const int c = i / 6, q = i - 6 * c;
    const float v = (float)d.x_pose[cur][6 * perm[c] + q];
    if (pose_out) pose_out[i] = v;
    if (ring) {
      const int r = (t0 + c) % R;
      ring[6 * (r < 0 ? r + R : r) + q] = v;
    }
  }
  if (pt_out)
    for (int k = i; k < 3 * P; k += gridDim.x * 256) pt_out[k] = (float)d.x_pt[cur][k];
}

// the same scattered into tables: pose c to row pose_row[c] of pose_tab, point i to row pt_row[i] of pt_tab (the
// keyframe store's write-back, lorb_kfba.hip); *done = 1
__global__ __launch_bounds__(256) void k_db_result_rows(BaDev d, int C, int P, const int* __restrict__ perm,
                                                        const int* __restrict__ pose_row, float* __restrict__ pose_tab,
                                                        const int* __restrict__ pt_row, float* __restrict__ pt_tab,
                                                        int* __restrict__ done) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int cur = d.st[0].cur;
  if (i < 6 * C) {
    const int c = i / 6, q = i - 6 * c;
    pose_tab[6 * (size_t)pose_row[c] + q] = (float)d.x_pose[cur][6 * perm[c] + q];
  }
  for (int k = i; k < 3 * P; k += gridDim.x * 256) {
    const int r = k / 3;
    pt_tab[3 * (size_t)pt_row[r] + (k - 3 * r)] = (float)d.x_pt[cur][k];
  }
  if (i == 0) *done = 1;
}

// the same in double (the Ceres parameter blocks after Solve) plus the summary, into one buffer for
// one D2H copy: [poses 6C (caller order) | points 3P | iterations, successful steps, termination,
// initial cost, final cost]
__global__ __launch_bounds__(256) void k_db_result64(BaDev d, int C, int P, const int* __restrict__ perm,
                                                     double* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const WinState& st = d.st[0];
  const int cur = st.cur;
  if (i < 6 * C) {
    const int c = i / 6, q = i - 6 * c;
    out[i] = d.x_pose[cur][6 * perm[c] + q];
  }
  for (int k = i; k < 3 * P; k += gridDim.x * 256) out[6 * C + k] = d.x_pt[cur][k];
  if (i == 0) {
    double* s = out + 6 * C + 3 * P;
    s[0] = st.iter; s[1] = st.n_success; s[2] = st.term; s[3] = st.initial_cost; s[4] = st.cost;
  }
}

template <typename T, typename Cap>
int grow(lorb_ba_plan* P, T** ptr, Cap* cap, size_t need) {
  if (*ptr && (size_t)*cap >= need) return LORB_OK;
  if (*ptr) LORB_TRY(dfree(P, *ptr));
  const size_t n = std::max<size_t>(need + need / 4, 16);
  LORB_TRY(dalloc(P, n, ptr));
  *cap = (Cap)n;
  P->cache.invalidate();  // kernel arguments changed
  P->gen++;
  return LORB_OK;
}

// capacity allocations (once per plan)
int dev_alloc(lorb_ctx* ctx, const lorb_ba_window_dev* w, lorb_ba_plan* P) {
  lorb_ba_devbuild& b = *P->devb;
  b.K_cap = w->max_obs; b.P_cap = w->max_points; b.C = w->n_poses; b.F = w->n_fixed;
  b.Wd = (std::max(b.P_cap, 1) + 63) / 64;
  const size_t K = (size_t)std::max(b.K_cap, 1), Pn = (size_t)std::max(b.P_cap, 1), C = (size_t)std::max(b.C, 1);
  BaDev& d = P->dev;
  if (b.C > kPmSpan)
    return lorb::set_error(ctx, LORB_E_UNSUPPORTED, "device-built plans hold windows of <= %d cameras (%d)", kPmSpan, b.C);
  LORB_TRY(dalloc(P, K, &b.key_out)); LORB_TRY(dalloc(P, K, &b.val_out));
  {
    const size_t ints = ((Pn + 1 + 8 + C * C + C) + 1) & ~(size_t)1;  // the u64 bitsets 8-byte aligned
    b.scr_bytes = sizeof(int) * ints + sizeof(unsigned long long) * C * (size_t)b.Wd;
    unsigned char* m;
    LORB_TRY(dalloc(P, b.scr_bytes, &m));
    b.scr = reinterpret_cast<int*>(m);
    b.pt_cnt = b.scr; b.hdr = b.pt_cnt + Pn + 1; b.cov = b.hdr + 8; b.cam_cnt = b.cov + C * C;
    b.bits = reinterpret_cast<unsigned long long*>(b.scr + ints);
  }
  LORB_TRY(dalloc(P, K, &d.obs_pt)); LORB_TRY(dalloc(P, K, &d.obs_cam)); LORB_TRY(dalloc(P, K, &d.obs_fix));
  LORB_TRY(dalloc(P, K, &d.obs_uv)); LORB_TRY(dalloc(P, C, &d.cam_active));
  LORB_TRY(dalloc(P, Pn + 1, &d.pt_obs_off)); LORB_TRY(dalloc(P, (size_t)std::max(b.F, 1) * 6, &d.fixed_pose));
  LORB_TRY(dalloc(P, C * 6, &d.x_init_pose)); LORB_TRY(dalloc(P, Pn * 3, &d.x_init_pt));
  LORB_TRY(dalloc(P, C * 6, &d.x_pose[0])); LORB_TRY(dalloc(P, C * 6, &d.x_pose[1]));
  LORB_TRY(dalloc(P, Pn * 3, &d.x_pt[0])); LORB_TRY(dalloc(P, Pn * 3, &d.x_pt[1]));
  LORB_TRY(dalloc(P, C * 6, &d.scale_pose)); LORB_TRY(dalloc(P, Pn * 3, &d.scale_pt));
  LORB_TRY(dalloc(P, Pn * 3, &d.etb)); LORB_TRY(dalloc(P, Pn * 6, &d.pinv));
  // the solve block is rhs (n) | wfail (1) | pad | env (up to the dense n x n): rhs and wfail at fixed
  // places, so the captured solve survives a rebuild that changes the band, and a sharded plan's
  // exchange 2 is one contiguous all-reduce of x2_off + env_total doubles
  const size_t n = 6 * C;
  P->x2_off = (n + 1 + 31) & ~(size_t)31;
  double *sol, *solp;
  LORB_TRY(alloc_exchange(P, C, 1, P->x2_off + n * n, &sol, &solp));
  d.rhs = sol; d.wfail = sol + n; d.env = sol + P->x2_off;
  d.rhs_part = solp; d.wfail_part = solp + n; d.env_part = solp + P->x2_off;
  LORB_TRY(dalloc(P, 2 * C, &d.rot_lin)); d.rot_stride = (int)C; LORB_TRY(dalloc(P, C, &d.rot_cand));
  LORB_TRY(dalloc(P, (size_t)std::max(b.F, 1), &d.rot_fix)); LORB_TRY(dalloc(P, (size_t)std::max(b.F, 1), &d.rotv_fix));
  LORB_TRY(dalloc(P, n, &d.ycam));
  LORB_TRY(dalloc(P, dbg_words(1, K + Pn + 1), &d.dbg));  // stamps: >= 8 per point group at any build
  LORB_TRY(dalloc(P, ((size_t)n / 16 + 2) * 1024, &d.kco));
  LORB_TRY(dalloc(P, (size_t)1, &P->d_state)); d.st = P->d_state;
  LORB_TRY(dalloc(P, (size_t)1, &d.st2)); LORB_TRY(dalloc(P, (size_t)1, &d.ls_fail));
  LORB_TRY(dalloc(P, (size_t)LORB_LM_TRACE_CAP, &d.trace));
  P->W = 1;
  P->hwin.assign(1, BaWin{});
  P->pt_launch = b.P_cap;
  return LORB_OK;
}

// (re)allocate the upload block for bp_need block pairs; repoints BaDev at it
int up_alloc(lorb_ba_plan* P, int bp_need) {
  lorb_ba_devbuild& b = *P->devb;
  if (b.up_dev && b.up_bp_cap >= bp_need) return LORB_OK;
  lorb_ctx* ctx = P->ctx;
  const int cap = std::max(bp_need + bp_need / 4, 16);
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t C = (size_t)std::max(b.C, 1);
  b.off_live = al(sizeof(BaWin));
  b.off_perm = b.off_live + 256;
  b.off_gcam = b.off_perm + al(4 * C);
  b.off_adj = b.off_gcam + al(4 * C);
  b.off_bp = b.off_adj + al(C * C);
  b.up_bytes = b.off_bp + sizeof(BlockPair) * (size_t)cap;
  b.spec_ok = false;  // the upload block moves: nothing of the last build is in the new one
  if (!b.spec_out) LORB_TRY(dalloc(P, (size_t)8, &b.spec_out));
  if (b.up_dev) {
    LORB_TRY(dfree(P, b.up_dev));
    (void)hipHostFree(b.up_host);
    b.up_host = nullptr;
  }
  LORB_TRY(dalloc(P, b.up_bytes, &b.up_dev));
  LORB_HIP(ctx, hipHostMalloc(reinterpret_cast<void**>(&b.up_host), b.up_bytes));
  LORB_HIP(ctx, hipHostGetDevicePointer((void**)&b.up_host_dev, b.up_host, 0));
  b.up_bp_cap = cap;
  BaDev& d = P->dev;
  d.win = reinterpret_cast<const BaWin*>(b.up_dev);
  d.live = reinterpret_cast<const int*>(b.up_dev + b.off_live);
  b.perm = reinterpret_cast<int*>(b.up_dev + b.off_perm);
  d.bp = reinterpret_cast<const BlockPair*>(b.up_dev + b.off_bp);
  P->grid_bp = cap;
  P->cache.invalidate();
  P->gen++;
  return LORB_OK;
}

// phase 1 of a build on the ctx stream: per-point counts, camera x point bitsets, point offsets,
// the counting sort by point when the slots are not sorted, covisibility counts; then the one
// readback (hdr | cov | cam_cnt are contiguous in the scratch: one copy) and an event behind it.
// The scratch is left clear by the previous build's k_db_gather; only a build that stopped before it
// (an error) leaves it dirty.
int db_phase1_issue(lorb_ctx* ctx, const lorb_ba_window_dev* w, lorb_ba_plan* P, bool sorted) {
  lorb_ba_devbuild& b = *P->devb;
  hipStream_t s = ctx->stream;
  BaDev& d = P->dev;
  const int C = b.C, F = b.F, Kc = w->max_obs;
  const size_t nrb = 8 + (size_t)C + (size_t)C * C;
  const int nb_obs = lorb::ceil_div(std::max(Kc, 1), 256), nb_pt = lorb::ceil_div(std::max(b.P_cap, 1), 256);
  if (b.pinned_n < nrb) {
    if (b.pinned) (void)hipHostFree(b.pinned);
    b.pinned = nullptr; b.pinned_n = 0;
    LORB_HIP(ctx, hipHostMalloc(reinterpret_cast<void**>(&b.pinned), sizeof(int) * nrb));
    b.pinned_n = nrb;
  }
  if (!b.rb_ev) LORB_HIP(ctx, hipEventCreateWithFlags(&b.rb_ev, hipEventDisableTiming));
  if (b.dirty) LORB_HIP(ctx, hipMemsetAsync(b.scr, 0, b.scr_bytes, s));
  b.dirty = true;
  const bool fuse = sorted && C > 0 && sizeof(int) * ((size_t)C * C + C) <= (size_t)kDbFuseLds;
  if (sorted) {
    const size_t lds = sizeof(unsigned long long) * kDbWords * std::max(C, 1) +
                       (fuse ? sizeof(int) * ((size_t)C * C + C) : 0);
    hipLaunchKernelGGL(fuse ? k_db_sorted<true> : k_db_sorted<false>, dim3(lorb::ceil_div(Kc + 1, 256)), dim3(256), lds, s,
                       *w, C, F, b.Wd, const_cast<int*>(d.pt_obs_off), b.hdr, b.bits, b.cov, b.cam_cnt);
  } else {
    hipLaunchKernelGGL(k_db_keys, dim3(nb_obs), dim3(256), 0, s, *w, C, F, b.Wd, b.pt_cnt, b.hdr, b.bits);
    hipLaunchKernelGGL(k_db_scan1, dim3(1), dim3(1024), 0, s, b.pt_cnt, const_cast<int*>(d.pt_obs_off), b.P_cap + 1,
                       w->d_n_points, b.hdr);
    if (Kc > 0) {
      hipLaunchKernelGGL(k_db_scatter, dim3(nb_obs), dim3(256), 0, s, *w, C, F, d.pt_obs_off, b.pt_cnt, b.val_out);
      hipLaunchKernelGGL(k_db_segsort, dim3(nb_pt), dim3(256), 0, s, *w, d.pt_obs_off, b.val_out, b.key_out);
    }
  }
  if (C > 0 && !fuse)
    hipLaunchKernelGGL(k_db_cov, dim3(lorb::ceil_div(C * (C + 1) / 2, 4)), dim3(256), 0, s, C, b.Wd, b.bits, b.cov,
                       b.cam_cnt);
  LORB_CHECK_LAUNCH(ctx);
  LORB_HIP(ctx, hipMemcpyAsync(b.pinned, b.hdr, sizeof(int) * nrb, hipMemcpyDeviceToHost, s));
  LORB_HIP(ctx, hipEventRecord(b.rb_ev, s));
  b.rb_sorted = sorted;
  b.rb_fuse = fuse;
  b.rb_pending = true;
  return LORB_OK;
}

// the readback of an issued phase 1 landed (polled); slots found out of order on the sorted path
// (or unused) rerun the general phase from a cleared scratch
int db_phase1_wait(lorb_ctx* ctx, const lorb_ba_window_dev* w, lorb_ba_plan* P) {
  lorb_ba_devbuild& b = *P->devb;
  for (;;) {
    b.rb_pending = false;
    LORB_HIP(ctx, lorb::spin_wait(b.rb_ev));
    if (!(b.rb_sorted && (b.pinned[2] & 16))) return LORB_OK;
    b.sorted_hint = false;
    LORB_TRY(db_phase1_issue(ctx, w, P, false));
  }
}

// the first half of a build: the shape check and phase 1 with its readback queued (no wait).  A
// rank-local failure of a sharded plan is kept for dev_build_finish (see there).
int dev_build_issue(lorb_ctx* ctx, const lorb_ba_window_dev* w, lorb_ba_plan* P, int* lerr_out) {
  lorb_ba_devbuild& b = *P->devb;
  const bool shape_ok = w->n_poses == b.C && w->n_fixed == b.F && w->max_obs <= b.K_cap && w->max_points <= b.P_cap;
  *lerr_out = shape_ok ? 0 : 32;
  if (!shape_ok && !P->comm)
    return lorb::set_error(ctx, LORB_E_INVALID, "window shape differs from the plan's (cameras %d/%d, fixed %d/%d)",
                           w->n_poses, b.C, w->n_fixed, b.F);
  if (!shape_ok) return LORB_OK;
  const int rc = db_phase1_issue(ctx, w, P, b.sorted_hint);
  if (rc != LORB_OK && P->comm) { *lerr_out |= 64; return LORB_OK; }
  return rc;
}

// LORB_HOST_PHASE=1 (diagnostics): the host phase of a build, from the readback landed to k_db_gather
// launched, and its six sections (mark(k) ends section k: 0 checks, 1 order, 2 blocks, 3 buffers,
// 4 staging, 5 launch, which ends the phase), summed in the plan and printed at its destruction
struct HostPhase {
  using Clock = std::chrono::steady_clock;
  lorb_ba_plan* P;
  const bool on;
  const Clock::time_point t0 = Clock::now();
  Clock::time_point last = t0;
  void mark(int k) {
    if (!on) return;
    const auto now = Clock::now();
    P->hp_sec[k] += std::chrono::duration<double, std::micro>(now - last).count();
    if (k == 5) { P->hp_us += std::chrono::duration<double, std::micro>(now - t0).count(); P->hp_n++; }
    last = now;
  }
};

// One build's host phase: what each step of dev_build_finish leaves for the later ones
struct DbBuild {
  int K, maxk, Pn, K_all;    // 1: this rank's valid observations, largest count per point, live points; all ranks' observations
  const int *cov, *cam_cnt;  //    this rank's C x C covisibility counts and observations per input camera
  const int *gcov, *gcam;    //    the same over all ranks (the camera-level structure; unsharded: cov, cam_cnt)
  std::vector<int> g_int;    //    sharded: holds gcov | gcam
  std::vector<BlockPair> bps;  // 3 (2, the camera order, is lorb_ba_devbuild::last_map): this rank's block list,
  int n_pairs = 0, bw = 0;     //    its pairs, the band
  int S, G, SF, NSG;           // 4: group size bound, point groups, groups per partial run, runs (k_db_gather fills
  long long part_total;        //    both), doubles of the partials
};

// Step 1 of dev_build_finish: lands the readback, all-reduces it when the plan is sharded, decodes
// the build's error bits.  Sharded plans are collective: a rank-local failure before the exchange
// (lerr: a shape that differs from the plan's, 32; a failed allocation or copy, 64, as is phase_rc)
// becomes an error bit of the all-reduce, so every rank reaches both all-reduces and returns the error.
int db_land(lorb_ctx* ctx, const lorb_ba_window_dev* w, lorb_ba_plan* P, int lerr, int phase_rc, DbBuild& r) {
  lorb_ba_devbuild& b = *P->devb;
  const bool shape_ok = !(lerr & 32), fuse = b.rb_fuse;
  const int C = b.C;
  const size_t nrb = 8 + (size_t)C + (size_t)C * C;
  if (phase_rc != LORB_OK) {
    if (!P->comm) return phase_rc;
    lerr |= 64;
  }
  // the readback landed by DMA: none of its lines are in the CPU's caches.  One sequential copy
  // (prefetched) into a reused host buffer, then the column-wise triangle fill and the scans of the
  // later steps run on cached data instead of one DRAM round trip per line touched out of order.
  b.h_copy.resize(nrb);
  if (lerr) std::fill(b.h_copy.begin(), b.h_copy.end(), 0);  // a failed rank contributes an empty structure
  else std::memcpy(b.h_copy.data(), b.pinned, sizeof(int) * nrb);
  int* H = b.h_copy.data();
  if (fuse)  // k_db_sorted<true> filled the lower triangle
    for (int i = 0; i < C; ++i)
      for (int j = i + 1; j < C; ++j) H[8 + (size_t)i * C + j] = H[8 + (size_t)j * C + i];
  r.K = r.K_all = H[0]; r.maxk = H[1]; r.Pn = H[3];
  r.cov = r.gcov = H + 8;
  r.cam_cnt = r.gcam = r.cov + (size_t)C * C;
  const int err = H[2], Pn = r.Pn;
  // sharded: the camera-level structure is global -- sum the ranks' covisibility and camera counts
  // (camera order, band and camera activity must agree on every rank) and their error flags (every
  // rank returns the same error, so none is left waiting in a later collective)
  int gerr = err, gmaxk = r.maxk;
  if (P->comm) {
    // [cov | cam_cnt (contiguous, m) | K | n_points out of range | error bits 0..6] summed; the largest
    // per-point count (the group size check) by a max
    const size_t m = (size_t)C * C + C;
    b.h_red.assign(m + 9, 0.0);
    for (size_t i = 0; i < m; ++i) b.h_red[i] = (double)r.cov[i];
    b.h_red[m] = r.K;
    b.h_red[m + 1] = (Pn < 0 || Pn > b.P_cap) ? 1.0 : 0.0;
    for (int q = 0; q < 7; ++q) b.h_red[m + 2 + q] = ((err | lerr) >> q) & 1;
    LORB_TRY(lorb::comm_allreduce_host(P->comm, b.h_red.data(), b.h_red.size(), LORB_OP_SUM));
    double mk = r.maxk;
    LORB_TRY(lorb::comm_allreduce_host(P->comm, &mk, 1, LORB_OP_MAX));
    r.g_int.resize(m);
    for (size_t i = 0; i < m; ++i) r.g_int[i] = (int)b.h_red[i];
    r.gcov = r.g_int.data();
    r.gcam = r.g_int.data() + (size_t)C * C;
    r.K_all = (int)b.h_red[m];
    gerr = b.h_red[m + 1] > 0.0 ? 16 : 0;
    for (int q = 0; q < 7; ++q) gerr |= b.h_red[m + 2 + q] > 0.0 ? 1 << q : 0;
    gmaxk = (int)mk;
  }
  if (gerr & 32)
    return lorb::set_error(ctx, LORB_E_INVALID, "window shape differs from the plan's on %s (cameras %d/%d, fixed %d/%d)",
                           shape_ok ? "another rank" : "this rank", w->n_poses, b.C, w->n_fixed, b.F);
  if (gerr & 64)
    return phase_rc != LORB_OK ? phase_rc
                               : lorb::set_error(ctx, LORB_E_DEVICE, "device plan build failed on another rank");
  // a count beyond capacity first: the slots read up to the capacity then hold no real observations
  if (gerr & 8) return lorb::set_error(ctx, LORB_E_INVALID, "live point / observation count outside [0, capacity] (%d / %d)",
                                       b.P_cap, b.K_cap);
  if (gerr & 1) return lorb::set_error(ctx, LORB_E_INVALID, "observation with a point index outside [0, n_points)");
  if (gerr & 2) return lorb::set_error(ctx, LORB_E_INVALID, "observation with a frame index >= n_poses");
  if (gerr & 4) return lorb::set_error(ctx, LORB_E_INVALID, "a point observed twice by one camera");
  if ((gerr & 16) || Pn < 0 || Pn > b.P_cap) return lorb::set_error(ctx, LORB_E_INVALID, "n_points %d outside [0, %d]", Pn, b.P_cap);
  if (kGB - gmaxk < 1)
    return lorb::set_error(ctx, LORB_E_UNSUPPORTED, "a point with %d observations (device plans hold <= %d)", gmaxk, kGB - 1);
  return LORB_OK;
}

// Step 2: the camera order (input camera -> plan camera), from the global structure.  It depends
// only on the adjacency pattern: compared in place against the last build's (no allocation on the
// step's host phase), recomputed when it changed.  Returns whether the pattern was the last build's.
bool db_camera_order(lorb_ba_devbuild& b, const DbBuild& r) {
  const int C = b.C;
  bool same_adj = b.last_adj.size() == (size_t)C * C;
  for (int i = 0; i < C && same_adj; ++i) {
    const int* row = r.gcov + (size_t)i * C;
    const char* last = b.last_adj.data() + (size_t)i * C;
    for (int j = 0; j < C; ++j)
      if (last[j] != (char)((i == j && r.gcam[i] > 0) || row[j] > 0)) { same_adj = false; break; }
  }
  if (!same_adj) {
    std::vector<char> adj((size_t)C * C, 0);
    for (int i = 0; i < C; ++i)
      for (int j = 0; j < C; ++j) adj[(size_t)i * C + j] = (i == j && r.gcam[i] > 0) || r.gcov[(size_t)i * C + j] > 0;
    b.last_map = camera_order(C, adj);
    b.last_adj.swap(adj);
  }
  return same_adj;
}

// Step 3: the (camera, camera) block list from this rank's observations, in the std::map order of
// the host builder ((ch, cl) ascending), and the band from the global structure
void db_blocks(const lorb_ba_devbuild& b, DbBuild& r) {
  const int C = b.C;
  std::vector<int> inv(C), fc(C);
  for (int c = 0; c < C; ++c) inv[b.last_map[c]] = c;
  for (int ch = 0; ch < C; ++ch) {
    fc[ch] = ch;
    for (int cl = 0; cl <= ch; ++cl) {
      const int cnt = ch == cl ? r.cam_cnt[inv[ch]] : r.cov[(size_t)inv[ch] * C + inv[cl]];
      if (ch != cl && r.gcov[(size_t)inv[ch] * C + inv[cl]] > 0) fc[ch] = std::min(fc[ch], cl);
      if (ch != cl && cnt == 0) continue;
      r.bps.push_back(BlockPair{0, ch, cl, r.n_pairs, cnt});
      r.n_pairs += cnt;
    }
  }
  r.bw = band_of(fc);
}

// Step 4: the point groups, the window's layout (BaWin) and the plan's counters
int db_layout(lorb_ctx* ctx, const lorb_ba_window_dev* w, lorb_ba_plan* P, DbBuild& r) {
  const int C = P->devb->C, n = 6 * C, K = r.K, Pn = r.Pn, bwid = r.bw;
  const int S = r.S = kGB - (r.maxk + 1) + 1;  // >= 1 (checked by db_land)
  const int G = r.G = Pn > 0 ? (K + Pn - 1) / S + 1 : 0;
  BaWin bw{};
  bw.pose_base = 0; bw.n_poses = C; bw.point_base = 0; bw.n_points = Pn; bw.pblk_base = 0; bw.n_pblk = G;
  bw.env_base = 0; bw.env_size = n * (bwid + 1); bw.n = n; bw.row_base = 0; bw.bw = bwid;
  bw.obs_base = 0; bw.n_obs = K; bw.n_obs_all = r.K_all;
  bw.fx = w->fx; bw.fy = w->fy; bw.cx = w->cx; bw.cy = w->cy;
  const int SF = r.SF = sg_factor(G), NSG = r.NSG = G > 0 ? (G + SF - 1) / SF : 0;
  bw.sg_base = 0; bw.n_sg = NSG;
  r.part_total = 0;
  pm_layout(bw, C, r.part_total);  // a group (or run) spans at most the window's C <= kPmSpan cameras
  LORB_TRY(part_budget_check(ctx, r.part_total));
  P->hwin[0] = bw;
  P->Ctot = C; P->Ptot = Pn; P->K = K; P->NF = P->devb->F; P->n_pblk = G; P->n_bp = (int)r.bps.size(); P->n_pairs = r.n_pairs;
  P->env_total = bw.env_size; P->n_total = n;
  P->max_env = bw.env_size + 2 * n; P->max_bw = bwid;
  P->min_bw = n > 0 ? bwid : (1 << 30);
  // the Cholesky's LDS is sized for a band of 48 (the widest k_ba_chol_w / _2s take) when that
  // fits, so that a narrower band after a rebuild keeps the captured solve
  const int n16 = (n + 15) & ~15;
  P->max_env_w = chol_lds_words(n16, bwid);
  if (bwid <= 48 && sizeof(double) * (size_t)chol_lds_words(n16, 48) <= (size_t)kLdsBudget)
    P->max_env_w = chol_lds_words(n16, 48);
  P->min_n16 = n16 > 0 ? n16 : (1 << 30);
  return LORB_OK;
}

// Step 5: the grow-only structure buffers (a reallocation re-captures the LM graph); the
// point-group kernels launch at capacity
int db_buffers(lorb_ba_plan* P, const DbBuild& r) {
  lorb_ba_devbuild& b = *P->devb;
  BaDev& d = P->dev;
  LORB_TRY(grow(P, &d.pblk, &b.pblk_cap, (size_t)std::max(r.G, 1)));
  LORB_TRY(grow(P, &d.part, &b.part_cap, (size_t)b.pblk_cap * 8));
  P->grid_pblk = b.pblk_cap;
  LORB_TRY(grow(P, &d.gpart, &b.gpart_cap, (size_t)std::max(r.part_total, 1ll)));  // the group partials
  LORB_TRY(grow(P, &d.gspan, &b.gspan_cap, (size_t)b.pblk_cap));
  LORB_TRY(grow(P, &d.sgrp, &b.sgrp_cap, (size_t)b.pblk_cap));
  P->has_super = r.SF > 1;
  P->grid_sg = b.pblk_cap;  // runs <= groups: launched at the groups' capacity, live[2] in use
  return up_alloc(P, (int)r.bps.size());
}

// Step 6: the build's one upload and the structure kernel.  The upload is staged in pinned memory
// (the next build writes the staging only after its own readback synchronised the stream); no copy
// launch: k_db_gather copies the staging over the bus and takes the camera tables as kernel
// arguments.  It also writes the zeros the next build starts from: the scratch is clean from here.
void db_stage_and_gather(lorb_ctx* ctx, const lorb_ba_window_dev* w, lorb_ba_plan* P, const DbBuild& r, HostPhase& hp) {
  lorb_ba_devbuild& b = *P->devb;
  const std::vector<int>& map = b.last_map;
  const std::vector<BlockPair>& bps = r.bps;
  const int C = b.C;
  unsigned char* h = b.up_host;
  memcpy(h, &P->hwin[0], sizeof(BaWin));
  const int live[3] = {r.G, (int)bps.size(), r.NSG};
  memcpy(h + b.off_live, live, sizeof(live));
  memcpy(h + b.off_perm, map.data(), sizeof(int) * C);
  memcpy(h + b.off_gcam, r.gcam, sizeof(int) * C);
  if (!b.last_adj.empty()) memcpy(h + b.off_adj, b.last_adj.data(), b.last_adj.size());  // (what a speculative build assumes)
  if (!bps.empty()) memcpy(h + b.off_bp, bps.data(), sizeof(BlockPair) * bps.size());
  const int up_words = (int)((b.off_bp + sizeof(BlockPair) * bps.size() + 3) / 4);
  hp.mark(4);
  // this rank's band starts from zeros (blocks it has no pairs of stay zero; sharded: the
  // all-reduce writes the global band every iteration)
  DbFused f{C, b.F, r.Pn, r.G, r.S, P->env_total, C * b.Wd, b.rb_sorted ? 1 : 0, b.bits, b.hdr, b.cov, C * C + C,
            reinterpret_cast<const int*>(b.up_host_dev), reinterpret_cast<int*>(b.up_dev), up_words};
  f.sgf = r.SF; f.nsg = r.NSG; f.sgrp = const_cast<int4*>(P->dev.sgrp);
  DbCams cams;
  for (int c = 0; c < C; ++c) { cams.perm[c] = map[c]; cams.gcam[c] = r.gcam[c]; }
  const int NB = lorb::ceil_div(r.K, 256);
  hipLaunchKernelGGL(k_db_gather<false>, dim3(std::max(NB, 1)), dim3(256), 0, ctx->stream, *w, P->dev, r.K, b.key_out,
                     b.val_out, f, cams, (const int*)nullptr);
  b.dirty = false;
  hp.mark(5);
}

// LORB_SPEC_SPOIL=1 (tests; read at every build): flips one entry of the kept adjacency pattern on
// the host, so the next speculative build's verification finds a changed pattern and falls back
void spec_spoil(lorb_ba_devbuild& b) {
  if (env_flag("LORB_SPEC_SPOIL") && b.last_adj.size() > 1) b.last_adj[1] ^= 1;
}

// A build may speculate when the plan is unsharded, its last build completed (and the upload block
// has not moved since), its slots take the sorted phase 1 and the context is not timing kernels;
// LORB_NO_SPEC=1 (read at every build) turns it off.
bool spec_allowed(const lorb_ctx* ctx, const lorb_ba_plan* P) {
  const lorb_ba_devbuild& b = *P->devb;
  return !P->comm && b.spec_ok && b.sorted_hint && b.C > 0 && !ctx->ktime && !env_flag("LORB_NO_SPEC");
}

// The speculative half of a build, behind an issued phase 1 (sorted and fused) and its readback copy,
// without waiting for it: k_db_spec, then the gather at a grid predicted from obs_hint (the caller's
// bound on the live observations).  The host's own plan fields stay the last build's until
// dev_spec_verify commits the new ones, so a solve enqueued in between makes its choices (fold_of,
// red_threads, graph_key) from the last build's values.
int dev_spec_issue(lorb_ctx* ctx, const lorb_ba_window_dev* w, lorb_ba_plan* P, int obs_hint) {
  lorb_ba_devbuild& b = *P->devb;
  const int C = b.C;
  DbCams cams;
  for (int c = 0; c < C; ++c) { cams.perm[c] = b.last_map[c]; cams.gcam[c] = 0; }
  const char* e = getenv("LORB_SG_F");
  const BaWin& hw = P->hwin[0];
  DbSpec s{C, w->max_points, w->max_obs, b.pblk_cap, (int)b.last_bps.size(), b.spec_sf, e && atoi(e) >= 1 ? atoi(e) : 0,
           hw.part_stride, (long long)b.gpart_cap, b.hdr, b.cov, b.cam_cnt, b.up_dev + b.off_adj,
           reinterpret_cast<BaWin*>(b.up_dev), reinterpret_cast<int*>(b.up_dev + b.off_live),
           reinterpret_cast<BlockPair*>(b.up_dev + b.off_bp), const_cast<int*>(P->dev.cam_active), b.spec_out};
  hipLaunchKernelGGL(k_db_spec, dim3(1), dim3(1024), 0, ctx->stream, s, cams);
  DbFused f{C, b.F, 0, 0, 1, P->env_total, C * b.Wd, 1, b.bits, b.hdr, b.cov, C * C + C, nullptr, nullptr, 0};
  f.sgf = b.spec_sf; f.nsg = 0; f.sgrp = const_cast<int4*>(P->dev.sgrp);
  const int NB = lorb::ceil_div(std::min(std::max(obs_hint, 1), std::max(w->max_obs, 1)), 256);
  hipLaunchKernelGGL(k_db_gather<true>, dim3(NB), dim3(256), 0, ctx->stream, *w, P->dev, 0, b.key_out, b.val_out, f, cams,
                     (const int*)b.spec_out);
  LORB_CHECK_LAUNCH(ctx);
  b.spec_pending = true;
  return LORB_OK;
}

// The other half, after the solve is enqueued: waits for the readback (the spin stays) and runs the
// host phase on it as dev_build_finish does (db_land to db_layout, and db_buffers' growth test without
// reallocating).  *hit: every product equals the assumption -- the adjacency pattern (hence the
// order), the block list, the band, the partial-run factor, no buffer has to grow, and the solve's
// launch shape (ba_plan_solve_key_same, on the new plan fields) is the one it ran with -- and the new
// host-side plan fields are committed.  An error of db_land / db_layout is returned as
// dev_build_finish returns it.  Otherwise (*hit false) the caller builds again by dev_build.
int dev_spec_verify(lorb_ctx* ctx, const lorb_ba_window_dev* w, lorb_ba_plan* P, bool* hit) {
  lorb_ba_devbuild& b = *P->devb;
  *hit = false;
  b.spec_pending = false;
  b.spec_ok = false;
  b.rb_pending = false;
  LORB_HIP(ctx, lorb::spin_wait(b.rb_ev));
  if (b.pinned[2] & 16) return LORB_OK;  // slots out of order: dev_build reruns the general phase
  const int bw_was = P->hwin[0].bw;
  DbBuild r;
  LORB_TRY(db_land(ctx, w, P, 0, LORB_OK, r));
  if (!db_camera_order(b, r)) return LORB_OK;
  db_blocks(b, r);
  bool same = r.bw == bw_was && r.bps.size() == b.last_bps.size();
  for (size_t i = 0; same && i < r.bps.size(); ++i) same = r.bps[i].ch == b.last_bps[i].ch && r.bps[i].cl == b.last_bps[i].cl;
  if (!same) return LORB_OK;
  LORB_TRY(db_layout(ctx, w, P, r));
  if (r.SF != b.spec_sf || r.G > b.pblk_cap || (size_t)std::max(r.part_total, 1ll) > b.gpart_cap ||
      (int)r.bps.size() > b.up_bp_cap || !lorb::ba_plan_solve_key_same(P))
    return LORB_OK;
  b.last_bps.swap(r.bps);
  b.dirty = false;  // the speculative gather left the scratch clear
  b.spec_ok = true;
  *hit = true;
  return LORB_OK;
}

// The second half of a build: wait for the readback, then the host phase: steps 1 to 6 above.
int dev_build_finish(lorb_ctx* ctx, const lorb_ba_window_dev* w, lorb_ba_plan* P, int lerr) {
  lorb_ba_devbuild& b = *P->devb;
  b.spec_ok = b.spec_pending = false;
  const int phase_rc = (lerr || !b.rb_pending) ? LORB_OK : db_phase1_wait(ctx, w, P);
  static const bool hp_log = env_flag("LORB_HOST_PHASE");
  HostPhase hp{P, hp_log};
  DbBuild r;
  LORB_TRY(db_land(ctx, w, P, lerr, phase_rc, r));
  hp.mark(0);
  db_camera_order(b, r);
  hp.mark(1);
  P->cam_map.assign(1, b.last_map);
  db_blocks(b, r);
  LORB_TRY(db_layout(ctx, w, P, r));
  hp.mark(2);
  LORB_TRY(db_buffers(P, r));
  hp.mark(3);
  db_stage_and_gather(ctx, w, P, r, hp);
  LORB_CHECK_LAUNCH(ctx);
  // what a speculative next build assumes (see lorb_ba_devbuild)
  b.last_bps.swap(r.bps);
  b.spec_sf = r.SF;
  b.spec_ok = !P->comm;
  return LORB_OK;
}

// a whole build: dev_build_issue + dev_build_finish
int dev_build(lorb_ctx* ctx, const lorb_ba_window_dev* w, lorb_ba_plan* P) {
  int lerr = 0;
  LORB_TRY(dev_build_issue(ctx, w, P, &lerr));
  return dev_build_finish(ctx, w, P, lerr);
}

// Behind the lorb_ba_plan_create* entry points (comm: null for an unsharded plan).  A communicator of
// another context is reported after the null checks and before a device window's contents are looked at.
int create_host_plan(lorb_ctx* ctx, lorb_comm* comm, int32_t n_windows, const lorb_ba_window* windows, lorb_ba_plan** out) {
  if (!ctx || !out || n_windows < 0 || (n_windows > 0 && !windows)) return LORB_E_INVALID;
  if (comm && comm->ctx != ctx) return lorb::set_error(ctx, LORB_E_INVALID, "communicator belongs to another context");
  *out = nullptr;
  lorb_ba_plan* P = new (std::nothrow) lorb_ba_plan();
  if (!P) return LORB_E_NOMEM;
  P->comm = comm;
  const int rc = build_plan(ctx, n_windows, windows, P);
  if (rc != LORB_OK) { delete P; return rc; }
  *out = P;
  return LORB_OK;
}
bool window_dev_ok(const lorb_ba_window_dev* w) {
  return w->n_poses >= 0 && w->n_fixed >= 0 && w->max_points >= 0 && w->max_obs >= 0 && w->d_n_points && w->d_n_obs &&
         (w->n_poses == 0 || w->d_pose_init) && (w->n_fixed == 0 || w->d_fixed_pose) &&
         (w->max_points == 0 || w->d_point_init) &&
         (w->max_obs == 0 || (w->d_obs_point && w->d_obs_frame && w->d_obs_uv));
}
int create_dev_plan(lorb_ctx* ctx, lorb_comm* comm, const lorb_ba_window_dev* win, lorb_ba_plan** out) {
  if (!ctx || !win || !out) return LORB_E_INVALID;
  if (comm && comm->ctx != ctx) return lorb::set_error(ctx, LORB_E_INVALID, "communicator belongs to another context");
  if (!window_dev_ok(win)) return LORB_E_INVALID;
  *out = nullptr;
  lorb_ba_plan* P = new (std::nothrow) lorb_ba_plan();
  if (!P) return LORB_E_NOMEM;
  P->ctx = ctx;
  P->comm = comm;
  P->devb = new (std::nothrow) lorb_ba_devbuild();
  // slots sorted by point take k_db_sorted (no counting sort; shard.shard_window sorts by point
  // too); unsorted ones fall back once and the plan keeps the general path from then on
  if (P->devb) P->devb->sorted_hint = true;
  int rc = P->devb ? dev_alloc(ctx, win, P) : LORB_E_NOMEM;
  if (rc == LORB_OK) rc = dev_build(ctx, win, P);
  if (rc != LORB_OK) { delete P; return rc; }
  *out = P;
  return LORB_OK;
}

}  // namespace

// the plan owns its device-build state and every allocation of `allocs`
lorb_ba_plan::~lorb_ba_plan() {
  print_diagnostics(*this);
  delete devb;
  for (void* p : allocs) (void)hipFree(p);
}

namespace lorb {
int ba_plan_update_dev_issue(lorb_ba_plan* P, const lorb_ba_window_dev* w) {
  if (!P || !w || !P->devb || P->comm) return LORB_E_INVALID;
  int lerr = 0;
  return dev_build_issue(P->ctx, w, P, &lerr);
}
int ba_plan_update_dev_finish(lorb_ba_plan* P, const lorb_ba_window_dev* w) {
  if (!P || !w || !P->devb || P->comm) return LORB_E_INVALID;
  return dev_build_finish(P->ctx, w, P, 0);
}
int ba_plan_update_dev_spec(lorb_ba_plan* P, const lorb_ba_window_dev* w, int obs_hint, bool* speculated) {
  if (!P || !w || !P->devb || !speculated) return LORB_E_INVALID;
  *speculated = false;
  lorb_ctx* ctx = P->ctx;
  lorb_ba_devbuild& b = *P->devb;
  if (!spec_allowed(ctx, P)) return dev_build(ctx, w, P);
  spec_spoil(b);
  int lerr = 0;
  LORB_TRY(dev_build_issue(ctx, w, P, &lerr));
  if (!(b.rb_sorted && b.rb_fuse)) return dev_build_finish(ctx, w, P, lerr);
  LORB_TRY(dev_spec_issue(ctx, w, P, obs_hint));
  *speculated = true;
  return LORB_OK;
}
int ba_plan_update_dev_verify(lorb_ba_plan* P, const lorb_ba_window_dev* w, bool* hit) {
  if (!P || !w || !P->devb || !hit || !P->devb->spec_pending) return LORB_E_INVALID;
  return dev_spec_verify(P->ctx, w, P, hit);
}
void ba_plan_sorted_hint(lorb_ba_plan* P, bool sorted) {
  if (P && P->devb) P->devb->sorted_hint = sorted;
}
const int* ba_plan_point_offsets(const lorb_ba_plan* P) { return P && P->devb ? P->dev.pt_obs_off : nullptr; }
void ba_plan_window_counts(const lorb_ba_plan* P, int* n_points, int* n_obs) {
  *n_points = P->Ptot;  // the live counts the last device build read back (its header)
  *n_obs = P->K;
}

// grid of the result kernels: a thread per pose component, the points strided over them
static dim3 result_grid(const lorb_ba_plan* P) {
  return dim3(lorb::ceil_div(std::max(std::max(6 * P->Ctot, 1), std::min(3 * P->Ptot, 256 * 1024)), 256));
}
int ba_plan_result_ring_dev(lorb_ba_plan* P, float* ring, int R, int t0, float* d_point_out) {
  if (!P || !P->devb || !ring || R < 1) return LORB_E_INVALID;
  hipLaunchKernelGGL(k_db_result, result_grid(P), dim3(256), 0, P->ctx->stream, P->dev, P->Ctot, P->Ptot,
                     P->devb->perm, (float*)nullptr, d_point_out, ring, R, t0);
  LORB_CHECK_LAUNCH(P->ctx);
  return LORB_OK;
}

int ba_plan_result_rows_dev(lorb_ba_plan* P, const int* pose_row, float* pose_tab, const int* pt_row, float* pt_tab,
                            int* done) {
  if (!P || !P->devb || !pose_row || !pose_tab || !pt_row || !pt_tab || !done) return LORB_E_INVALID;
  hipLaunchKernelGGL(k_db_result_rows, result_grid(P), dim3(256), 0, P->ctx->stream, P->dev, P->Ctot, P->Ptot,
                     P->devb->perm, pose_row, pose_tab, pt_row, pt_tab, done);
  LORB_CHECK_LAUNCH(P->ctx);
  return LORB_OK;
}

int ba_plan_result64_dev(lorb_ba_plan* P, double* d_out) {
  if (!P || !P->devb || !d_out) return LORB_E_INVALID;
  hipLaunchKernelGGL(k_db_result64, result_grid(P), dim3(256), 0, P->ctx->stream, P->dev, P->Ctot, P->Ptot, P->devb->perm,
                     d_out);
  LORB_CHECK_LAUNCH(P->ctx);
  return LORB_OK;
}

}  // namespace lorb

extern "C" {

int lorb_ba_plan_create(lorb_ctx* ctx, int32_t n_windows, const lorb_ba_window* windows, lorb_ba_plan** out) {
  return create_host_plan(ctx, nullptr, n_windows, windows, out);
}

int lorb_ba_plan_create_sharded(lorb_ctx* ctx, lorb_comm* comm, int32_t n_windows, const lorb_ba_window* shards,
                                lorb_ba_plan** out) {
  if (!comm) return LORB_E_INVALID;
  return create_host_plan(ctx, comm, n_windows, shards, out);
}

int lorb_ba_plan_create_dev(lorb_ctx* ctx, const lorb_ba_window_dev* win, lorb_ba_plan** out) {
  return create_dev_plan(ctx, nullptr, win, out);
}

int lorb_ba_plan_create_sharded_dev(lorb_ctx* ctx, lorb_comm* comm, const lorb_ba_window_dev* shard,
                                    lorb_ba_plan** out) {
  if (!comm) return LORB_E_INVALID;
  return create_dev_plan(ctx, comm, shard, out);
}

int lorb_ba_plan_update_dev(lorb_ba_plan* plan, const lorb_ba_window_dev* win) {
  if (!plan || !win) return LORB_E_INVALID;
  if (!plan->devb) return lorb::set_error(plan->ctx, LORB_E_INVALID, "not a device-built plan");
  return dev_build(plan->ctx, win, plan);
}

int lorb_ba_plan_result_dev(lorb_ba_plan* plan, float* d_pose_out, float* d_point_out) {
  if (!plan) return LORB_E_INVALID;
  if (!plan->devb) return lorb::set_error(plan->ctx, LORB_E_INVALID, "not a device-built plan");
  const int C = plan->Ctot, Pn = plan->Ptot;
  const int m = std::max(6 * C, std::min(3 * Pn, 256 * 1024));
  if (m > 0)
    hipLaunchKernelGGL(k_db_result, dim3(lorb::ceil_div(m, 256)), dim3(256), 0, plan->ctx->stream, plan->dev, C, Pn,
                       plan->devb->perm, d_pose_out, d_point_out, (float*)nullptr, 1, 0);
  LORB_CHECK_LAUNCH(plan->ctx);
  return LORB_OK;
}

int lorb_ba_plan_destroy(lorb_ba_plan* plan) {
  if (!plan) return LORB_OK;
  if (plan->ctx) (void)hipStreamSynchronize(plan->ctx->stream);
  delete plan;
  return LORB_OK;
}

}  // extern "C"
