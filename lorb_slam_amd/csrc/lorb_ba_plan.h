// lorb_ba_plan.h -- the bundle-adjustment plan as its two host units see it: lorb_ba.hip (solve
// sequencing, groups) and lorb_ba_build.hip (the host and device plan builders, which also own the
// plan's destruction); how a device-built plan is constructed (lorb_ba_devbuild) is known to the
// latter alone.  Included after the unit's `#pragma clang fp contract(fast)` block, like lorb_ba_dev.h.
#pragma once
#include "lorb_ba_dev.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace lorb::ba {

// an environment switch: on when its value starts with 1 (callers read theirs once)
inline bool env_flag(const char* name) { const char* e = getenv(name); return e && e[0] == '1'; }

// Words of BaDev::dbg, for its allocation and lorb_ba_plan_debug_stamps: the two-sided Cholesky's
// event trace (LORB_CHOL_TRACE builds), k_ba_ls's phase stamps, a slot per point group (LORB_LS_STAMPS)
inline size_t dbg_words(size_t windows, size_t stamp_slots) {
#ifdef LORB_CHOL_TRACE
  return windows * 512;
#elif defined(LORB_LS_STAMPS)
  return stamp_slots * 8;
#else
  return windows * 8;
#endif
}

// One captured solve (a plan's, or a plan group's) and its executable.
struct GraphCache {
  const char* what;  // names the owner in the capture error ("graph", "group graph")
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  bool valid = false;
  int captures = 0;
  int kernel_nodes = 0;  // kernel launches the captured solve holds
  explicit GraphCache(const char* what_) : what(what_) {}
  GraphCache(const GraphCache&) = delete;  // owns the two handles
  GraphCache& operator=(const GraphCache&) = delete;
  ~GraphCache() { destroy(); }
  // the next replay captures anew (kernel arguments or the launch shape changed); the old graph is
  // destroyed then, not here: it may still be running
  void invalidate() { valid = false; }
  // Launches the captured solve on the ctx stream; when there is none, or the caller's key differs
  // (!same), first captures what enqueue() puts on the stream and, once the graph is instantiated,
  // calls remember() for the caller to store the key.  A failed capture leaves no graph.
  template <typename F, typename R>
  int replay_or_capture(lorb_ctx* ctx, bool same, F enqueue, R remember) {
    if (!valid || !same) {
      destroy();
      LORB_HIP(ctx, hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
      const int rc = enqueue();
      hipGraph_t g = nullptr;
      const hipError_t e = hipStreamEndCapture(ctx->stream, &g);
      if (rc != LORB_OK) { if (g) (void)hipGraphDestroy(g); return rc; }
      if (e != hipSuccess) return lorb::set_error(ctx, LORB_E_DEVICE, "%s capture failed: %s", what, hipGetErrorString(e));
      graph = g;
      LORB_HIP(ctx, hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
      {
        size_t nn = 0;
        LORB_HIP(ctx, hipGraphGetNodes(graph, nullptr, &nn));
        std::vector<hipGraphNode_t> nodes(nn);
        if (nn) LORB_HIP(ctx, hipGraphGetNodes(graph, nodes.data(), &nn));
        kernel_nodes = 0;
        for (size_t i = 0; i < nn; ++i) {
          hipGraphNodeType ty;
          LORB_HIP(ctx, hipGraphNodeGetType(nodes[i], &ty));
          kernel_nodes += ty == hipGraphNodeTypeKernel;
        }
      }
      remember();
      valid = true;
      captures++;
    }
    LORB_HIP(ctx, hipGraphLaunch(exec, ctx->stream));
    return LORB_OK;
  }

 private:
  void destroy() {
    if (exec) { (void)hipGraphExecDestroy(exec); exec = nullptr; }
    if (graph) { (void)hipGraphDestroy(graph); graph = nullptr; }
    valid = false;
  }
};

}  // namespace lorb::ba

struct lorb_ba_devbuild;  // lorb_ba_build.hip

struct lorb_ba_plan {
  lorb_ctx* ctx = nullptr;
  int W = 0, Ctot = 0, Ptot = 0, K = 0, NF = 0, n_pblk = 0, n_bp = 0, n_pairs = 0;
  int env_total = 0, n_total = 0, max_env = 0, max_bw = 0, max_env_w = 0, min_n16 = 1 << 30;
  int min_bw = 1 << 30;  // narrowest band of a non-empty window (k_ba_chol_2s needs >= 15)
  // LORB_HOST_PHASE=1 (diagnostics): host time of the device builds' host phase (readback landed ->
  // k_db_gather launched), printed at destruction
  double hp_us = 0.0, hp_sec[6] = {};
  int hp_n = 0;
  std::vector<lorb::ba::BaWin> hwin;
  std::vector<void*> allocs;
  lorb::ba::BaDev dev{};
  lorb::ba::WinState* d_state = nullptr;
  // the captured solve, with the options it was captured for (and gkey, its launch shape)
  lorb::ba::GraphCache cache{"graph"};
  lorb::ba::LMOpt graph_opt{};
  unsigned gen = 0;  // bumped whenever the plan's buffers move (a lorb_ba_group's graph then re-captures)
  // launch shape of the captured solve: a rebuild that keeps it (device-built plans launch the
  // point-group / block-pair kernels at capacity) replays the graph without a new capture
  struct GraphKey {
    int kind = -1, lds = 0, memset_env = 0, env_total = 0, grid_pblk = 0, grid_bp = 0, pt_launch = 0, x2_n = 0;
    int red_wide = 0, sup = 0, grid_sg = 0;
    int fold = 0;  // the folded iteration tail (lorb_ba_plan::fold)
    bool operator==(const GraphKey& o) const { return memcmp(this, &o, sizeof(GraphKey)) == 0; }
  } gkey;
  GraphKey skey;  // the launch shape of the last solve, captured or not (a speculative build's verification)
  int grid_pblk = 0, grid_bp = 0;  // launch grids of the point-group and block-pair kernels
  int grid_sg = 0;                 // k_ba_ls_sup's grid (partial runs)
  bool has_super = false;          // some window's partial runs hold more than one point group
  // this solve folds every iteration's tail but the last into the next k_ba_ls (fold_of, decided at
  // every solve: LORB_NO_FOLD=1 keeps the k_ba_lm_end kernel)
  bool fold = false;
  int pt_launch = 0;               // points k_ba_init copies (Ptot, or the capacity)
  int* live = nullptr;             // device [n_pblk, n_bp] (BaDev::live)
  lorb_comm* comm = nullptr;  // sharded plan (not owned)
  // exchange 2 of a sharded plan: [send, send + n) -> [recv, ...) (host plans: env | rhs | wfail;
  // device-built plans: rhs | wfail | pad | env, the band's size decides n)
  double *x2_send = nullptr, *x2_recv = nullptr;
  // sharded fused iteration: exchanges 1 and 2 as ONE all-reduce over [lin | pad | solve], which are
  // contiguous (U_part -> U, fx_n doubles)
  size_t fx_n = 0;
  size_t x2_off = 0;  // device-built: offset of env after rhs | wfail | pad
  // per window: camera relabelling (input pose index -> plan camera index; RCM order, §8 item 4)
  std::vector<std::vector<int>> cam_map;
  int chol_kind = -1;         // last launched Cholesky: 0 k_ba_chol, 1 k_ba_chol_w, 2 k_ba_chol_2s
  lorb_ba_devbuild* devb = nullptr;  // device-built plan (lorb_ba_plan_create_dev): its build state, owned
  ~lorb_ba_plan();  // lorb_ba_build.hip: prints the enabled diagnostics, frees the build state and buffers
};
