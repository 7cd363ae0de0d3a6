// lorb_ba_slots.h -- resident device-built BA plans, one per camera count, in a small LRU with capacities that
// only grow: the slot logic of lorb_ba_solver (windows from host arrays) and of the keyframe store's local BA
// (windows gathered on the device, lorb_kfba.hip).  Implemented in lorb_ba_solver.hip.
#pragma once

#include "lorb_internal.h"

namespace lorb {

struct PlanSlot {
  int C = -1, F_cap = 0, P_cap = 0, K_cap = 0;
  lorb_ba_plan* plan = nullptr;
  // the owner's device blocks, sized by the capacities and freed with the slot (the solver's packed window and
  // result; unused by the store, whose window lives in its own arena)
  unsigned char* d_in = nullptr;
  size_t in_bytes = 0;
  double* d_out = nullptr;
  unsigned long long last_use = 0;
};

struct PlanSlots {
  static constexpr int kSlots = 4;
  PlanSlot slot[kSlots];
  unsigned long long clock = 0;
  int creations = 0;

  // the slot for C cameras with room for F fixed rows, P points, K observations, each capacity at most its
  // `max` (0: unbounded).  A slot that is new, or was outgrown and released, comes back with plan == nullptr
  // and no blocks.  Evicting or regrowing waits for the stream.
  int pick(lorb_ctx* ctx, int C, int F, int P, int K, PlanSlot** out, int F_max = 0, int P_max = 0, int K_max = 0);
  // the slot's plan built from the window's current contents: lorb_ba_plan_create_dev the first time, then
  // lorb_ba_plan_update_dev under the sorted hint.  The plan's error is returned as it is; a slot whose first
  // build failed has no plan.
  int build(lorb_ctx* ctx, PlanSlot* s, const lorb_ba_window_dev* w, bool sorted);
  void release(PlanSlot& s);
  void release_all();
  int resident() const;
};

}  // namespace lorb
