// lorb_kfcompact.hip -- reclaiming the keyframe store's dead point rows: lorb_kf_store_compact_dev, the store's
// Map::EraseMapPoint (src/map.cpp).  A point is dropped when it is bad, has no observation and is named by no
// keyframe slot and no examined entry of a caller's gid table; the survivors keep their order and take the index
// new(p) = the kept points below p.  The contract is in lorb_c.h.
//
// Rows cannot move left in place across workgroups (tile t's destination is tile t-1's source), so they go
// through staging the store owns (lorb_kfstore.h: cp_*; the offsets ride in off2, the tile counts in tile_cnt):
// count - scan - scatter as k_kf_obs_count / k_kf_obs_scatter do it, then a copy back.  FIVE launches on the ctx
// stream:
//   k_kf_compact_head     one thread: status -- the source word, every table's count, the store's counts -- before
//                         the first write; the true counts into KfCompactCtl, the record at its start
//   k_kf_compact_hold     keyframe slots and table entries: a bad point one of them names is held (a byte per
//                         point, at rest between calls; lanes that meet store the same 1)
//   k_kf_compact_count    a thread per point: the verdict, the point's rank among its tile's kept points (cp_map),
//                         the tile's kept count; the holds go back to rest; the record's counters and n_drop by
//                         integer atomics
//   k_kf_compact_scatter  d_map; with rows to drop: base = the sum of the earlier tiles' counts, cp_map becomes the
//                         new index, the kept rows go to staging at that index
//   k_kf_compact_back     staging back over [0, new n_points), the fresh state over [new n_points, P), the keyframe
//                         slots and the tables through cp_map, the true n_points
// The last one returns at once, and the scatter after d_map, when nothing is dropped (KfCompactCtl::n_drop).
#include <algorithm>

#include "lorb_internal.h"
#include "lorb_kfstore.h"

namespace {

constexpr int kT = lorb::kKfTile;  // threads per workgroup = points per tile
constexpr int kMaxGrid = 2048;  // workgroups of the grid-stride kernels
using Ctl = lorb::KfCompactCtl;

struct Table {
  int* gid;
  const int* count;
  int n_max;
};

struct CompactArgs {
  int max_points, max_kf_slots, n_tables;
  const int* src_status;  // or null
  int* cnt;
  lorb::KfPointRows row;  // the point rows
  int* kf_slot_point;
  lorb::KfPointRows stage;  // their staging
  int *tile, *map;
  uint8_t* hold;
  Ctl* ctl;
  int* d_map;  // or null
  lorb_kf_compact_result* rec;
  Table tab[LORB_KF_COMPACT_MAX_TABLES];
};

// a. status, before the first write
__global__ __launch_bounds__(64) void k_kf_compact_head(CompactArgs a) {
  if (threadIdx.x != 0) return;
  const int P = a.cnt[1], O = a.cnt[2], S = a.cnt[3];
  bool ok = !(a.src_status && *a.src_status != 0) && P >= 0 && P <= a.max_points && O >= 0 && S >= 0 && S <= a.max_kf_slots;
  for (int k = 0; k < a.n_tables; ++k) {
    const int n = a.tab[k].count[0];
    ok = ok && n >= 0 && n <= a.tab[k].n_max;
  }
  if (!ok) {
    a.rec->status = 1;
    a.ctl->go = 0;
    a.ctl->n_drop = 0;
    return;
  }
  *a.ctl = Ctl{1, P, O, S, 0, {0, 0, 0}};
  *a.rec = lorb_kf_compact_result{0, P, 0, P, 0, 0, 0};
}

// b. the holds: a bad point a keyframe slot or an examined table entry names
__global__ __launch_bounds__(kT) void k_kf_compact_hold(CompactArgs a) {
  const Ctl& h = *a.ctl;
  if (!h.go) return;
  const int P = h.P, S = h.S;
  const long long i0 = (long long)blockIdx.x * kT + threadIdx.x, step = (long long)gridDim.x * kT;
  for (long long i = i0; i < S; i += step) {
    const int g = a.kf_slot_point[i];
    if ((unsigned)g < (unsigned)P && a.row.is_bad[g]) a.hold[g] = 1;
  }
  for (int k = 0; k < a.n_tables; ++k) {
    const int* gid = a.tab[k].gid;
    const int n = a.tab[k].count[0];  // inside [0, n_max]: the head saw it
    for (long long j = i0; j < n; j += step) {
      const int g = gid[j];
      if ((unsigned)g < (unsigned)P && a.row.is_bad[g]) a.hold[g] = 1;
    }
  }
}

// c. the verdict of point p and its rank among the kept points of its tile
__global__ __launch_bounds__(kT) void k_kf_compact_count(CompactArgs a) {
  __shared__ lorb::I4 wsum4[16];
  const Ctl& h = *a.ctl;
  if (!h.go) return;
  const int t = threadIdx.x, b = blockIdx.x, p = b * kT + t;
  const int P = h.P, O = h.O;
  if ((long long)b * kT >= P) return;
  int keep = 0, bad = 0;
  if (p < P) {
    const auto [lo, hi] = lorb::kf_range(a.row.obs_off, p, O);
    const int held = a.hold[p];
    bad = a.row.is_bad[p] != 0;
    keep = !(bad && hi == lo && !held);
    if (held) a.hold[p] = 0;  // back at rest
  }
  lorb::I4 tot;
  const lorb::I4 at = lorb::block_excl_scan4<kT>(lorb::I4{{keep, keep & bad, 0, 0}}, wsum4, &tot);
  if (p < P) a.map[p] = keep ? at.v[0] : -1;
  if (t != 0) return;
  a.tile[b] = tot.v[0];
  const int dropped = min(P - b * kT, kT) - tot.v[0];
  if (dropped) {
    atomicAdd(&a.ctl->n_drop, dropped);
    atomicAdd(&a.rec->n_dropped, dropped);
    atomicSub(&a.rec->n_points, dropped);
  }
  if (tot.v[1]) atomicAdd(&a.rec->n_bad_kept, tot.v[1]);
}

// d + e. d_map; the kept rows to staging at their new index
__global__ __launch_bounds__(kT) void k_kf_compact_scatter(CompactArgs a) {
  __shared__ int wsum[16];
  const Ctl& h = *a.ctl;
  if (!h.go) return;
  const int t = threadIdx.x, b = blockIdx.x, p = b * kT + t;
  const int P = h.P;
  if ((long long)b * kT >= P) return;
  if (h.n_drop == 0) {  // the identity, and not a byte of the store
    if (a.d_map && p < P) a.d_map[p] = p;
    return;
  }
  const int base = lorb::tile_base_1024(a.tile, b, wsum);
  if (p >= P) return;
  const int r = a.map[p], q = r < 0 ? -1 : base + r;
  a.map[p] = q;
  if (a.d_map) a.d_map[p] = q;
  if (q < 0) return;
  a.stage.copy_row((size_t)q, a.row, (size_t)p);
}

// e, f, g. the rows back, the fresh state behind them, the indices through the map, the true count
__global__ __launch_bounds__(kT) void k_kf_compact_back(CompactArgs a) {
  __shared__ lorb::I4 wsum4[16];
  const Ctl& h = *a.ctl;
  if (!h.go || h.n_drop == 0) return;
  const int t = threadIdx.x;
  const int P = h.P, O = h.O, S = h.S, N = P - h.n_drop;
  const long long i0 = (long long)blockIdx.x * kT + t, step = (long long)gridDim.x * kT;
  for (long long i = i0; i <= P; i += step) {
    const size_t o = (size_t)i;
    if (i < N) {
      a.row.copy_row(o, a.stage, o);
    } else {
      a.row.obs_off[o] = i == N ? O : 0;
      if (i < P) a.row.fresh_row(o);  // what a fresh store has there
    }
  }
  lorb::I4 c = {{0, 0, 0, 0}}, tot;
  for (long long i = i0; i < S; i += step) {
    const int g = a.kf_slot_point[i];
    if ((unsigned)g < (unsigned)P) {
      a.kf_slot_point[i] = a.map[g];
      ++c.v[0];
    }
  }
  for (int k = 0; k < a.n_tables; ++k) {
    int* gid = a.tab[k].gid;
    const int n = a.tab[k].count[0];
    for (long long j = i0; j < n; j += step) {
      const int g = gid[j];
      if ((unsigned)g < (unsigned)P) {
        gid[j] = a.map[g];
        ++c.v[1];
      }
    }
  }
  lorb::block_excl_scan4<kT>(c, wsum4, &tot);
  if (t != 0) return;
  if (tot.v[0]) atomicAdd(&a.rec->n_kf_slots_mapped, tot.v[0]);
  if (tot.v[1]) atomicAdd(&a.rec->n_gids_mapped, tot.v[1]);
  if (blockIdx.x == 0) a.cnt[1] = N;
}

}  // namespace

extern "C" {

int lorb_kf_store_compact_dev(lorb_ctx* ctx, lorb_kf_store* S, const int32_t* d_src_status, const lorb_kf_gid_table* tables,
                              int32_t n_tables, int32_t* d_map, lorb_kf_compact_result* d_result) {
  if (!d_result) return LORB_E_INVALID;
  LORB_TRY(lorb::kf_enter(ctx, S));
  if (n_tables < 0 || n_tables > LORB_KF_COMPACT_MAX_TABLES)
    return lorb::set_error(ctx, LORB_E_INVALID, "%d gid tables: outside [0, %d]", n_tables, LORB_KF_COMPACT_MAX_TABLES);
  if (n_tables > 0 && !tables) return lorb::set_error(ctx, LORB_E_INVALID, "null tables");
  CompactArgs a{};
  size_t tab_max = 0;
  for (int k = 0; k < n_tables; ++k) {
    const lorb_kf_gid_table& tb = tables[k];
    if (!tb.d_gid || !tb.d_count) return lorb::set_error(ctx, LORB_E_INVALID, "gid table %d: null array", k);
    if (tb.n_max < 1) return lorb::set_error(ctx, LORB_E_INVALID, "gid table %d: bound %d must be positive", k, tb.n_max);
    bool twice = false;  // the same table named again is mapped once
    for (int i = 0; i < a.n_tables && !twice; ++i)
      if (a.tab[i].gid == tb.d_gid) {
        if (a.tab[i].n_max != tb.n_max || a.tab[i].count != tb.d_count)
          return lorb::set_error(ctx, LORB_E_INVALID, "gid table %d: the array of an earlier table with another bound or count", k);
        twice = true;
      }
    if (twice) continue;
    a.tab[a.n_tables++] = Table{tb.d_gid, tb.d_count, tb.n_max};
    tab_max = std::max(tab_max, (size_t)tb.n_max);
  }
  a.max_points = S->cap.max_points; a.max_kf_slots = S->cap.max_kf_slots; a.src_status = d_src_status; a.cnt = S->cnt;
  a.row = S->point_rows(); a.kf_slot_point = S->kf_slot_point; a.stage = S->stage_rows();
  a.tile = S->tile_cnt; a.map = S->cp_map; a.hold = S->cp_hold; a.ctl = S->cp_ctl; a.d_map = d_map; a.rec = d_result;
  hipStream_t st = ctx->stream;
  // grids from the host's bounds: the kernels read the true counts
  const unsigned pt_blocks = std::max(lorb::ceil_div((size_t)S->b_points, kT), 1u);
  const size_t walk = std::max(std::max((size_t)S->b_slots, tab_max), (size_t)1);
  const unsigned hold_blocks = std::min(lorb::ceil_div(walk, kT), (unsigned)kMaxGrid);
  const unsigned back_blocks = std::min(lorb::ceil_div(std::max(walk, (size_t)S->b_points + 1), kT), (unsigned)kMaxGrid);
  hipLaunchKernelGGL(k_kf_compact_head, dim3(1), dim3(64), 0, st, a);
  LORB_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(k_kf_compact_hold, dim3(hold_blocks), dim3(kT), 0, st, a);
  LORB_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(k_kf_compact_count, dim3(pt_blocks), dim3(kT), 0, st, a);
  LORB_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(k_kf_compact_scatter, dim3(pt_blocks), dim3(kT), 0, st, a);
  LORB_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(k_kf_compact_back, dim3(back_blocks), dim3(kT), 0, st, a);
  LORB_CHECK_LAUNCH(ctx);
  S->window_current = false;  // w_l2g may hold the old numbers (lorb_kf_store_refresh_dev refuses it)
  return LORB_OK;
}

}  // extern "C"
