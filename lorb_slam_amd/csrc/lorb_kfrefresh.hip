// lorb_kfrefresh.hip -- the appearance of the keyframe store and lorb_kf_store_refresh_dev: MapPoint::ComputeDescriptor
// (src/map_point.cpp:69-129) and MapPoint::UpdateNormalAndDepth (:224-264) over the points of the window the store
// last gathered, with Frame::SetPose -> UpdatePoseMat (src/frame.cpp:577-594) for the camera centres of the window's
// keyframes; lorb_kf_store_appear_write / _read / _view.  The contract is in lorb_c.h.
//
// The appearance (kf_slot_desc and kf_slot_octave per keyframe slot, kf_center per keyframe) lives in the store's
// arena; k_kf_head (lorb_kfstore.hip) writes it for keyframe K.
//
// A refresh is three launches on the ctx stream:
//   k_kfr_head    one workgroup: status; a thread per local keyframe for the centres (pose_to_Tcw, inv4_lu32f); the
//                 record's fixed fields
//   k_kfr_points  one wavefront per window point, four per workgroup, lane = observation (rows lane, lane + 64, ...):
//                 the per-observation terms of the normal in parallel, added in list order from LDS; the usable
//                 descriptors collected once by ballot compaction into LDS, the 9-step median search of
//                 k_compute_descriptor (lorb_bf.hip) reading them as broadcasts; the point's own row and its verdict
//   k_kfr_record  one workgroup: the verdicts summed into the record
// No atomics: every point writes its own row and its own verdict.
#include <algorithm>

#include "lorb_internal.h"
#include "lorb_kfstore.h"

namespace {

using Hdr = lorb::KfBaHdr;
using Stat = lorb::KfRefreshStat;
constexpr int kT = 256;                         // threads per workgroup
constexpr int kWaves = kT / 64;                 // window points per workgroup
constexpr int kMaxLocal = lorb::kKfBaMaxLocal;  // local frames <= threads of the head
constexpr int kMaxDesc = 256;                   // usable observations staged per point: the gather refuses 256 or more
constexpr int kAll = LORB_KF_REFRESH_CENTERS | LORB_KF_REFRESH_NORMAL_DEPTH | LORB_KF_REFRESH_DESCRIPTOR;
static_assert(kMaxLocal <= kT, "a thread per local keyframe");

struct Args {
  lorb_frame_params fp;
  int what, max_kf, max_points;
  const lorb_kf_ba_result* ba;
  const Hdr* hdr;
  const int *local, *l2g;
  const int* cnt;
  const uint8_t *kf_bad, *is_bad;
  const int *obs_off, *obs_kf, *obs_slot, *kf_slot_off, *kf_slot_octave;
  const uint4* kf_slot_desc;
  const float *kf_pose, *pos;
  float *kf_center, *normal, *max_dist, *min_dist;
  uint4* desc;
  Stat* stat;
  lorb_kf_refresh_result* rec;
};

using lorb::clampi;

// LDS written by some lanes of a wavefront is read by others
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// a. the refresh runs: the BA's record and the window it belongs to are good
__device__ __forceinline__ bool runs(const Args& a) { return a.ba->status == 0 && a.hdr->status == 0; }

__global__ __launch_bounds__(kT) void k_kfr_head(Args a) {
  const int t = threadIdx.x;
  if (!runs(a)) {
    if (t == 0) a.rec->status = 1;
    return;
  }
  const Hdr& h = *a.hdr;
  const int nk = min(a.cnt[0], a.max_kf), C = clampi(h.C, 0, kMaxLocal);
  const bool centers = (a.what & LORB_KF_REFRESH_CENTERS) && a.ba->written == 1;
  // b. SetPose(Tvec, Rvec) -> UpdatePoseMat of every local keyframe (src/frame.cpp:577-594)
  if (centers && t < C) {
    const int f = a.local[t];
    if ((unsigned)f < (unsigned)nk) {
      float p[6], T[16], Twc[16];
#pragma unroll
      for (int k = 0; k < 6; ++k) p[k] = a.kf_pose[6 * (size_t)f + k];
      lorb::pose_to_Tcw(p, p + 3, T);
      lorb::inv4_lu32f(T, Twc);
      a.kf_center[3 * (size_t)f] = Twc[3];
      a.kf_center[3 * (size_t)f + 1] = Twc[7];
      a.kf_center[3 * (size_t)f + 2] = Twc[11];
    }
  }
  if (t == 0) {
    a.rec->status = 0;
    a.rec->kf = h.kf;
    a.rec->n_points = clampi(h.P, 0, a.max_points);
    a.rec->n_centers = centers ? C : 0;
  }
}

__device__ __forceinline__ uint32_t hamming256(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
  return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) + __popc(a1.x ^ b1.x) +
         __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

__global__ __launch_bounds__(kT) void k_kfr_points(Args a) {
#pragma clang fp contract(off)
  __shared__ uint4 s_desc[kWaves][2 * kMaxDesc];  // the usable descriptors of each wave's point, in list order
  __shared__ float s_term[kWaves][3 * 64];        // one chunk's terms of the normal, in list order
  if (!runs(a)) return;
  const Hdr& h = *a.hdr;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = blockIdx.x * kWaves + wv;
  if (i >= min(h.P, a.max_points)) return;  // wave-uniform: no workgroup barrier below
  const int nk = min(a.cnt[0], a.max_kf), P = a.cnt[1], O = a.cnt[2], S = a.cnt[3];
  const int g = a.l2g[i];
  Stat st{0, 0, 0, 0};
  if ((unsigned)g >= (unsigned)P || a.is_bad[g]) {  // :230 (a cull may have run since the gather)
    st.kind = 1;
    if (lane == 0) a.stat[i] = st;
    return;
  }
  const auto [lo, hi] = lorb::kf_range(a.obs_off, g, O);
  const float px = a.pos[3 * (size_t)g], py = a.pos[3 * (size_t)g + 1], pz = a.pos[3 * (size_t)g + 2];
  const unsigned long long below = (1ull << lane) - 1ull;
  float sx = 0.0f, sy = 0.0f, sz = 0.0f;  // the sum, the same in every lane
  int n_all = 0, n_use = 0, n_bad_slot = 0;
  int ref_f = -1, ref_at = -1;  // mpRefKF and its slot: the first observation inside the store
  for (int o0 = lo; o0 < hi; o0 += 64) {
    const int o = o0 + lane;
    int f = -1, at = -1;
    bool in = false, use = false;
    if (o < hi) {
      f = a.obs_kf[o];
      if ((unsigned)f < (unsigned)nk) {
        const auto [l0, l1] = lorb::kf_range(a.kf_slot_off, f, S);
        const int j = a.obs_slot[o];
        if ((unsigned)j < (unsigned)(l1 - l0)) {
          in = true;
          at = l0 + j;
          use = !a.kf_bad[f];  // :77-78; UpdateNormalAndDepth does not ask
        }
      }
    }
    const unsigned long long m_in = __ballot(in), m_use = __ballot(use), m_out = __ballot(o < hi && !in);
    n_bad_slot += __popcll(m_out);
    if (ref_f < 0 && m_in) {
      const int first = __ffsll((long long)m_in) - 1;
      ref_f = __shfl(f, first, 64);
      ref_at = __shfl(at, first, 64);
    }
    if (a.what & LORB_KF_REFRESH_NORMAL_DEPTH) {
      const int k = __popcll(m_in & below), n_in = __popcll(m_in);
      if (in) {  // normali / cv::norm(normali), :246-248
        const float dx = px - a.kf_center[3 * (size_t)f], dy = py - a.kf_center[3 * (size_t)f + 1],
                    dz = pz - a.kf_center[3 * (size_t)f + 2];
        const double nd = sqrt((double)dx * (double)dx + (double)dy * (double)dy + (double)dz * (double)dz);
        const float inv = (float)(1.0 / nd);
        s_term[wv][3 * k] = dx * inv;
        s_term[wv][3 * k + 1] = dy * inv;
        s_term[wv][3 * k + 2] = dz * inv;
      }
      wave_sync();
      for (int q = 0; q < n_in; ++q) {  // in list order: the order fixes the bits
        sx = sx + s_term[wv][3 * q];
        sy = sy + s_term[wv][3 * q + 1];
        sz = sz + s_term[wv][3 * q + 2];
      }
      wave_sync();
    }
    if (a.what & LORB_KF_REFRESH_DESCRIPTOR) {
      const int k = n_use + __popcll(m_use & below);
      if (use && k < kMaxDesc) {
        s_desc[wv][2 * k] = a.kf_slot_desc[2 * (size_t)at];
        s_desc[wv][2 * k + 1] = a.kf_slot_desc[2 * (size_t)at + 1];
      }
    }
    n_all += __popcll(m_in);
    n_use += __popcll(m_use);
  }
  st.n_bad_slot = n_bad_slot;
  if (n_all == 0) {  // :238, and a list with no observation inside the store
    st.kind = 2;
    if (lane == 0) a.stat[i] = st;
    return;
  }
  if ((a.what & LORB_KF_REFRESH_NORMAL_DEPTH) && lane == 0) {
    const float invn = (float)(1.0 / (double)n_all);  // normal / n, :262
    a.normal[3 * (size_t)g] = sx * invn;
    a.normal[3 * (size_t)g + 1] = sy * invn;
    a.normal[3 * (size_t)g + 2] = sz * invn;
    const float dx = px - a.kf_center[3 * (size_t)ref_f], dy = py - a.kf_center[3 * (size_t)ref_f + 1],
                dz = pz - a.kf_center[3 * (size_t)ref_f + 2];
    const float dist = (float)sqrt((double)dx * (double)dx + (double)dy * (double)dy + (double)dz * (double)dz);  // :252-253
    const int lvl = clampi(a.kf_slot_octave[ref_at], 0, LORB_MAX_LEVELS - 1), top = clampi(a.fp.n_levels - 1, 0, LORB_MAX_LEVELS - 1);
    const float mx = dist * a.fp.scale_factors[lvl];  // :260
    a.max_dist[g] = mx;
    a.min_dist[g] = mx / a.fp.scale_factors[top];  // :261
  }
  if ((a.what & LORB_KF_REFRESH_DESCRIPTOR) && n_use > 0 && n_use <= kMaxDesc) {
    wave_sync();
    const int n = n_use, k = (n - 1) / 2;  // vDist[0.5 * (n - 1)], :118
    const uint4* D = s_desc[wv];
    unsigned long long bestkey = ~0ull;
    for (int c0 = 0; c0 < n; c0 += 64) {
      const int c = c0 + lane;
      const bool act = c < n;
      const uint4 a0 = act ? D[2 * c] : make_uint4(0, 0, 0, 0), a1 = act ? D[2 * c + 1] : make_uint4(0, 0, 0, 0);
      int blo = 0, bhi = act ? 256 : 0;  // the smallest v in [0, 256] with #{j : d(c, j) <= v} > k
      while (__any(blo < bhi)) {
        const int mid = (blo + bhi) >> 1;
        int cnt = 0;
        for (int j = 0; j < n; ++j) cnt += (int)(hamming256(a0, a1, D[2 * j], D[2 * j + 1]) <= (uint32_t)mid);
        if (blo < bhi) {
          if (cnt > k) bhi = mid;
          else blo = mid + 1;
        }
      }
      if (act) {
        const unsigned long long key = ((unsigned long long)blo << 32) | (unsigned)c;
        bestkey = key < bestkey ? key : bestkey;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {  // the smallest median, the first index of equals (strict '<', :119)
      const unsigned long long o = __shfl_xor(bestkey, off, 64);
      bestkey = o < bestkey ? o : bestkey;
    }
    const int bi = (int)(bestkey & 0xffffffffu);
    int bits = 0;
    if (lane < 2) {
      const uint4 nw = D[2 * bi + lane], old = a.desc[2 * (size_t)g + lane];
      bits = __popc(nw.x ^ old.x) + __popc(nw.y ^ old.y) + __popc(nw.z ^ old.z) + __popc(nw.w ^ old.w);
      a.desc[2 * (size_t)g + lane] = nw;
    }
    st.n_desc_bits = bits + __shfl(bits, 1, 64);
  }
  if (lane == 0) a.stat[i] = st;
}

__global__ __launch_bounds__(1024) void k_kfr_record(Args a) {
  __shared__ lorb::I4 wsum4[16];
  if (!runs(a)) return;
  const int t = threadIdx.x, P = clampi(a.hdr->P, 0, a.max_points);
  lorb::I4 c = {{0, 0, 0, 0}}, tot;
  int bits = 0;
  for (int i = t; i < P; i += 1024) {
    const Stat s = a.stat[i];
    c.v[0] += s.kind == 0;
    c.v[1] += s.kind == 1;
    c.v[2] += s.kind == 2;
    c.v[3] += s.n_bad_slot;
    bits += s.n_desc_bits;
  }
  lorb::block_excl_scan4<1024>(c, wsum4, &tot);
  lorb::I4 tot2;
  lorb::block_excl_scan4<1024>(lorb::I4{{bits, 0, 0, 0}}, wsum4, &tot2);
  if (t != 0) return;
  a.rec->n_refreshed = tot.v[0];
  a.rec->n_bad = tot.v[1];
  a.rec->n_empty = tot.v[2];
  a.rec->n_obs_bad_slot = tot.v[3];
  a.rec->n_desc_changed = tot2.v[0];
}

}  // namespace

extern "C" {

int lorb_kf_store_appear_view(const lorb_kf_store* S, lorb_kf_store_appear_host* v) {
  if (!S || !v) return LORB_E_INVALID;
  *v = lorb_kf_store_appear_host{S->cap.max_kf, S->cap.max_kf_slots, S->kf_slot_desc, S->kf_slot_octave, S->kf_center};
  return LORB_OK;
}

int lorb_kf_store_appear_read(lorb_kf_store* S, const lorb_kf_store_appear_host* h) {
  if (!S || !h) return LORB_E_INVALID;
  lorb_ctx* ctx = S->ctx;
  int32_t cnt[6];
  LORB_TRY(lorb::kf_true_counts(S, cnt));
  const int nk = cnt[0], ns = cnt[3];
  if (((h->kf_slot_desc || h->kf_slot_octave) && h->n_kf_slots < ns) || (h->kf_center && h->n_kf < nk))
    return lorb::set_error(ctx, LORB_E_INVALID, "an output array is smaller than the store's count (%d kf, %d slots)", nk, ns);
  LORB_HIP(ctx, lorb::kf_down(S, h->kf_slot_desc, S->kf_slot_desc, (size_t)ns * 32));
  LORB_HIP(ctx, lorb::kf_down(S, h->kf_slot_octave, S->kf_slot_octave, (size_t)ns * 4));
  LORB_HIP(ctx, lorb::kf_down(S, h->kf_center, S->kf_center, (size_t)nk * 12));
  LORB_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return LORB_OK;
}

int lorb_kf_store_appear_write(lorb_kf_store* S, const lorb_kf_store_appear_host* h) {
  if (!S || !h) return LORB_E_INVALID;
  lorb_ctx* ctx = S->ctx;
  int32_t cnt[6];
  LORB_TRY(lorb::kf_true_counts(S, cnt));
  const int nk = cnt[0], ns = cnt[3];
  if (h->n_kf != nk || h->n_kf_slots != ns)
    return lorb::set_error(ctx, LORB_E_INVALID, "appearance: counts %d / %d differ from the store's %d / %d (kf, slots)", h->n_kf,
                           h->n_kf_slots, nk, ns);
  if (h->kf_slot_octave)
    for (int s = 0; s < ns; ++s)
      if (h->kf_slot_octave[s] < 0 || h->kf_slot_octave[s] >= LORB_MAX_LEVELS)
        return lorb::set_error(ctx, LORB_E_INVALID, "appearance: kf_slot_octave[%d] = %d is outside [0, %d)", s,
                               h->kf_slot_octave[s], LORB_MAX_LEVELS);
  LORB_HIP(ctx, lorb::kf_up(S, S->kf_slot_desc, h->kf_slot_desc, (size_t)ns * 32));
  LORB_HIP(ctx, lorb::kf_up(S, S->kf_slot_octave, h->kf_slot_octave, (size_t)ns * 4));
  LORB_HIP(ctx, lorb::kf_up(S, S->kf_center, h->kf_center, (size_t)nk * 12));
  LORB_HIP(ctx, hipStreamSynchronize(ctx->stream));
  // complete once a call has given every array that has rows
  if ((ns == 0 || (h->kf_slot_desc && h->kf_slot_octave)) && (nk == 0 || h->kf_center)) S->appear_ok = true;
  return LORB_OK;
}

int lorb_kf_store_refresh_dev(lorb_ctx* ctx, lorb_kf_store* S, const lorb_frame_params* frame,
                              const lorb_kf_ba_result* d_ba_result, int32_t what, lorb_kf_refresh_result* d_result) {
  if (!frame || !d_ba_result || !d_result) return LORB_E_INVALID;
  LORB_TRY(lorb::kf_enter(ctx, S, lorb::kKfNeedGeom | lorb::kKfNeedAppear));
  if (what == 0 || (what & ~kAll)) return lorb::set_error(ctx, LORB_E_INVALID, "refresh flags 0x%x: empty or unknown", what);
  if (frame->n_levels < 1 || frame->n_levels > LORB_MAX_LEVELS)
    return lorb::set_error(ctx, LORB_E_INVALID, "n_levels %d outside [1, %d]", frame->n_levels, LORB_MAX_LEVELS);
  if (!S->window_current)
    return lorb::set_error(ctx, LORB_E_INVALID, "no current window: the store gathered none, or was compacted since "
                                                "(lorb_kf_store_ba_gather_dev)");
  Args a{};
  a.fp = *frame; a.what = what; a.max_kf = S->cap.max_kf; a.max_points = S->cap.max_points; a.ba = d_ba_result; a.hdr = S->ba_hdr;
  a.local = S->w_local; a.l2g = S->w_l2g; a.cnt = S->cnt; a.kf_bad = S->kf_bad; a.is_bad = S->is_bad;
  a.obs_off = S->obs_off; a.obs_kf = S->obs_kf; a.obs_slot = S->obs_slot; a.kf_slot_off = S->kf_slot_off;
  a.kf_slot_octave = S->kf_slot_octave; a.kf_slot_desc = reinterpret_cast<const uint4*>(S->kf_slot_desc);
  a.kf_pose = S->kf_pose; a.pos = S->pos; a.kf_center = S->kf_center; a.normal = S->normal; a.max_dist = S->max_dist;
  a.min_dist = S->min_dist; a.desc = reinterpret_cast<uint4*>(S->desc); a.stat = S->rf_stat; a.rec = d_result;
  hipStream_t st = ctx->stream;
  // the grid from the header the gather's wait left on the host: the window's point count (the kernels read the
  // device's copy)
  const int Pw = std::min(std::max(S->h_hdr->status == 0 ? S->h_hdr->P : 0, 0), S->cap.max_points);
  hipLaunchKernelGGL(k_kfr_head, dim3(1), dim3(kT), 0, st, a);
  LORB_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(k_kfr_points, dim3(std::max(lorb::ceil_div((size_t)Pw, kWaves), 1u)), dim3(kT), 0, st, a);
  LORB_CHECK_LAUNCH(ctx);
  hipLaunchKernelGGL(k_kfr_record, dim3(1), dim3(1024), 0, st, a);
  LORB_CHECK_LAUNCH(ctx);
  return LORB_OK;
}

}  // extern "C"
