// lorb_internal.h -- shared internals of liblorb.so (HIP runtime for gfx950 / MI355X).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/lorb_c.h"

struct lorb_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  hipEvent_t ev[64] = {};
  // grow-only device scratch buffers, one per slot
  static constexpr int kScratch = 128;
  void* scratch[kScratch] = {};
  size_t scratch_sz[kScratch] = {};
  // host copy of the bytes last uploaded into a slot (lorb::upload); an identical re-upload of
  // per-call constants (problem offsets, scan tiles) is skipped.  Cleared whenever the slot is
  // handed out as kernel-written scratch.
  std::vector<unsigned char> up_mirror[kScratch];
  // per-kernel event timing
  bool ktime = false;
  std::vector<hipEvent_t> kev_pool;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> kev[LORB_K_COUNT];
  // S_BF_TKEY entries known to hold all-ones (0: re-fill before use), for the buffer tkey_buf
  size_t tkey_ready = 0;
  void* tkey_buf = nullptr;
  void* done_buf = nullptr;  // S_BF_DONE as last zeroed
  // pinned host staging
  void* pinned = nullptr;
  size_t pinned_sz = 0;
  // spin_sync's event (no timing)
  hipEvent_t spin_ev = nullptr;
  // lorb_ctx_ba_solver's solver (destroyed with the ctx)
  lorb_ba_solver* solver = nullptr;
  // pinned (coherent, mapped) staging of lorb::InPack / OutPack and its device-side addresses
  void* io_in = nullptr;
  void* io_in_dev = nullptr;
  size_t io_in_sz = 0;
  void* io_out = nullptr;
  void* io_out_dev = nullptr;
  size_t io_out_sz = 0;
  bool io_pending = false;  // an InPack pull may still read the staging (cleared by OutPack::fetch)
  // S_TM_ZERO as last cleared: an all-EMPTY slot-state array nothing ever writes (lorb_track_motion*)
  void* zero_ss = nullptr;
  size_t zero_ss_sz = 0;
};

namespace lorb {
// Wait for the stream by polling an event from the host instead of a blocking synchronize: the
// device plan build's one readback sits on the step's critical path, and a blocked host thread
// wakes up tens of microseconds after the copy lands.
inline hipError_t spin_wait(hipEvent_t ev) {
  hipError_t e;
  while ((e = hipEventQuery(ev)) == hipErrorNotReady) {
  }
  return e;
}
inline hipError_t spin_sync(lorb_ctx* ctx) {
  hipError_t e = hipEventRecord(ctx->spin_ev, ctx->stream);
  if (e != hipSuccess) return e;
  return spin_wait(ctx->spin_ev);
}
}  // namespace lorb

// multi-GPU communicator (lorb_comm.hip): RCCL over xGMI, or a host callback transport
struct lorb_comm {
  lorb_ctx* ctx = nullptr;
  int nranks = 1, rank = 0;
  bool rccl = false;
  void* nccl = nullptr;                    // ncclComm_t
  lorb_host_allreduce_fn fn = nullptr;     // host transport
  void* user = nullptr;
  double* pinned = nullptr;                // host staging for the callback transport
  size_t pinned_n = 0;
  double* dbuf = nullptr;                  // device staging of comm_allreduce_host (RCCL; grow-only)
  size_t dbuf_n = 0;
};

namespace lorb {

int set_error(lorb_ctx* ctx, int code, const char* fmt, ...);
// stream-ordered all-reduce of device doubles on comm->ctx->stream (send may equal recv)
int comm_allreduce(lorb_comm* comm, const double* d_send, double* d_recv, size_t n, int op);
// blocking all-reduce of a host array (plan construction)
int comm_allreduce_host(lorb_comm* comm, double* h_buf, size_t n, int op);

#define LORB_HIP(ctx, call)                                                              \
  do {                                                                                   \
    hipError_t e_ = (call);                                                              \
    if (e_ != hipSuccess)                                                                \
      return ::lorb::set_error((ctx), LORB_E_DEVICE, "%s failed: %s (%s:%d)", #call,    \
                               hipGetErrorString(e_), __FILE__, __LINE__);               \
  } while (0)

#define LORB_CHECK_LAUNCH(ctx) LORB_HIP(ctx, hipGetLastError())

#define LORB_TRY(expr)          \
  do {                          \
    int rc_ = (expr);           \
    if (rc_ != LORB_OK) return rc_; \
  } while (0)

// device-built plan (lorb_ba_plan_create_dev): the solution in double, caller camera order, plus
// the LM summary, into d_out = [poses 6C | points 3P | iterations, successful, termination, initial
// cost, final cost] (async on the plan's stream)
int ba_plan_result64_dev(lorb_ba_plan* P, double* d_out);
// the same as lorb_ba_plan_result_dev with the poses written into a keyframe ring (pose c of the
// window to slot (t0 + c) mod R, 6 floats each) instead of a pose array
int ba_plan_result_ring_dev(lorb_ba_plan* P, float* ring, int R, int t0, float* d_point_out);
// the same conversion scattered into tables: pose c of the window to row pose_row[c] of pose_tab (6 floats), point
// i to row pt_row[i] of pt_tab (3 floats); *done = 1.  One launch.  All device pointers.
int ba_plan_result_rows_dev(lorb_ba_plan* P, const int* pose_row, float* pose_tab, const int* pt_row, float* pt_tab,
                            int* done);
// a device-built plan whose callers keep the observation slots sorted by point (stably, no unused
// slots) builds without the counting sort; slots found out of order fall back to it (same result)
void ba_plan_sorted_hint(lorb_ba_plan* P, bool sorted);
// lorb_ba_plan_update_dev in two halves (unsharded device-built plans): issue queues the build's
// first phase and its readback on the ctx stream; finish waits for that readback and completes the
// build.  Work for other plans may be queued in between (lorb_map_group builds its maps this way).
int ba_plan_update_dev_issue(lorb_ba_plan* P, const lorb_ba_window_dev* w);
int ba_plan_update_dev_finish(lorb_ba_plan* P, const lorb_ba_window_dev* w);
// lorb_ba_plan_update_dev that speculates on the plan's structure where it may (lorb_ba_build.hip,
// dev_spec_issue): *speculated -- phase 1, its readback and a gather that assumes the last build's
// adjacency pattern are queued and the host has not waited; the caller enqueues the solve and then
// calls ..._verify, which waits for the readback and runs the host phase on it: *hit -- the assumption
// held and the plan is the one lorb_ba_plan_update_dev would have built; an error is the build's; else
// the caller builds again (lorb_ba_plan_update_dev) and solves again.  Not speculated: the build is
// complete (or failed) as lorb_ba_plan_update_dev leaves it.  obs_hint: a bound on the live observations.
int ba_plan_update_dev_spec(lorb_ba_plan* P, const lorb_ba_window_dev* w, int obs_hint, bool* speculated);
int ba_plan_update_dev_verify(lorb_ba_plan* P, const lorb_ba_window_dev* w, bool* hit);
// the launch shape (graph key, fold) the plan's fields give now equals the last solve's (lorb_ba.hip)
bool ba_plan_solve_key_same(lorb_ba_plan* P);
// the window's live point / observation counts as the last lorb_ba_plan_update_dev read them
void ba_plan_window_counts(const lorb_ba_plan* P, int* n_points, int* n_obs);
// the last device build's per-point observation offsets (point-sorted slots), device pointer
const int* ba_plan_point_offsets(const lorb_ba_plan* P);

// crossCheck keys of ONE brute-force problem (lorb_bf_match_dev without its finalisation): per
// query (dist << 32 | train) or all-ones; *qkey_out is ctx scratch valid until the next matcher call
int match1_keys_dev(lorb_ctx* ctx, const uint8_t* d_q, int nq, const uint8_t* d_t, int nt,
                    unsigned long long** qkey_out, hipStream_t stream = nullptr);  // null: ctx->stream
// the same into caller-owned buffers: qkey (nq entries), tkey (nt entries, all-ones on entry and
// again once the call's kernels have run), on stream st
int match1_keys_into(lorb_ctx* ctx, const uint8_t* d_q, int nq, const uint8_t* d_t, int nt,
                     unsigned long long* qkey, uint32_t* tkey, hipStream_t st);

// grow-only scratch: returns device pointer in *out
int scratch(lorb_ctx* ctx, int slot, size_t bytes, void** out);
template <typename T>
int scratch_t(lorb_ctx* ctx, int slot, size_t count, T** out) {
  void* p = nullptr;
  int rc = scratch(ctx, slot, count * sizeof(T) + 16, &p);
  *out = static_cast<T*>(p);
  return rc;
}

// H2D into scratch slot (sync w.r.t. host buffer: uses hipMemcpyAsync + stream sync at end
// of the calling API).
int upload(lorb_ctx* ctx, int slot, const void* host, size_t bytes, void** dev);
template <typename T>
int upload_t(lorb_ctx* ctx, int slot, const T* host, size_t count, T** dev) {
  void* p = nullptr;
  if (host == nullptr || count == 0) { *dev = nullptr; return scratch(ctx, slot, 16, &p) == LORB_OK ? (*dev = nullptr, LORB_OK) : LORB_E_DEVICE; }
  int rc = upload(ctx, slot, host, count * sizeof(T), &p);
  *dev = static_cast<T*>(p);
  return rc;
}

// Host-array entry points (the per-frame calls a host caller issues, e.g. SearchByProjection on the
// live tracking path): every input array is packed into ONE pinned staging buffer that ONE pull
// kernel on the ctx stream copies into a device block (a kernel reading the mapped host buffer: an
// SDMA copy would cost the engine-to-queue hand-off, ~10 us on the tracking path); the outputs live
// in ONE block: device memory that ONE device-to-host copy brings back, or (alloc(true)) the mapped
// pinned buffer itself, written by the call's last kernel with plain stores (no atomics, no reads).
// Usage: InPack::add() per input (before commit), commit() (pack + pull), dev<T>(i) per input;
// OutPack::add() per output, alloc(direct), dev<T>(i), fetch() (copy if needed + wait), then
// host<T>(i).  One of each per ctx is in use at a time (calls on one ctx are serialized).
class InPack {
 public:
  explicit InPack(lorb_ctx* c) : ctx(c) {}
  int add(const void* host, size_t bytes) {  // returns the part index
    parts.push_back({host, bytes, total});
    total += (bytes + 255) & ~size_t(255);
    return (int)parts.size() - 1;
  }
  template <typename T>
  int add_t(const T* host, size_t count) { return add(host, host ? count * sizeof(T) : 0); }
  // mapped: no pull -- dev<T>() then addresses the mapped staging itself (for a kernel that reads
  // each input once: one PCIe round trip instead of a pull launch and its hand-off)
  int commit(bool mapped = false);
  template <typename T>
  T* dev(int i) const { return parts[i].bytes ? reinterpret_cast<T*>(static_cast<unsigned char*>(base) + parts[i].off) : nullptr; }

 private:
  struct Part { const void* host; size_t bytes, off; };
  lorb_ctx* ctx;
  std::vector<Part> parts;
  size_t total = 0;
  void* base = nullptr;
};
class OutPack {
 public:
  explicit OutPack(lorb_ctx* c) : ctx(c) {}
  int add(size_t bytes) {
    parts.push_back({bytes, total});
    total += (bytes + 255) & ~size_t(255);
    return (int)parts.size() - 1;
  }
  int alloc(bool direct = false);
  int fetch();  // one D2H copy into pinned memory (unless direct), then waits for the stream
  template <typename T>
  T* dev(int i) const { return reinterpret_cast<T*>(static_cast<unsigned char*>(dbase) + parts[i].off); }
  template <typename T>
  const T* host(int i) const { return reinterpret_cast<const T*>(static_cast<const unsigned char*>(hbase) + parts[i].off); }

 private:
  struct Part { size_t bytes, off; };
  lorb_ctx* ctx;
  std::vector<Part> parts;
  size_t total = 0;
  void* dbase = nullptr;
  void* hbase = nullptr;
  bool direct = false;
};

// brackets one kernel launch with events when ctx->ktime is set
struct KernelTimer {
  lorb_ctx* ctx; int k; hipEvent_t b = nullptr, e = nullptr;
  KernelTimer(lorb_ctx* c, int kid);
  ~KernelTimer();
};

inline unsigned ceil_div(size_t a, size_t b) { return static_cast<unsigned>((a + b - 1) / b); }

// Exclusive scan of one int per thread across a 1024-thread workgroup (16 wavefronts): wave
// inclusive scan with DPP-lowered shuffles, then the 16 wave totals from LDS.  Returns the
// exclusive prefix of this thread; *total = the workgroup sum.  wsum: __shared__ int[16].
// Every thread of the workgroup must call it (two barriers).
__device__ __forceinline__ int block_excl_scan_1024(int v, int* wsum, int* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(incl, o, 64);
    if (lane >= o) incl += u;
  }
  if (lane == 63) wsum[wv] = incl;
  __syncthreads();
  int pre = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < 16; ++w) {
    const int s = wsum[w];
    pre += w < wv ? s : 0;
    tot += s;
  }
  __syncthreads();
  *total = tot;
  return pre + incl - v;
}

// The same for any workgroup size NT (a multiple of 64); wsum: __shared__ int[NT / 64].
template <int NT>
__device__ __forceinline__ int block_excl_scan(int v, int* wsum, int* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(incl, o, 64);
    if (lane >= o) incl += u;
  }
  if (lane == 63) wsum[wv] = incl;
  __syncthreads();
  int pre = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) {
    const int s = wsum[w];
    pre += w < wv ? s : 0;
    tot += s;
  }
  __syncthreads();
  *total = tot;
  return pre + incl - v;
}

// Exclusive prefix sums of one tile in[0 .. n), n <= kScanTile, into out by ONE 1024-thread
// workgroup, plus `carry`: coalesced 16-byte loads into LDS (one pad word per 16 so that each
// thread's 16 consecutive values are conflict-free), a 16-value serial scan per thread, the
// workgroup scan of the thread sums, coalesced stores.  s_tile: __shared__ int[kScanTileLds].
// Returns the tile sum; *mx (optional) gets this thread's max of its values.
constexpr int kScanTile = 16384, kScanTileLds = kScanTile + kScanTile / 16;
__device__ __forceinline__ int wg_scan_tile(const int* __restrict__ in, int* __restrict__ out, int n, int carry,
                                            int* s_tile, int* wsum, int* mx = nullptr) {
  const int t = threadIdx.x;
  auto pad = [](int i) { return i + (i >> 4); };
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int i = 4 * (t + 1024 * u);
    int4 v = make_int4(0, 0, 0, 0);
    if (i + 3 < n && ((reinterpret_cast<size_t>(in) & 15) == 0)) {
      v = *reinterpret_cast<const int4*>(in + i);
    } else {
      v.x = i < n ? in[i] : 0; v.y = i + 1 < n ? in[i + 1] : 0;
      v.z = i + 2 < n ? in[i + 2] : 0; v.w = i + 3 < n ? in[i + 3] : 0;
    }
    s_tile[pad(i)] = v.x; s_tile[pad(i + 1)] = v.y; s_tile[pad(i + 2)] = v.z; s_tile[pad(i + 3)] = v.w;
  }
  __syncthreads();
  int v[16], loc = 0, m = 0;
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    v[u] = s_tile[17 * t + u];
    m = max(m, v[u]);
    loc += v[u];
  }
  int tot;
  int run = carry + block_excl_scan_1024(loc, wsum, &tot);
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    s_tile[17 * t + u] = run;
    run += v[u];
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int i = 4 * (t + 1024 * u);
    const int4 r = make_int4(s_tile[pad(i)], s_tile[pad(i + 1)], s_tile[pad(i + 2)], s_tile[pad(i + 3)]);
    if (i + 3 < n && ((reinterpret_cast<size_t>(out) & 15) == 0)) {
      *reinterpret_cast<int4*>(out + i) = r;
    } else {
      if (i < n) out[i] = r.x;
      if (i + 1 < n) out[i + 1] = r.y;
      if (i + 2 < n) out[i + 2] = r.z;
      if (i + 3 < n) out[i + 3] = r.w;
    }
  }
  __syncthreads();  // s_tile is reused by the next tile
  if (mx) *mx = max(*mx, m);
  return tot;
}

// The same over any n, tile after tile (one workgroup).  Returns the total.
__device__ __forceinline__ int wg_excl_scan(const int* __restrict__ in, int* __restrict__ out, int n, int* s_tile,
                                            int* wsum, int* mx = nullptr) {
  int carry = 0;
  for (int base = 0; base < n; base += kScanTile)
    carry += wg_scan_tile(in + base, out + base, min(n - base, kScanTile), carry, s_tile, wsum, mx);
  return carry;
}

// Exclusive max-scan (identity `lo`) across an NT-thread workgroup; wmax: __shared__ int[NT / 64].
template <int NT>
__device__ __forceinline__ int block_excl_max(int v, int lo, int* wmax) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(incl, o, 64);
    if (lane >= o) incl = max(incl, u);
  }
  int ex = __shfl_up(incl, 1, 64);
  if (lane == 0) ex = lo;
  if (lane == 63) wmax[wv] = incl;
  __syncthreads();
  int pre = lo;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) pre = w < wv ? max(pre, wmax[w]) : pre;
  __syncthreads();
  return max(pre, ex);
}

// A 4x4 float matrix passed by value as a kernel argument (no upload).
struct Mat4f {
  float v[16];
};

// Frame::UnprojectStereo for one keypoint with depth z > 0 (src/frame.cpp:335-356): camera
// coordinates in float, then Twc * [x y z 1] accumulated in double as cv::Mat's float gemm does.
// Shared by k_unproject and the LocalMapping append (compiled -ffp-contract=off: same bits).
__device__ __forceinline__ void unproject_point(float fx, float fy, float cx, float cy, const Mat4f& Twc, float u,
                                                float v, float z, float* out) {
  const float xx = (u - cx) * z / fx;
  const float yy = (v - cy) * z / fy;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double s = (double)Twc.v[4 * r] * xx + (double)Twc.v[4 * r + 1] * yy + (double)Twc.v[4 * r + 2] * z +
                     (double)Twc.v[4 * r + 3] * 1.0f;
    out[r] = (float)s;
  }
}
// (a20) Frame::UnprojectStereo of one keypoint: the origin where it has no depth (src/frame.cpp:352-355).
// Shared by k_unproject, k_slots_fill and the keyframe insertion (lorb_kfstore.hip).
__device__ __forceinline__ void unproject_kp(const lorb_frame_params& fp, const Mat4f& Twc, float x, float y, float z,
                                             float* out) {
  if (z > 0) {
    unproject_point(fp.fx, fp.fy, fp.cx, fp.cy, Twc, x, y, z, out);
  } else {
    out[0] = 0.0f; out[1] = 0.0f; out[2] = 0.0f;
  }
}
// cv::Mat::inv() of a 4x4 CV_32F: hal::LU32f (partial pivoting, float only), host and device.  Contraction is off
// in the body whatever the including unit says (the BA units contract), as in pose_to_Tcw below: the device value
// has the bits of the host's.  Device code: lorb_window.hip and the centres of lorb_kfrefresh.hip.
__host__ __device__ inline bool inv4_lu32f(const float* Ain, float* out) {
#pragma clang fp contract(off)
  float A[16], b[16];
  for (int i = 0; i < 16; i++) A[i] = Ain[i];
  for (int i = 0; i < 16; i++) b[i] = (i % 5 == 0) ? 1.0f : 0.0f;
  const float eps = 1.1920928955078125e-07f * 10;
  for (int i = 0; i < 4; i++) {
    int k = i;
    for (int j = i + 1; j < 4; j++)
      if (fabsf(A[j * 4 + i]) > fabsf(A[k * 4 + i])) k = j;
    if (fabsf(A[k * 4 + i]) < eps) {
      for (int j = 0; j < 16; j++) out[j] = 0.0f;
      return false;
    }
    if (k != i) {
      for (int j = i; j < 4; j++) { const float v = A[i * 4 + j]; A[i * 4 + j] = A[k * 4 + j]; A[k * 4 + j] = v; }
      for (int j = 0; j < 4; j++) { const float v = b[i * 4 + j]; b[i * 4 + j] = b[k * 4 + j]; b[k * 4 + j] = v; }
    }
    const float dd = -1 / A[i * 4 + i];
    for (int j = i + 1; j < 4; j++) {
      const float alpha = A[j * 4 + i] * dd;
      for (int kk = i + 1; kk < 4; kk++) A[j * 4 + kk] += alpha * A[i * 4 + kk];
      for (int kk = 0; kk < 4; kk++) b[j * 4 + kk] += alpha * b[i * 4 + kk];
    }
  }
  for (int i = 3; i >= 0; i--)
    for (int j = 0; j < 4; j++) {
      float s = b[i * 4 + j];
      for (int k = i + 1; k < 4; k++) s -= A[i * 4 + k] * b[k * 4 + j];
      b[i * 4 + j] = s / A[i * 4 + i];
    }
  for (int i = 0; i < 16; i++) out[i] = b[i];
  return true;
}

// cv::Rodrigues (vector -> matrix, double internally) + Frame::UpdatePoseMat write-back: the body of
// lorb_pose_to_Tcw, and on the device the pose hand-over of lorb_track_local_frames_dev.  Contraction
// is off in the body whatever the including unit says (lorb_ba.hip contracts), so it rounds like the
// reference's un-contracted host build; the device's double sin / cos are not libm's functions.
__host__ __device__ inline void pose_to_Tcw(const float rvec[3], const float tvec[3], float T[16]) {
#pragma clang fp contract(off)
  double rx = rvec[0], ry = rvec[1], rz = rvec[2];
  const double theta = sqrt(rx * rx + ry * ry + rz * rz);
  double R[9];
  if (theta < 2.220446049250313e-16) {
    for (int k = 0; k < 9; ++k) R[k] = (k % 4 == 0) ? 1.0 : 0.0;
  } else {
    const double c = cos(theta), s = sin(theta), c1 = 1. - c;
    const double it = theta ? 1. / theta : 0.;
    rx *= it; ry *= it; rz *= it;
    const double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
    const double rxm[9] = {0, -rz, ry, rz, 0, -rx, -ry, rx, 0};
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int k = 0; k < 9; ++k) R[k] = c * I[k] + c1 * rrt[k] + s * rxm[k];
  }
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) T[4 * r + c] = (float)R[3 * r + c];
    T[4 * r + 3] = tvec[r];
  }
  T[12] = 0.f; T[13] = 0.f; T[14] = 0.f; T[15] = 1.f;
}

// R <- U * V^T of the SVD of a 3 x 3 double matrix (row-major, in place): the orthogonal polar factor,
// which is unique for a non-singular R whatever the order and the signs of the singular vectors, so no
// sorting.  One-sided Jacobi (Hestenes): plane rotations from the right make the columns of A = R * V
// orthogonal, then U = A * diag(1 / |a_j|).  A column of norm zero (a singular R: no rotation) stays
// zero where OpenCV's JacobiSVD completes U with a vector of its own.  Every index is a compile-time
// constant after unrolling: the matrices stay in registers on the device.
__host__ __device__ inline void polar_uvt3(double R[9]) {
#pragma clang fp contract(off)
  double A[9], V[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) { A[k] = R[k]; V[k] = (k % 4 == 0) ? 1.0 : 0.0; }
  for (int sweep = 0; sweep < 30; ++sweep) {
    bool changed = false;
#pragma unroll
    for (int pq = 0; pq < 3; ++pq) {
      const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
      const double al = A[p] * A[p] + A[3 + p] * A[3 + p] + A[6 + p] * A[6 + p];
      const double be = A[q] * A[q] + A[3 + q] * A[3 + q] + A[6 + q] * A[6 + q];
      const double ga = A[p] * A[q] + A[3 + p] * A[3 + q] + A[6 + p] * A[6 + q];
      if (fabs(ga) <= 2.220446049250313e-16 * sqrt(al * be)) continue;  // also a zero column
      changed = true;
      const double zeta = (be - al) / (2.0 * ga);
      const double t = (zeta < 0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
      const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const double x = A[3 * i + p], y = A[3 * i + q];
        A[3 * i + p] = c * x - s * y;
        A[3 * i + q] = s * x + c * y;
        const double vx = V[3 * i + p], vy = V[3 * i + q];
        V[3 * i + p] = c * vx - s * vy;
        V[3 * i + q] = s * vx + c * vy;
      }
    }
    if (!changed) break;
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double n = sqrt(A[j] * A[j] + A[3 + j] * A[3 + j] + A[6 + j] * A[6 + j]);
    const double inv = n > 0 ? 1.0 / n : 0.0;
    A[j] *= inv; A[3 + j] *= inv; A[6 + j] *= inv;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k) R[3 * i + k] = A[3 * i] * V[3 * k] + A[3 * i + 1] * V[3 * k + 1] + A[3 * i + 2] * V[3 * k + 2];
}

// cv::Rodrigues (matrix -> vector) of the rotation block of a 4 x 4 float pose: OpenCV 3.x
// cvRodrigues2's 3 x 3 branch, all arithmetic in double, the vector rounded to float; the counterpart of
// pose_to_Tcw, the body of lorb_Tcw_to_pose, and on the device the motion-model prediction's
// Frame::UpdatePoseVector.  Contraction is off in the body as there; the orthogonalisation is
// polar_uvt3, and the device's double acos is not libm's function.
__host__ __device__ inline void Tcw_to_rvec(const float T[16], float rvec[3]) {
#pragma clang fp contract(off)
  double R[9];
  bool in_range = true;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    R[k] = (double)T[4 * (k / 3) + k % 3];
    in_range = in_range && R[k] >= -100.0 && R[k] < 100.0;  // cv::checkRange: false on NaN / inf too
  }
  double rx = 0, ry = 0, rz = 0;
  if (in_range) {
    polar_uvt3(R);
    rx = R[7] - R[5]; ry = R[2] - R[6]; rz = R[3] - R[1];
    const double s = sqrt((rx * rx + ry * ry + rz * rz) * 0.25);
    double c = (R[0] + R[4] + R[8] - 1) * 0.5;
    c = c > 1. ? 1. : c < -1. ? -1. : c;
    double theta = acos(c);
    if (s < 1e-5) {
      if (c > 0) {
        rx = 0; ry = 0; rz = 0;
      } else {
        double t = (R[0] + 1) * 0.5;
        rx = sqrt(t > 0. ? t : 0.);
        t = (R[4] + 1) * 0.5;
        ry = sqrt(t > 0. ? t : 0.) * (R[1] < 0 ? -1. : 1.);
        t = (R[8] + 1) * 0.5;
        rz = sqrt(t > 0. ? t : 0.) * (R[2] < 0 ? -1. : 1.);
        if (fabs(rx) < fabs(ry) && fabs(rx) < fabs(rz) && (R[5] > 0) != (ry * rz > 0)) rz = -rz;
        theta /= sqrt(rx * rx + ry * ry + rz * rz);
        rx *= theta; ry *= theta; rz *= theta;
      }
    } else {
      double vth = 1 / (2 * s);
      vth *= theta;
      rx *= vth; ry *= vth; rz *= vth;
    }
  }
  rvec[0] = (float)rx; rvec[1] = (float)ry; rvec[2] = (float)rz;
}

// C = A * B for 4 x 4 CV_32F through cv::gemm: float operands, double accumulation in k order, one
// rounding to float (the convention of the oracle's gemv3_row).  C may alias neither operand.
__host__ __device__ inline void gemm4_f32(const float* A, const float* B, float* C) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double s = (double)A[4 * i] * (double)B[j];
#pragma unroll
      for (int k = 1; k < 4; ++k) s += (double)A[4 * i + k] * (double)B[4 * k + j];
      C[4 * i + j] = (float)s;
    }
}

// a4's motion direction (src/matcher.cpp:74-87) from the two poses: Rcw / tcw of the current frame,
// twc = -Rcw^T * tcw, tlc = Rlw * twc + tlw (cv::gemm: double accumulation), its z against the
// baseline.  One definition for the host-pose calls (frame_params_a4) and the device-pose chain's
// first kernel (lorb_window.hip, compiled -ffp-contract=off; the pragma keeps it so anywhere else).
__host__ __device__ inline void a4_motion_direction(const float* cur_Tcw, const float* last_Tcw, float b, float Rcw[9],
                                                    float tcw[3], int* mode_forward, int* mode_backward) {
#pragma clang fp contract(off)
  const float* T = cur_Tcw;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) Rcw[3 * r + c] = T[4 * r + c];
    tcw[r] = T[4 * r + 3];
  }
  float twc[3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const double s = (double)Rcw[i] * tcw[0] + (double)Rcw[3 + i] * tcw[1] + (double)Rcw[6 + i] * tcw[2];
    twc[i] = (float)(-s);
  }
  const float* L = last_Tcw;
  const double s2 = (double)L[8] * twc[0] + (double)L[9] * twc[1] + (double)L[10] * twc[2];
  const float tlc2 = (float)(s2 + (double)L[11]);
  *mode_forward = tlc2 > b;
  *mode_backward = -tlc2 > b;
}

// The tail of the motion-tracking chain (lorb_track_motion*, lorb_window.hip): one launch of
// k_track_tail (lorb_ba.hip) after both a4 passes -- pass decision, final assign, residual
// compaction, pose-only LM, result record.  All pointers are device pointers.
struct TrackTail {
  int nk;
  const int *nm1, *nm2;          // the passes' match counts (nm2 is read only if the retry ran)
  const int *assign2;            // pass 2's codes (pass 1's are already in assign)
  int* assign;                   // nk: pass 1's codes on entry, the codes that count on exit
  const uint8_t* slot_state;     // null: all EMPTY
  const float *slot_pos, *last_pos, *x, *y;
  int min_matches;
  float fx, fy_eff, cx, cy, pose_init[6];
  float* list;                   // 5 floats per slot (point | observation): residuals past the
                                 // LM's register-resident ones
  lorb_track_motion_result* rec; // the record (device memory, or the mapped result block)
  int* assign_out;               // non-null: the final codes are also stored here (mapped block)
};
int launch_track_tail(lorb_ctx* ctx, const TrackTail& t, const lorb_lm_options* opt);

// The device-count form of the a4 chain (lorb_track_motion_frames_dev): the two keypoint counts live
// in device memory (entry 0 of each built frame's counts, the left side) and the host knows only the
// caller's bounds, which size every grid, stride and scratch buffer.  A kernel of that form reads both
// counts once, through wave-uniform (scalar) loads, and checks them before any other load.
struct FrameCounts {
  const int *last, *cur;
  int max_last, max_cur;
};
// false: a count is negative or above its bound (the chain's status 1: the kernel writes nothing)
__device__ __forceinline__ bool frame_counts(const FrameCounts& c, int* n_last, int* n_cur) {
  const int l = c.last[0], k = c.cur[0];
  *n_last = l;
  *n_cur = k;
  return l >= 0 && l <= c.max_last && k >= 0 && k <= c.max_cur;
}
// What k_track_frames_tail (lorb_ba.hip) has beyond k_track_tail: TrackTail::nk is read from the
// counts, and after the LM the codes that count are applied to the current frame's slots.
struct FramesTail {
  FrameCounts dc;
  lorb_frame_slots cur, last;
  int given;  // 0: the current slots are all EMPTY on entry, whatever the arrays hold
};
int launch_track_frames_tail(lorb_ctx* ctx, const TrackTail& t, const FramesTail& f, const lorb_lm_options* opt);

// The device-pose form of that chain (lorb_track_motion_frames_pose_dev).  Its first kernel
// (k_slots_fill's POSE form, lorb_window.hip) leaves this block in device memory; the candidate kernel
// and the tail read from it what the host-pose form bakes into their kernel arguments (WinParams::Rcw /
// tcw / mode_*, TrackTail::pose_init).  n_last is the last frame's count, or -1 when the call's status
// is 1: as FrameCounts::last of the later kernels it makes every one of them return on that status.
struct MotionPose {
  float Rcw[9], tcw[3], pose_init[6];
  int mode_forward, mode_backward, n_last;
};
// k_track_frames_tail_pose (lorb_ba.hip): k_track_frames_tail started from pose->pose_init
int launch_track_frames_tail_pose(lorb_ctx* ctx, const TrackTail& t, const FramesTail& f, const MotionPose* pose,
                                  const lorb_lm_options* opt);

// The id a current-frame slot holds after a motion stage, from that stage's final code for the slot:
// the rule of lorb_track_local_id_source, which is the rule the stage's tail applied to the slot itself.
// code >= 0: the id of source slot `code` (an index outside the table counts as -1); LORB_ASSIGN_NULL:
// -1; LORB_ASSIGN_UNCHANGED: the id the slot had (`id`) when `keep` -- pass 1 stood and the slots were
// given -- else -1.  One definition for k_local_head, k_lm_vote and both kernels of
// lorb_track_motion_refer_pose_dev.
__device__ __forceinline__ int motion_entry_id(int id, int code, bool keep, const int* src_id, int n_max_src) {
  if (code >= 0) return code < n_max_src ? src_id[code] : -1;
  if (code == LORB_ASSIGN_NULL || !keep) return -1;
  return id;
}

// The second motion attempt (lorb_track_motion_refer_pose_dev): what its tail has beyond
// k_track_frames_tail_pose -- the final codes applied to the current frame's slot ids with the refer
// frame's ids as the source.  cur_gid null: no id bookkeeping.
struct ReferGids {
  const int* refer_gid;
  int n_max_refer;
  int* cur_gid;
};
int launch_track_frames_tail_refer(lorb_ctx* ctx, const TrackTail& t, const FramesTail& f, const MotionPose* pose,
                                   const ReferGids& g, const lorb_lm_options* opt);

// The tail of the local-map tracking chain (lorb_track_local*, lorb_window.hip): one launch of
// k_local_tail (lorb_ba.hip) after a8 + a5 -- the in-view count, the nmatches > min_matches gate,
// residual compaction, pose-only LM, result record.  All pointers are device pointers.
struct LocalTail {
  int nk, np;
  const int* nm;                 // a5's match count
  const int* assign;             // nk: a5's codes
  const uint8_t* in_view;        // np: a8's flags
  const uint8_t* slot_state;     // null: all EMPTY
  const float *slot_pos, *pt_pos, *x, *y;
  int min_matches;
  float fx, fy_eff, cx, cy, pose_init[6];
  float* list;                   // as TrackTail::list
  lorb_track_local_result* rec;  // the record (device memory, or the mapped result block)
  int* assign_out;               // non-null: the codes are also stored here (mapped block)
};
int launch_local_tail(lorb_ctx* ctx, const LocalTail& t, const lorb_lm_options* opt);

// The device-count, device-pose form of the local-map chain (lorb_track_local_frames_dev).  Its first
// kernel (k_local_head, lorb_window.hip) leaves this block in device memory; the candidate kernel and
// the tail read the pose from it where the host-pose form reads FrustumIn::T / Ow and
// LocalTail::pose_init out of its kernel arguments.  np is d_pts->n, or -1 when the call's status is
// 1: as FrameCounts::last of the later kernels it makes every one of them return on that status.
struct LocalPose {
  float T[16], Ow[3], pose_in[6];
  int np;
};
// What k_local_frames_tail (lorb_ba.hip) has beyond k_local_tail: nk / np are read through dc, the
// LM starts from pose->pose_in, and after it the record's Tcw is written and the codes are applied to
// the frame's slots and their ids.
struct LocalFramesTail {
  FrameCounts dc;
  const LocalPose* pose;
  lorb_frame_slots cur;
  int* slot_id;
  const uint8_t *pt_locked, *pt_desc;
  lorb_track_local_frames_result* rec;
};
int launch_local_frames_tail(lorb_ctx* ctx, const LocalTail& t, const LocalFramesTail& f, const lorb_lm_options* opt);

// Device memory owned by one object (not a ctx scratch slot): add() every array, commit() allocates
// one block and sets the pointers (256-byte aligned, 16 spare bytes each as scratch_t gives).
struct Arena {
  struct Item { void** p; size_t off; };
  std::vector<Item> items;
  size_t total = 0;
  void* base = nullptr;
  template <typename T>
  void add(T** p, size_t count) {
    items.push_back({reinterpret_cast<void**>(p), total});
    total += (count * sizeof(T) + 16 + 255) & ~size_t(255);
  }
  hipError_t commit() {
    const hipError_t e = hipMalloc(&base, total ? total : 256);
    if (e != hipSuccess) { base = nullptr; return e; }
    for (const Item& it : items) *it.p = static_cast<unsigned char*>(base) + it.off;
    return hipSuccess;
  }
  void release() {
    if (base) (void)hipFree(base);
    base = nullptr;
  }
};

// The extractor over a stereo pair (lorb_orb.hip; used by lorb_frame.hip's builder): the plan and
// scratch of one geometry, and its 13 launches per frame on the ctx stream -- no host copy, no wait.
// The kernels and launch sites are the one-image entry points' (k_orb_copy, k_orb_resize, k_orb_fast,
// k_orb_octree, k_orb_gather, k_orb_blur, k_orb_desc), the image grid dimension at extent 2.
// Per image the outputs of lorb_orb_extract_dev; d_counts[2] receives {n_left, n_right} (-1: that
// image's quadtree overflowed its node capacity).
struct OrbPair;
struct OrbPairSide {
  uint8_t* pyramid;
  float *x, *y;
  int* octave;
  float *size, *angle, *response;
  uint8_t* desc;
  int* level_off;
};
int orb_pair_create(lorb_ctx* ctx, int rows, int cols, int n_levels, const float* sf, const int32_t* n_desired,
                    int ini_th, int min_th, const int32_t* pattern, OrbPair** out);
void orb_pair_destroy(OrbPair* B);
void orb_pair_info(const OrbPair* B, int* capacity, int64_t* pyr_bytes, lorb_image_pyramid* layout);
int orb_pair_enqueue(lorb_ctx* ctx, OrbPair* B, const uint8_t* d_img0, int step0, const uint8_t* d_img1, int step1,
                     const OrbPairSide& o0, const OrbPairSide& o1, int* d_counts);

// Frame::ComputeStereoMatches with the keypoint counts in device memory (lorb_stereo.hip): d_counts =
// {n_left, n_right}, each bounded by its side's capacity; a negative count makes both 0.  The three
// scratch arrays are the caller's: row_off (rows + 1), row_list (stereo_row_list_len), sad (left cap).
struct StereoSideDev {
  const float *x, *y;
  const int* octave;
  const uint8_t* desc;
  const uint8_t* pyramid;
  int capacity;
};
size_t stereo_row_list_len(const lorb_frame_params* fp, int right_capacity);
int enqueue_stereo_counts(lorb_ctx* ctx, const lorb_frame_params* fp, const lorb_image_pyramid* layout,
                          const StereoSideDev& L, const StereoSideDev& R, const int* d_counts, int* row_off,
                          int* row_list, int* sad, float* d_ur, float* d_dp);

// Four counters (plain POD: HIP's int4 member proxies are avoided in arithmetic-heavy code).
struct I4 {
  int v[4];
};

// Exclusive scan of four counters at once across an NT-thread workgroup; wsum: __shared__ I4[NT / 64].
template <int NT>
__device__ __forceinline__ I4 block_excl_scan4(const I4& v, I4* wsum, I4* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  I4 incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int u = __shfl_up(incl.v[q], o, 64);
      if (lane >= o) incl.v[q] += u;
    }
  }
  if (lane == 63) wsum[wv] = incl;
  __syncthreads();
  I4 pre = {{0, 0, 0, 0}}, tot = {{0, 0, 0, 0}};
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) {
    const I4 s = wsum[w];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      pre.v[q] += w < wv ? s.v[q] : 0;
      tot.v[q] += s.v[q];
    }
  }
  __syncthreads();
  *total = tot;
  I4 r;
#pragma unroll
  for (int q = 0; q < 4; ++q) r.v[q] = pre.v[q] + incl.v[q] - v.v[q];
  return r;
}

}  // namespace lorb

// Scratch slot plan: every family of ctx->scratch slots, declared once.  Calls on one ctx are
// serialized, so per-call families may share slots (the aliases below); a persistent slot keeps its
// contents from one API call to the next and is shared with nothing.
struct SlotFamily {
  int base, n;
  bool persistent;
};
// slots named one by one
enum {
  S_BF_Q = 0, S_BF_T, S_BF_TL, S_BF_TILES, S_BF_K1, S_BF_K2, S_BF_QKEY, S_BF_OUT0, S_BF_OUT1,
  S_BF_OUT2, S_BF_OUT3, S_BF_OUT4, S_BF_OUT5, S_BF_OFF,  // brute-force matcher
  S_W0 = 14, S_W1, S_W2, S_W3, S_W4, S_W5, S_W6, S_W7, S_W8, S_W9,  // frame-side calls; S_W9: candidate lists
  // persistent
  S_BF_TKEY = 120, /* crossCheck per-train keys: all-ones between calls (the merge resets them) */
  S_IO_IN = 121,   /* InPack device block */
  S_IO_OUT = 122,  /* OutPack device block */
  S_BF_DONE = 123, /* k_bf_cc1's workgroup counter: zero between calls (the last workgroup resets it) */
  S_TM_ZERO = 124  /* all-EMPTY slot states: zeroed when (re)allocated, never written (empty_slots) */
};
// families addressed by offset: slot<S_WX, 3>()
inline constexpr SlotFamily
    S_KP = {24, 10, false},   // keypoint grid of a search (7 .. 9; 0 .. 6 are free: the keypoints travel in the InPack)
    S_WX = {34, 8, false},    // windowed-matcher working buffers
    S_ST = {48, 15, false},   // stereo matcher
    S_ORB = {48, 50, false},  // ORB extractor.  Alias: over S_ST, S_TL, S_TM, S_TF and S_TLC -- no call runs two of them
    S_TL = {64, 20, false},   // lorb_track_local_map's staging.  Alias: inside S_ORB's range, as above
    S_TM = {88, 3, false},    // motion chain: pass 2's codes + both counts, the residual list, the host form's codes
    S_TF = {91, 1, false},    // frames chain (which also uses S_TM 0 and 1): the last frame's mp_locked flags
    S_TLC = {92, 6, false},   // local-map chain: match count, residual list; the host form's codes, in-view flags, fields, levels
    S_TLF = {98, 2, false},   // its frames form (which also uses S_TLC 0 and 1): the LocalPose block, the in_frame mask
    S_TP = {100, 1, false};   // the frames chain's device-pose form (which also uses S_TM 0 and 1 and S_TF): the MotionPose block
inline constexpr SlotFamily kSlotPlan[] = {
    {S_BF_Q, 14, false}, {S_W0, 10, false}, S_KP, S_WX, S_ST, S_ORB, S_TL, S_TM, S_TF, S_TLC, S_TLF, S_TP,
    {S_BF_TKEY, 1, true}, {S_IO_IN, 1, true}, {S_IO_OUT, 1, true}, {S_BF_DONE, 1, true}, {S_TM_ZERO, 1, true}};

// slot K of family F; an offset past the family's end does not compile
template <const SlotFamily& F, int K>
constexpr int slot() {
  static_assert(K >= 0 && K < F.n, "scratch slot offset outside its family");
  return F.base + K;
}
constexpr bool slot_plan_fits() {
  for (const SlotFamily& f : kSlotPlan)
    if (f.base < 0 || f.n < 1 || f.base + f.n > lorb_ctx::kScratch) return false;
  return true;
}
constexpr bool slot_plan_keeps_persistent() {  // no family's range contains a persistent slot of another
  for (const SlotFamily& p : kSlotPlan)
    for (const SlotFamily& f : kSlotPlan)
      if (p.persistent && &f != &p && f.base < p.base + p.n && p.base < f.base + f.n) return false;
  return true;
}
static_assert(S_BF_OFF == S_BF_Q + 13 && S_W9 == S_W0 + 9, "the named slots fill their families");
static_assert(slot_plan_fits(), "the scratch slot plan exceeds lorb_ctx::kScratch");
static_assert(slot_plan_keeps_persistent(), "a scratch family's range contains a persistent slot");
