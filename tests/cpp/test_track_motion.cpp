// tests/cpp/test_track_motion.cpp -- lorb::EstimatePoseMotion (include/lorb/adapters.hpp) driven
// as VisualOdometry::EstimatePoseMotion drives Matcher / BA (src/visual_odometry.cpp:124-137), on
// plain test frames, against the reference's three calls composed from the oracle in C:
// or_search_by_projection_frame at 15, the <= 20 rule, the same at 30 over emptied slots,
// or_ba_pose_only over the slots that hold a map point afterwards.  Three frame pairs: one where
// the first radius stands, one that retries, one that fails.  `oracle` as the only argument prints
// the oracle's branch of every pair and stops (no GPU needed).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/lorb/adapters.hpp"
#include "../../oracle/lorb_oracle.h"

struct TmPoint {
  float pos[3];
  uint8_t desc[32];
  size_t nobs = 0;
};
struct TmFrame {
  std::vector<float> x, y, angle, uR;
  std::vector<int> octave;
  std::vector<uint8_t> desc;
  std::vector<TmPoint*> mps;
  std::vector<bool> outlier;
  float Tcw[16];
  float rvec[3], tvec[3];
  lorb_frame_params fp;
};

namespace lorb {
template <> struct FrameTraits<TmFrame> {
  using point_type = TmPoint;
  static size_t num_keypoints(TmFrame* f) { return f->x.size(); }
  static void keypoint(TmFrame* f, size_t i, float* x, float* y, int* o, float* a) {
    *x = f->x[i]; *y = f->y[i]; *o = f->octave[i]; *a = f->angle[i];
  }
  static void descriptor(TmFrame* f, size_t i, uint8_t* d) { memcpy(d, &f->desc[32 * i], 32); }
  static bool has_right(TmFrame* f) { return !f->uR.empty(); }
  static float u_right(TmFrame* f, size_t i) { return f->uR[i]; }
  static TmPoint* map_point(TmFrame* f, size_t i) { return f->mps[i]; }
  static void set_map_point(TmFrame* f, size_t i, TmPoint* p) { f->mps[i] = p; }
  static bool outlier(TmFrame* f, size_t i) { return f->outlier[i]; }
  static void params(TmFrame* f, lorb_frame_params* fp) { *fp = f->fp; }
  static void Tcw(TmFrame* f, float* T) { memcpy(T, f->Tcw, sizeof(f->Tcw)); }
  static void pose_vectors(TmFrame* f, float* r, float* t) { memcpy(r, f->rvec, 12); memcpy(t, f->tvec, 12); }
  static void set_pose(TmFrame* f, const float* t, const float* r) {
    memcpy(f->rvec, r, 12); memcpy(f->tvec, t, 12);
    lorb_pose_to_Tcw(r, t, f->Tcw);
  }
};
template <> struct PointTraits<TmPoint> {
  static size_t num_obs(TmPoint* p) { return p->nobs; }
  static void descriptor(TmPoint* p, uint8_t* d) { memcpy(d, p->desc, 32); }
  static void pos(TmPoint* p, float* X) { memcpy(X, p->pos, 12); }
};
}  // namespace lorb

static uint64_t s_rng = 0x2545F4914F6CDD1Dull;
static uint32_t rnd() { s_rng ^= s_rng << 13; s_rng ^= s_rng >> 7; s_rng ^= s_rng << 17; return (uint32_t)(s_rng >> 11); }
static float urand(float a, float b) { return a + (b - a) * (float)(rnd() & 0xffffff) / 16777216.0f; }

static lorb_frame_params make_fp() {
  lorb_frame_params fp;
  memset(&fp, 0, sizeof(fp));
  fp.fx = fp.fy = 435.2f; fp.cx = 367.5f; fp.cy = 252.2f; fp.bf = 47.9f; fp.b = fp.bf / fp.fx;
  fp.min_x = 0; fp.max_x = 752; fp.min_y = 0; fp.max_y = 480;
  fp.grid_w_inv = 64.0f / 752.0f; fp.grid_h_inv = 48.0f / 480.0f;
  fp.n_levels = 8; fp.log_scale_factor = logf(1.2f);
  float s = 1.0f;
  for (int i = 0; i < 8; i++) { fp.scale_factors[i] = s; s *= 1.2f; }
  return fp;
}

static void project(const float* T, const float* X, const lorb_frame_params& fp, float* u, float* v) {
  float Xc[3];
  for (int r = 0; r < 3; r++) Xc[r] = T[4 * r] * X[0] + T[4 * r + 1] * X[1] + T[4 * r + 2] * X[2] + T[4 * r + 3];
  *u = fp.fx * Xc[0] / Xc[2] + fp.cx;
  *v = fp.fy * Xc[1] / Xc[2] + fp.cy;
}

static TmFrame* make_frame(int n, const float r[3], const float t[3]) {
  TmFrame* f = new TmFrame();
  f->fp = make_fp();
  memcpy(f->rvec, r, 12); memcpy(f->tvec, t, 12);
  lorb_pose_to_Tcw(r, t, f->Tcw);
  for (int i = 0; i < n; i++) {
    f->x.push_back(urand(0, 752)); f->y.push_back(urand(0, 480));
    f->angle.push_back(urand(0, 360)); f->octave.push_back((int)(rnd() % 8) < 4 ? 0 : (int)(rnd() % 8));
    f->uR.push_back(-1.0f);
    for (int b = 0; b < 32; b++) f->desc.push_back((uint8_t)rnd());
  }
  f->mps.assign(n, nullptr);
  f->outlier.assign(n, false);
  return f;
}

static int g_fail = 0;
#define EXPECT(c, ...) do { if (!(c)) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); g_fail++; } } while (0)

// the reference's EstimatePoseMotion body on a copy of cur's slots, from oracle calls
struct Want {
  std::vector<TmPoint*> slots;
  int pass, n1, n2;
  double pose[6];
};
static Want oracle_chain(TmFrame* cur, TmFrame* last) {
  const int N = (int)cur->x.size();
  const size_t nl = last->x.size();
  lorb::KeypointsSoA ks = lorb::gather_keypoints(cur);
  lorb_keypoints kv = ks.view();
  std::vector<uint8_t> st = lorb::gather_slot_state(cur), empty(N, LORB_SLOT_EMPTY);
  std::vector<uint8_t> has(nl), out(nl, 0), lk(nl), ld(32 * nl);
  std::vector<float> pos(3 * nl), ang(last->angle);
  std::vector<int32_t> oct(last->octave.begin(), last->octave.end());
  for (size_t i = 0; i < nl; i++) {
    TmPoint* p = last->mps[i];
    has[i] = p != nullptr;
    if (!p) continue;
    lk[i] = p->nobs > 0;
    memcpy(&pos[3 * i], p->pos, 12);
    memcpy(&ld[32 * i], p->desc, 32);
  }
  lorb_last_frame L{(int32_t)nl, last->Tcw, has.data(), out.data(), lk.data(), pos.data(), ld.data(), oct.data(), ang.data()};
  Want w;
  w.slots = cur->mps;
  std::vector<int32_t> assign(N);
  int32_t nm = 0;
  or_search_by_projection_frame(&cur->fp, cur->Tcw, &kv, st.data(), &L, 15.0f, assign.data(), &nm);
  w.n1 = nm; w.n2 = -1; w.pass = 1;
  if (nm <= 20) {
    std::fill(w.slots.begin(), w.slots.end(), (TmPoint*)nullptr);
    or_search_by_projection_frame(&cur->fp, cur->Tcw, &kv, empty.data(), &L, 30.0f, assign.data(), &nm);
    w.n2 = nm; w.pass = nm > 20 ? 2 : 0;
  }
  for (int j = 0; j < N; j++) {
    if (assign[j] == LORB_ASSIGN_NULL) w.slots[j] = nullptr;
    else if (assign[j] >= 0) w.slots[j] = last->mps[assign[j]];
  }
  float pinit[6];
  memcpy(pinit, cur->rvec, 12); memcpy(pinit + 3, cur->tvec, 12);
  for (int k = 0; k < 6; k++) w.pose[k] = pinit[k];
  if (w.pass) {
    std::vector<float> P3, P2;
    for (int j = 0; j < N; j++)
      if (w.slots[j]) { P3.insert(P3.end(), w.slots[j]->pos, w.slots[j]->pos + 3); P2.push_back(cur->x[j]); P2.push_back(cur->y[j]); }
    const float intr[4] = {cur->fp.fx, cur->fp.fx, cur->fp.cx, cur->fp.cy};
    const int32_t ro[2] = {0, (int32_t)(P2.size() / 2)};
    lorb_pose_problem_batch b{1, ro, intr, pinit, P3.data(), P2.data()};
    lorb_lm_options opt;
    lorb_lm_options_default(&opt);
    or_ba_pose_only(&b, &opt, w.pose, nullptr, nullptr);
  }
  return w;
}

int main(int argc, char** argv) {
  const bool oracle_only = argc > 1 && !strcmp(argv[1], "oracle");
  const int N = 600;
  const float r0[3] = {0, 0, 0}, t0[3] = {0, 0, 0};
  const float r1[3] = {0.01f, -0.005f, 0.002f}, t1[3] = {0.05f, 0.0f, 0.02f};
  TmFrame* last = make_frame(N, r0, t0);
  std::vector<TmPoint*> pts;
  std::vector<int> pts_kp;  // the point's keypoint in the last frame
  for (int i = 0; i < N; i++) {
    if (rnd() % 2) continue;
    TmPoint* p = new TmPoint();
    p->pos[0] = urand(-5, 5); p->pos[1] = urand(-3, 3); p->pos[2] = urand(2, 10);
    memcpy(p->desc, &last->desc[32 * i], 32);
    p->nobs = rnd() % 2;
    last->mps[i] = p;
    float u, v;
    project(last->Tcw, p->pos, last->fp, &u, &v);
    last->x[i] = u; last->y[i] = v;
    pts.push_back(p);
    pts_kp.push_back(i);
  }
  // the current frame at its true pose; every pair below starts from a copy with its own prediction
  TmFrame* truth = make_frame(N, r1, t1);
  int k = 0;
  for (size_t q = 0; q < pts.size(); q++) {
    TmPoint* p = pts[q];
    float u, v;
    project(truth->Tcw, p->pos, truth->fp, &u, &v);
    if (u < 0 || u >= 752 || v < 0 || v >= 480 || k >= N) continue;
    truth->x[k] = u + urand(-0.5f, 0.5f); truth->y[k] = v + urand(-0.5f, 0.5f);
    memcpy(&truth->desc[32 * k], p->desc, 32);
    truth->desc[32 * k + (rnd() % 32)] ^= (uint8_t)(1u << (rnd() % 8));
    // re-observed at the same pyramid level, rotated by a few degrees (a consistent rotation bin)
    truth->octave[k] = last->octave[pts_kp[q]];
    truth->angle[k] = fmodf(last->angle[pts_kp[q]] - urand(2, 8) + 360.0f, 360.0f);
    k++;
  }
  // slots already holding a point before the call (kept, overwritten or emptied by the first pass;
  // ignored by a retry): some locked, some free, at random keypoints
  std::vector<TmPoint*> held;
  for (int j = 0; j < N; j += 9) {
    TmPoint* p = new TmPoint();
    p->pos[0] = urand(-5, 5); p->pos[1] = urand(-3, 3); p->pos[2] = urand(2, 10);
    for (int b = 0; b < 32; b++) p->desc[b] = (uint8_t)rnd();
    p->nobs = rnd() % 2;
    truth->mps[j] = p;
    held.push_back(p);
  }

  struct Pair { const char* name; float dx; int pass; };
  const Pair pairs[3] = {{"no retry", 0.0f, 1}, {"retry", 0.7f, 2}, {"failing", 3.0f, 0}};
  lorb_ctx* ctx = oracle_only ? nullptr : lorb::thread_ctx(0);
  for (const Pair& pr : pairs) {
    TmFrame cur = *truth;  // the motion model's prediction: the true pose shifted along x
    const float tp[3] = {t1[0] + pr.dx, t1[1], t1[2]};
    memcpy(cur.tvec, tp, 12);
    lorb_pose_to_Tcw(cur.rvec, cur.tvec, cur.Tcw);
    const Want w = oracle_chain(&cur, last);
    EXPECT(w.pass == pr.pass, "%s: the oracle takes pass %d (%d -> %d matches), the pair is built for %d", pr.name,
           w.pass, w.n1, w.n2, pr.pass);
    printf("%s: oracle %d -> %d matches, pass %d\n", pr.name, w.n1, w.n2, w.pass);
    if (oracle_only) continue;
    size_t nm = 0;
    const bool ok = lorb::EstimatePoseMotion(ctx, &cur, last, &nm);
    EXPECT(ok == (w.pass != 0), "%s: returned %d", pr.name, (int)ok);
    EXPECT((int)nm == (w.pass == 1 ? w.n1 : w.n2), "%s: nMatches %zu", pr.name, nm);
    int mism = 0;
    for (int j = 0; j < N; j++)
      if (cur.mps[j] != w.slots[j]) mism++;
    EXPECT(mism == 0, "%s: %d slot mismatches", pr.name, mism);
    double md = 0;
    for (int i = 0; i < 3; i++) {
      md = std::max(md, (double)fabsf(cur.rvec[i] - (float)w.pose[i]) / std::max(1.0, fabs(w.pose[i])));
      md = std::max(md, (double)fabsf(cur.tvec[i] - (float)w.pose[3 + i]) / std::max(1.0, fabs(w.pose[3 + i])));
    }
    EXPECT(md <= 1e-5, "%s: pose rel diff %g", pr.name, md);
    if (w.pass == 0) EXPECT(md == 0.0, "%s: a failing pair must leave the pose as predicted", pr.name);
    printf("%s: EstimatePoseMotion -> %d, %zu matches, t = %.5f %.5f %.5f (max rel diff %.2e)\n", pr.name, (int)ok, nm,
           cur.tvec[0], cur.tvec[1], cur.tvec[2], md);
  }
  printf(g_fail ? "RESULT FAIL (%d)\n" : "RESULT PASS\n", g_fail);
  return g_fail ? 1 : 0;
}
