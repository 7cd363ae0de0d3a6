// tests/cpp/test_track_local.cpp -- lorb::EstimatePoseLocal (include/lorb/adapters.hpp) driven as
// VisualOdometry::EstimatePoseLocal runs after UpdateLocalMap (src/visual_odometry.cpp:149-209), on
// plain test frames, against the reference's sequence composed from the oracle in C: the held-slot
// loop, or_is_in_frustum for every point neither in the frame nor bad, or_search_by_projection_local
// at th 1, the <= 20 gate, or_ba_pose_only over the slots that hold a map point afterwards.  Three
// frames: one that passes, one that fails the gate, one with bad held points whose slots must come
// out NULL.  `oracle` as the only argument prints the oracle's branch of every frame and stops (no
// GPU needed).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <vector>

#include "../../include/lorb/adapters.hpp"
#include "../../oracle/lorb_oracle.h"

struct TlPoint {
  float pos[3], normal[3], maxd, mind;
  uint8_t desc[32];
  size_t nobs = 0, last_seen = 0;
  bool bad = false;
  int visible = 1;
  bool in_view = false;  // mbTrackInView and the tracking fields
  float track[4] = {0, 0, 0, 0};
  int level = 0;
};
struct TlFrame {
  size_t id = 7;
  std::vector<float> x, y, angle, uR;
  std::vector<int> octave;
  std::vector<uint8_t> desc;
  std::vector<TlPoint*> mps;
  float Tcw[16];
  float rvec[3], tvec[3];
  lorb_frame_params fp;
};

namespace lorb {
template <> struct FrameTraits<TlFrame> {
  using point_type = TlPoint;
  static size_t num_keypoints(TlFrame* f) { return f->x.size(); }
  static void keypoint(TlFrame* f, size_t i, float* x, float* y, int* o, float* a) {
    *x = f->x[i]; *y = f->y[i]; *o = f->octave[i]; *a = f->angle[i];
  }
  static void descriptor(TlFrame* f, size_t i, uint8_t* d) { memcpy(d, &f->desc[32 * i], 32); }
  static bool has_right(TlFrame* f) { return !f->uR.empty(); }
  static float u_right(TlFrame* f, size_t i) { return f->uR[i]; }
  static TlPoint* map_point(TlFrame* f, size_t i) { return f->mps[i]; }
  static void set_map_point(TlFrame* f, size_t i, TlPoint* p) { f->mps[i] = p; }
  static void params(TlFrame* f, lorb_frame_params* fp) { *fp = f->fp; }
  static void Tcw(TlFrame* f, float* T) { memcpy(T, f->Tcw, sizeof(f->Tcw)); }
  static void pose_vectors(TlFrame* f, float* r, float* t) { memcpy(r, f->rvec, 12); memcpy(t, f->tvec, 12); }
  static void set_pose(TlFrame* f, const float* t, const float* r) {
    memcpy(f->rvec, r, 12); memcpy(f->tvec, t, 12);
    lorb_pose_to_Tcw(r, t, f->Tcw);
  }
  static size_t id(TlFrame* f) { return f->id; }
};
template <> struct PointTraits<TlPoint> {
  static size_t num_obs(TlPoint* p) { return p->nobs; }
  static void descriptor(TlPoint* p, uint8_t* d) { memcpy(d, p->desc, 32); }
  static void pos(TlPoint* p, float* X) { memcpy(X, p->pos, 12); }
  static bool is_bad(TlPoint* p) { return p->bad; }
  static void normal(TlPoint* p, float* n) { memcpy(n, p->normal, 12); }
  static void distances(TlPoint* p, float* mx, float* mn) { *mx = p->maxd; *mn = p->mind; }
  static size_t last_frame_seen(TlPoint* p) { return p->last_seen; }
  static void set_last_frame_seen(TlPoint* p, size_t id) { p->last_seen = id; }
  static void set_tracking(TlPoint* p, bool in_view, const float* t, int level) {
    p->in_view = in_view;
    if (in_view) { memcpy(p->track, t, 16); p->level = level; }
  }
  static void increase_visible(TlPoint* p) { p->visible++; }
};
}  // namespace lorb

static uint64_t s_rng = 0x9E3779B97F4A7C15ull;
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

static int g_fail = 0;
#define EXPECT(c, ...) do { if (!(c)) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); g_fail++; } } while (0)

// what the reference's EstimatePoseLocal leaves behind, from oracle calls (nothing is modified)
struct Want {
  std::vector<TlPoint*> slots;
  std::map<TlPoint*, TlPoint> pts;  // every local point's state afterwards
  bool ok;
  int nm, n_in_view;
  double pose[6];
};
static Want oracle_chain(TlFrame* F, const std::set<TlPoint*>& local) {
  const int N = (int)F->x.size();
  Want w;
  w.slots = F->mps;
  for (TlPoint* p : local) w.pts[p] = *p;
  std::map<TlPoint*, TlPoint> held;  // held points need not be local points
  for (int j = 0; j < N; j++)
    if (TlPoint* p = w.slots[j]) held.emplace(p, *p);
  auto state = [&](TlPoint* p) -> TlPoint& { return w.pts.count(p) ? w.pts[p] : held[p]; };
  for (int j = 0; j < N; j++) {  // src/visual_odometry.cpp:153-171
    TlPoint* p = w.slots[j];
    if (!p) continue;
    if (p->bad) { w.slots[j] = nullptr; continue; }
    TlPoint& s = state(p);
    s.visible++; s.last_seen = F->id; s.in_view = false;
  }
  std::vector<TlPoint*> mps(local.begin(), local.end());
  const size_t n = mps.size();
  std::vector<float> pos(3 * n + 3), nrm(3 * n + 3), maxd(n + 1), mind(n + 1), px(n + 1), py(n + 1), pxr(n + 1), vc(n + 1);
  std::vector<uint8_t> iv(n + 1), bad(n + 1), lk(n + 1), desc(32 * n + 32);
  std::vector<int32_t> lev(n + 1);
  for (size_t i = 0; i < n; i++) {
    memcpy(&pos[3 * i], mps[i]->pos, 12); memcpy(&nrm[3 * i], mps[i]->normal, 12);
    maxd[i] = mps[i]->maxd; mind[i] = mps[i]->mind;
    memcpy(&desc[32 * i], mps[i]->desc, 32);
    bad[i] = mps[i]->bad; lk[i] = mps[i]->nobs > 0;
  }
  lorb_frustum_points fr{(int32_t)n, pos.data(), nrm.data(), maxd.data(), mind.data()};
  or_is_in_frustum(&F->fp, F->Tcw, &fr, 0.5f, iv.data(), px.data(), py.data(), pxr.data(), lev.data(), vc.data());
  w.n_in_view = 0;
  for (size_t i = 0; i < n; i++) {  // :176-195
    TlPoint& s = w.pts[mps[i]];
    if (s.last_seen == F->id || s.bad) { iv[i] = 0; continue; }
    s.in_view = iv[i] != 0;
    if (iv[i]) {
      s.track[0] = px[i]; s.track[1] = py[i]; s.track[2] = pxr[i]; s.track[3] = vc[i]; s.level = lev[i];
      s.visible++;
      w.n_in_view++;
    }
  }
  w.nm = 0;
  if (w.n_in_view > 0) {  // :197-202
    lorb::KeypointsSoA ks = lorb::gather_keypoints(F);
    lorb_keypoints kv = ks.view();
    std::vector<uint8_t> st(N, LORB_SLOT_EMPTY);
    for (int j = 0; j < N; j++)
      if (w.slots[j]) st[j] = w.slots[j]->nobs > 0 ? LORB_SLOT_LOCKED : LORB_SLOT_FREE;
    lorb_local_points L;
    L.n = (int32_t)n; L.track_in_view = iv.data(); L.is_bad = bad.data(); L.locked = lk.data();
    L.proj_x = px.data(); L.proj_y = py.data(); L.proj_xr = pxr.data(); L.pred_level = lev.data();
    L.view_cos = vc.data(); L.desc = desc.data();
    std::vector<int32_t> assign(N + 1);
    int32_t nm = 0;
    or_search_by_projection_local(&F->fp, &kv, st.data(), &L, 1.0f, assign.data(), &nm);
    w.nm = nm;
    for (int j = 0; j < N; j++)
      if (assign[j] >= 0) w.slots[j] = mps[assign[j]];
  }
  float pinit[6];
  memcpy(pinit, F->rvec, 12); memcpy(pinit + 3, F->tvec, 12);
  for (int k = 0; k < 6; k++) w.pose[k] = pinit[k];
  w.ok = w.nm > 20;  // :204-205
  if (w.ok) {
    std::vector<float> P3, P2;
    for (int j = 0; j < N; j++)
      if (w.slots[j]) { P3.insert(P3.end(), w.slots[j]->pos, w.slots[j]->pos + 3); P2.push_back(F->x[j]); P2.push_back(F->y[j]); }
    const float intr[4] = {F->fp.fx, F->fp.fx, F->fp.cx, F->fp.cy};
    const int32_t ro[2] = {0, (int32_t)(P2.size() / 2)};
    lorb_pose_problem_batch b{1, ro, intr, pinit, P3.data(), P2.data()};
    lorb_lm_options opt;
    lorb_lm_options_default(&opt);
    or_ba_pose_only(&b, &opt, w.pose, nullptr, nullptr);
  }
  return w;
}

// a point seen from the camera at Xc (camera coordinates) under T
static TlPoint* make_point(const float* T, const float* Xc) {
  TlPoint* p = new TlPoint();
  float Ow[3], d[3];
  for (int c = 0; c < 3; c++) {  // world = R^T (Xc - t), Ow = -R^T t
    p->pos[c] = T[c] * (Xc[0] - T[3]) + T[4 + c] * (Xc[1] - T[7]) + T[8 + c] * (Xc[2] - T[11]);
    Ow[c] = -(T[c] * T[3] + T[4 + c] * T[7] + T[8 + c] * T[11]);
  }
  for (int c = 0; c < 3; c++) d[c] = p->pos[c] - Ow[c];
  const float dist = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  for (int c = 0; c < 3; c++) p->normal[c] = d[c] / dist;
  p->maxd = dist * urand(1.0f, 3.0f);
  p->mind = p->maxd / 3.5831808f;  // 1.2^7
  for (int b = 0; b < 32; b++) p->desc[b] = (uint8_t)rnd();
  p->nobs = rnd() % 4 ? 1 : 0;
  return p;
}

int main(int argc, char** argv) {
  const bool oracle_only = argc > 1 && !strcmp(argv[1], "oracle");
  const int N = 600, M = 1000;
  const float r1[3] = {0.01f, -0.005f, 0.002f}, t1[3] = {0.05f, 0.0f, 0.02f};
  TlFrame* truth = new TlFrame();
  truth->fp = make_fp();
  memcpy(truth->rvec, r1, 12); memcpy(truth->tvec, t1, 12);
  lorb_pose_to_Tcw(r1, t1, truth->Tcw);
  for (int i = 0; i < N; i++) {
    truth->x.push_back(urand(0, 752)); truth->y.push_back(urand(0, 480));
    truth->angle.push_back(urand(0, 360)); truth->octave.push_back((int)(rnd() % 8));
    truth->uR.push_back(-1.0f);
    for (int b = 0; b < 32; b++) truth->desc.push_back((uint8_t)rnd());
  }
  truth->mps.assign(N, nullptr);
  // local map points: most in front of the camera, some behind it or outside the image; every
  // third one in view is re-observed by a keypoint at its projection, at its predicted level
  std::set<TlPoint*> local;
  std::vector<TlPoint*> all;
  int k = 0;
  for (int i = 0; i < M; i++) {
    const float Xc[3] = {urand(-6, 6), urand(-4, 4), urand(-1, 12)};
    TlPoint* p = make_point(truth->Tcw, Xc);
    if (rnd() % 50 == 0) p->bad = true;
    local.insert(p);
    all.push_back(p);
    const float u = truth->fp.fx * Xc[0] / Xc[2] + truth->fp.cx, v = truth->fp.fy * Xc[1] / Xc[2] + truth->fp.cy;
    if (Xc[2] < 0.5f || u < 1 || u > 751 || v < 1 || v > 479 || i % 3 || k >= N) continue;
    const float dist = sqrtf(Xc[0] * Xc[0] + Xc[1] * Xc[1] + Xc[2] * Xc[2]);
    const int lev = std::min(7, std::max(0, (int)ceilf(logf(p->maxd / dist) / logf(1.2f))));
    truth->x[k] = u + urand(-0.5f, 0.5f); truth->y[k] = v + urand(-0.5f, 0.5f);
    truth->octave[k] = std::max(0, lev - (int)(rnd() % 2));
    memcpy(&truth->desc[32 * k], p->desc, 32);
    for (int f = 0; f < 6; f++) truth->desc[32 * k + (rnd() % 32)] ^= (uint8_t)(1u << (rnd() % 8));
    k += 2;  // the odd keypoints stay random
  }
  // slots stage 1 filled: every 9th keypoint holds a point of its own (some of them local points
  // too, one of them twice), locked or free; the third frame marks some of them bad
  std::vector<TlPoint*> held;
  for (int j = 1; j < N; j += 9) {
    const float z = urand(2, 10);
    const float Xc[3] = {(truth->x[j] - truth->fp.cx) / truth->fp.fx * z, (truth->y[j] - truth->fp.cy) / truth->fp.fy * z, z};
    TlPoint* p = make_point(truth->Tcw, Xc);
    truth->mps[j] = p;
    held.push_back(p);
    if (held.size() % 4 == 0) local.insert(p);
  }
  truth->mps[5] = held[3];  // one point in two slots: IncreaseVisible twice (:165)
  all.insert(all.end(), held.begin(), held.end());
  std::vector<TlPoint> snapshot;
  for (TlPoint* p : all) snapshot.push_back(*p);

  struct Case { const char* name; float dx; bool bad_held; bool ok; };
  const Case cases[3] = {{"passes", 0.0f, false, true}, {"fails the gate", 0.3f, false, false},
                         {"bad held slots", 0.0f, true, true}};
  lorb_ctx* ctx = oracle_only ? nullptr : lorb::thread_ctx(0);
  for (const Case& c : cases) {
    for (size_t i = 0; i < all.size(); i++) *all[i] = snapshot[i];
    if (c.bad_held)
      for (size_t i = 0; i < held.size(); i += 3) held[i]->bad = true;  // held[3] among them: both its slots
    TlFrame cur = *truth;  // the pose stage 1 left: the true pose shifted along x
    const float tp[3] = {t1[0] + c.dx, t1[1], t1[2]};
    memcpy(cur.tvec, tp, 12);
    lorb_pose_to_Tcw(cur.rvec, cur.tvec, cur.Tcw);
    const Want w = oracle_chain(&cur, local);
    EXPECT(w.ok == c.ok, "%s: the oracle finds %d matches, the frame is built to %s", c.name, w.nm, c.ok ? "pass" : "fail");
    int kept = 0, nulled = 0;
    for (int j = 0; j < N; j++) {
      if (truth->mps[j] && w.slots[j] == truth->mps[j]) kept++;
      if (truth->mps[j] && !w.slots[j]) nulled++;
    }
    printf("%s: oracle %d in view, %d matches, ok %d, %d held slots kept, %d emptied\n", c.name, w.n_in_view, w.nm,
           (int)w.ok, kept, nulled);
    if (c.bad_held) EXPECT(nulled >= 2 && !w.slots[5], "%s: the bad held points' slots must be emptied", c.name);
    if (oracle_only) continue;
    size_t nm = 0;
    const bool ok = lorb::EstimatePoseLocal(ctx, &cur, local, &nm);
    EXPECT(ok == w.ok, "%s: returned %d", c.name, (int)ok);
    EXPECT((int)nm == w.nm, "%s: nMatches %zu, the oracle's %d", c.name, nm, w.nm);
    int mism = 0;
    for (int j = 0; j < N; j++)
      if (cur.mps[j] != w.slots[j]) mism++;
    EXPECT(mism == 0, "%s: %d slot mismatches", c.name, mism);
    int vis = 0, seen = 0, trk = 0;
    for (const auto& kv : w.pts) {
      const TlPoint *g = kv.first, *e = &kv.second;
      if (g->visible != e->visible) vis++;
      if (g->last_seen != e->last_seen) seen++;
      if (g->in_view != e->in_view || (e->in_view && (memcmp(g->track, e->track, 16) || g->level != e->level))) trk++;
    }
    EXPECT(vis == 0, "%s: %d IncreaseVisible counts differ", c.name, vis);
    EXPECT(seen == 0, "%s: %d mnLastFrameSeen differ", c.name, seen);
    EXPECT(trk == 0, "%s: %d points' tracking fields differ", c.name, trk);
    for (TlPoint* p : held)
      if (!w.pts.count(p)) {
        const int e = p->bad ? 1 : 2 + (p == held[3]);
        EXPECT(p->visible == e && p->last_seen == (p->bad ? 0 : cur.id), "%s: a held point's counts", c.name);
      }
    double md = 0;
    for (int i = 0; i < 3; i++) {
      md = std::max(md, (double)fabsf(cur.rvec[i] - (float)w.pose[i]) / std::max(1.0, fabs(w.pose[i])));
      md = std::max(md, (double)fabsf(cur.tvec[i] - (float)w.pose[3 + i]) / std::max(1.0, fabs(w.pose[3 + i])));
    }
    EXPECT(md <= 1e-5, "%s: pose rel diff %g", c.name, md);
    if (!w.ok) EXPECT(md == 0.0, "%s: a failing frame must leave the pose as it was", c.name);
    printf("%s: EstimatePoseLocal -> %d, %zu matches, t = %.5f %.5f %.5f (max rel diff %.2e)\n", c.name, (int)ok, nm,
           cur.tvec[0], cur.tvec[1], cur.tvec[2], md);
  }
  printf(g_fail ? "RESULT FAIL (%d)\n" : "RESULT PASS\n", g_fail);
  return g_fail ? 1 : 0;
}
