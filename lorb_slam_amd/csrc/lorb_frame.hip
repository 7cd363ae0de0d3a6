// lorb_frame.hip -- the stereo Frame constructor, Frame::Frame(imgLeft, imgRight, camera)
// (src/frame.cpp:17-63), as one device-resident call: ORBextractor::operator() on both images
// (:42-45), UndistortKeyPoints (:358-362, a copy) and ComputeStereoMatches (:125-333).
//
// The builder (lorb_frame_builder) holds what depends only on the geometry: lorb_orb.hip's OrbPair
// (pyramid layout, resize taps, FAST cells, quadtree plan, blur tiles, pattern, the scratch of both
// images) and the stereo stage's row table, row lists and SAD array -- all in memory of its own.
// A frame is then lorb::orb_pair_enqueue (13 launches, the image as a grid dimension) followed by
// lorb::enqueue_stereo_counts (3 launches reading {n_left, n_right} from device memory): no stream
// synchronise, no device-to-host read, no host-to-device copy.  The kernels live in the units that
// launch them (lorb_orb.hip, lorb_stereo.hip); this unit has none of its own.
//
// The host-array form stages both images through one pinned block (one host-to-device copy), runs
// the same launches into a block of the builder's, and fetches that block with one copy and one wait.
#include <algorithm>

#include "lorb_internal.h"

struct lorb_frame_builder {
  lorb_ctx* ctx = nullptr;
  lorb_frame_config cfg{};
  lorb::OrbPair* orb = nullptr;
  lorb_image_pyramid layout{};
  int cap = 0;
  int64_t pyr_bytes = 0;
  // stereo scratch
  lorb::Arena scratch;
  int *row_off = nullptr, *row_list = nullptr, *sad = nullptr;
  // host form: device staging of the two images (packed, step = cols), the two pyramids, and the
  // output block with its pinned mirror
  uint8_t* d_img = nullptr;
  uint8_t* d_pyr[2] = {};
  lorb::Arena outs;
  lorb_frame_out d_out{};
  void* h_in = nullptr;
  void* h_out = nullptr;
};

namespace {

int check_side(const lorb_frame_side& s) {
  return s.x && s.y && s.octave && s.size && s.angle && s.response && s.desc && s.level_off;
}

lorb::OrbPairSide side_of(const lorb_frame_side& s) {
  return lorb::OrbPairSide{s.pyramid, s.x, s.y, s.octave, s.size, s.angle, s.response, s.desc, s.level_off};
}

int enqueue_frame(lorb_frame_builder* B, const uint8_t* d_left, int left_step, const uint8_t* d_right, int right_step,
                  const lorb_frame_out& o) {
  lorb_ctx* ctx = B->ctx;
  LORB_TRY(lorb::orb_pair_enqueue(ctx, B->orb, d_left, left_step, d_right, right_step, side_of(o.left), side_of(o.right),
                                  o.counts));
  const lorb::StereoSideDev L{o.left.x, o.left.y, o.left.octave, o.left.desc, o.left.pyramid, B->cap};
  const lorb::StereoSideDev R{o.right.x, o.right.y, o.right.octave, o.right.desc, o.right.pyramid, B->cap};
  return lorb::enqueue_stereo_counts(ctx, &B->cfg.frame, &B->layout, L, R, o.counts, B->row_off, B->row_list, B->sad,
                                     o.u_right, o.depth);
}

void add_side(lorb::Arena& M, lorb_frame_side& s, size_t cap) {
  M.add(&s.x, cap); M.add(&s.y, cap); M.add(&s.octave, cap); M.add(&s.size, cap); M.add(&s.angle, cap);
  M.add(&s.response, cap); M.add(&s.desc, cap * 32); M.add(&s.level_off, (size_t)LORB_MAX_LEVELS + 1);
}

// the host address mirroring device address d of the output block
template <typename T>
const T* mirror(const lorb_frame_builder* B, const T* d) {
  return reinterpret_cast<const T*>(static_cast<const unsigned char*>(B->h_out) +
                                    (reinterpret_cast<const unsigned char*>(d) -
                                     static_cast<const unsigned char*>(B->outs.base)));
}

void pack_image(uint8_t* dst, const uint8_t* src, int rows, int cols, int step) {
  if (step == cols) { std::memcpy(dst, src, (size_t)rows * cols); return; }
  for (int r = 0; r < rows; r++) std::memcpy(dst + (size_t)r * cols, src + (size_t)r * step, (size_t)cols);
}

void fetch_side(const lorb_frame_builder* B, const lorb_frame_side& d, const lorb_frame_side& h, int n, int n_levels) {
  std::memcpy(h.level_off, mirror(B, d.level_off), sizeof(int32_t) * (n_levels + 1));
  if (n <= 0) return;
  std::memcpy(h.x, mirror(B, d.x), sizeof(float) * n);
  std::memcpy(h.y, mirror(B, d.y), sizeof(float) * n);
  std::memcpy(h.octave, mirror(B, d.octave), sizeof(int32_t) * n);
  std::memcpy(h.size, mirror(B, d.size), sizeof(float) * n);
  std::memcpy(h.angle, mirror(B, d.angle), sizeof(float) * n);
  std::memcpy(h.response, mirror(B, d.response), sizeof(float) * n);
  std::memcpy(h.desc, mirror(B, d.desc), (size_t)32 * n);
}

}  // namespace

extern "C" {

int lorb_frame_builder_destroy(lorb_frame_builder* B) {
  if (!B) return LORB_E_INVALID;
  lorb::orb_pair_destroy(B->orb);
  B->scratch.release();
  B->outs.release();
  if (B->h_in) (void)hipHostFree(B->h_in);
  if (B->h_out) (void)hipHostFree(B->h_out);
  delete B;
  return LORB_OK;
}

int lorb_frame_builder_create(lorb_ctx* ctx, const lorb_frame_config* cfg, lorb_frame_builder** out) {
  if (!ctx) return LORB_E_INVALID;
  if (!cfg || !out) return lorb::set_error(ctx, LORB_E_INVALID, "null config / output");
  *out = nullptr;
  if (!cfg->pattern) return lorb::set_error(ctx, LORB_E_INVALID, "null pattern");
  const int nl = cfg->frame.n_levels;
  if (cfg->rows < 1 || cfg->cols < 1 || nl < 1 || nl > LORB_MAX_LEVELS)
    return lorb::set_error(ctx, LORB_E_INVALID, "bad image size %d x %d / n_levels %d", cfg->rows, cfg->cols, nl);
  if (cfg->rows > 4096)
    return lorb::set_error(ctx, LORB_E_INVALID, "image rows %d > 4096 (the stereo row table)", cfg->rows);
  lorb_frame_builder* B = new (std::nothrow) lorb_frame_builder;
  if (!B) return lorb::set_error(ctx, LORB_E_NOMEM, "out of host memory");
  struct Guard {
    lorb_frame_builder* b;
    ~Guard() { if (b) lorb_frame_builder_destroy(b); }
  } guard{B};
  B->ctx = ctx;
  B->cfg = *cfg;
  B->cfg.pattern = nullptr;  // copied to the device by orb_pair_create; the caller's pointer is not kept
  LORB_TRY(lorb::orb_pair_create(ctx, cfg->rows, cfg->cols, nl, cfg->frame.scale_factors, cfg->n_desired, cfg->ini_th,
                                 cfg->min_th, cfg->pattern, &B->orb));
  lorb::orb_pair_info(B->orb, &B->cap, &B->pyr_bytes, &B->layout);
  const size_t cap = (size_t)std::max(B->cap, 1), img = (size_t)cfg->rows * cfg->cols;
  B->scratch.add(&B->row_off, (size_t)cfg->rows + 1);
  B->scratch.add(&B->row_list, lorb::stereo_row_list_len(&B->cfg.frame, B->cap));
  B->scratch.add(&B->sad, cap);
  B->scratch.add(&B->d_img, 2 * img);
  B->scratch.add(&B->d_pyr[0], (size_t)B->pyr_bytes);
  B->scratch.add(&B->d_pyr[1], (size_t)B->pyr_bytes);
  LORB_HIP(ctx, B->scratch.commit());
  add_side(B->outs, B->d_out.left, cap);
  add_side(B->outs, B->d_out.right, cap);
  B->outs.add(&B->d_out.u_right, cap);
  B->outs.add(&B->d_out.depth, cap);
  B->outs.add(&B->d_out.counts, (size_t)2);
  LORB_HIP(ctx, B->outs.commit());
  B->d_out.left.pyramid = B->d_pyr[0];
  B->d_out.right.pyramid = B->d_pyr[1];
  LORB_HIP(ctx, hipHostMalloc(&B->h_in, 2 * img, hipHostMallocDefault));
  LORB_HIP(ctx, hipHostMalloc(&B->h_out, B->outs.total, hipHostMallocDefault));
  guard.b = nullptr;
  *out = B;
  return LORB_OK;
}

int lorb_frame_builder_capacity(const lorb_frame_builder* B, int32_t* max_keypoints, int64_t* pyramid_bytes) {
  if (!B || !max_keypoints) return LORB_E_INVALID;
  *max_keypoints = B->cap;
  if (pyramid_bytes) *pyramid_bytes = B->pyr_bytes;
  return LORB_OK;
}

int lorb_frame_build_dev(lorb_frame_builder* B, const uint8_t* d_left, int32_t left_step, const uint8_t* d_right,
                         int32_t right_step, const lorb_frame_out* o) {
  if (!B) return LORB_E_INVALID;
  lorb_ctx* ctx = B->ctx;
  if (!d_left || !d_right || !o) return lorb::set_error(ctx, LORB_E_INVALID, "null image / output struct");
  if (left_step < B->cfg.cols || right_step < B->cfg.cols)
    return lorb::set_error(ctx, LORB_E_INVALID, "image step %d / %d below cols %d", left_step, right_step, B->cfg.cols);
  if (!check_side(o->left) || !check_side(o->right) || !o->left.pyramid || !o->right.pyramid || !o->u_right ||
      !o->depth || !o->counts)
    return lorb::set_error(ctx, LORB_E_INVALID, "null output array");
  return enqueue_frame(B, d_left, left_step, d_right, right_step, *o);
}

int lorb_frame_build(lorb_frame_builder* B, const uint8_t* left, int32_t left_step, const uint8_t* right,
                     int32_t right_step, int32_t max_keypoints, const lorb_frame_out* o) {
  if (!B) return LORB_E_INVALID;
  lorb_ctx* ctx = B->ctx;
  if (!left || !right || !o || max_keypoints < 0)
    return lorb::set_error(ctx, LORB_E_INVALID, "null image / output struct");
  const int rows = B->cfg.rows, cols = B->cfg.cols, nl = B->cfg.frame.n_levels;
  if (left_step < cols || right_step < cols)
    return lorb::set_error(ctx, LORB_E_INVALID, "image step %d / %d below cols %d", left_step, right_step, cols);
  if (!o->counts || !o->left.level_off || !o->right.level_off ||
      (max_keypoints > 0 && (!check_side(o->left) || !check_side(o->right) || !o->u_right || !o->depth)))
    return lorb::set_error(ctx, LORB_E_INVALID, "null output array");
  const size_t img = (size_t)rows * cols;
  uint8_t* hin = static_cast<uint8_t*>(B->h_in);
  pack_image(hin, left, rows, cols, left_step);
  pack_image(hin + img, right, rows, cols, right_step);
  LORB_HIP(ctx, hipMemcpyAsync(B->d_img, hin, 2 * img, hipMemcpyHostToDevice, ctx->stream));
  LORB_TRY(enqueue_frame(B, B->d_img, cols, B->d_img + img, cols, B->d_out));
  LORB_HIP(ctx, hipMemcpyAsync(B->h_out, B->outs.base, B->outs.total, hipMemcpyDeviceToHost, ctx->stream));
  LORB_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const int32_t* cnt = mirror(B, B->d_out.counts);
  const int nL = cnt[0], nR = cnt[1];
  o->counts[0] = nL; o->counts[1] = nR;
  if (nL < 0 || nR < 0) return lorb::set_error(ctx, LORB_E_UNSUPPORTED, "DistributeOctTree exceeded its node capacity");
  if (nL > max_keypoints || nR > max_keypoints)
    return lorb::set_error(ctx, LORB_E_INVALID, "%d / %d keypoints exceed max_keypoints = %d", nL, nR, max_keypoints);
  fetch_side(B, B->d_out.left, o->left, nL, nl);
  fetch_side(B, B->d_out.right, o->right, nR, nl);
  if (nL > 0) {
    std::memcpy(o->u_right, mirror(B, B->d_out.u_right), sizeof(float) * nL);
    std::memcpy(o->depth, mirror(B, B->d_out.depth), sizeof(float) * nL);
  }
  return LORB_OK;
}

}  // extern "C"
