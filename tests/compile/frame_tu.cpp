// Compile-only TU (tests/test_frame_abi.py): lorb::FrameBuilder / lorb::BuildFrame instantiate
// against the reference's Frame (with the friend declaration of INTEGRATION.md §4: the descriptor
// matrices are private), as the body a caller writes in place of the extraction and stereo part of
// Frame::Frame (src/frame.cpp:42-51).  AssignFeaturesToGrid stays the caller's.
#include "lorb_traits.hpp"

namespace Simple_ORB_SLAM {

size_t lorb_compile_check_frame(Frame* F, const cv::Mat& imgLeft, const cv::Mat& imgRight, const int* pattern,
                                const int* features_per_level) {
  lorb_frame_config cfg{};
  cfg.rows = imgLeft.rows; cfg.cols = imgLeft.cols;
  lorb::FrameTraits<Frame>::params(F, &cfg.frame);
  for (int l = 0; l < cfg.frame.n_levels; ++l) cfg.n_desired[l] = features_per_level[l];
  cfg.ini_th = 20; cfg.min_th = 7; cfg.pattern = pattern;
  static thread_local lorb::FrameBuilder builder(lorb::thread_ctx(), cfg);
  lorb::BuildFrame(builder, F, imgLeft.ptr<uint8_t>(), (int)imgLeft.step, imgRight.ptr<uint8_t>(), (int)imgRight.step);
  return F->mnMapPoints + (size_t)builder.capacity();
}

}  // namespace Simple_ORB_SLAM
