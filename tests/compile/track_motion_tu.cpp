// Compile-only TU (tests/test_track_motion_abi.py): lorb::EstimatePoseMotion instantiates against
// the reference's UNCHANGED Frame / MapPoint headers (it reads public members only), as the opt-in
// replacement of src/visual_odometry.cpp:124-135 that INTEGRATION.md describes.
#include "lorb_traits.hpp"

namespace Simple_ORB_SLAM {

bool lorb_compile_check_track_motion(Frame* cur, Frame* last) {
  size_t nMatches = 0;
  const bool ok = lorb::EstimatePoseMotion(lorb::thread_ctx(), cur, last, &nMatches);
  return ok && nMatches > 20;
}

}  // namespace Simple_ORB_SLAM
