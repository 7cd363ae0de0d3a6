// Compile-only TU (tests/test_track_local_abi.py): lorb::EstimatePoseLocal instantiates against
// the reference's UNCHANGED Frame / MapPoint headers (it reads public members only), as the opt-in
// replacement of src/visual_odometry.cpp:149-209 that INTEGRATION.md describes.
#include "lorb_traits.hpp"

namespace Simple_ORB_SLAM {

bool lorb_compile_check_track_local(Frame* cur, const std::set<MapPoint*>& localMPs) {
  size_t nMatches = 0;
  const bool ok = lorb::EstimatePoseLocal(lorb::thread_ctx(), cur, localMPs, &nMatches);
  return ok && nMatches > 20;
}

}  // namespace Simple_ORB_SLAM
