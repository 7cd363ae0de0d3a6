/*
 * lorb_c.h -- C-ABI drop-in boundary of the MI355X-native LORB_SLAM hot path.
 *
 * Everything here is `extern "C"`, POD structs and plain pointers + sizes.  No torch, no
 * OpenCV, no Ceres types cross this boundary.  Each entry point names the reference
 * interface it replaces (paths relative to the reference repo abstract-liu/LORB_SLAM @ v0).
 *
 * Conventions
 *   - Every function returns int: LORB_OK (0) or a negative LORB_E_* code.  The message of
 *     the last error on a context is available from lorb_last_error(ctx).  No C++ exception
 *     ever crosses the ABI.
 *   - Functions without a `_dev` suffix take HOST pointers; they stage through device
 *     buffers owned by the context and are synchronous.  `_dev` variants take DEVICE
 *     pointers (allocated with lorb_malloc) and are asynchronous on the context's stream.
 *   - The library never takes ownership of caller memory.
 *   - One lorb_ctx per calling thread (it owns one hipStream_t).  A ctx is not thread-safe.
 *   - Keypoint / map-point identity: the C-ABI never sees MapPoint*.  Results are returned as
 *     per-slot "assign" codes that the C++ adapter applies to Frame::mvpMapPoints.
 */
#ifndef LORB_C_H
#define LORB_C_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LORB_ABI_VERSION 1

#define LORB_OK 0
#define LORB_E_INVALID (-1)   /* bad argument / shape */
#define LORB_E_DEVICE  (-2)   /* HIP runtime error (no device, launch failure, OOM) */
#define LORB_E_NOMEM   (-3)   /* host allocation failure */
#define LORB_E_UNSUPPORTED (-4)
#define LORB_E_COMM    (-5)   /* RCCL error */

/* Matcher constants, src/matcher.cpp:6-8 */
#define LORB_TH_HIGH 100
#define LORB_TH_LOW 50
#define LORB_HISTO_LENGTH 30
/* Frame grid, include/frame.h:13-14 */
#define LORB_GRID_ROWS 48
#define LORB_GRID_COLS 64
#define LORB_DESC_BYTES 32
#define LORB_MAX_LEVELS 16

/* assign codes written per current-frame keypoint slot by the windowed matchers */
#define LORB_ASSIGN_UNCHANGED (-1)  /* slot keeps whatever MapPoint* it held */
#define LORB_ASSIGN_NULL      (-2)  /* slot set to NULL (rotation-consistency null-out) */

/* slot state of a current-frame keypoint before a windowed match
 * (reference test: `if(F->mvpMapPoints[i] && F->mvpMapPoints[i]->mnObs>0) continue;`,
 *  src/matcher.cpp:149-151, 273-275) */
#define LORB_SLOT_EMPTY   0  /* mvpMapPoints[i] == NULL            */
#define LORB_SLOT_FREE    1  /* MapPoint present with mnObs == 0   */
#define LORB_SLOT_LOCKED  2  /* MapPoint present with mnObs  > 0   */

typedef struct lorb_ctx lorb_ctx;

/* ----------------------------------------------------------------------------------------
 * Context / runtime
 * -------------------------------------------------------------------------------------- */
int lorb_abi_version(void);
int lorb_device_count(int* count);
int lorb_create(int device, lorb_ctx** out);
int lorb_destroy(lorb_ctx* ctx);
const char* lorb_last_error(const lorb_ctx* ctx);
int lorb_sync(lorb_ctx* ctx);                       /* hipStreamSynchronize(ctx stream) */
int lorb_malloc(lorb_ctx* ctx, void** dptr, size_t bytes);
int lorb_free(lorb_ctx* ctx, void* dptr);
int lorb_memcpy_h2d(lorb_ctx* ctx, void* dst, const void* src, size_t bytes);  /* sync */
int lorb_memcpy_d2h(lorb_ctx* ctx, void* dst, const void* src, size_t bytes);  /* sync */
int lorb_memset_dev(lorb_ctx* ctx, void* dst, int value, size_t bytes);        /* async */
/* hipEvent timer on the ctx stream: marks, then elapsed ms between two marks */
int lorb_timer_mark(lorb_ctx* ctx, int slot);        /* slot in [0,64) */
int lorb_timer_elapsed_ms(lorb_ctx* ctx, int slot_begin, int slot_end, float* ms);
/* Per-kernel device timing (HIP events recorded around every launch of the named kernel
 * family on the ctx stream).  Used by bench.py for roofline.achieved.  Kernel ids: */
#define LORB_K_BF_SCAN_TOP2 0
#define LORB_K_BF_SCAN_TOP1 1
#define LORB_K_BA_SCHUR     2
#define LORB_K_BA_LINEARIZE 3
#define LORB_K_BA_CHOLESKY  4
#define LORB_K_WINDOW_CAND  5
#define LORB_K_STEREO       6
#define LORB_K_ALLREDUCE    7   /* the sharded plans' ncclAllReduce exchanges (eager, timed runs) */
#define LORB_K_COUNT        8
int lorb_kernel_timing_enable(lorb_ctx* ctx, int enable);
/* sums (and resets) the recorded launches of kernel id k: total ms and launch count */
int lorb_kernel_timing_read(lorb_ctx* ctx, int k, double* total_ms, int* launches);

/* ----------------------------------------------------------------------------------------
 * Frame description shared by the matchers (all fields are the reference Frame's, float)
 * -------------------------------------------------------------------------------------- */
typedef struct lorb_frame_params {
  float fx, fy, cx, cy;               /* Frame::fx,fy,cx,cy        include/frame.h:96 */
  float bf, b;                        /* Frame::mbf, Frame::mb     include/frame.h:96 */
  float min_x, max_x, min_y, max_y;   /* Frame::mnMinX..mnMaxY     include/frame.h:98-101 */
  float grid_w_inv, grid_h_inv;       /* mfGridElementWidthInv/HeightInv, src/frame.cpp:83-84 */
  int32_t n_levels;                   /* mnScaleLevels */
  float log_scale_factor;             /* mfLogScaleFactor */
  float scale_factors[LORB_MAX_LEVELS]; /* mvScaleFactors */
} lorb_frame_params;

/* SoA view of a frame's undistorted keypoints (Frame::mvKeysUn) + stereo + descriptors */
typedef struct lorb_keypoints {
  int32_t n;                 /* Frame::mnMapPoints */
  const float* x;            /* mvKeysUn[i].pt.x */
  const float* y;            /* mvKeysUn[i].pt.y */
  const int32_t* octave;     /* mvKeysUn[i].octave */
  const float* angle;        /* mvKeysUn[i].angle */
  const float* u_right;      /* mvuRight[i] (NULL => all -1) */
  const uint8_t* desc;       /* mDescriptors, n x 32 bytes row-major */
} lorb_keypoints;

/* ----------------------------------------------------------------------------------------
 * (a2/a3) brute-force Hamming + OpenCV-3.x crossCheck + the reference's outlier filter.
 * Replaces cv::BFMatcher(NORM_HAMMING,true).match at src/matcher.cpp:36-39 and :342-345 and
 * the minDist filter at src/matcher.cpp:42-56 / :348-362.
 *
 * Batched over n_problems independent (query set, train set) pairs, concatenated:
 *   problem p owns queries [q_off[p], q_off[p+1]) and trains [t_off[p], t_off[p+1]).
 *   q_off / t_off are HOST arrays of n_problems+1 entries (also for the _dev variant).
 * Outputs per query (global query index):
 *   cc_train[q]  : OpenCV crossCheck train index (problem-local) or -1 (no DMatch emitted)
 *   cc_dist[q]   : its Hamming distance (undefined when cc_train == -1)
 *   match_train[q]: cc_train[q] if cc_dist <= max(2*minDist, 30) else -1   (src/matcher.cpp:52)
 * n_matches[p] : number of accepted matches of problem p (the reference's return value).
 * -------------------------------------------------------------------------------------- */
int lorb_bf_match(lorb_ctx* ctx, int32_t n_problems,
                  const uint8_t* q_desc, const int32_t* q_off,
                  const uint8_t* t_desc, const int32_t* t_off,
                  int32_t* cc_train, int32_t* cc_dist, int32_t* match_train,
                  int32_t* n_matches);
int lorb_bf_match_dev(lorb_ctx* ctx, int32_t n_problems,
                      const uint8_t* d_q_desc, const int32_t* q_off,
                      const uint8_t* d_t_desc, const int32_t* t_off,
                      int32_t* d_cc_train, int32_t* d_cc_dist, int32_t* d_match_train,
                      int32_t* d_n_matches);

/* ----------------------------------------------------------------------------------------
 * (a5 with an unbounded window; BASELINE config "2000x2000 random 256-bit, ratio test")
 * Brute-force best/second-best with the reference's exact tie semantics
 * (src/matcher.cpp:289-301: strict '<', first candidate in train order wins) and the
 * level-gated ratio test + TH_HIGH acceptance (src/matcher.cpp:305-311).
 * t_level: per-train octave (NULL => all 0, i.e. ratio test always active).
 * Outputs per query: best_idx (-1 if none), best_dist (256 if none), best_level (-1),
 *   second_dist (256), second_level (-1), accepted (0/1).
 * -------------------------------------------------------------------------------------- */
int lorb_bf_top2(lorb_ctx* ctx, int32_t n_problems,
                 const uint8_t* q_desc, const int32_t* q_off,
                 const uint8_t* t_desc, const int32_t* t_off, const int32_t* t_level,
                 int32_t* best_idx, int32_t* best_dist, int32_t* best_level,
                 int32_t* second_dist, int32_t* second_level, uint8_t* accepted);
int lorb_bf_top2_dev(lorb_ctx* ctx, int32_t n_problems,
                     const uint8_t* d_q_desc, const int32_t* q_off,
                     const uint8_t* d_t_desc, const int32_t* t_off, const int32_t* d_t_level,
                     int32_t* d_best_idx, int32_t* d_best_dist, int32_t* d_best_level,
                     int32_t* d_second_dist, int32_t* d_second_level, uint8_t* d_accepted);

/* ----------------------------------------------------------------------------------------
 * (a4) Matcher::SearchByProjection(Frame* CurrentFrame, Frame* LastFrame, const float th)
 *      src/matcher.cpp:64-218, incl. Frame::GetFeaturesInArea (src/frame.cpp:370-423),
 *      the grid (src/frame.cpp:87-115) and the rotation histogram / ComputeThreeMaxima.
 * -------------------------------------------------------------------------------------- */
typedef struct lorb_last_frame {
  int32_t n;                 /* LastFrame->mnMapPoints */
  const float* Tcw;          /* LastFrame->mTcw, 4x4 row-major */
  const uint8_t* has_mp;     /* mvpMapPoints[i] != NULL */
  const uint8_t* outlier;    /* mvbOutlier[i] (NULL => all false) */
  const uint8_t* mp_locked;  /* mvpMapPoints[i]->mnObs > 0 */
  const float* mp_pos;       /* mvpMapPoints[i]->GetPos(), n x 3 */
  const uint8_t* mp_desc;    /* mvpMapPoints[i]->GetDescriptor(), n x 32 */
  const int32_t* octave;     /* LastFrame->mvKeys[i].octave */
  const float* angle;        /* LastFrame->mvKeysUn[i].angle */
} lorb_last_frame;

/* assign[j] for current keypoint j: LORB_ASSIGN_UNCHANGED, LORB_ASSIGN_NULL, or i >= 0 meaning
 * CurrentFrame->mvpMapPoints[j] = LastFrame->mvpMapPoints[i].  *nmatches = return value. */
int lorb_search_by_projection_frame(lorb_ctx* ctx,
                                    const lorb_frame_params* cur, const float cur_Tcw[16],
                                    const lorb_keypoints* cur_kps, const uint8_t* cur_slot_state,
                                    const lorb_last_frame* last, float th,
                                    int32_t* assign, int32_t* nmatches);
/* device-pointer variant: every array of d_cur_kps, d_cur_slot_state (NULL => all EMPTY) and every
 * array of d_last except d_last->Tcw is a DEVICE pointer; the structs, cur_Tcw, d_last->Tcw and th
 * are host values.  Outputs d_assign (n ints) and d_nmatches (one int) on the device.  Asynchronous
 * on the ctx stream while n_last * n_cur <= 8M (larger calls read the candidate count back once).
 * A last-frame point whose octave is outside [0, cur->n_levels) is treated as having no map point
 * (the host form rejects such a call instead). */
int lorb_search_by_projection_frame_dev(lorb_ctx* ctx,
                                        const lorb_frame_params* cur, const float cur_Tcw[16],
                                        const lorb_keypoints* d_cur_kps, const uint8_t* d_cur_slot_state,
                                        const lorb_last_frame* d_last, float th,
                                        int32_t* d_assign, int32_t* d_nmatches);

/* ----------------------------------------------------------------------------------------
 * (a5) Matcher::SearchByProjection(Frame* F, const std::set<MapPoint*>&, const float th)
 *      src/matcher.cpp:220-316.  Points are given flattened in std::set iteration order.
 * -------------------------------------------------------------------------------------- */
typedef struct lorb_local_points {
  int32_t n;
  const uint8_t* track_in_view;   /* mbTrackInView */
  const uint8_t* is_bad;          /* IsBad() (NULL => none) */
  const uint8_t* locked;          /* mnObs > 0 */
  const float* proj_x;            /* mTrackProjX */
  const float* proj_y;            /* mTrackProjY */
  const float* proj_xr;           /* mTrackProjXR */
  const int32_t* pred_level;      /* mnTrackScaleLevel */
  const float* view_cos;          /* mTrackViewCos */
  const uint8_t* desc;            /* GetDescriptor(), n x 32 */
} lorb_local_points;

/* assign[j]: LORB_ASSIGN_UNCHANGED or local point index k (F->mvpMapPoints[j] = point k). */
int lorb_search_by_projection_local(lorb_ctx* ctx,
                                    const lorb_frame_params* frame, const lorb_keypoints* kps,
                                    const uint8_t* slot_state,
                                    const lorb_local_points* pts, float th,
                                    int32_t* assign, int32_t* nmatches);

/* ----------------------------------------------------------------------------------------
 * (a8) Frame::IsInFrustum (src/frame.cpp:425-494) + MapPoint::PredictScale
 *      (src/map_point.cpp:267-284), batched over points.  Writes the tracking fields.
 * -------------------------------------------------------------------------------------- */
typedef struct lorb_frustum_points {
  int32_t n;
  const float* pos;        /* GetPos(), n x 3 */
  const float* normal;     /* mNormalVector, n x 3 */
  const float* max_dist;   /* mfMaxDistance  (GetMaxDistanceInvariance = 1.2f*mfMaxDistance) */
  const float* min_dist;   /* mfMinDistance  (GetMinDistanceInvariance = 0.8f*mfMinDistance) */
} lorb_frustum_points;
int lorb_is_in_frustum(lorb_ctx* ctx, const lorb_frame_params* frame, const float Tcw[16],
                       const lorb_frustum_points* pts, float viewing_cos_limit,
                       uint8_t* in_view, float* proj_x, float* proj_y, float* proj_xr,
                       int32_t* pred_level, float* view_cos);

/* device-resident local-map tracking -- VisualOdometry::EstimatePoseLocal's
 * sequence (src/visual_odometry.cpp:173-201): IsInFrustum(MP, viewing_cos_limit) for every local
 * map point that is neither already matched in the frame (mnLastFrameSeen == frame id) nor bad,
 * then SearchByProjection(F, localMPs, th), with frame and map data resident on the device.
 * All pointers below are DEVICE pointers (a lorb_keypoints whose arrays live on the device);
 * frame / Tcw are host values.  Outputs: d_in_view (mbTrackInView), d_track (n x 4 as four
 * planes: mTrackProjX, mTrackProjY, mTrackProjXR, mTrackViewCos), d_level (mnTrackScaleLevel),
 * d_assign / d_nmatches as lorb_search_by_projection_local.  Asynchronous on the ctx stream while
 * n_points * n_keypoints <= 8M; larger calls read the candidate count back once. */
typedef struct lorb_map_points_dev {
  int32_t n;
  const float* pos;          /* GetPos(), n x 3 */
  const float* normal;       /* mNormalVector, n x 3 */
  const float* max_dist;     /* mfMaxDistance */
  const float* min_dist;     /* mfMinDistance */
  const uint8_t* desc;       /* GetDescriptor(), n x 32 */
  const uint8_t* locked;     /* mnObs > 0 */
  const uint8_t* is_bad;     /* IsBad() (NULL => none) */
  const uint8_t* in_frame;   /* mnLastFrameSeen == frame id (NULL => none) */
} lorb_map_points_dev;
int lorb_track_local_map_dev(lorb_ctx* ctx, const lorb_frame_params* frame, const float Tcw[16],
                             const lorb_keypoints* d_kps, const uint8_t* d_slot_state,
                             const lorb_map_points_dev* pts, float viewing_cos_limit, float th,
                             uint8_t* d_in_view, float* d_track, int32_t* d_level,
                             int32_t* d_assign, int32_t* d_nmatches);
/* host-pointer variant (synchronous): the same structs with host arrays; d_track -> track (4 x n) */
int lorb_track_local_map(lorb_ctx* ctx, const lorb_frame_params* frame, const float Tcw[16],
                         const lorb_keypoints* kps, const uint8_t* slot_state,
                         const lorb_map_points_dev* pts, float viewing_cos_limit, float th,
                         uint8_t* in_view, float* track, int32_t* level,
                         int32_t* assign, int32_t* nmatches);

/* (a20) Frame::UnprojectStereo, src/frame.cpp:335-356, batched over keypoints. */
int lorb_unproject_stereo(lorb_ctx* ctx, const lorb_frame_params* frame, const float Tcw[16],
                          int32_t n, const float* x, const float* y, const float* depth,
                          float* out_xyz);
/* device-pointer variant (async on the ctx stream); frame / Tcw are host values */
int lorb_unproject_stereo_dev(lorb_ctx* ctx, const lorb_frame_params* frame, const float Tcw[16],
                              int32_t n, const float* d_x, const float* d_y, const float* d_depth,
                              float* d_out_xyz);

/* Frame::ComputeStereoMatches, src/frame.cpp:125-333 -- per left keypoint the
 * best right keypoint in its row band (Hamming < (TH_HIGH+TH_LOW)/2, octave within +-1, disparity in
 * [0, bf/b]), 11x11 SAD refinement over +-5 columns on the keypoint's pyramid level, parabola
 * sub-pixel fit, and the 2.1 x median SAD outlier rejection.  One image pyramid per camera
 * (ORBextractor::mvImagePyramid): level l is rows[l] x cols[l] u8 pixels at data + offset[l],
 * step[l] bytes per row. */
typedef struct lorb_image_pyramid {
  int32_t n_levels;
  const uint8_t* data;
  int64_t offset[LORB_MAX_LEVELS];
  int32_t rows[LORB_MAX_LEVELS], cols[LORB_MAX_LEVELS], step[LORB_MAX_LEVELS];
} lorb_image_pyramid;
/* SoA view of one camera's distorted keypoints (Frame::mvKeys / mvKeysRight) + descriptors */
typedef struct lorb_stereo_keys {
  int32_t n;
  const float* x;            /* kp.pt.x */
  const float* y;            /* kp.pt.y */
  const int32_t* octave;     /* kp.octave */
  const uint8_t* desc;       /* mDescriptors / mDescriptorsRight, n x 32 */
} lorb_stereo_keys;
/* Outputs mvuRight / mvDepth (n_left floats each, -1 where no depth).  Host pointers. */
int lorb_compute_stereo_matches(lorb_ctx* ctx, const lorb_frame_params* frame,
                                const lorb_stereo_keys* left, const lorb_stereo_keys* right,
                                const lorb_image_pyramid* left_pyr, const lorb_image_pyramid* right_pyr,
                                float* u_right, float* depth);
/* device-pointer variant: every array (keys, pyramid data, outputs) lives on the device; the structs
 * themselves and frame are host values.  Async on the ctx stream. */
int lorb_compute_stereo_matches_dev(lorb_ctx* ctx, const lorb_frame_params* frame,
                                    const lorb_stereo_keys* d_left, const lorb_stereo_keys* d_right,
                                    const lorb_image_pyramid* d_left_pyr, const lorb_image_pyramid* d_right_pyr,
                                    float* d_u_right, float* d_depth);

/* SURVEY §8f row 3 (descriptor stage of ORBextractor::operator(), src/ORBextractor.cpp:1087-1154):
 * for every keypoint (level coordinates, i.e. before the `pt *= scale` of :1144-1149) the IC_Angle
 * orientation on its raw pyramid level (computeOrientation, :79-107, :487-493; cv::fastAtan2) and
 * the 32-byte rBRIEF descriptor on the level blurred by GaussianBlur(7x7, sigma 2,
 * BORDER_REFLECT_101) (:1131-1132, :110-150).  pattern: the 512 test points as 1024 ints
 * (x0, y0, x1, y1, ...), the reference's bit_pattern_31_ (:152).  Outputs: angle[n] (KeyPoint::angle,
 * degrees) and desc (n x 32).  Defined for keypoints at least 19 px (EDGE_THRESHOLD, :76) inside
 * their level, as the extractor produces them; the host entry point rejects others. */
int lorb_orb_describe(lorb_ctx* ctx, const lorb_image_pyramid* pyr, int32_t n, const float* x, const float* y,
                      const int32_t* level, const int32_t* pattern, float* angle, uint8_t* desc);
int lorb_orb_describe_dev(lorb_ctx* ctx, const lorb_image_pyramid* d_pyr, int32_t n, const float* d_x,
                          const float* d_y, const int32_t* d_level, const int32_t* d_pattern, float* d_angle,
                          uint8_t* d_desc);

/* SURVEY §8f row 3, FAST stage of ORBextractor::ComputeKeyPointsOctTree (src/ORBextractor.cpp:
 * 803-872): per level the grid of 30-pixel cells with a 6-pixel overlap inside the
 * EDGE_THRESHOLD - 3 = 16-pixel border, and per cell cv::FAST(cell, ini_th, nonmax = true), re-run
 * with min_th when the cell found NO corner (:855-859).  Keypoints come out in level coordinates,
 * grouped by level, then cell (row-major), then FAST's scan order -- the order of vToDistributeKeys
 * -- with response = FAST score.  Cell c of level l spans [cell_off[cell_base[l] + l + c],
 * cell_off[cell_base[l] + l + c + 1]); cell_base has n_levels + 1 entries.  Host pointers; sync. */
int lorb_orb_fast_cells(lorb_ctx* ctx, const lorb_image_pyramid* pyr, int32_t ini_th, int32_t min_th,
                        int32_t max_keypoints, float* x, float* y, float* response, int32_t max_cells,
                        int32_t* cell_base, int32_t* cell_off, int32_t* n_keypoints);

/* SURVEY §8f row 3, ORBextractor::ComputePyramid (src/ORBextractor.cpp:1157-1184): level 0 is
 * the image, level l = cv::resize(level l-1, cvRound(size / scale_factors[l]), INTER_LINEAR)
 * (OpenCV 3.1's 8U fixed-point resize incl. its SSE2 vertical pass, see oracle/orb.c).  Levels are
 * packed row-major into `out` (out_bytes capacity); `layout` receives the lorb_image_pyramid view
 * (data = out).  The reference's copyMakeBorder margins are never read downstream and are not
 * produced.  _dev: device image and out (returns after the levels are written). */
int lorb_orb_pyramid(lorb_ctx* ctx, const uint8_t* image, int32_t rows, int32_t cols, int32_t step, int32_t n_levels,
                     const float* scale_factors, uint8_t* out, int64_t out_bytes, lorb_image_pyramid* layout);
int lorb_orb_pyramid_dev(lorb_ctx* ctx, const uint8_t* d_image, int32_t rows, int32_t cols, int32_t step,
                         int32_t n_levels, const float* scale_factors, uint8_t* d_out, int64_t out_bytes,
                         lorb_image_pyramid* layout);

/* SURVEY §8f row 3, ORBextractor::ComputeKeyPointsOctTree without the orientation
 * (src/ORBextractor.cpp:799-892): lorb_orb_fast_cells, then DistributeOctTree per level
 * (:554-797; N = n_desired[l] = mnFeaturesPerLevel[l]) -- the quadtree that keeps the strongest
 * keypoint of every node -- then the border offset, octave and size (PATCH_SIZE * scale_factors[l]
 * truncated to int, :881).  Per keypoint: x, y (level coordinates), octave, size, response, in the
 * reference's order (level, then the final std::list order of the quadtree nodes);
 * level_off[n_levels + 1].  Nodes holding equal key counts are ranked by creation order where the
 * reference compares std::list node addresses (:717).  Host pointers; synchronous. */
int lorb_orb_detect(lorb_ctx* ctx, const lorb_image_pyramid* pyr, const int32_t* n_desired,
                    const float* scale_factors, int32_t ini_th, int32_t min_th, int32_t max_keypoints, float* x,
                    float* y, int32_t* octave, float* size, float* response, int32_t* level_off,
                    int32_t* n_keypoints);

/* SURVEY §8f row 3, the whole ORBextractor::operator()(image, mask, keypoints, descriptors)
 * (src/ORBextractor.cpp:1087-1151): ComputePyramid, ComputeKeyPointsOctTree (+ IC_Angle
 * orientation), GaussianBlur + rBRIEF per level with the caller's 256-pair pattern
 * (bit_pattern_31_, :152), and the coordinates of level > 0 keypoints scaled to level 0 (:1141-1147).
 * Outputs in the reference's keypoint order: x, y, octave, size, angle (degrees), response and the
 * 32-byte descriptors; level_off[n_levels + 1]; *n_keypoints.  max_keypoints must be at least
 * lorb_orb_extract_capacity()'s bound for the _dev variant.  Host pointers; synchronous. */
int lorb_orb_extract(lorb_ctx* ctx, const uint8_t* image, int32_t rows, int32_t cols, int32_t step, int32_t n_levels,
                     const float* scale_factors, const int32_t* n_desired, int32_t ini_th, int32_t min_th,
                     const int32_t* pattern, int32_t max_keypoints, float* x, float* y, int32_t* octave, float* size,
                     float* angle, float* response, uint8_t* desc, int32_t* level_off, int32_t* n_keypoints);
/* device variant: image, pattern (1024 ints), the pyramid buffer (pyramid_bytes) and every output
 * are device arrays, d_level_off (n_levels + 1) and d_n (1) too.  Returns once the pyramid is
 * built (its resize tables are host-staged); detection and description run asynchronously on the
 * ctx stream.  *d_n = -1 when a quadtree exceeded its node capacity. */
int lorb_orb_extract_dev(lorb_ctx* ctx, const uint8_t* d_image, int32_t rows, int32_t cols, int32_t step,
                         int32_t n_levels, const float* scale_factors, const int32_t* n_desired, int32_t ini_th,
                         int32_t min_th, const int32_t* d_pattern, int32_t max_keypoints, uint8_t* d_pyramid,
                         int64_t pyramid_bytes, float* d_x, float* d_y, int32_t* d_octave, float* d_size,
                         float* d_angle, float* d_response, uint8_t* d_desc, int32_t* d_level_off, int32_t* d_n);
/* output capacity (keypoints) and pyramid bytes lorb_orb_extract_dev needs for an image size */
int lorb_orb_extract_capacity(int32_t rows, int32_t cols, int32_t n_levels, const float* scale_factors,
                              const int32_t* n_desired, int32_t* max_keypoints, int64_t* pyramid_bytes);

/* ----------------------------------------------------------------------------------------
 * The stereo Frame constructor, Frame::Frame(imgLeft, imgRight, camera) (src/frame.cpp:17-63), as
 * one call: ORBextractor::operator() on both images (:42-45; the reference runs them in two
 * threads), UndistortKeyPoints (:358-362, a copy: mvKeysUn = mvKeys, :361) and
 * ComputeStereoMatches (:125-333).  The result is the frame that lorb_track_motion_dev,
 * lorb_unproject_stereo_dev and lorb_track_local_dev read: the left side's x, y, octave, angle,
 * u_right and desc ARE the lorb_keypoints view (of mvKeysUn, which is mvKeys) as they stand.
 *
 * A builder holds everything that depends only on the geometry, built once by _create: the
 * pyramid layout, the resize tap tables of every level, the FAST cell table, the quadtree plan,
 * the blur tiles, the pattern, and all scratch for two images and the stereo stage (row table, row
 * lists, SAD array).  The memory is the builder's own (not the ctx's scratch), so a builder does
 * not disturb interleaved calls of the other entry points nor a second builder on the same ctx.
 *
 * Count protocol: counts[2] = {n_left, n_right} stays in device memory.  Every kernel after the
 * quadtree is launched over the capacity (lorb_frame_builder_capacity) and reads its count there,
 * bounded by the capacity; nothing is written past n_left / n_right entries of any array.  A side
 * whose quadtree overflowed its node capacity has count -1; the stereo stage then treats both
 * counts as 0 and writes nothing.  u_right / depth hold -1 where a left keypoint has no depth.
 *
 * Left to the host: Frame::AssignFeaturesToGrid (:87-103) is NOT an output -- every consumer
 * (the grid of lorb_search_by_projection_*, lorb_track_*) builds its grid from x, y -- and the
 * map-point slots (mvpMapPoints, mnMapPoints = 0), which lorb_frame_slots_fill_dev and
 * lorb_track_motion_frames_dev (below) keep as a device object of the caller's.
 * -------------------------------------------------------------------------------------- */
typedef struct lorb_frame_config {
  int32_t rows, cols;                    /* both images */
  lorb_frame_params frame;               /* n_levels, scale_factors, bf, b are read */
  int32_t n_desired[LORB_MAX_LEVELS];    /* ORBextractor::mnFeaturesPerLevel */
  int32_t ini_th, min_th;                /* iniThFAST, minThFAST */
  const int32_t* pattern;                /* host, 1024 ints: bit_pattern_31_ (copied by _create) */
} lorb_frame_config;
/* one camera's outputs: the content and order of lorb_orb_extract_dev's */
typedef struct lorb_frame_side {
  float* x;                /* kp.pt.x (level 0 coordinates) */
  float* y;
  int32_t* octave;
  float* size;
  float* angle;            /* degrees */
  float* response;
  uint8_t* desc;           /* capacity x 32 */
  int32_t* level_off;      /* n_levels + 1 */
  uint8_t* pyramid;        /* pyramid_bytes (ORBextractor::mvImagePyramid); ignored by lorb_frame_build */
} lorb_frame_side;
typedef struct lorb_frame_out {   /* a host struct of device (_dev) or host pointers */
  lorb_frame_side left, right;    /* mvKeys + mDescriptors, mvKeysRight + mDescriptorsRight */
  float* u_right;                 /* mvuRight, left only */
  float* depth;                   /* mvDepth, left only */
  int32_t* counts;                /* {n_left, n_right} */
} lorb_frame_out;
typedef struct lorb_frame_builder lorb_frame_builder;
/* Fails as lorb_orb_extract does for the geometries it rejects (LORB_E_UNSUPPORTED: 0 or 5 initial
 * quadtree nodes; LORB_E_INVALID: a level with no 30-pixel cell, a cell beyond the LDS tile) and
 * with LORB_E_INVALID for rows > 4096 (the stereo row table) or a null pattern. */
int lorb_frame_builder_create(lorb_ctx* ctx, const lorb_frame_config* cfg, lorb_frame_builder** out);
/* per image: the bounds of lorb_orb_extract_capacity */
int lorb_frame_builder_capacity(const lorb_frame_builder* builder, int32_t* max_keypoints, int64_t* pyramid_bytes);
/* Both images and every array of d_out are device memory (keypoint arrays: max_keypoints entries;
 * pyramids: pyramid_bytes; counts: 2 ints).  Asynchronous on the ctx stream: 16 kernel launches
 * (n_levels = 8), no stream synchronise, no device-to-host read and no host-to-device copy. */
int lorb_frame_build_dev(lorb_frame_builder* builder, const uint8_t* d_left, int32_t left_step,
                         const uint8_t* d_right, int32_t right_step, const lorb_frame_out* d_out);
/* Host arrays (each keypoint array holds max_keypoints entries): one staging copy of the two images,
 * the same launches, one fetch and one wait.  LORB_E_UNSUPPORTED when a quadtree overflowed
 * (counts still show which), LORB_E_INVALID when a count exceeds max_keypoints. */
int lorb_frame_build(lorb_frame_builder* builder, const uint8_t* left, int32_t left_step, const uint8_t* right,
                     int32_t right_step, int32_t max_keypoints, const lorb_frame_out* out);
int lorb_frame_builder_destroy(lorb_frame_builder* builder);

/* ----------------------------------------------------------------------------------------
 * Bundle adjustment: Ceres-default Levenberg-Marquardt + DENSE_SCHUR restated
 * (src/bundle_adjust.cpp:158-202 and :207-330; solver defaults in SURVEY Appendix B).
 * -------------------------------------------------------------------------------------- */
#define LORB_TERM_NO_CONVERGENCE 0   /* max_num_iterations reached */
#define LORB_TERM_FUNCTION_TOL   1
#define LORB_TERM_GRADIENT_TOL   2
#define LORB_TERM_PARAMETER_TOL  3
#define LORB_TERM_MIN_RADIUS     4
#define LORB_TERM_FAILURE        5   /* too many consecutive invalid steps */

typedef struct lorb_lm_options {       /* defaults == ceres::Solver::Options defaults */
  int32_t max_num_iterations;          /* 50 */
  double function_tolerance;           /* 1e-6 */
  double gradient_tolerance;           /* 1e-10 */
  double parameter_tolerance;          /* 1e-8 */
  double initial_trust_region_radius;  /* 1e4 */
  double max_trust_region_radius;      /* 1e16 */
  double min_trust_region_radius;      /* 1e-32 */
  double min_relative_decrease;        /* 1e-3 */
  double min_lm_diagonal;              /* 1e-6 */
  double max_lm_diagonal;              /* 1e32 */
  int32_t max_num_consecutive_invalid_steps; /* 5 */
  int32_t jacobi_scaling;              /* 1 */
} lorb_lm_options;
void lorb_lm_options_default(lorb_lm_options* opt);

typedef struct lorb_ba_summary {
  int32_t iterations;          /* LM iterations performed (successful + unsuccessful) */
  int32_t successful_steps;
  int32_t termination;         /* LORB_TERM_* */
  int32_t pad_;
  double initial_cost;         /* 0.5 * sum r^2 */
  double final_cost;
} lorb_ba_summary;

/* Per-iteration record of a local-BA solve (diagnostics / parity): one record per
 * LM iteration that computed a step, as Ceres' IterationSummary holds it (trust_region_minimizer.cc:
 * cost, model cost change, the candidate's cost, the radius the step was computed with, |step|).
 * The first LORB_LM_TRACE_CAP iterations of every window are recorded. */
#define LORB_LM_STEP_INVALID   0   /* linear solve failed / non-positive model decrease */
#define LORB_LM_STEP_ACCEPTED  1
#define LORB_LM_STEP_REJECTED  2   /* relative decrease <= min_relative_decrease */
#define LORB_LM_STEP_PARAM_TOL 3   /* solve ends: |step| <= parameter_tolerance * (|x| + ptol) */
#define LORB_LM_STEP_FUNC_TOL  4   /* solve ends: |cost change| <= function_tolerance * cost */
#define LORB_LM_TRACE_CAP 64
typedef struct lorb_lm_iteration {
  int32_t iteration;           /* 1-based */
  int32_t outcome;             /* LORB_LM_STEP_* */
  double cost;                 /* cost at the current point */
  double model_cost_change;    /* -(J step)^T (r + J step / 2), the linear model's decrease */
  double new_cost;             /* cost at the candidate x + step (valid steps) */
  double radius;               /* trust-region radius the step was computed with */
  double step_norm;            /* |x_candidate - x| (valid steps) */
} lorb_lm_iteration;

/* (a12) BA::ProjectPoseOptimization: pose-only, one PoseCost per matched map point.
 * The PoseCost quirk (v projected with fx, src/bundle_adjust.cpp:51) is reproduced by passing
 * fy_eff = fx; pass the real fy to get the "fixed" projection.  Batched over frames:
 * frame f owns residuals [res_off[f], res_off[f+1]) (HOST array).
 * pose_init: n_frames x 6 floats = (mRvec | mTvec)  (src/bundle_adjust.cpp:163-168)
 * pose_out:  n_frames x 6 doubles (the Ceres parameter blocks after Solve)
 * Tcw_out (optional): n_frames x 16 floats, Frame::SetPose(T,R) write-back via Rodrigues
 *   (src/bundle_adjust.cpp:198-201 -> src/frame.cpp:577-594). */
typedef struct lorb_pose_problem_batch {
  int32_t n_frames;
  const int32_t* res_off;      /* n_frames+1 */
  const float* intr;           /* n_frames x 4: fx, fy_eff, cx, cy */
  const float* pose_init;      /* n_frames x 6 */
  const float* pts3d;          /* n_res x 3 (MapPoint::GetPos) */
  const float* obs2d;          /* n_res x 2 (Frame::GetKp2d) */
} lorb_pose_problem_batch;
int lorb_ba_pose_only(lorb_ctx* ctx, const lorb_pose_problem_batch* prob,
                      const lorb_lm_options* opt, double* pose_out, float* Tcw_out,
                      lorb_ba_summary* summaries);
/* device-pointer variant: the five arrays of d_prob (res_off included) are DEVICE pointers,
 * n_frames a host value; d_pose_out (n_frames x 6 doubles) and d_summaries (n_frames records) are
 * written on the device.  Asynchronous on the ctx stream. */
int lorb_ba_pose_only_dev(lorb_ctx* ctx, const lorb_pose_problem_batch* d_prob,
                          const lorb_lm_options* opt, double* d_pose_out, lorb_ba_summary* d_summaries);

/* ----------------------------------------------------------------------------------------
 * VisualOdometry::EstimatePoseMotion (src/visual_odometry.cpp:117-138) as ONE call: a4 at
 * th_first; if that finds <= min_matches, every slot is emptied and a4 runs again at th_retry
 * (its codes then replace the first pass's); if the pass that counts found > min_matches, a12
 * (BA::ProjectPoseOptimization, src/bundle_adjust.cpp:158-202) over the slots that hold a map
 * point afterwards.  The retry decision and the residual gathering happen on the device: nothing
 * is read back between the first launch and the last.
 *
 * Residuals, one per slot j holding a map point after the matching, in ascending j, observation
 * (x[j], y[j]):  pass 1: assign[j] >= 0 -> last.mp_pos[assign[j]];  assign[j] == UNCHANGED and
 * slot_state[j] != EMPTY -> slot_pos[j];  NULL -> none.  pass 2 (and 0): assign[j] >= 0 only.
 * -------------------------------------------------------------------------------------- */
typedef struct lorb_track_motion_params {
  float th_first;        /* 15 */
  float th_retry;        /* 30 */
  int32_t min_matches;   /* 20: a pass stands when it finds MORE than this */
  float fy_eff;          /* PoseCost's v focal length: fx for the reference's quirk (see a12) */
} lorb_track_motion_params;

typedef struct lorb_track_motion_result {
  int32_t pass;            /* 1: first radius stood; 2: the retry stood; 0: both found <= min_matches
                              (the reference returns false and never optimises) */
  int32_t nmatches_first;
  int32_t nmatches_retry;  /* -1 when the retry did not run */
  int32_t n_residuals;     /* slots holding a map point after the matching (not nmatches: two
                              last-frame points can win the same slot) */
  double pose[6];          /* the optimised (mRvec | mTvec); pass 0: pose_init widened to double */
  lorb_ba_summary summary; /* pass 0: zeroed, as a12's empty problem */
} lorb_track_motion_result;

/* Device form.  cur, cur_Tcw (the predicted pose the matcher projects with), pose_init (the same
 * pose as mRvec | mTvec), the structs, d_last->Tcw, par and opt are host values; every array of
 * d_cur_kps and d_last, d_slot_state and d_slot_pos are DEVICE pointers.  d_slot_state NULL means
 * all EMPTY (the live path); d_slot_pos (n x 3: the position of the map point a non-empty slot
 * holds) may be NULL only then.  Outputs on the device: d_assign (n ints, the codes of the pass
 * that counts; pass 0: the retry's) and d_result (one record).  Asynchronous on the ctx stream: no
 * host readback and no stream synchronise while n_last * n_cur <= 8M.  Last-frame points whose
 * octave is outside [0, cur->n_levels) are treated as having no map point. */
int lorb_track_motion_dev(lorb_ctx* ctx, const lorb_frame_params* cur, const float cur_Tcw[16],
                          const float pose_init[6], const lorb_keypoints* d_cur_kps,
                          const uint8_t* d_slot_state, const float* d_slot_pos,
                          const lorb_last_frame* d_last, const lorb_track_motion_params* par,
                          const lorb_lm_options* opt, int32_t* d_assign,
                          lorb_track_motion_result* d_result);
/* Host-array form (synchronous): the same with host arrays; one staging of every input, the same
 * launches, one fetch of assign + record.  Octaves outside [0, LORB_MAX_LEVELS) are rejected as a4
 * does (those from cur->n_levels up are inactive, as in the device form: both forms give the same
 * bits).  Tcw_out (optional, 16 floats): Frame::SetPose write-back of the rounded pose (pass 0: of
 * pose_init). */
int lorb_track_motion(lorb_ctx* ctx, const lorb_frame_params* cur, const float cur_Tcw[16],
                      const float pose_init[6], const lorb_keypoints* cur_kps,
                      const uint8_t* slot_state, const float* slot_pos,
                      const lorb_last_frame* last, const lorb_track_motion_params* par,
                      const lorb_lm_options* opt, int32_t* assign,
                      lorb_track_motion_result* result, float* Tcw_out);

/* ----------------------------------------------------------------------------------------
 * VisualOdometry::EstimatePoseLocal after UpdateLocalMap (src/visual_odometry.cpp:173-209) as
 * ONE call: a8 (IsInFrustum + PredictScale, :181-195) for every local map point that is neither
 * already in the frame nor bad, a5 (SearchByProjection(F, localMPs, th), :196-202) over the
 * points in view, the nMatches <= 20 gate (:204-207) and, when it passes, a12
 * (BA::ProjectPoseOptimization, src/bundle_adjust.cpp:158-202) over the slots that hold a map
 * point afterwards.  The gate and the residual gathering happen on the device: nothing is read
 * back between the first launch and the last.
 *
 * Slots: slot_state / slot_pos describe the slots as stage 1 left them, with the slots whose point
 * is bad already EMPTY (the :153-171 loop is the caller's).  The frustum test and the search behave
 * exactly as lorb_track_local_map_dev; with nothing in view nothing matches (:198 skips the search).
 * assign[j] is LORB_ASSIGN_UNCHANGED or a point index, written whether or not the gate passes (the
 * reference keeps the matcher's writes when it returns false).
 *
 * Residuals, one per slot j holding a map point after the search, in ascending j
 * (src/bundle_adjust.cpp:173-186), observation (x[j], y[j]):  assign[j] >= 0 -> pts.pos[assign[j]];
 * assign[j] == UNCHANGED and slot_state[j] != EMPTY -> slot_pos[j].
 * -------------------------------------------------------------------------------------- */
typedef struct lorb_track_local_params {
  float viewing_cos_limit;  /* 0.5  (src/visual_odometry.cpp:188) */
  float th;                 /* 1    (:201) */
  int32_t min_matches;      /* 20: the stage stands when the search finds MORE than this (:204) */
  float fy_eff;             /* PoseCost's v focal length: fx for the reference's quirk (see a12) */
} lorb_track_local_params;

typedef struct lorb_track_local_result {
  int32_t ok;           /* 1: nmatches > min_matches and the pose was optimised; 0: the reference returns false */
  int32_t nmatches;     /* SearchByProjection's return value (0 when nothing is in view, :198) */
  int32_t n_in_view;    /* nToMatch (:193): points IsInFrustum accepted */
  int32_t n_residuals;  /* slots holding a map point after the search (not nmatches plus the kept
                           slots: two unlocked points can win one slot, the later one stands) */
  double pose[6];       /* optimised (mRvec | mTvec); ok == 0: pose_init widened to double */
  lorb_ba_summary summary;  /* ok == 0: zeroed, as a12's empty problem */
} lorb_track_local_result;

/* Device form.  frame, Tcw (the pose a8 projects with), pose_init (the same pose as mRvec | mTvec,
 * the a12 start, src/bundle_adjust.cpp:163-168), the structs, par and opt are host values; every
 * array of d_kps and d_pts, d_slot_state and d_slot_pos are DEVICE pointers.  d_slot_state NULL
 * means all EMPTY; d_slot_pos (n x 3) may be NULL only then.  Outputs on the device: d_in_view,
 * d_track (four planes), d_level as lorb_track_local_map_dev; d_assign (n_keypoints codes);
 * d_result (one record).  Asynchronous on the ctx stream: no host readback and no stream
 * synchronise while n_points * n_keypoints <= 8M; past that the candidate total is read back once,
 * as lorb_track_local_map_dev does. */
int lorb_track_local_dev(lorb_ctx* ctx, const lorb_frame_params* frame, const float Tcw[16],
                         const float pose_init[6], const lorb_keypoints* d_kps,
                         const uint8_t* d_slot_state, const float* d_slot_pos,
                         const lorb_map_points_dev* d_pts, const lorb_track_local_params* par,
                         const lorb_lm_options* opt, uint8_t* d_in_view, float* d_track,
                         int32_t* d_level, int32_t* d_assign, lorb_track_local_result* d_result);
/* Host-array form (synchronous): the same with host arrays; one staging of every input, the same
 * launches, one completion wait for the tracking fields, assign and the record (both forms give
 * the same bits).  Tcw_out (optional, 16 floats): Frame::SetPose write-back of the rounded pose
 * (ok == 0: of pose_init). */
int lorb_track_local(lorb_ctx* ctx, const lorb_frame_params* frame, const float Tcw[16],
                     const float pose_init[6], const lorb_keypoints* kps,
                     const uint8_t* slot_state, const float* slot_pos,
                     const lorb_map_points_dev* pts, const lorb_track_local_params* par,
                     const lorb_lm_options* opt, uint8_t* in_view, float* track, int32_t* level,
                     int32_t* assign, lorb_track_local_result* result, float* Tcw_out);

/* ----------------------------------------------------------------------------------------
 * The map-point slots of a built frame as a device object, and motion tracking straight from two
 * device-built frames: VisualOdometry::EstimatePoseMotion(pF) after its SetPose
 * (src/visual_odometry.cpp:121-137) enqueued behind lorb_frame_build_dev with the keypoint counts
 * never read by the host.
 *
 * lorb_frame_slots is Frame::mvpMapPoints as the matchers see it: state is d_slot_state of the
 * tracking calls, pos their d_slot_pos; (state != EMPTY, state == LOCKED, pos, desc) are has_mp,
 * mp_locked, mp_pos and mp_desc of the next frame's lorb_last_frame.  MapPoint::mNormalVector and
 * mfMaxDistance / mfMinDistance of created points are NOT produced: UpdateNormalAndDepth's OpenCV
 * arithmetic (cv::norm, Mat division) is unpinned, so they stay with the host.
 * -------------------------------------------------------------------------------------- */
typedef struct lorb_frame_slots {   /* Frame::mvpMapPoints as the matchers see it; device arrays of n_max entries */
  uint8_t* state;                   /* LORB_SLOT_EMPTY / LORB_SLOT_FREE / LORB_SLOT_LOCKED */
  float*   pos;                     /* n_max x 3, GetPos() of the held point */
  uint8_t* desc;                    /* n_max x 32, GetDescriptor() of the held point */
} lorb_frame_slots;

#define LORB_SLOTS_UPDATE_FRAME 0   /* VisualOdometry::UpdateFrame, src/visual_odometry.cpp:215-230 */
#define LORB_SLOTS_INITIALIZE   1   /* VisualOdometry::Initialize's loop, src/visual_odometry.cpp:86-99 */

/* Gives the slots of a built frame their map points.  frame and Tcw (the frame's pose) are host
 * values; d_frame is a host struct of DEVICE pointers (its left x, y, desc, its depth and counts[0]
 * are read), d_slots a host struct of device arrays of n_max entries each, d_n_created (nullable)
 * one device int.  n_left = d_frame->counts[0] is read on the device; nothing at or past n_left
 * is written.  A count that is negative or above n_max writes no slot and stores -1 at
 * d_n_created.
 *   LORB_SLOTS_UPDATE_FRAME: every EMPTY slot i < n_left becomes FREE (the MapPoint constructor of
 *     src/map_point.cpp:26-35 leaves mnObs = 0) with pos = UnprojectStereo(i) -- the bits of
 *     lorb_unproject_stereo_dev, so (0,0,0) for a keypoint without depth -- and desc = the frame's
 *     descriptor i; non-empty slots are untouched.  *d_n_created = slots filled.
 *   LORB_SLOTS_INITIALIZE: slots with depth >= 0 become LOCKED (AddObservation: mnObs = 1) with the
 *     unprojected pos and the frame's descriptor (ComputeDescriptor over one observation is that
 *     descriptor); slots with depth < 0 become EMPTY.  *d_n_created = slots LOCKED.  The
 *     mnMapPoints < 300 gate (src/visual_odometry.cpp:80) stays the caller's.
 * Asynchronous on the ctx stream: one launch, no stream synchronise, no copy. */
int lorb_frame_slots_fill_dev(lorb_ctx* ctx, const lorb_frame_params* frame, const float Tcw[16],
                              const lorb_frame_out* d_frame, int32_t n_max, int32_t mode,
                              const lorb_frame_slots* d_slots, int32_t* d_n_created);

typedef struct lorb_track_frames_result {
  lorb_track_motion_result motion;
  int32_t n_last, n_cur;   /* the counts the call read */
  int32_t n_created;       /* points UpdateFrame made */
  int32_t status;          /* 0, or 1: a count was negative or above its bound: nothing else was written */
} lorb_track_frames_result;

/* EstimatePoseMotion(pF) after its SetPose (src/visual_odometry.cpp:121-137) on two frames built by
 * lorb_frame_build_dev.  cur, cur_Tcw (the predicted pose), pose_init (the same pose as mRvec |
 * mTvec), last_Tcw, par, opt, the bounds and cur_slots_given are host values; d_cur / d_last are
 * host structs of device pointers; the slot structs are host structs of device arrays (n_max_cur /
 * n_max_last entries); d_last_outlier (n_max_last bytes, Frame::mvbOutlier) may be NULL: none.
 *   1. The LORB_SLOTS_UPDATE_FRAME fill of d_last_slots (:121).
 *   2. Both a4 passes and the tail exactly as lorb_track_motion_dev, with the last frame
 *      {n = d_last->counts[0], has_mp = state != EMPTY, mp_locked = state == LOCKED, mp_pos / mp_desc
 *      = the slots, octave / angle = d_last->left} and the current keypoints d_cur's left arrays +
 *      u_right, n = d_cur->counts[0].  On entry d_cur_slots is taken as all EMPTY (and never read)
 *      unless cur_slots_given.
 *   3. The codes that count applied to d_cur_slots: i >= 0 copies last slot i (state, pos, desc);
 *      LORB_ASSIGN_NULL gives EMPTY; UNCHANGED keeps the entry state when pass 1 stood and gives
 *      EMPTY when the retry ran (:128 empties first), as for pass 0.
 * d_assign: n_max_cur ints.  d_result: one record; status 1 (a count negative or above its bound)
 * leaves assign, both slot sets and the rest of the record untouched.  Nothing at or past a count
 * is written.  The bounds size grids, strides and scratch: a caller who knows nfeatures passes a
 * little more than that rather than the builder's capacity, whose square would leave a4's one-pass
 * candidate layout.  LORB_E_INVALID when n_max_last * n_max_cur > 8M (the asynchronous limit of a4).
 * Asynchronous on the ctx stream: no stream synchronise, no device-to-host read and no
 * host-to-device copy.  The slots left behind are d_slot_state / d_slot_pos of lorb_track_local_dev
 * and the last-frame arrays of the next frame's call. */
int lorb_track_motion_frames_dev(lorb_ctx* ctx, const lorb_frame_params* cur, const float cur_Tcw[16],
                                 const float pose_init[6], const lorb_frame_out* d_cur, int32_t n_max_cur,
                                 const lorb_frame_slots* d_cur_slots, int32_t cur_slots_given,
                                 const float last_Tcw[16], const lorb_frame_out* d_last, int32_t n_max_last,
                                 const lorb_frame_slots* d_last_slots, const uint8_t* d_last_outlier,
                                 const lorb_track_motion_params* par, const lorb_lm_options* opt,
                                 int32_t* d_assign, lorb_track_frames_result* d_result);

/* ----------------------------------------------------------------------------------------
 * Local-map tracking straight from a built frame: VisualOdometry::EstimatePoseLocal after
 * UpdateLocalMap (the held-slot loop, src/visual_odometry.cpp:153-171, then the tracking of
 * src/visual_odometry.cpp:173-209) enqueued behind lorb_track_motion_frames_dev, with the pose, the keypoint count and the frame's slots never read by the host.  One tracked frame is
 * then lorb_frame_build_dev, lorb_track_motion_frames_dev, lorb_track_local_frames_dev and ONE wait.
 *
 * Host values: frame, par, opt, n_max_cur (the bound on the keypoint count) and d_pts->n (the local
 * map is the caller's: UpdateLocalMap is not part of this call).  Device inputs:
 *   d_cur           host struct of device pointers; the left keypoint arrays and u_right are read,
 *                   counts[0] is read on the device
 *   d_cur_slots     n_max_cur entries, read and written (the slots lorb_track_motion_frames_dev left)
 *   d_cur_slot_id   n_max_cur int32, read and written: the index into d_pts of the point slot j
 *                   holds, or -1 for a point outside the table (points UpdateFrame created: always -1)
 *   d_pose          6 doubles, (mRvec | mTvec); in the frame chain &d_motion_result->motion.pose[0]
 *   d_src_status    nullable, one int32; in the frame chain &d_motion_result->status
 *   d_pts           its in_frame MUST be NULL: the call derives the mask (LORB_E_INVALID otherwise)
 *   ids             nullable.  NULL: d_cur_slot_id is taken as given.  Otherwise slot j's id on entry
 *                   is computed from the motion stage's final code c = d_motion_assign[j] by the rule
 *                   its tail applied to the slots: c >= 0 -> d_last_slot_id[c]; LORB_ASSIGN_NULL -> -1;
 *                   LORB_ASSIGN_UNCHANGED -> the id already in d_cur_slot_id[j] when
 *                   d_motion_result->motion.pass == 1 and cur_slots_given, else -1.
 * On the device, in this order:
 *   a. Status: counts[0] negative or above n_max_cur, or *d_src_status != 0, stores status = 1 in the
 *      record and NOTHING else -- no slot, id, field, code or other part of the record is touched.
 *   b. Pose hand-over: pose_in = (float) of the six doubles (the rounding of
 *      BA::ProjectPoseOptimization's write-back, src/bundle_adjust.cpp:198-201); Tcw_in = the arithmetic
 *      of lorb_pose_to_Tcw on pose_in; the camera centre from cv::Mat::inv() of Tcw_in.
 *   c. The held-slot loop (src/visual_odometry.cpp:153-171): a non-EMPTY slot whose id >= 0 names a
 *      point with is_bad set becomes EMPTY with id -1; every other non-EMPTY slot with id >= 0 marks its
 *      point as already in the frame (mnLastFrameSeen).
 *   d. a8 + a5 (:173-202) exactly as lorb_track_local_dev with that mask, Tcw_in and the slots of c.
 *   e. The tail (:204-209) as lorb_track_local_dev from pose_in, then the codes applied to the slots
 *      whether or not the gate passes (the reference keeps the matcher's writes): assign[j] = k >= 0
 *      gives state = locked[k] ? LOCKED : FREE, pos = pts.pos[k], desc = pts.desc[k], id = k;
 *      UNCHANGED slots stay as they are.
 * What the device pose is equal to: the BA's pose agrees with the oracle to 1e-5, not bit for bit, and
 * the device's double sin / cos is not libm's function, so Tcw_in is DEFINED as what the record
 * reports; the matching is bit-exact given that Tcw_in (lorb_track_local_dev on the record's Tcw_in,
 * pose_in, n_cur and the slots and mask of step c gives the same bits).
 * Outputs as lorb_track_local_dev: d_in_view, d_track, d_level (d_pts->n entries each), d_assign
 * (n_max_cur entries).  Nothing at or past counts[0] is written.  LORB_E_INVALID, before anything is
 * enqueued: a null required argument, n_max_cur < 1, d_pts->n < 0, d_pts->n * n_max_cur > 8M (past
 * that the candidate total would have to be read back), n_levels out of range, a negative
 * min_matches, a non-NULL d_pts->in_frame.  Asynchronous on the ctx stream: no stream synchronise, no
 * device-to-host read and no host-to-device copy.
 * -------------------------------------------------------------------------------------- */
typedef struct lorb_track_local_id_source {
  const int32_t* d_motion_assign;                  /* n_max_cur: lorb_track_motion_frames_dev's d_assign */
  const lorb_track_frames_result* d_motion_result; /* its record (motion.pass is read) */
  const int32_t* d_last_slot_id;                   /* n_max_last: the last frame's slot ids */
  int32_t n_max_last;
  int32_t cur_slots_given;                         /* as passed to lorb_track_motion_frames_dev */
} lorb_track_local_id_source;

typedef struct lorb_track_local_frames_result {
  lorb_track_local_result local;  /* as lorb_track_local_dev */
  float pose_in[6];               /* (float) of d_pose: the a12 start */
  float Tcw_in[16];               /* the pose a8 projected with */
  float Tcw[16];                  /* Frame::SetPose of local.pose rounded to float; ok == 0: Tcw_in */
  int32_t n_cur;                  /* the count the call read */
  int32_t n_held;                 /* slots non-EMPTY after step c */
  int32_t n_in_frame;             /* points of d_pts the frame held after step c */
  int32_t status;                 /* 0, or 1: nothing else was written */
} lorb_track_local_frames_result;

int lorb_track_local_frames_dev(lorb_ctx* ctx, const lorb_frame_params* frame, const lorb_frame_out* d_cur,
                                int32_t n_max_cur, const lorb_frame_slots* d_cur_slots, int32_t* d_cur_slot_id,
                                const double* d_pose, const int32_t* d_src_status,
                                const lorb_track_local_id_source* ids, const lorb_map_points_dev* d_pts,
                                const lorb_track_local_params* par, const lorb_lm_options* opt,
                                uint8_t* d_in_view, float* d_track, int32_t* d_level, int32_t* d_assign,
                                lorb_track_local_frames_result* d_result);

/* ----------------------------------------------------------------------------------------
 * VisualOdometry::UpdateLocalMap (src/visual_odometry.cpp:234-340) in the frame chain: the local map
 * built on the device from the slots the motion stage has just written, so that a tracked frame with
 * the reference's own local map is lorb_frame_build_dev, lorb_track_motion_frames_dev,
 * lorb_local_map_update_dev, lorb_track_local_frames_dev, lorb_local_map_ids_back_dev and ONE wait.
 *
 * The map store is the caller's: a host struct of device arrays with host counts (the mapper changes
 * the map from the host side).  Ordering convention: keyframe index order stands for the iteration
 * order of std::map<Frame*, ...>, point index order for that of std::set<MapPoint*>; the adapters
 * flatten sets the same way.
 *   points          the n_points map points (points.n); points.in_frame MUST be NULL; points.desc is
 *                   16-byte aligned
 *   obs_off/obs_kf  MapPoint::GetObservations() as a CSR over the points: the keyframe indices of
 *                   point p are obs_kf[obs_off[p] .. obs_off[p + 1]); only membership is read
 *   kf_bad          Frame::IsBad() per keyframe
 *   kf_slot_off / kf_slot_point   Frame::GetMapPoints() as a CSR over the keyframes: a global point
 *                   index, or -1 for a NULL slot
 *   cov_off/cov_kf  mvpOrderedKeyFrames as a CSR over the keyframes, in the reference's order;
 *                   GetBestCovisibleFrames(10) reads at most the first 10 of a list (src/frame.cpp:735-741)
 * n_obs, n_kf_slots and n_cov are the lengths of obs_kf, kf_slot_point and cov_kf: a CSR range is
 * clipped to them, and an index outside its table (a keyframe outside [0, n_kf), a point outside
 * [-1, n_points)) is skipped, so a damaged store cannot make the device write out of bounds.
 * -------------------------------------------------------------------------------------- */
typedef struct lorb_map_store {
  lorb_map_points_dev points;
  const int32_t* obs_off;        /* n_points + 1 */
  const int32_t* obs_kf;         /* n_obs */
  const uint8_t* kf_bad;         /* n_kf */
  const int32_t* kf_slot_off;    /* n_kf + 1 */
  const int32_t* kf_slot_point;  /* n_kf_slots */
  const int32_t* cov_off;        /* n_kf + 1 */
  const int32_t* cov_kf;         /* n_cov */
  int32_t n_kf, n_obs, n_kf_slots, n_cov;
} lorb_map_store;

/* The local map as a device object.  It owns the local table (the arrays of a lorb_map_points_dev of
 * max_local rows), l2g[max_local] (local row -> global point), g2l[max_points] (global point -> local
 * row, -1 elsewhere), kf_votes[max_kf] (step 1.1's frameCounter), local_kf[max_kf] (mpLocalKeyFrames in
 * the reference's order) and its scratch.  create zero-fills every table column once and sets is_bad = 1
 * in every row.  view returns those arrays; view->points has n = max_local and is handed to
 * lorb_track_local_frames_dev as it stands: rows at or past the local count have is_bad = 1, and the
 * local stage skips a bad point before it reads anything else of it.  That stage's candidate layout is
 * sized by max_local * n_max_cur, which must stay <= 8M. */
typedef struct lorb_local_map lorb_local_map;
typedef struct lorb_local_map_arrays {
  lorb_map_points_dev points;    /* n = max_local, in_frame NULL */
  const int32_t* l2g;            /* max_local; rows < n_local are written */
  const int32_t* g2l;            /* max_points; entries < n_points are written */
  const int32_t* kf_votes;       /* max_kf; entries < n_kf are written */
  const int32_t* local_kf;       /* max_kf; entries < n_local_kf are written */
  int32_t max_local, max_kf, max_points;
} lorb_local_map_arrays;
typedef struct lorb_local_map_result {
  int32_t status;      /* 0; 1: a bad count or source status, nothing else was written; 2: n_local > max_local */
  int32_t n_cur;       /* the count the call read */
  int32_t n_held;      /* slots non-EMPTY after step c */
  int32_t n_nulled;    /* slots step c emptied (their point was bad) */
  int32_t n_voted;     /* keyframes with a vote that are not bad: the list before the expansion */
  int32_t n_local_kf;  /* the list after the expansion */
  int32_t refer_kf;    /* pFMax, or -1 when mReferFrame stays */
  int32_t n_local;     /* local points (the true count also under status 2) */
} lorb_local_map_result;
/* max_local, max_kf, max_points >= 1 (LORB_E_INVALID otherwise).  Allocates; waits for the stream. */
int lorb_local_map_create(lorb_ctx* ctx, int32_t max_local, int32_t max_kf, int32_t max_points, lorb_local_map** out);
int lorb_local_map_destroy(lorb_local_map* map);
int lorb_local_map_view(const lorb_local_map* map, lorb_local_map_arrays* out);

/* UpdateLocalMap (src/visual_odometry.cpp:234-340) on the slots of a built frame.  Host values: the
 * store's counts and n_max_cur.  d_cur->counts[0] is read on the device; d_cur_slots (states read and
 * written), d_cur_slot_gid (n_max_cur int32: the GLOBAL point index slot j holds, -1 for a point
 * outside the store -- those UpdateFrame created), d_cur_slot_id (n_max_cur int32, written: the LOCAL
 * row) and d_result are device memory; d_src_status is nullable (in the frame chain
 * &d_motion_result->status); ids is nullable.  On the device, in this order:
 *   a. Status: counts[0] negative or above n_max_cur, or *d_src_status != 0, stores status = 1 and
 *      NOTHING else, as the two frame calls do.
 *   b. Entry ids: ids == NULL takes d_cur_slot_gid as given; otherwise slot j's gid is computed from
 *      the motion stage's codes by exactly the rule of lorb_track_local_id_source, with d_last_slot_id
 *      and d_cur_slot_gid holding global indices.  An index outside [0, n_points) counts as -1.
 *   c. Step 1.1 (:241-259), for every non-EMPTY slot j < n_cur with gid g >= 0: point g bad makes the
 *      slot EMPTY and its gid -1; otherwise every keyframe of the point's observation list gets one
 *      vote.  Slots with gid -1 vote for nothing (a created point has no observations).
 *   d. Steps 1.2-1.3 (:263-312): the voted keyframes in ascending index, bad ones skipped, are the
 *      list; pFMax is the first with the strictly largest vote (:274).  The expansion (:282-307) is an
 *      INDEX loop over the growing list that stops as soon as the list holds more than 10 entries;
 *      each visited entry appends the first non-bad frame among the first 10 of its covisible list
 *      that is not in the list yet, and goes on to the next entry.  (The reference iterates by
 *      iterator while it push_backs, which is undefined on reallocation: DESIGN section 7.)
 *   e. Step 2 (:315-336): every non-bad point held in a slot of a local keyframe is local, once, in
 *      ascending global index: l2g, g2l (-1 elsewhere) and the gathered table rows (pos, normal,
 *      max_dist, min_dist, desc, locked, is_bad = 0); rows from n_local up to max_local get is_bad = 1.
 *   f. Local ids: d_cur_slot_id[j] = g2l[gid] for non-EMPTY slots with gid >= 0, else -1.  The local
 *      stage is then called with ids = NULL and d_src_status = &d_result->status.
 * n_local > max_local is status 2: the effects of c and d stand, every table row has is_bad = 1,
 * g2l is -1 throughout, l2g and d_cur_slot_id are untouched and n_local reports the true count.
 * Nothing at or past a count is written (d_cur_slot_gid / d_cur_slot_id: counts[0]; kf_votes: n_kf;
 * local_kf: n_local_kf; l2g and the gathered columns: n_local; g2l: n_points).
 * LORB_E_INVALID, before anything is enqueued: a null required argument, a map of another ctx,
 * n_max_cur < 1, a negative count, n_points above max_points, n_kf above max_kf, max_local *
 * n_max_cur > 8M, a non-NULL points.in_frame, a points.desc that is not 16-byte aligned.
 * Asynchronous on the ctx stream: 5 kernel launches (4 for a store without points), no stream
 * synchronise, no device-to-host read and no host-to-device copy. */
int lorb_local_map_update_dev(lorb_ctx* ctx, lorb_local_map* map, const lorb_map_store* store,
                              const lorb_frame_out* d_cur, int32_t n_max_cur, const lorb_frame_slots* d_cur_slots,
                              int32_t* d_cur_slot_gid, int32_t* d_cur_slot_id, const int32_t* d_src_status,
                              const lorb_track_local_id_source* ids, lorb_local_map_result* d_result);

/* After the local stage: the slots' local rows back into the global index space (one launch).  For
 * each slot j < counts[0]: d_cur_slot_id[j] = lid >= 0 gives d_cur_slot_gid[j] = l2g[lid]; an EMPTY
 * slot gives -1; any other slot keeps its gid (a held point outside the local map, or a created one).
 * A count out of range or *d_local_status != 0 (nullable; in the chain the local stage's
 * &d_result->status) writes nothing.  The gids are the next frame's d_last_slot_id. */
int lorb_local_map_ids_back_dev(lorb_ctx* ctx, const lorb_local_map* map, const lorb_frame_out* d_cur,
                                int32_t n_max_cur, const lorb_frame_slots* d_cur_slots, const int32_t* d_cur_slot_id,
                                const int32_t* d_local_status, int32_t* d_cur_slot_gid);

/* ----------------------------------------------------------------------------------------
 * The pose hand-over between frames as device objects: VisualOdometry::Run's motion model
 * (src/visual_odometry.cpp:65-66, :119) and Frame::SetPose(Tcw) (src/frame.cpp:570-575) with no host
 * value in between, so that any number of frames can be enqueued behind one another and waited for once.
 * Both blocks are plain device memory; the first frame's are uploaded with lorb_memcpy_h2d (the
 * identity from lorb_frame_pose_from_Tcw, mTcc = I: src/visual_odometry.cpp:84,112).
 * -------------------------------------------------------------------------------------- */
typedef struct lorb_frame_pose {   /* one per frame; a caller keeps two and swaps them with the frames */
  float Tcw[16];     /* Frame::GetPose()    */
  float Twc[16];     /* Frame::GetInvPose(): cv::Mat::inv() of Tcw (LU32f) */
  float pose[6];     /* mRvec | mTvec       */
  int32_t status;    /* 0; 1: nothing in the block is valid */
} lorb_frame_pose;
typedef struct lorb_motion_model { float Tcc[16]; int32_t status; } lorb_motion_model;   /* mTcc */

/* lorb_track_motion_frames_dev with the three poses in device memory.  Every other argument is that
 * call's.  On the device, in the chain's first launch and before anything else:
 *   Status: a count negative or above its bound, d_last_pose->status != 0, or d_model given with
 *     status != 0, stores status = 1 in the record and in d_cur_pose and NOTHING else.
 *   Prediction, only when d_model is given (:119, then SetPose(Tcw)): d_cur_pose->Tcw = last.Tcw * Tcc
 *     as cv::gemm on CV_32F (float operands, double accumulation in k order, one rounding to float), Twc
 *     = cv::Mat::inv() of it, pose = the vector of lorb_Tcw_to_pose, status = 0.  With d_model == NULL
 *     d_cur_pose is read as given.
 * The rest of the stage reads both blocks: the fill's Twc is d_last_pose->Twc, a4's motion direction
 * comes from d_cur_pose->Tcw and d_last_pose->Tcw, the LM starts from d_cur_pose->pose.  Given the same
 * poses every output has the bits of lorb_track_motion_frames_dev (which computes Twc from last_Tcw).
 * Asynchronous on the ctx stream: the same launches, no stream synchronise, no copy. */
int lorb_track_motion_frames_pose_dev(lorb_ctx* ctx, const lorb_frame_params* cur, lorb_frame_pose* d_cur_pose,
                                      const lorb_frame_out* d_cur, int32_t n_max_cur,
                                      const lorb_frame_slots* d_cur_slots, int32_t cur_slots_given,
                                      const lorb_frame_pose* d_last_pose, const lorb_motion_model* d_model,
                                      const lorb_frame_out* d_last, int32_t n_max_last,
                                      const lorb_frame_slots* d_last_slots, const uint8_t* d_last_outlier,
                                      const lorb_track_motion_params* par, const lorb_lm_options* opt,
                                      int32_t* d_assign, lorb_track_frames_result* d_result);

/* The second motion attempt of VisualOdometry::Run, on the reference keyframe, decided on the device
 * (src/visual_odometry.cpp:50-54,117-138):
 *     bool tag = EstimatePoseMotion(mPrevFrame);  if(tag == false) tag = EstimatePoseMotion(mReferFrame);
 * Enqueued directly behind lorb_track_motion_frames_pose_dev with that call's d_assign, d_result,
 * d_cur_pose, d_cur_slots and d_model (required here); the refer objects are the frame the caller
 * believes is mReferFrame.  Two optional groups, each given whole or not at all:
 *   gids   d_last_slot_gid (n_max_last), d_refer_slot_gid (n_max_refer), d_cur_slot_gid (n_max_cur, read
 *          and written): the global point index each slot holds.  NULL: no id bookkeeping.
 *   guard  d_refer_kf (one device int32, read and written: the keyframe index of mReferFrame, initialised
 *          once by the caller) and d_prev_update (the PREVIOUS frame's lorb_local_map_update_dev record);
 *          refer_kf is the index of the frame passed as d_refer.  NULL: no guard.
 * On the device, in the chain's first launch and before anything else, in this order:
 *   a. The first attempt's record has status != 0: due = ran = stale = 0 (and both figures 0) is stored in
 *      d_refer_result and NOTHING else is written; the record keeps its status 1.
 *   b. The reference-frame word (:311-312): d_prev_update->status == 0 with refer_kf >= 0 stores that
 *      index in *d_refer_kf -- the previous frame's UpdateLocalMap is the last thing that can have moved
 *      mReferFrame.  Enqueued every frame, the word follows mReferFrame exactly.
 *   c. Entry ids (gids given): d_cur_slot_gid[j], j < n_cur, from the first attempt's codes by exactly the
 *      rule of lorb_track_local_id_source, with d_last_slot_gid and first_slots_given (cur_slots_given as
 *      passed to the first attempt); an index outside its table counts as -1.  Always done, due or not:
 *      behind this call lorb_local_map_update_dev is given ids = NULL.
 *   d. due = (motion.pass == 0); stale = due and the guard is given and *d_refer_kf != refer_kf.  Not due,
 *      or stale: d_refer_result is stored and NOTHING else is written -- d_assign, d_result, both slot
 *      sets, d_cur_pose, d_model and the refer frame's slots stay as they are, every later kernel of the
 *      call returns at once, and the refer frame's count, pose status and bounds are not examined.
 *   e. Due and not stale (ran = 1): the stage is exactly lorb_track_motion_frames_pose_dev with the refer
 *      objects as d_last*, d_model given and cur_slots_given = 1 -- both a4 passes start from the slots the
 *      failed first attempt left (:128-131 leaves its <= 20 matches in mvpMapPoints) -- into the same
 *      d_assign and d_result: the status (the refer count, d_refer_pose->status; status 1 in the record
 *      and in d_cur_pose and nothing else), the prediction d_cur_pose = SetPose(refer.Tcw * Tcc), the
 *      UPDATE_FRAME fill of d_refer_slots with refer.Twc, the tail and its slot write-back.
 *      first_nmatches_first / _retry keep the first attempt's figures.  With gids given the tail applies
 *      the final codes to d_cur_slot_gid: c >= 0 -> d_refer_slot_gid[c] (outside the table: -1);
 *      LORB_ASSIGN_NULL -> -1; LORB_ASSIGN_UNCHANGED -> the id step c left when pass 1 stood, else -1.
 * A stale reference frame is reported, not followed: the caller sees stale = 1 and a
 * record with pass 0.  Downstream nothing changes: &d_result->status, &d_result->motion.pose[0] and
 * lorb_frame_pose_finish_dev (mTcc is still formed against the previous frame's block, :65) as before.
 * LORB_E_INVALID as lorb_track_motion_frames_pose_dev (bounds n_max_refer and n_max_cur), and for a null
 * d_model or d_refer_result, a partially given gid group (or n_max_last < 1 with it) and a partially
 * given guard pair.  Asynchronous on the ctx stream: the launches of lorb_track_motion_frames_pose_dev
 * for the same bounds and no more, no stream synchronise, no copy. */
typedef struct lorb_track_refer_result {
  int32_t due;    /* 1: the first attempt's record had status 0 and motion.pass == 0 */
  int32_t ran;    /* 1: the second attempt ran (due, and not stale) */
  int32_t stale;  /* 1: due, but *d_refer_kf != refer_kf: not run */
  int32_t first_nmatches_first, first_nmatches_retry;  /* the first attempt's (0 under a), kept for the caller when ran */
} lorb_track_refer_result;
int lorb_track_motion_refer_pose_dev(lorb_ctx* ctx, const lorb_frame_params* cur, lorb_frame_pose* d_cur_pose,
                                     const lorb_frame_out* d_cur, int32_t n_max_cur, const lorb_frame_slots* d_cur_slots,
                                     int32_t first_slots_given, const lorb_frame_pose* d_refer_pose,
                                     const lorb_motion_model* d_model, const lorb_frame_out* d_refer, int32_t n_max_refer,
                                     const lorb_frame_slots* d_refer_slots, const uint8_t* d_refer_outlier,
                                     const int32_t* d_last_slot_gid, int32_t n_max_last, const int32_t* d_refer_slot_gid,
                                     int32_t* d_cur_slot_gid, int32_t refer_kf, int32_t* d_refer_kf,
                                     const lorb_local_map_result* d_prev_update, const lorb_track_motion_params* par,
                                     const lorb_lm_options* opt, int32_t* d_assign, lorb_track_frames_result* d_result,
                                     lorb_track_refer_result* d_refer_result);

/* After the local stage (:65-66), one launch.  d_local_result->status == 0: cur.Tcw = the record's Tcw,
 * cur.pose = (float) of local.pose when local.ok, else pose_in; cur.Twc = cv::Mat::inv() of cur.Tcw;
 * cur.status = 0; model.Tcc = last.Twc * cur.Tcw (the gemm convention above), model.status = 0.  A
 * non-zero status stores cur.status = 1 and leaves the model untouched: the next frame's motion stage
 * then has status 1 too, and so has every frame behind it.  All five arguments are required. */
int lorb_frame_pose_finish_dev(lorb_ctx* ctx, const lorb_track_local_frames_result* d_local_result,
                               const lorb_frame_pose* d_last_pose, lorb_frame_pose* d_cur_pose,
                               lorb_motion_model* d_model);

/* ----------------------------------------------------------------------------------------
 * The map store as a device object that grows in the frame chain: VisualOdometry::AddKeyFrame
 * (src/visual_odometry.cpp:356-404) and the map part of Initialize (:86-103), LocalMapping::ProcessNewFrames
 * step 1 (src/local_mapping.cpp:57-70) and Frame::UpdateConnections (src/frame.cpp:801-869) with AddConnection
 * and UpdateBestCovisibleFrames (:754-788), as ONE enqueued call behind lorb_frame_pose_finish_dev.
 *
 * A lorb_kf_store owns every array of a lorb_map_store (the layout and ordering convention above) plus each
 * keyframe's mConnectedKeyFrameWeights (the reference rebuilds mvpOrderedKeyFrames from that map, so the store
 * keeps it).  lorb_kf_store_host is the same store in host arrays: `init` of create (the n_* fields are the
 * counts; NULL: an empty store) and the target of read (the n_* fields are the CAPACITIES of the caller's
 * arrays, in entries of each table; any array may be NULL: not read).  conn_off / conn_kf / conn_w is the weight
 * map as a CSR over the keyframes, entries in ascending keyframe index (std::map<Frame*, size_t> order).
 *
 * Capacities: max_kf in [1, 4096] (the counter and the per-row sort of an insertion keep a keyframe row in
 * LDS), max_points, max_obs, max_kf_slots >= 1; the covisibility table holds max_kf * max_kf entries.
 *
 * Counts.  The TRUE counts (n_kf, n_points, n_obs, n_kf_slots, n_cov, n_conn) live on the device, because the
 * gate of an insertion is decided there.  The host keeps upper BOUNDS it can advance without waiting: one
 * keyframe, n_max_cur points and n_max_cur keyframe slots per enqueued insertion (each clipped to its capacity),
 * and the table capacities for n_obs and n_cov.  lorb_kf_store_view returns the device arrays with those bounds
 * as the host counts (no wait; the pointers never change, so a view taken before the insertions in front of it
 * have run stays valid).  Rows between a true count and its bound are inert: is_bad = 1 and kf_bad = 1 (set at
 * create over the whole capacity) and no slot, observation or covisibility list refers to them, so the view
 * handed to lorb_local_map_update_dev gives the record, slots, gids, local ids, votes, list, l2g, g2l and table
 * rows the same call gives on an exact store (kf_votes / g2l entries between truth and bound are written as 0
 * / -1: they are below the counts that call was given).  The slot gids handed to it must be indices the store
 * issued.  lorb_kf_store_counts waits for the stream, stores the first min(n, 6) true counts in the order above
 * and replaces the bounds by the truth.  lorb_kf_store_read waits and copies the true rows of every non-NULL
 * member (LORB_E_INVALID when a capacity field is below its true count).
 * create validates `init` (counts within the capacities, offsets ascending from 0 and ending at their table's
 * length, every index inside its table, weight-map rows strictly ascending) and waits for the stream.
 * -------------------------------------------------------------------------------------- */
typedef struct lorb_kf_store lorb_kf_store;
typedef struct lorb_kf_store_caps { int32_t max_kf, max_points, max_obs, max_kf_slots; } lorb_kf_store_caps;
typedef struct lorb_kf_store_host {
  int32_t n_kf, n_points, n_obs, n_kf_slots, n_cov, n_conn;
  float* pos;                 /* n_points x 3 */
  float* normal;              /* n_points x 3 */
  float* max_dist;            /* n_points */
  float* min_dist;            /* n_points */
  uint8_t* desc;              /* n_points x 32 */
  uint8_t* locked;            /* n_points */
  uint8_t* is_bad;            /* n_points */
  int32_t* obs_off;           /* n_points + 1 */
  int32_t* obs_kf;            /* n_obs, each list in ascending keyframe index */
  uint8_t* kf_bad;            /* n_kf */
  int32_t* kf_slot_off;       /* n_kf + 1 */
  int32_t* kf_slot_point;     /* n_kf_slots */
  int32_t* cov_off;           /* n_kf + 1 */
  int32_t* cov_kf;            /* n_cov: mvpOrderedKeyFrames */
  int32_t* conn_off;          /* n_kf + 1 */
  int32_t* conn_kf;           /* n_conn: mConnectedKeyFrameWeights, keys */
  int32_t* conn_w;            /* n_conn: its weights */
} lorb_kf_store_host;
int lorb_kf_store_create(lorb_ctx* ctx, const lorb_kf_store_caps* caps, const lorb_kf_store_host* init, lorb_kf_store** out);
int lorb_kf_store_destroy(lorb_kf_store* store);
int lorb_kf_store_view(const lorb_kf_store* store, lorb_map_store* out);         /* no wait */
int lorb_kf_store_counts(lorb_kf_store* store, int32_t* out, int32_t n);         /* waits; tightens the host bounds */
int lorb_kf_store_read(lorb_kf_store* store, const lorb_kf_store_host* out);     /* waits */

#define LORB_KF_GATE_RATIO 0   /* AddKeyFrame's ratio test, src/visual_odometry.cpp:360-372 */
#define LORB_KF_GATE_NONE  1   /* Initialize (:86-103): always inserted; mnMapPoints < 300 (:80) stays the caller's */
typedef struct lorb_kf_insert_result {
  int32_t status;      /* 0; 1: bad count or source status; 2: a capacity */
  int32_t inserted;    /* 0: the gate said no */
  int32_t n_cur, n_map;
  int32_t kf;          /* K, or -1 */
  int32_t n_observed;  /* observations added to points the store already had */
  int32_t n_adopted, n_created;
  int32_t n_connected; /* length of K's ordered list */
  int32_t n_points, n_kf, n_obs;   /* the store after the call */
} lorb_kf_insert_result;

/* Inserts the current frame as keyframe K = the true n_kf on entry.  In the frame chain it is enqueued behind
 * lorb_frame_pose_finish_dev with the frame's lorb_local_map_ids_back_dev gids and d_src_status =
 * &d_local_result->status.  Host values: frame (fx, fy, cx, cy, n_levels, scale_factors are read), n_max_cur,
 * gate.  d_cur is a host struct of device pointers (counts[0], the left x, y, octave, desc and depth are read),
 * d_cur_slots a host struct of device arrays (read and written), d_cur_slot_gid n_max_cur device int32 (read and
 * written), d_cur_pose the frame's block (Twc and status are read); d_src_status, d_refer_kf and d_update are
 * nullable.  On the device, in this order:
 *   a. Status: counts[0] negative or above n_max_cur, d_cur_pose->status != 0 or *d_src_status != 0 stores
 *      status = 1 and NOTHING else.
 *   b. Gate (:360-372), LORB_KF_GATE_RATIO: nMap = the non-EMPTY slots j < n_cur, ratio = (float)nMap /
 *      (float)n_cur; ratio > 0.35f stores inserted = 0, n_map and status = 0 and NOTHING else.  n_cur = 0 makes the
 *      ratio NaN: the comparison is false and an empty keyframe is inserted, as in the reference.
 *      LORB_KF_GATE_NONE always goes on.
 *   c. Capacity: status = 2 (with the counts the call found: n_cur, n_map, kf = -1, n_observed, n_adopted,
 *      n_created, and the store's unchanged n_points, n_kf, n_obs) and nothing written to the store, the slots or
 *      the gids when K + 1 would exceed max_kf or the new points, observations or keyframe slots would pass
 *      max_points, max_obs, max_kf_slots.  Decided before the first store write.
 *   d. Every slot j < n_cur with gid g (an index outside [0, n_points) counts as -1):
 *        held, g >= 0, point bad      nothing is added (src/local_mapping.cpp:60-61); slot, gid and K's row keep g
 *        held, g >= 0, not bad        AddObservation(K, j) (src/local_mapping.cpp:62-65, src/map_point.cpp:133-139):
 *                                     K joins the point's observation list ONCE however many slots hold g (the
 *                                     lowest slot adds it), last -- lists stay in ascending keyframe index;
 *                                     locked[g] = 1 and the slot becomes LOCKED
 *        held, g == -1                a point UpdateFrame created: ADOPTED as a new store point with the slot's
 *                                     position and descriptor; the slot becomes LOCKED
 *        EMPTY, depth[j] >= 0         CREATED by Initialize's live rule (:88-98): position = the bits of
 *                                     lorb_unproject_stereo_dev under d_cur_pose->Twc, descriptor = the frame's
 *                                     descriptor j; the slot becomes LOCKED with that position and descriptor
 *        EMPTY, depth[j] < 0          stays EMPTY; its gid and K's row entry are -1
 *      New points, adopted and created alike, are numbered from n_points in ascending slot order, each with
 *      locked = 1, is_bad = 0, observation list {K} and its slot's gid set to the new index.  normal, max_dist
 *      and min_dist are UpdateNormalAndDepth over that one observation (src/map_point.cpp:224-264), RESTATED, not
 *      verified against OpenCV (as cv::gemm and cv::Mat::inv are restated): d = pos - Ow in float, Ow = (Twc[3],
 *      Twc[7], Twc[11]); nd = sqrt((double)d.x*d.x + (double)d.y*d.y + (double)d.z*d.z) summed in that order;
 *      normal = d * (float)(1.0 / nd), a float multiply; dist = (float)nd; max_dist = dist *
 *      scale_factors[octave[j]]; min_dist = max_dist / scale_factors[n_levels - 1]; no FMA contraction.
 *   e. K's row: kf_slot_point gets the n_cur gids after step d; kf_bad[K] = 0.
 *   f. UpdateConnections(K) (src/frame.cpp:801-869).  The counter is taken per SLOT (a point held in two slots
 *      counts twice) over K's non-EMPTY slots with a non-bad store point and that point's observers other than K.
 *      For keyframes f in ascending index with count w: w >= 3 enters K's pairs and f.AddConnection(K, w).  With no
 *      pair at all the reference compares against size_t nMax = -1 and dereferences NULL (:825-848); ORB-SLAM2's
 *      intent is restated: the first keyframe with the strictly largest count gets the one connection; every
 *      count zero: none.  K's weight map is the whole counter, entries below 3 included (:855); K's ordered list
 *      is the pairs ascending by (weight, index) (:851).  f.AddConnection(K, w) (:777-788) sets f's weight for K and
 *      rebuilds f's ordered list from ALL of f's weight map ascending by (weight, index) (:754-774), entries below
 *      3 included.  Ascending order means GetBestCovisibleFrames(10) returns the weakest ten: kept.
 *   g. mReferFrame = mCurrFrame (:402): K is stored at d_refer_kf and in d_update->refer_kf (this frame's
 *      lorb_local_map_update_dev record, which the next frame's lorb_track_motion_refer_pose_dev re-applies to the
 *      word in its step b), each when given.  Only on insertion.
 *   h. The device counts and the record.
 * Nothing at or past a new true count is written, in any array of the store, the slots or the gids.
 * LORB_E_INVALID, before anything is enqueued: a null required argument, a store of another ctx, n_max_cur < 1 or
 * above max_kf_slots, an unknown gate, n_levels outside [1, LORB_MAX_LEVELS], a null array in d_cur / d_cur_slots, a
 * descriptor array (the frame's left.desc, the slots' desc) that is not 16-byte aligned.
 * Asynchronous on the ctx stream: 6 kernel launches, no stream synchronise, no device-to-host read and no
 * host-to-device copy. */
int lorb_kf_store_insert_dev(lorb_ctx* ctx, lorb_kf_store* store, const lorb_frame_params* frame,
                             const lorb_frame_out* d_cur, int32_t n_max_cur, const lorb_frame_slots* d_cur_slots,
                             int32_t* d_cur_slot_gid, const lorb_frame_pose* d_cur_pose, const int32_t* d_src_status,
                             int32_t gate, int32_t* d_refer_kf, lorb_local_map_result* d_update,
                             lorb_kf_insert_result* d_result);

/* ----------------------------------------------------------------------------------------
 * The store's geometry, and BA::LocalPoseOptimization(mpCurrFrame) (src/bundle_adjust.cpp:207-330, call site
 * src/local_mapping.cpp:32) fed straight from the store: tracker -> keyframe -> local BA -> refined poses and
 * points in the store the next frame's lorb_local_map_update_dev reads.
 *
 * Geometry.  Beside the arrays of lorb_kf_store_host the store keeps, at capacity and at addresses that never
 * change:
 *   kf_pose      max_kf x 6 float        mRvec | mTvec of each keyframe
 *   kf_slot_uv   max_kf_slots x 2 float  GetKp2d(j) of each keyframe slot, parallel to kf_slot_point (the
 *                                        observation source include/lorb/adapters.hpp uses for a13)
 *   obs_slot     max_obs int32           parallel to obs_kf: the slot of point p in keyframe obs_kf[o]
 *                                        (mObservations[f], the it->second of src/bundle_adjust.cpp:273-296)
 * INVARIANT: kf_slot_point[kf_slot_off[f] + obs_slot[o]] == p for every observation o of p in f = obs_kf[o].
 * lorb_kf_store_insert_dev maintains them for keyframe K (still six launches, no wait, no copy): kf_pose[K] = the
 * bits of d_cur_pose->pose; K's uv row = the frame's left x, y of the slots j < n_cur; obs_slot of the observation
 * added to a held point = the lowest slot that holds it; obs_slot of a new point's observation = the slot that
 * adopted or created it; obs_slot moves with obs_kf when the observation CSR is rebuilt.  Nothing at or past a new
 * true count is written in these arrays either.
 * lorb_kf_store_create_geom is lorb_kf_store_create with the geometry of the initial keyframes (n_kf, n_kf_slots,
 * n_obs must equal init's; init NULL: all three 0).  It checks the invariant on the host -- every obs_slot inside
 * its keyframe's row and pointing back at its point -- and returns LORB_E_INVALID with a message naming the
 * offending entry.  A store made by lorb_kf_store_create with n_kf > 0 has no geometry for its initial keyframes:
 * the calls below refuse it with LORB_E_INVALID.  An empty store is complete by construction.
 * lorb_kf_store_geom_read waits and copies the true rows of every non-NULL member (the n_* fields are the
 * CAPACITIES of the caller's arrays; LORB_E_INVALID when one is below its true count).
 * -------------------------------------------------------------------------------------- */
typedef struct lorb_kf_store_geom_host {
  int32_t n_kf, n_kf_slots, n_obs;   /* create: must equal init's; read: capacities */
  float* kf_pose;                    /* n_kf x 6 */
  float* kf_slot_uv;                 /* n_kf_slots x 2 */
  int32_t* obs_slot;                 /* n_obs */
} lorb_kf_store_geom_host;
int lorb_kf_store_create_geom(lorb_ctx* ctx, const lorb_kf_store_caps* caps, const lorb_kf_store_host* init,
                              const lorb_kf_store_geom_host* geom, lorb_kf_store** out);
int lorb_kf_store_geom_read(lorb_kf_store* store, const lorb_kf_store_geom_host* out);   /* waits */
/* the device arrays themselves, the n_* fields their capacities (no wait; the pointers never change) */
int lorb_kf_store_geom_view(const lorb_kf_store* store, lorb_kf_store_geom_host* out);

#define LORB_KF_BA_MAX_LOCAL 128   /* local frames of one window: the device plans' camera limit */
typedef struct lorb_kf_ba_result {   /* device memory, like every record of the chain */
  int32_t status;        /* 0; 1: source status or kf outside the store; 2: more than 128 local frames; 3: no points
                            or no observations; 4: a point with 256 or more usable observations */
  int32_t kf;
  int32_t n_poses, n_fixed, n_points, n_obs;   /* the window */
  int32_t n_cov_bad;       /* bad covisible frames skipped (:215-217) */
  int32_t n_obs_bad_kf;    /* observations skipped: the observing keyframe is bad (:278) */
  int32_t n_obs_bad_slot;  /* observations skipped: a keyframe or slot outside the store (a damaged store) */
  int32_t written;         /* 1: the solution was written back */
} lorb_kf_ba_result;
typedef struct lorb_kf_ba_window_host {   /* the last gathered window; n_*: the capacities of the caller's arrays */
  int32_t n_poses, n_fixed, n_points, n_obs;
  int32_t* local_kf;     /* n_poses: keyframe index of each optimised pose */
  int32_t* fixed_kf;     /* n_fixed: keyframe index of each fixed pose */
  int32_t* l2g;          /* n_points: store index of each window point */
  float* pose_init;      /* n_poses x 6 */
  float* fixed_pose;     /* n_fixed x 6 */
  float* point_init;     /* n_points x 3 */
  int32_t* obs_point;    /* n_obs */
  int32_t* obs_frame;    /* n_obs: >= 0 optimised pose, -1 - j fixed pose j */
  float* obs_uv;         /* n_obs x 2 */
} lorb_kf_ba_window_host;

/* lorb_kf_store_ba_gather_dev builds the window of keyframe *d_kf in the store's own device memory;
 * lorb_kf_store_local_ba_dev does the same, solves it and writes the solution back into the store.  d_kf is a
 * device word -- in the chain &d_insert_result->kf, so a refused insertion's -1 makes the call a no-op -- and
 * d_src_status a nullable device word (&d_insert_result->status).  frame supplies fx, fy, cx, cy
 * (pCurrFrame->mpCamera).  On the device, in this order, all index arithmetic integer, no result depending on the
 * order atomics arrive in:
 *   a. Status: *d_src_status != 0, or kf outside [0, true n_kf), stores status = 1 and NOTHING else.
 *   b. Frames (:210-220): local[0] = kf (the reference does not ask whether it is bad), then the entries of kf's
 *      covisibility row (cov_kf: the whole mvpOrderedKeyFrames, src/frame.cpp:729-732) in row order, skipping
 *      kf_bad ones (counted in n_cov_bad).  An entry outside [0, n_kf), equal to kf, or already listed is skipped.
 *      More than LORB_KF_BA_MAX_LOCAL local frames stores status = 2 and nothing else.
 *   c. Points (:224-241): over the local frames in list order and each frame's slots in slot order, a point index
 *      that is not -1 and not is_bad enters at its first appearance: l2g[i].
 *   d. Observations (:270-303): window point i's list in list order (ascending keyframe index = std::map<Frame*,
 *      size_t> order).  A bad keyframe is skipped (:278, n_obs_bad_kf).  A local keyframe gives obs_frame = its
 *      rank in the list of b; any other keyframe is a FIXED frame, -1 - j, the fixed frames numbered in ascending
 *      keyframe index among those that occur (the numbering changes no arithmetic: a fixed pose enters only
 *      through its own observations).  obs_uv = kf_slot_uv[kf_slot_off[f] + obs_slot].  An obs_kf outside
 *      [0, n_kf) or an obs_slot outside its row is skipped (n_obs_bad_slot).  Observations come out sorted by
 *      point.
 *   e. Initial values: pose_init / fixed_pose = the kf_pose rows, point_init = the pos rows.  No points or no
 *      observations: status = 3, nothing is solved and nothing is written back.  A window point with 256 or more
 *      usable observations (the device plans' point group): status = 4, likewise.
 *   f. Solve (lorb_kf_store_local_ba_dev): the window is handed in place, as a lorb_ba_window_dev, to a resident
 *      device-built plan -- one per camera count in a small LRU with capacities that only grow, the slot logic
 *      lorb_ba_solver uses -- then lorb_ba_plan_solve(opt).
 *   g. Write-back (:317-329), one launch: kf_pose[local[i]] and pos[l2g[i]] take the solution rounded to float
 *      (lorb_ba_plan_result_dev's conversion), whatever the termination, as in the reference; written = 1.
 *      Nothing else in the store changes: normal, max / min distance, descriptors, flags, every list and every
 *      count stay (SetWorldPos, src/map_point.cpp:52-55, sets the position only).
 * Host side.  The gather is 6 kernel launches, then ONE copy of a 64-byte header (status and the window's counts,
 * which pick the plan) and ONE wait.  lorb_kf_store_ba_gather_dev ends there.  lorb_kf_store_local_ba_dev goes on
 * with the plan build (lorb_ba_plan_update_dev: its launches, one small readback, one wait), the captured LM
 * graph and 1 write-back launch, all left enqueued; summary != NULL adds one copy and a final wait.  In steady
 * state (a camera count already seen, sizes within the slot's capacities) the call allocates nothing.
 * Returns LORB_OK for status 0, 1 and 3.  LORB_E_INVALID before anything is enqueued: a null required argument,
 * a store of another ctx, a store without geometry.  LORB_E_UNSUPPORTED with the store untouched: status 2 or 4
 * (no host-plan fallback is built).  Every path leaves the per-point scratch at rest: a failed call followed by
 * a good one gives the window the good call alone gives.
 * lorb_kf_ba_window_read waits and copies the last gathered window's true rows (counts as the record's) into
 * every non-NULL member; LORB_E_INVALID when a capacity is below its count or no window was gathered.
 * Out of scope: a host-array form or a C++ adapter; lorb_frame_pose blocks the caller holds for a reference
 * keyframe (NOT updated by the write-back); running the BA on a second stream beside the tracker;
 * KeyFramesCulling (MapPointsCulling is lorb_kf_store_cull_dev below, enqueued in front of this call);
 * lorb_map_step_dev, which keeps its own ring map. */
int lorb_kf_store_ba_gather_dev(lorb_ctx* ctx, lorb_kf_store* store, const lorb_frame_params* frame,
                                const int32_t* d_kf, const int32_t* d_src_status, lorb_kf_ba_result* d_result);
int lorb_kf_store_local_ba_dev(lorb_ctx* ctx, lorb_kf_store* store, const lorb_frame_params* frame,
                               const int32_t* d_kf, const int32_t* d_src_status, const lorb_lm_options* opt,
                               lorb_kf_ba_result* d_result, lorb_ba_summary* summary);
int lorb_kf_ba_window_read(lorb_kf_store* store, const lorb_kf_ba_window_host* out);   /* waits */

/* ----------------------------------------------------------------------------------------
 * The life of the store's points and LocalMapping::MapPointsCulling (src/local_mapping.cpp:82-108) on the store:
 * the mapper step ProcessNewFrames -> MapPointsCulling -> BA::LocalPoseOptimization (src/local_mapping.cpp:24-36) as
 * lorb_kf_store_insert_dev -> lorb_kf_store_cull_dev -> lorb_kf_store_local_ba_dev, each behind the other on the
 * insertion's record words.
 *
 * Life state.  Beside its other arrays the store keeps, at capacity and at addresses that never change:
 *   visible     max_points int32   MapPoint::mnVisible
 *   found       max_points int32   MapPoint::mnFound
 *   first_fid   max_points int32   MapPoint::mnFirstFId
 *   recent      max_points uint8   1: the point is a member of LocalMapping::mvpRecentAddPoints
 *   kf_fid      max_kf int32       Frame::mnId of each keyframe
 *   frame word  one int32          the id of the frame the tracker last observed (lorb_kf_store_observe_dev)
 * The reference's list is a FLAG per point here: a point's verdict depends on that point alone, and a second visit
 * of a duplicate entry finds the point bad or gone, so the set of culled points and of remaining members is the
 * list's.  A store from lorb_kf_store_create / _create_geom starts with visible = found = 1 (the MapPoint
 * constructors, src/map_point.cpp:16-17,33-34), first_fid = 0, recent = 0 and kf_fid = 0 over its initial rows and
 * a frame word of 0.
 * lorb_kf_store_life_write waits and replaces the true rows by every non-NULL member: n_kf and n_points must EQUAL
 * the true counts; visible < 1 or found < 0 is LORB_E_INVALID with a message naming the entry.
 * lorb_kf_store_life_read waits and copies the true rows into every non-NULL member (the n_* fields are the
 * CAPACITIES of the caller's arrays; LORB_E_INVALID when one is below its true count).  lorb_kf_store_life_view
 * returns the device arrays themselves, the n_* fields their capacities, and lorb_kf_store_frame_word_view the
 * address of the frame word (no wait; the pointers never change).
 * lorb_kf_store_insert_dev maintains the state for keyframe K (still six launches, no wait, no copy): kf_fid[K] =
 * the frame word; every new point, adopted or created, gets first_fid = the frame word and visible = found = 1;
 * recent = 1 for CREATED points only (a created point already has K as an observation, so src/local_mapping.cpp:62-69
 * pushes it; an adopted one gets AddObservation there and is not pushed) and for an old point K holds in two or
 * more slots (the lowest slot adds the observation, every later slot finds IsInFrame true and pushes).  A held bad
 * point changes nothing.  An adopted point's life before it had a store row is not tracked.  Nothing at or past a
 * new true count is written.
 * -------------------------------------------------------------------------------------- */
typedef struct lorb_kf_store_life_host {
  int32_t n_kf, n_points;   /* write: must equal the true counts; read: capacities */
  int32_t* visible;         /* n_points */
  int32_t* found;           /* n_points */
  int32_t* first_fid;       /* n_points */
  uint8_t* recent;          /* n_points */
  int32_t* kf_fid;          /* n_kf */
} lorb_kf_store_life_host;
int lorb_kf_store_life_write(lorb_kf_store* store, const lorb_kf_store_life_host* in);   /* waits */
int lorb_kf_store_life_read(lorb_kf_store* store, const lorb_kf_store_life_host* out);   /* waits */
int lorb_kf_store_life_view(const lorb_kf_store* store, lorb_kf_store_life_host* out);   /* no wait */
int lorb_kf_store_frame_word_view(const lorb_kf_store* store, int32_t** d_word);         /* no wait */

#define LORB_KF_FOUND_NEVER 0   /* the reference: IncreaseFound is never called, GetFoundRatio() is 1 / mnVisible */
#define LORB_KF_FOUND_SLOTS 1   /* ORB-SLAM2's TrackLocalMap intent: every slot that holds a point after the local stage */
typedef struct lorb_kf_observe_result {
  int32_t status;      /* 0; 1: a bad count or source status, nothing else was written */
  int32_t n_held;      /* increments of step c */
  int32_t n_in_view;   /* increments of step d */
  int32_t n_found;     /* increments of step e */
} lorb_kf_observe_result;

/* The tracker's two IncreaseVisible sites (src/visual_odometry.cpp:165,191) on the store.  Enqueued behind
 * lorb_track_local_frames_dev and in front of lorb_local_map_ids_back_dev.  Host values: frame_id
 * (mCurrFrame->mnId), n_max_cur, found_rule.  Device inputs: the frame (counts[0]), its slots (state), d_cur_slot_gid
 * (still the gids lorb_local_map_update_dev left, bad held points already at -1), d_cur_slot_id (the local rows
 * after the local stage), lmap (the lorb_local_map_view arrays: l2g and max_local are read), d_update (that
 * frame's lorb_local_map_update_dev record: status and n_local are read on the device), d_in_view (the local
 * stage's), d_local_status (nullable; in the chain the local stage's &d_result->status).  On the device, in this
 * order:
 *   a. Status: counts[0] negative or above n_max_cur, n_local negative or above max_local, *d_local_status != 0 or
 *      d_update->status != 0 stores status = 1 in the record and NOTHING else -- the frame word included.
 *   b. The frame word = frame_id.
 *   c. Every slot j < n_cur with a gid in [0, true n_points): visible[g] += 1 (:153-171).  Per slot: a point in two
 *      slots gets 2.
 *   d. Every local row k < n_local with in_view[k] != 0 and l2g[k] inside the store: visible[l2g[k]] += 1 (:188-194).
 *   e. found_rule.  LORB_KF_FOUND_NEVER (the reference): nothing.  LORB_KF_FOUND_SLOTS: every slot that is non-EMPTY
 *      after the stage adds 1 to found of the store point it holds -- l2g[lid] when lid = d_cur_slot_id[j] >= 0
 *      (lid < n_local), else the slot's gid -- when that index is inside the store.  This is ORB-SLAM2's
 *      TrackLocalMap intent; the reference does not do it.
 *   f. The record.
 * The increments are integer atomics: no result depends on the order they arrive in.  LORB_E_INVALID, before
 * anything is enqueued: a null required argument, a store of another ctx, n_max_cur < 1, an unknown rule, a null
 * array in d_cur / d_cur_slots / lmap.  Asynchronous on the ctx stream: 1 kernel launch, no stream synchronise, no
 * device-to-host read and no host-to-device copy. */
int lorb_kf_store_observe_dev(lorb_ctx* ctx, lorb_kf_store* store, int32_t frame_id, const lorb_frame_out* d_cur,
                              int32_t n_max_cur, const lorb_frame_slots* d_cur_slots, const int32_t* d_cur_slot_gid,
                              const int32_t* d_cur_slot_id, const lorb_local_map_arrays* lmap,
                              const lorb_local_map_result* d_update, const uint8_t* d_in_view,
                              const int32_t* d_local_status, int32_t found_rule, lorb_kf_observe_result* d_result);

typedef struct lorb_kf_cull_params {   /* a host struct */
  float min_found_ratio;   /* GetFoundRatio() below this culls (src/local_mapping.cpp:92) */
  int32_t age_obs;         /* at this age in frame ids ... */
  int32_t min_obs;         /* ... fewer observations than this culls (:98) */
  int32_t age_out;         /* at this age the point leaves the list (:104) */
} lorb_kf_cull_params;
#define LORB_KF_CULL_REFERENCE { 0.25f, 2, 3, 3 }
typedef struct lorb_kf_cull_result {   /* device memory, like every record of the chain */
  int32_t status;          /* 0; 1: source status or kf outside the store, nothing else was written */
  int32_t kf;
  int32_t n_examined;      /* members of the list on entry */
  int32_t n_bad_before;    /* verdict 1: already bad, left the list */
  int32_t n_culled_ratio;  /* verdict 2 */
  int32_t n_culled_obs;    /* verdict 3 */
  int32_t n_aged_out;      /* verdict 4: left the list */
  int32_t n_recent;        /* verdict 5: members left */
  int32_t n_obs_removed;   /* observations of the culled points */
  int32_t n_slots_erased;  /* keyframe slots set to -1 */
  int32_t n_frame_slots_emptied;   /* slots of the tracker's frame made EMPTY */
  int32_t n_obs_bad_slot;  /* observations of culled points whose keyframe or slot is outside the store or holds
                              another point (a damaged store): skipped */
  int32_t n_obs;           /* the store after the call */
} lorb_kf_cull_result;

/* MapPointsCulling() after ProcessNewFrames, with a real MapPoint::SetBadFlag (src/map_point.cpp:184-199).  Enqueued
 * behind lorb_kf_store_insert_dev and in front of lorb_kf_store_local_ba_dev, with d_kf = &d_insert_result->kf and
 * d_src_status = &d_insert_result->status (nullable) as the BA takes them: a refused insertion's -1 makes the call a
 * no-op.  par is a host struct; LORB_KF_CULL_REFERENCE holds the reference's thresholds.  The group d_cur, n_max_cur,
 * d_cur_slots, d_cur_slot_gid is the tracker's objects of the frame that became K: all given or all NULL.  The
 * store must have its geometry (SetBadFlag needs obs_slot).  On the device, in this order:
 *   a. Status: *d_src_status != 0, or kf outside [0, true n_kf), stores status = 1 and NOTHING else.
 *   b. Verdicts.  cur = kf_fid[kf].  Every p < n_points with recent[p] is examined in the order of
 *      include/lorb/local_mapping.hpp:66-71 (the reference's loop, src/local_mapping.cpp:85-106, without its
 *      erase-then-increment fault):
 *        1. is_bad[p]: it leaves the list.
 *        2. (float)found / (float)visible < min_found_ratio: culled.
 *        3. age = (uint32)(cur - first_fid[p]); age >= age_obs and the observation list shorter than min_obs: culled.
 *        4. age >= age_out: it leaves the list.
 *        5. Otherwise it stays.
 *   c. SetBadFlag of every culled point: is_bad = 1 and recent = 0; for each of its observations (f, s) with f
 *      inside the store, s inside f's row and kf_slot_point[kf_slot_off[f] + s] == p that entry becomes -1
 *      (Frame::EraseMapPoint, src/frame.cpp:896-899; f bad or not), others are counted in n_obs_bad_slot and skipped;
 *      its list is removed from obs_off / obs_kf / obs_slot: every later list moves left, order kept, and the true
 *      n_obs drops.  Left as they are, as in the reference: locked, pos, normal, the distances, desc, the weight
 *      maps, the ordered lists and cov_*.  Point rows are not reclaimed by this call: indices stay stable until the
 *      caller enqueues lorb_kf_store_compact_dev.
 *   d. With the frame group: every slot j < counts[0] whose gid names a point culled BY THIS CALL becomes EMPTY
 *      with gid -1 (K's Frame is the tracker's frame in the reference).  A slot holding a point that was bad before
 *      the call stays as it is.  counts[0] outside [0, n_max_cur]: no slot is touched.
 *   e. The true counts and the record.
 * When no point is culled the kernels after the verdicts return at once: the CSR is not rewritten.  The invariant
 * kf_slot_point[kf_slot_off[f] + obs_slot[o]] == p holds after the call, so lorb_kf_store_ba_gather_dev and
 * lorb_local_map_update_dev read the store as before: a culled point is bad, in no keyframe row and has no
 * observation.  Nothing at or past a true count is written.  All counting is integer.  The per-point scratch mark
 * is back at rest when the call ends, on every path.
 * LORB_E_INVALID, before anything is enqueued: a null required argument, a store of another ctx, a store without
 * geometry, a negative age or a NaN ratio, a frame group given in part (or n_max_cur < 1 with it).
 * Asynchronous on the ctx stream: 4 kernel launches, no stream synchronise, no device-to-host read and no
 * host-to-device copy.
 * Out of scope: KeyFramesCulling (empty in the reference, src/local_mapping.cpp:110-113); reclaiming rows (point
 * rows are not reclaimed here: lorb_kf_store_compact_dev below); MapPoint::EraseObservation's own SetBadFlag at mnObs <= 2 (nothing in the chain erases a
 * single observation); the life of an adopted point before it had a store row. */
int lorb_kf_store_cull_dev(lorb_ctx* ctx, lorb_kf_store* store, const int32_t* d_kf, const int32_t* d_src_status,
                           const lorb_kf_cull_params* par, const lorb_frame_out* d_cur, int32_t n_max_cur,
                           const lorb_frame_slots* d_cur_slots, int32_t* d_cur_slot_gid, lorb_kf_cull_result* d_result);

/* ----------------------------------------------------------------------------------------
 * Reclaiming dead point rows: Map::EraseMapPoint for the store.  lorb_kf_store_cull_dev leaves a culled point its
 * index and its row; lorb_kf_store_compact_dev deletes the rows nothing can name any more, renumbers the survivors
 * in their order and rewrites every place that holds a point index -- in the store, and in the gid tables the
 * caller names.  It is a pure renumbering: every later call gives what it would have given without it, up to the
 * index map.
 * -------------------------------------------------------------------------------------- */
#define LORB_KF_COMPACT_MAX_TABLES 8
typedef struct lorb_kf_gid_table {   /* a host struct of device addresses: one frame's gids */
  int32_t* d_gid;            /* n_max int32: the array lorb_track_motion_refer_pose_dev reads as d_last_slot_gid /
                                d_refer_slot_gid, or any table of store indices the caller keeps */
  int32_t n_max;             /* its bound */
  const int32_t* d_count;    /* the device word with the number of entries in use: the frame's counts[0] */
} lorb_kf_gid_table;
typedef struct lorb_kf_compact_result {   /* device memory, like every record of the chain */
  int32_t status;             /* 0; 1: a source status, a table count outside [0, n_max] or a damaged count of the
                                 store: nothing else was written */
  int32_t n_points_before;    /* the true n_points on entry */
  int32_t n_dropped;          /* rows reclaimed */
  int32_t n_points;           /* the store after the call */
  int32_t n_bad_kept;         /* bad points that keep their row: still observed, or held by a keyframe slot or a table */
  int32_t n_kf_slots_mapped;  /* keyframe slots rewritten through the map (0 when nothing was dropped) */
  int32_t n_gids_mapped;      /* table entries rewritten through the map (0 when nothing was dropped) */
} lorb_kf_compact_result;

/* Enqueued behind lorb_kf_store_local_ba_dev of a keyframe step (or of every n-th one), in front of the next
 * frame's motion stage, with d_src_status = &d_insert_result->status (nullable).  tables is a host array of
 * n_tables <= LORB_KF_COMPACT_MAX_TABLES entries (NULL with n_tables = 0): in the loop the gids of the frame that
 * becomes d_last, of the refer frame, and of every other frame the caller keeps.  Two entries with the same d_gid,
 * n_max and d_count are one table; tables must not overlap otherwise.  d_map is nullable: max_points device int32.
 * NOT between a frame's lorb_local_map_update_dev and its lorb_local_map_ids_back_dev / lorb_kf_store_observe_dev:
 * that frame's local map (l2g, g2l) holds the old indices until the next update rebuilds it.  A lorb_local_map is
 * not remapped.  On the device, in this order, P, O, S the true n_points, n_obs, n_kf_slots on entry:
 *   a. Status, in the first launch and before the first write: *d_src_status != 0, a table's *d_count outside
 *      [0, n_max], or P / S outside the store's capacities stores status = 1 and NOTHING else.  A table that cannot
 *      be examined refuses the whole call: skipping it would leave stale indices in it.
 *   b. Holds.  A bad point p < P named by a keyframe slot kf_slot_point[i], i < S, or by an entry j < *d_count of a
 *      table is held.  (The insertion's "held, point bad: slot, gid and K's row keep g" and the cull's "a slot
 *      holding a point that was bad before the call stays as it is" produce such holds; both stay as they are.)
 *   c. Verdict.  p < P is DROPPED when is_bad[p], its observation list is empty (obs_off clamped to [0, O] as the
 *      cull reads it) and it is not held; every other point is kept.  A point lorb_kf_store_cull_dev culled is
 *      dropped; a bad point that is still observed, or held, is kept (n_bad_kept) and goes in a later call once it
 *      is released.  new(p) = the number of kept points below p: the order of the survivors is preserved, so the
 *      local point table, the numbering of new points and every tile scan see the order they saw before.
 *   d. d_map, when given: new(p) for kept and -1 for dropped p < P; the identity when nothing is dropped.
 *   With nothing to drop the call ends here: NOT A BYTE of the store or of a table changes.
 *   e. Rows.  pos, normal, max_dist, min_dist, desc, locked, is_bad, obs_off, visible, found, first_fid, recent of
 *      every kept p move to row new(p), as bytes, through staging memory the store owns (the pointers of
 *      lorb_kf_store_view / _geom_view / _life_view never change).  obs_kf and obs_slot do not move -- dropped
 *      points have empty lists -- and obs_off[new n_points] = O.  Rows [new n_points, P) return to what a fresh
 *      store has there: zero bytes, is_bad = 1; obs_off (new n_points, P] = 0.
 *   f. Indices.  Every kf_slot_point[i], i < S, and every table entry j < *d_count that holds an index in [0, P)
 *      becomes new(index) -- never -1, by b.  The invariant kf_slot_point[kf_slot_off[f] + obs_slot[o]] == p holds
 *      for the new p.  -1, an index outside [0, P) and entries at or past *d_count stay as they are.
 *   g. The true n_points and the record.  The counters are integer: no result depends on the order atomics arrive.
 * Nothing at or past the OLD true count is written in any array of the store (obs_off: past P), nothing at or past
 * *d_count in a table.  The per-point words at rest between calls (the insertion's owner, the BA's first position,
 * the cull's mark, this call's hold) are at rest over the whole capacity when the call ends, on every path.  The
 * host's bounds stay valid upper bounds and are not touched; lorb_kf_store_counts tightens them at the caller's
 * next wait.  Capacity is decided on the device against the true counts: the next insertion can use the reclaimed
 * rows at once.
 * LORB_E_INVALID, before anything is enqueued: a null required argument (ctx, store, d_result; tables with
 * n_tables > 0), a store of another ctx, n_tables outside [0, LORB_KF_COMPACT_MAX_TABLES], a null d_gid or d_count,
 * n_max < 1, two entries with the same d_gid but another n_max or d_count.
 * Asynchronous on the ctx stream: 5 kernel launches, no stream synchronise, no device-to-host read and no
 * host-to-device copy.
 * Out of scope: keyframe rows and KeyFramesCulling; the weight maps' layout; a host-array form or a C++ adapter;
 * remapping a lorb_local_map; lorb_map_step_dev. */
int lorb_kf_store_compact_dev(lorb_ctx* ctx, lorb_kf_store* store, const int32_t* d_src_status,
                              const lorb_kf_gid_table* tables, int32_t n_tables, int32_t* d_map,
                              lorb_kf_compact_result* d_result);

/* ----------------------------------------------------------------------------------------
 * The appearance of the store and the refresh of a window's points: MapPoint::ComputeDescriptor
 * (src/map_point.cpp:69-129) and MapPoint::UpdateNormalAndDepth (:224-264) on the keyframe store.  The reference
 * calls the two only where a point has exactly one observation (src/visual_odometry.cpp:94-95,392-393); ORB-SLAM2,
 * which it follows, calls them in ProcessNewKeyFrame and after LocalBundleAdjustment.  Like MapPointsCulling it is a
 * call of its own: the mapper step becomes lorb_kf_store_insert_dev -> _cull_dev -> _local_ba_dev -> _refresh_dev ->
 * _compact_dev, and a caller who leaves the refresh out gets the store the other four give.
 *
 * Appearance.  Beside its other arrays the store keeps, at capacity and at addresses that never change:
 *   kf_slot_desc    max_kf_slots x 32 uint8, 16-byte aligned   Frame::GetDescriptor(j) of every keyframe slot,
 *                                                              parallel to kf_slot_point
 *   kf_slot_octave  max_kf_slots int32                         mvKeysUn[j].octave
 *   kf_center       max_kf x 3 float                           mptCameraCenter of every keyframe
 * lorb_kf_store_insert_dev maintains them for keyframe K (still six launches, no wait, no copy): K's descriptor and
 * octave rows are the frame's left descriptors and octave[j] of the slots j < n_cur, kf_center[K] = (Twc[3], Twc[7],
 * Twc[11]) of d_cur_pose -- exactly the values a new point's row is made from.  Nothing at or past a new true count
 * is written; a refused, failed or full insertion writes none of it.  lorb_kf_store_cull_dev and
 * lorb_kf_store_compact_dev renumber neither slots nor keyframes and leave the three arrays alone.
 * A store created with n_kf > 0 has no appearance for its initial keyframes until lorb_kf_store_appear_write:
 * lorb_kf_store_refresh_dev refuses it, as the BA refuses a store without geometry.  An empty store is complete by
 * construction.
 * lorb_kf_store_appear_write waits and replaces the true rows by every non-NULL member: n_kf and n_kf_slots must EQUAL
 * the true counts; an octave outside [0, LORB_MAX_LEVELS) is LORB_E_INVALID with a message naming the entry.  The
 * store is complete once one call has given every array that has rows.  lorb_kf_store_appear_read waits and copies
 * the true rows into every non-NULL member (the n_* fields are the CAPACITIES of the caller's arrays; LORB_E_INVALID
 * when one is below its true count).  lorb_kf_store_appear_view returns the device arrays themselves, the n_* fields
 * their capacities (no wait; the pointers never change).
 * -------------------------------------------------------------------------------------- */
typedef struct lorb_kf_store_appear_host {
  int32_t n_kf, n_kf_slots;   /* write: must equal the true counts; read: capacities */
  uint8_t* kf_slot_desc;      /* n_kf_slots x 32 */
  int32_t* kf_slot_octave;    /* n_kf_slots */
  float* kf_center;           /* n_kf x 3 */
} lorb_kf_store_appear_host;
int lorb_kf_store_appear_write(lorb_kf_store* store, const lorb_kf_store_appear_host* in);   /* waits */
int lorb_kf_store_appear_read(lorb_kf_store* store, const lorb_kf_store_appear_host* out);   /* waits */
int lorb_kf_store_appear_view(const lorb_kf_store* store, lorb_kf_store_appear_host* out);   /* no wait */

#define LORB_KF_REFRESH_CENTERS      1   /* Frame::SetPose of the window's keyframes: kf_center from kf_pose */
#define LORB_KF_REFRESH_NORMAL_DEPTH 2   /* MapPoint::UpdateNormalAndDepth: normal, max_dist, min_dist */
#define LORB_KF_REFRESH_DESCRIPTOR   4   /* MapPoint::ComputeDescriptor: desc */
#define LORB_KF_REFRESH_ALL          7
typedef struct lorb_kf_refresh_result {   /* device memory, like every record of the chain */
  int32_t status;          /* 0; 1: the BA record's status is not 0 (or no good window), nothing else was written */
  int32_t kf;              /* the window's keyframe */
  int32_t n_points;        /* window points */
  int32_t n_refreshed;     /* points whose rows were recomputed */
  int32_t n_bad;           /* skipped: is_bad (:230) */
  int32_t n_empty;         /* skipped: no observation (:238), or none inside the store */
  int32_t n_obs_bad_slot;  /* observations skipped in both halves: a keyframe or slot outside the store */
  int32_t n_desc_changed;  /* BITS of desc that changed, over all points */
  int32_t n_centers;       /* camera centres recomputed: the window's poses, or 0 */
} lorb_kf_refresh_result;

/* Enqueued behind lorb_kf_store_local_ba_dev (or behind a bare lorb_kf_store_ba_gather_dev) and in front of
 * lorb_kf_store_compact_dev.  frame supplies n_levels and scale_factors; d_ba_result is that call's record (status
 * and written are read on the device); what is a non-empty OR of the LORB_KF_REFRESH_* flags.  The point set is the
 * window the store last gathered (its header, local frames and l2g), read in place in device memory.  On the
 * device, in this order:
 *   a. Status: d_ba_result->status != 0 stores status = 1 and NOTHING else.  (1: the BA was a no-op; 3: there are no
 *      points; 2 and 4 already failed on the host.)
 *   b. Centres, with LORB_KF_REFRESH_CENTERS and only when d_ba_result->written == 1: SetPose(Tvec, Rvec) ->
 *      UpdatePoseMat, src/frame.cpp:577-594.  For every local keyframe f = local[i], i < n_poses: Tcw =
 *      pose_to_Tcw(kf_pose[f]), Twc = cv::Mat::inv() (lorb_pose_to_Tcw's and lorb_frame_pose_from_Tcw's arithmetic),
 *      kf_center[f] = (Twc[3], Twc[7], Twc[11]).  Fixed frames and keyframes outside the window are not touched: the
 *      reference moves only the window's frames.  As for Tcw_in of the local stage, the device's double sin / cos are
 *      not libm's, so kf_center is DEFINED as what the store reports; a pose whose rvec is exactly 0 takes
 *      Rodrigues' identity branch and has the host's bits.
 *   c. Points.  For every window point i < n_points, g = l2g[i]: a point with is_bad[g] is skipped and counted in
 *      n_bad (:230; a cull may have run since the gather); an empty observation list is skipped and counted in
 *      n_empty (:238); an observation whose keyframe or slot lies outside the store is skipped in both halves and
 *      counted in n_obs_bad_slot (a list with no other observation counts as empty).
 *      UpdateNormalAndDepth (LORB_KF_REFRESH_NORMAL_DEPTH) over ALL of the point's observations in list order -- the
 *      reference does not skip bad keyframes here -- OpenCV's arithmetic restated as the insertion's one-observation
 *      form restates it, no FMA contraction: d = pos - kf_center[f] in float; nd = sqrt((double)dx dx + (double)dy dy
 *      + (double)dz dz) in that order; sum += d * (float)(1.0 / nd), a float multiply and then a float add per
 *      component, from 0, in list order; normal = sum * (float)(1.0 / (double)n).  mpRefKF is the FIRST entry of the
 *      list: lists ascend by keyframe index and no operation of the store erases an observation of a live point, so
 *      that is the keyframe that created the point (:23, and EraseObservation's mObservations.begin(), :147-148).
 *      dist = (float)norm(pos - kf_center[ref]); max_dist = dist * scale_factors[octave of ref's slot, clamped to
 *      [0, LORB_MAX_LEVELS)]; min_dist = max_dist / scale_factors[n_levels - 1]: the insertion's clamps.
 *      ComputeDescriptor (LORB_KF_REFRESH_DESCRIPTOR) over the observations whose keyframe is not kf_bad (:77-78), in
 *      list order, by lorb_compute_descriptor's rule: element (n - 1) / 2 of each sorted row of the all-pairs
 *      Hamming matrix, self-distance included (:115-118); the smallest median wins, the first index on ties (:119).
 *      desc[g] becomes that observation's kf_slot_desc row.  With no usable observation the descriptor STAYS (the
 *      reference indexes an empty vector there).
 *   d. The record.
 * A point with one observation, created by an insertion, is a fixed point: the inputs are the ones its row was made
 * from, and all four columns keep their bits.  Nothing else in the store changes: no pos, no list, no count, no
 * flag, no life word; the tracker's slots keep their own copies of a descriptor; the BA's per-point scratch stays at
 * rest.  No atomics: every point writes only its own row.
 * Divergences: the four-argument MapPoint constructor (:26-49) leaves mpRefKF unset where this
 * call takes the first observer; an adopted point's first observer is K, the keyframe that adopted it, not the
 * frame whose tracker created it.
 * LORB_E_INVALID, before anything is enqueued: a null argument, a store of another ctx, a store without geometry or
 * without appearance, what zero or with an unknown bit, n_levels outside [1, LORB_MAX_LEVELS], no CURRENT window.
 * Whether the window is current is a host flag: a gather sets it and lorb_kf_store_compact_dev clears it, because
 * a compaction renumbers the points l2g names.  Returns LORB_OK for status 0 and 1.
 * Asynchronous on the ctx stream: 3 kernel launches, the centres in front of the points, no stream synchronise, no
 * device-to-host read and no host-to-device copy.
 * Out of scope: the tracker's slot copies of a descriptor; a host-array form or a C++ adapter; KeyFramesCulling;
 * running the BA on a second stream. */
int lorb_kf_store_refresh_dev(lorb_ctx* ctx, lorb_kf_store* store, const lorb_frame_params* frame,
                              const lorb_kf_ba_result* d_ba_result, int32_t what, lorb_kf_refresh_result* d_result);

/* ----------------------------------------------------------------------------------------
 * Retiring keyframes: Frame::SetBadFlag (src/frame.cpp:684-714) on the keyframe store, with Frame::EraseConnection
 * and its re-sort (:791-798, :754-774) and MapPoint::EraseObservation with the mpRefKF hand-over and the cascade into
 * MapPoint::SetBadFlag (src/map_point.cpp:141-153, :184-199).  The reference's KeyFramesCulling is empty
 * (src/local_mapping.cpp:110-113): it has the mechanism and no rule, so the call takes the keyframes to retire as a
 * list in device memory -- a later rule kernel or the host can both supply it without a wait.  The mapper step
 * becomes lorb_kf_store_insert_dev -> _cull_dev -> _local_ba_dev -> _refresh_dev -> _retire_dev -> _compact_dev.  The
 * call renumbers nothing, so it is also legal anywhere between two frames, and a live lorb_local_map keeps valid
 * indices.
 * -------------------------------------------------------------------------------------- */
#define LORB_KF_RETIRE_MAX_LIST 1024
#define LORB_KF_RETIRE_MAX_PROTECT 4
typedef struct lorb_kf_retire_result {   /* device memory, like every record of the chain */
  int32_t status;            /* 0; 1: a source status, *d_n_list outside [0, n_max_list] or a damaged count of the
                                store: nothing else was written */
  int32_t n_skip_range;      /* list entries outside [0, true n_kf) */
  int32_t n_skip_dup;        /* ... equal to an earlier entry */
  int32_t n_skip_bad;        /* ... whose kf_bad is already set */
  int32_t n_skip_first;      /* ... whose kf_fid is 0 (src/frame.cpp:686-687) */
  int32_t n_skip_protected;  /* ... equal to a protected word */
  int32_t n_retired;         /* the set V */
  int32_t n_obs_erased;      /* entries removed from the lists of points that live on */
  int32_t n_points_bad;      /* points the cascade ran on (MapPoint::SetBadFlag) */
  int32_t n_obs_removed;     /* all entries that left the observation CSR */
  int32_t n_slots_erased;    /* slots of keyframes outside V set to -1 by the cascade */
  int32_t n_obs_bad_slot;    /* observations of such points, keyframe outside V, whose keyframe or slot is outside the
                                store or holds another point (a damaged store): skipped */
  int32_t n_conn_erased;     /* weight-map entries removed from keyframes outside V */
  int32_t n_rows_reordered;  /* keyframes outside V whose ordered list was rebuilt */
  int32_t n_obs, n_cov, n_conn;   /* the store after the call */
} lorb_kf_retire_result;

/* d_list holds n_max_list device int32 keyframe indices, *d_n_list (a device word) of them in use.  d_protect
 * (NULL with n_protect = 0) holds up to LORB_KF_RETIRE_MAX_PROTECT device words: a listed keyframe equal to one of
 * them is skipped -- in the loop the d_refer_kf word and &d_insert_result->kf, which the host cannot know without a
 * wait.  d_src_status is nullable.  The store must have its geometry (the cascade needs obs_slot).  On the device, in
 * this order:
 *   a. Status: *d_src_status != 0, *d_n_list outside [0, n_max_list], or a true count outside its capacity stores
 *      status = 1 and NOTHING else.
 *   b. The set V.  Every list entry is classified in this order, one counter of the record per class: 1. outside
 *      [0, true n_kf); 2. equal to an earlier entry; 3. kf_bad already set; 4. kf_fid[f] == 0 -- the reference's
 *      if(mnId == 0) return; (src/frame.cpp:686-687): a store fresh from create has kf_fid = 0 everywhere and
 *      nothing in it can be retired until lorb_kf_store_life_write says otherwise; 5. protected.  What remains is V
 *      (n_retired).  With an empty V the call ends here: NOT A BYTE of the store changes.
 *   c. Observations (:696-703, src/map_point.cpp:141-153).  For every p < n_points, bad or not, r = the entries of
 *      its list whose keyframe is in V.  r == 0: untouched.  r > 0 and len - r > 2: the entries are removed, order
 *      kept, obs_kf and obs_slot together; mpRefKF stays "the first entry of the list", which is
 *      mObservations.begin()->first (:147-148) because lists ascend by keyframe index, and which is how
 *      lorb_kf_store_refresh_dev reads it.  r > 0 and len - r <= 2: MapPoint::SetBadFlag exactly as
 *      lorb_kf_store_cull_dev step c does it -- is_bad = 1; every remaining observation (f, s), f outside V, with f
 *      inside the store, s inside f's row and kf_slot_point[kf_slot_off[f] + s] == p sets that entry to -1
 *      (n_slots_erased), the others are counted in n_obs_bad_slot; the whole list leaves the CSR; recent, locked,
 *      pos, normal, the distances and desc stay (the reference's list keeps the pointer, and the next cull's verdict 1
 *      drops it).  An observation of a keyframe of V is counted in neither: step e clears that row whole.  The
 *      verdict is taken from the lists alone, whatever a retired keyframe's row says; on a sound store (the invariant
 *      kf_slot_point[kf_slot_off[f] + obs_slot[o]] == p) that is the reference's slot loop.  The CSR is rebuilt by
 *      count, scan and scatter over 1024-point tiles, and the true n_obs drops.
 *   d. Connections (:690-693, :791-798).  For every f in V and every key g of f's weight map with g not in V: if
 *      g's weight map has the key f that entry is removed, the row keeps ascending key order, and g's ordered list is
 *      rebuilt from ALL of g's weight map, ascending by (weight, index), entries below 3 included (:754-774), as the
 *      insertion's step f does for a touched neighbour.  A g whose map names f while f's map does not name g keeps
 *      that entry: the reference iterates f's map.
 *   e. The retired keyframes (:705-711).  For each f in V: conn_n[f] = 0, ord_n[f] = 0, kf_bad[f] = 1, and its whole
 *      slot row becomes -1 (a divergence, DESIGN section 7: the reference leaves mvpMapPoints of an erased frame
 *      alone and nothing reads it again; here a row that still named dead points would hold them against
 *      lorb_kf_store_compact_dev for ever).  kf_pose, kf_slot_uv, the appearance rows, kf_fid and kf_center stay.
 *      cov_off / cov_kf are rebuilt from the first changed row on; the true n_cov and n_conn follow.
 *   f. The record.
 * Order independence: the reference retires keyframes one after another, this call retires a set.  The two agree --
 * for the list in any order -- because a point's count only falls and a retired keyframe's own maps are cleared
 * whatever its neighbours did before.
 * All counting is integer: no result depends on the order atomics arrive in.  Nothing at or past a true count is
 * written.  Every per-point and per-keyframe scratch word at rest between calls (the insertion's owner, the BA's
 * first position, the cull's mark, the compaction's hold, this call's per-keyframe mark) is at rest over the whole
 * capacity when the call ends, on every path.  The host's bounds are not touched.  Keyframe rows are not reclaimed
 * and keyframes are not renumbered.
 * LORB_E_INVALID, before anything is enqueued: a null required argument (ctx, store, d_list, d_n_list, d_result), a
 * store of another ctx, a store without geometry, n_max_list outside [1, LORB_KF_RETIRE_MAX_LIST], n_protect outside
 * [0, LORB_KF_RETIRE_MAX_PROTECT], n_protect > 0 with a null d_protect.
 * Asynchronous on the ctx stream: 6 kernel launches, no stream synchronise, no device-to-host read and no
 * host-to-device copy.
 * Out of scope: a culling rule (KeyFramesCulling); reclaiming or renumbering keyframe rows; the CSR form of the
 * weight maps; a caller's lorb_frame_pose block or slot set of a retired reference keyframe (d_protect exists so that
 * it is not retired); lorb_map_step_dev; a host-array form or a C++ adapter. */
int lorb_kf_store_retire_dev(lorb_ctx* ctx, lorb_kf_store* store, const int32_t* d_list, const int32_t* d_n_list,
                             int32_t n_max_list, const int32_t* d_protect, int32_t n_protect,
                             const int32_t* d_src_status, lorb_kf_retire_result* d_result);

/* (a13) BA::LocalPoseOptimization: poses + points, MPCost for out-of-window (fixed) frames,
 * PoseMPCost for window frames.  One window per problem; batched over windows.
 * obs_frame[k] >= 0 : optimised pose index (PoseMPCost, src/bundle_adjust.cpp:293-301)
 * obs_frame[k] <  0 : fixed frame index (-1 - obs_frame[k]) (MPCost, :283-290) */
typedef struct lorb_ba_window {
  int32_t n_poses, n_fixed, n_points, n_obs;
  float fx, fy, cx, cy;
  const float* pose_init;      /* n_poses x 6 (mRvec|mTvec) */
  const float* fixed_pose;     /* n_fixed x 6 */
  const float* point_init;     /* n_points x 3 */
  const int32_t* obs_point;    /* n_obs */
  const int32_t* obs_frame;    /* n_obs */
  const float* obs_uv;         /* n_obs x 2 */
} lorb_ba_window;

/* (a13) BA::LocalPoseOptimization (src/bundle_adjust.cpp:207-330) over independent windows.  Any
 * number of cameras; LORB_E_UNSUPPORTED for a point observed by more than 256 cameras, or by two
 * cameras more than 127 apart in the plan's camera order (the point-major Schur's point groups,
 * DESIGN.md §7). */
int lorb_ba_local(lorb_ctx* ctx, int32_t n_windows, const lorb_ba_window* windows,
                  const lorb_lm_options* opt, double* const* pose_out,
                  double* const* point_out, lorb_ba_summary* summaries);

/* Device-resident plan for repeated solves of the same window batch (benchmarks, LM in
 * a captured HIP graph).  create: uploads + builds the Schur structure; solve: runs the LM
 * from the uploaded initial values entirely on the device (async); read: copies results. */
typedef struct lorb_ba_plan lorb_ba_plan;
int lorb_ba_plan_create(lorb_ctx* ctx, int32_t n_windows, const lorb_ba_window* windows,
                        lorb_ba_plan** out);
int lorb_ba_plan_solve(lorb_ba_plan* plan, const lorb_lm_options* opt);
int lorb_ba_plan_read(lorb_ba_plan* plan, double* const* pose_out, double* const* point_out,
                      lorb_ba_summary* summaries);
int lorb_ba_plan_destroy(lorb_ba_plan* plan);
/* Device-resident plan of ONE window whose arrays already live in HBM (the LocalMapping step
 * appends the new keyframe's observations on the device).  Sizes that change from call to call are
 * device ints; the capacities bound them.  Observation slots k < *d_n_obs with
 * d_obs_frame[k] < -n_fixed are unused (skipped) -- how a keyframe leaves the window without a
 * compaction.  Observations of one point come out in slot order, as lorb_ba_window's do.  A point
 * may be observed at most once per camera (the reference keys observations by Frame*,
 * include/map_point.h:83).  create: capacity allocations + the first build; update: rebuild from
 * the arrays' current contents (one small readback of counts and the camera covisibility, then
 * sorting and point groups on the device).  solve / read / info / destroy as
 * lorb_ba_plan_*; result_dev writes the solution as float in the caller's pose order (device
 * pointers, either may be NULL; async). */
typedef struct lorb_ba_window_dev {
  int32_t n_poses, n_fixed;          /* host values */
  int32_t max_points, max_obs;       /* capacities of the arrays below */
  const int32_t* d_n_points;         /* device: points in use (<= max_points) */
  const int32_t* d_n_obs;            /* device: observation slots in use (<= max_obs) */
  float fx, fy, cx, cy;
  const float* d_pose_init;          /* n_poses x 6 (mRvec | mTvec) */
  const float* d_fixed_pose;         /* n_fixed x 6 */
  const float* d_point_init;         /* max_points x 3 */
  const int32_t* d_obs_point;        /* max_obs */
  const int32_t* d_obs_frame;        /* max_obs: >= 0 optimised pose, -1-j fixed pose j, < -n_fixed unused */
  const float* d_obs_uv;             /* max_obs x 2 */
} lorb_ba_window_dev;
/* n_poses <= 128 (the camera tables travel as kernel arguments; LORB_E_UNSUPPORTED above) */
int lorb_ba_plan_create_dev(lorb_ctx* ctx, const lorb_ba_window_dev* win, lorb_ba_plan** out);
int lorb_ba_plan_update_dev(lorb_ba_plan* plan, const lorb_ba_window_dev* win);
int lorb_ba_plan_result_dev(lorb_ba_plan* plan, float* d_pose_out, float* d_point_out);
/* (a13) BA::LocalPoseOptimization for a caller that gathers a NEW window on every call -- the drop-in
 * (src/bundle_adjust.cpp:207-330; the call site src/local_mapping.cpp:32).  Same inputs, outputs and
 * errors as lorb_ba_local with one window, but the solver keeps device-built plans
 * (lorb_ba_plan_create_dev) resident across calls, one per camera count (a small LRU), with capacities
 * that grow, so a call costs one host-to-device copy of the window, the device plan build (one small
 * readback), the captured LM graph and one device-to-host copy of the solution -- no per-call plan
 * construction, allocation or graph capture.  Windows the device plans do not take (no cameras /
 * points / observations, more than 128 cameras, a point with 256 or more observations) run through lorb_ba_local's
 * host-built plan on the same GPU kernels.  A point observed twice by one camera is an error (both
 * plan builders; the reference keys observations by Frame*).  One solver per ctx / thread.
 * pose_out: n_poses x 6 doubles (caller order), point_out: n_points x 3 doubles.  Synchronous. */
typedef struct lorb_ba_solver lorb_ba_solver;
int lorb_ba_solver_create(lorb_ctx* ctx, lorb_ba_solver** out);
int lorb_ba_solver_solve(lorb_ba_solver* solver, const lorb_ba_window* window, const lorb_lm_options* opt,
                         double* pose_out, double* point_out, lorb_ba_summary* summary);
/* first n of: [0] resident plans, [1] plan creations so far, [2] 1 if the last call ran on the host-built
 * plan, [3] its S half band, [4] its Cholesky kernel, [5] 1 if its cameras were reordered (RCM) */
int lorb_ba_solver_info(lorb_ba_solver* solver, int32_t* info, int32_t n);
/* the last call's per-iteration records (lorb_ba_plan_trace of the resident plan it ran on; none after a
 * call that took the host-built plan) */
int lorb_ba_solver_trace(lorb_ba_solver* solver, lorb_lm_iteration* out, int32_t cap, int32_t* n_out);
int lorb_ba_solver_destroy(lorb_ba_solver* solver);
/* The ctx's own solver: created on the first call, destroyed by lorb_destroy(ctx) (so it never
 * outlives its ctx, and a new ctx never inherits it).  Not to be passed to lorb_ba_solver_destroy.
 * The adapters' LocalPoseOptimization uses it (include/lorb/adapters.hpp). */
int lorb_ctx_ba_solver(lorb_ctx* ctx, lorb_ba_solver** out);
/* plan structure, first n of: [0] S half band (max over windows, scalar rows), [1] Cholesky kernel of
 * the last solve (0 k_ba_chol, 1 k_ba_chol_w, 2 k_ba_chol_2s, -1 none yet), [2] (camera, camera)
 * blocks, [3] point groups, [4] observations, [5] points, [6] cameras, [7] 1 if some window's
 * cameras were reordered (reverse Cuthill-McKee on the covisibility graph; outputs keep the
 * caller's order), [8] 1: the point-major Schur path (the only one since round 6; point groups span
 * <= 128 cameras), [9] its partial-reduction width (threads per block: 256, 512 or 1024), [10] partial
 * runs of the last build (0: one partial per point group; else the runs of several groups that
 * k_ba_ls_sup folds into one partial each -- windows of more than 512 point groups), [11] kernel
 * launches in the captured graph of the last solve (0: none captured) */
int lorb_ba_plan_info(lorb_ba_plan* plan, int32_t* info, int32_t n);
/* the last solve's per-iteration records of window w (at most min(cap, LORB_LM_TRACE_CAP)); *n_out =
 * records written.  Synchronises. */
int lorb_ba_plan_trace(lorb_ba_plan* plan, int32_t window, lorb_lm_iteration* out, int32_t cap, int32_t* n_out);
/* diagnostics: the plan's stamp buffer -- the two-sided Cholesky's event trace of window 0 (512
 * entries, LORB_CHOL_TRACE builds) or k_ba_ls's phase stamps (8 per point group, LORB_LS_STAMPS
 * builds); 8 entries nothing writes in a regular build */
int lorb_ba_plan_debug_stamps(lorb_ba_plan* plan, unsigned long long* out8);
/* Plan group: the LM solves of several plans on ONE ctx launched as one set of kernels (one launch per
 * kernel for all members, one captured graph), as a plan of several windows is -- for independent
 * windows whose plans are built separately (the device-built plans of several lorb_map windows:
 * lorb_map_group_*).  No reference counterpart (the reference solves one window per call,
 * src/bundle_adjust.cpp:308-314).  Each member's results (poses, points, summary, trace) are
 * bit-identical to lorb_ba_plan_solve of that plan.  Up to 4 members run fused when every member is
 * an unsharded plan on the two-sided Cholesky (lorb_ba_plan_info [1] == 2 after a solve; C3 / C4
 * windows); otherwise the members are solved one after another.  The group does not own its plans:
 * they must outlive it, and may be rebuilt (lorb_ba_plan_update_dev) between solves.  solve is
 * asynchronous (read the members with lorb_ba_plan_read). */
typedef struct lorb_ba_group lorb_ba_group;
int lorb_ba_group_create(lorb_ctx* ctx, int32_t n_plans, lorb_ba_plan* const* plans, lorb_ba_group** out);
int lorb_ba_group_solve(lorb_ba_group* group, const lorb_lm_options* opt);
/* first n of: [0] member plans, [1] solves that ran as one set of launches, [2] graph captures,
 * [3] kernel launches in the captured graph */
int lorb_ba_group_info(lorb_ba_group* group, int32_t* info, int32_t n);
int lorb_ba_group_destroy(lorb_ba_group* group);

/* ----------------------------------------------------------------------------------------
 * SURVEY §8 a17, the LocalMapping "full step" (SURVEY §7 item 8): a local map resident in HBM and
 * the chained step over it.  Replaces LocalMapping::ProcessNewFrames' disabled steps 1-3 followed by
 * BA::LocalPoseOptimization (src/local_mapping.cpp:24-33, 55-76; src/bundle_adjust.cpp:207-330).
 *
 * The map holds keyframes by id: the window [t0, t0 + W) is optimised, the F keyframes before it
 * are fixed (MPCost), older ones are gone.  create: keyframes [0, W) optimised, [-F, 0) fixed.
 * Per step the new keyframe gets id t0 + W and:
 *   1. its descriptors are matched against the map's points (Matcher::SearchLocalPoints,
 *      src/matcher.cpp:319-366 -- crossCheck + minDist filter, trains in map order);
 *   2. a matched keypoint adds an observation (point, keyframe, keypoint uv) to its point
 *      (MapPoint::AddObservation, src/local_mapping.cpp:57-70); an unmatched keypoint with
 *      depth > 0 becomes a new map point at Frame::UnprojectStereo (src/frame.cpp:335-356) with the
 *      keypoint's descriptor, observed by the keyframe.  Appended in keypoint order;
 *   3. the window slides by one keyframe: points that no window keyframe observes leave the map,
 *      observations by keyframes older than the F fixed ones are dropped; order is kept (stable);
 *   4. BA::LocalPoseOptimization of the window (device-built plan, LM with `opt`), then the float
 *      write-back of the window's poses and all points (src/bundle_adjust.cpp:317-329).
 * step_dev is asynchronous except for one small readback (the plan's counts and covisibility).
 * Errors: a step whose new points / observations would exceed the capacities returns LORB_E_NOMEM
 * and leaves the map as it was.  A step that fails later (the plan build of step 4, e.g. a point
 * with 256 or more observations) returns that error with steps 1-3 applied: the map stays usable
 * (its host counts are re-read from the device) and the next step rebuilds the plan.  If even that
 * re-read fails, the map is marked broken and every later step returns LORB_E_DEVICE.
 * ---------------------------------------------------------------------------------------- */
typedef struct lorb_map lorb_map;
typedef struct lorb_map_init {
  int32_t n_window, n_fixed;          /* W <= 128 optimised keyframes (ids 0..W-1), F fixed (ids -1..-F) */
  int32_t max_points, max_obs, max_keypoints;   /* capacities */
  float fx, fy, cx, cy;
  const float* pose;                  /* W x 6 (mRvec | mTvec), row j = keyframe j */
  const float* fixed_pose;            /* F x 6, row j = keyframe -1-j */
  int32_t n_points, n_obs;
  const float* point;                 /* n_points x 3 (MapPoint::GetPos) */
  const uint8_t* point_desc;          /* n_points x 32 (MapPoint::GetDescriptor) */
  const int32_t* obs_point;           /* n_obs */
  const int32_t* obs_kf;              /* n_obs: keyframe id in [-F, W); a point at most once per keyframe */
  const float* obs_uv;                /* n_obs x 2 */
} lorb_map_init;
/* host buffers for lorb_map_read (any may be NULL): sizes from lorb_map_counts */
typedef struct lorb_map_state {
  float* point;                       /* n_points x 3 */
  uint8_t* point_desc;                /* n_points x 32 */
  int32_t* obs_point;                 /* n_obs */
  int32_t* obs_kf;                    /* n_obs: keyframe ids */
  float* obs_uv;                      /* n_obs x 2 */
  int32_t* obs_frame;                 /* n_obs: the BA slot (lorb_ba_window convention) */
  float* pose;                        /* W x 6: keyframes t0 .. t0 + W - 1 */
  float* fixed_pose;                  /* F x 6: keyframes t0 - 1 .. t0 - F */
  int32_t* match_train;               /* last step's keypoints: matched map point (pre-step index) or -1 */
  lorb_ba_summary* summary;           /* last BA solve */
} lorb_map_state;
int lorb_map_create(lorb_ctx* ctx, const lorb_map_init* init, lorb_map** out);
/* frame / pose (the tracked mRvec | mTvec) / Tcw (its 4x4) are host values; descriptors, x, y
 * (Frame::mvKeysUn) and depth (Frame::mvDepth) are device arrays of n keypoints */
int lorb_map_step_dev(lorb_map* map, const lorb_frame_params* frame, const float pose[6], const float Tcw[16],
                      int32_t n, const uint8_t* d_desc, const float* d_x, const float* d_y, const float* d_depth,
                      const lorb_lm_options* opt);
/* Overlap of consecutive steps (default off): with enable = 1, step t+1's match and append run on a
 * stream the map owns, concurrently with step t's BA solve, ordered only after step t's plan build
 * (they touch the map's descriptors, new slots and counts and the map's own key buffers -- nothing
 * the solve or its write-back reads or writes).  Results are bit-identical to enable = 0.
 * REQUIREMENT while enabled: the keyframe arrays handed to lorb_map_step_dev (d_desc, d_x, d_y,
 * d_depth) must be complete when the call is made -- uploaded or produced by work the caller has
 * already synchronised.  The map's stream is not ordered after work still queued on the ctx stream
 * or any other stream, so inputs produced asynchronously need enable = 0 (then every kernel of a
 * step runs on the ctx stream, in order).  The reference's LocalMapping::Run consumes keyframes the
 * tracking thread has finished (src/local_mapping.cpp:19-40), which is the enabled case.  Per-kernel
 * timing (lorb_kernel_timing_enable) runs the steps serially either way. */
int lorb_map_set_overlap(lorb_map* map, int32_t enable);
/* first n of: [0] points, [1] observations, [2] t0, [3] last step's keypoints, [4] its new points,
 * [5] its new observations (matches + new points), [6] its matches, [7] W, [8] steps whose match and
 * append ran overlapped (lorb_map_set_overlap).  Synchronises. */
int lorb_map_counts(lorb_map* map, int32_t* out, int32_t n);
int lorb_map_read(lorb_map* map, const lorb_map_state* state);
int lorb_map_plan(lorb_map* map, lorb_ba_plan** out);   /* the map's BA plan (owned by the map) */
int lorb_map_destroy(lorb_map* map);
/* Several maps stepped together (independent LocalMapping windows on one GPU, north_star's sharding
 * unit): every map on the same ctx.  A group step gives each map its keyframe (kfs[i] for maps[i]) and
 * runs steps 1-3 and the plan build of every map, then ONE BA solve over all of their plans
 * (lorb_ba_group, fused for up to 4 maps per group of launches), then the write-backs.  Each map's
 * state after the step is bit-identical to lorb_map_step_dev of that map alone.  Errors: a map whose
 * steps 1-3 or plan build fail is left as lorb_map_step_dev leaves it after that error; when a map's
 * steps 1-3 fail, the maps after it in the group are not stepped; every other map completes its step
 * (solve and write-back).  The first error is returned.  The group does not own its maps: they must
 * outlive it. */
typedef struct lorb_map_group lorb_map_group;
typedef struct lorb_map_keyframe {
  const lorb_frame_params* frame;
  const float* pose;                  /* 6 (host) */
  const float* Tcw;                   /* 16 (host) */
  int32_t n;
  const uint8_t* d_desc;              /* device arrays of n keypoints, as lorb_map_step_dev */
  const float* d_x;
  const float* d_y;
  const float* d_depth;
} lorb_map_keyframe;
int lorb_map_group_create(int32_t n_maps, lorb_map* const* maps, lorb_map_group** out);
int lorb_map_group_step_dev(lorb_map_group* group, const lorb_map_keyframe* kfs, const lorb_lm_options* opt);
/* first n of: [0] maps, [1] plan groups, [2] steps whose solves all ran as one set of launches per plan
 * group, [3] graph captures over the plan groups */
int lorb_map_group_info(lorb_map_group* group, int32_t* info, int32_t n);
int lorb_map_group_destroy(lorb_map_group* group);

/* ----------------------------------------------------------------------------------------
 * Multi-GPU: point-partitioned ("sharded") local BA.  No reference counterpart:
 * the reference is single-process (its Ceres solve is src/bundle_adjust.cpp:308-314).
 *
 * One process (or thread) per GPU, each with its own lorb_ctx.  Every rank passes the SAME
 * window poses / fixed poses / intrinsics and only ITS points with all of their observations
 * (every observation of a point on the rank that owns the point).  Per LM iteration the ranks
 * all-reduce (i) the camera normal blocks, cost and gradient norms of the linearisation,
 * (ii) the reduced camera system S and its right-hand side, (iii) the model/candidate cost
 * and step norms.  The Cholesky of S and every LM decision are replicated, so all ranks hold
 * identical poses; each rank holds its own points.
 *
 * Communicators: RCCL (ncclAllReduce on the ctx stream, capturable in the LM hipGraph) or a
 * host callback (any host transport, e.g. gloo in tests; the plan then runs eagerly).
 * -------------------------------------------------------------------------------------- */
#define LORB_OP_SUM 0
#define LORB_OP_MAX 1
#define LORB_OP_MIN 2
#define LORB_UNIQUE_ID_BYTES 128
typedef struct lorb_comm lorb_comm;
/* host all-reduce over all ranks, in place on `buf` (count doubles); returns 0 on success */
typedef int (*lorb_host_allreduce_fn)(void* user, double* buf, int64_t count, int32_t op);

int lorb_comm_unique_id(void* id_out /* LORB_UNIQUE_ID_BYTES */);        /* rank 0 only */
int lorb_comm_init_rccl(lorb_ctx* ctx, int32_t nranks, int32_t rank, const void* unique_id,
                        lorb_comm** out);
int lorb_comm_init_host(lorb_ctx* ctx, int32_t nranks, int32_t rank, lorb_host_allreduce_fn fn,
                        void* user, lorb_comm** out);
int lorb_comm_destroy(lorb_comm* comm);
/* ranks in the communicator (ncclCommCount / ncclCommUserRank for RCCL); rank may be NULL */
int lorb_comm_size(lorb_comm* comm, int32_t* nranks, int32_t* rank);
/* all-reduce of device doubles on the ctx stream (send == recv allowed) */
int lorb_comm_allreduce_f64(lorb_comm* comm, const double* d_send, double* d_recv, int64_t count,
                            int32_t op);

/* plan over this rank's shard of each window; solve / read / destroy as lorb_ba_plan_*.
 * read returns the (replicated) poses and this rank's points. */
int lorb_ba_plan_create_sharded(lorb_ctx* ctx, lorb_comm* comm, int32_t n_windows,
                                const lorb_ba_window* shards, lorb_ba_plan** out);

/* the device-built plan (lorb_ba_plan_create_dev) over this rank's shard of ONE window: the shard's
 * points with all of their observations in device arrays (lorb_ba_window_dev; point indices local to
 * the shard), the same n_poses / n_fixed / poses on every rank.  Each build all-reduces the camera
 * covisibility and counts (camera order, band and activity are global; the block pair lists are this
 * rank's), so lorb_ba_plan_update_dev is collective: every rank calls it, and an error on any rank
 * is returned on all of them.  solve / read / result_dev as for lorb_ba_plan_create_sharded. */
int lorb_ba_plan_create_sharded_dev(lorb_ctx* ctx, lorb_comm* comm, const lorb_ba_window_dev* shard,
                                    lorb_ba_plan** out);

/* (a2/a3) with query rows split over ranks.  This rank holds queries
 * [q_base[p], q_base[p] + q_off[p+1] - q_off[p]) of problem p (global numbering) and ALL of its
 * trains.  Outputs as lorb_bf_match_dev for the local queries (global train indices);
 * n_matches[p] is the count over all ranks.  q_off / t_off / q_base are HOST arrays. */
int lorb_bf_match_sharded_dev(lorb_ctx* ctx, lorb_comm* comm, int32_t n_problems,
                              const uint8_t* d_q_desc, const int32_t* q_off, const int32_t* q_base,
                              const uint8_t* d_t_desc, const int32_t* t_off,
                              int32_t* d_cc_train, int32_t* d_cc_dist, int32_t* d_match_train,
                              int32_t* d_n_matches);

/* MapPoint::ComputeDescriptor (src/map_point.cpp:69-129; called at src/visual_odometry.cpp:94,392),
 * batched over map points.  Point p's candidate descriptors -- its observations in
 * std::map<Frame*, size_t> order, bad frames skipped (:74-81) -- are rows [d_off[p], d_off[p+1]) of
 * desc (32 bytes each).  best[p] = index within the point's list of the descriptor whose median
 * Hamming distance to the list (self included; element floor((n-1)/2) of the sorted row) is
 * smallest, first index on ties; -1 for an empty list (the reference indexes an empty vector
 * there).  out_desc (optional, n_points x 32) receives the chosen descriptor (zeros when -1).
 * d_off is a HOST array for lorb_compute_descriptor and a DEVICE array for the _dev variant. */
int lorb_compute_descriptor(lorb_ctx* ctx, int32_t n_points, const int32_t* d_off,
                            const uint8_t* desc, int32_t* best, uint8_t* out_desc);
int lorb_compute_descriptor_dev(lorb_ctx* ctx, int32_t n_points, const int32_t* d_off,
                                const uint8_t* d_desc, int32_t* d_best, uint8_t* d_out_desc);

/* Rodrigues vector -> Tcw (float), cv::Rodrigues semantics (double internally). */
void lorb_pose_to_Tcw(const float rvec[3], const float tvec[3], float Tcw[16]);
/* Tcw -> Rodrigues vector | translation: cv::Rodrigues matrix -> vector (OpenCV 3.x cvRodrigues2's
 * 3 x 3 branch, double internally, the result rounded to float) and column 3
 * (Frame::UpdatePoseVector, src/frame.cpp:590-605).  The orthogonalisation R <- U * V^T is the
 * library's own one-sided Jacobi iteration, not OpenCV's.  LORB_E_INVALID on a null
 * argument. */
int lorb_Tcw_to_pose(const float Tcw[16], float R[3], float T[3]);
/* Frame::SetPose(Tcw) (src/frame.cpp:570-575): the matrix as given, the vector of it, Twc =
 * cv::Mat::inv() (LU32f), status 0.  LORB_E_INVALID on a null argument. */
int lorb_frame_pose_from_Tcw(const float Tcw[16], lorb_frame_pose* out);

#ifdef __cplusplus
}
#endif
#endif /* LORB_C_H */
