/*
 * orbx_c.h — C ABI of the MI355X-native ORB front-end (liborbx.so).
 *
 * This is the drop-in boundary for ORB-SLAM2's ORBextractor / ORBmatcher hot
 * path (reference: falfab/orb_slam_cuda). Plain C types only; device memory
 * is addressed by plain pointers and HIP streams by `void*`.
 *
 * Entry points and the reference interface each one replaces:
 *   orbx_create            ORBextractor::ORBextractor(nfeatures, scaleFactor,
 *                          nlevels, iniThFAST, minThFAST, width, height)
 *                          include/ORBextractor.h:82-83, src/ORBextractor.cc:496-560
 *   orbx_destroy           ORBextractor::~ORBextractor  src/ORBextractor.cc:800
 *   orbx_extract           ORBextractor::operator()(image, mask, keypoints,
 *                          descriptors)  include/ORBextractor.h:90-92,
 *                          src/ORBextractor.cc:1538-1815 (CPU branch 1701-1809)
 *   orbx_extract_batch     same, B frames per call, device-resident in/out
 *                          (frame batching for MI355X; no reference equivalent)
 *   orbx_get_scales        GetScaleFactors / GetInverseScaleFactors /
 *                          GetScaleSigmaSquares / GetInverseScaleSigmaSquares
 *                          include/ORBextractor.h:94-114
 *   orbx_get_levels_info   GetLevels + per-level sizes / mnFeaturesPerLevel
 *   orbx_get_level         public mvImagePyramid[level]  include/ORBextractor.h:116
 *                          (read by Frame::ComputeStereoMatches src/Frame.cc:472,562,579)
 *   orbx_set_host_pyramid / orbx_get_host_pyramid  the same, filled by
 *                          orbx_extract itself into pinned memory (opt-in)
 *   orbm_descriptor_distance  ORBmatcher::DescriptorDistance
 *                          include/ORBmatcher.h:44, src/ORBmatcher.cc:1647-1663
 *   orbm_search_for_initialization  ORBmatcher::SearchForInitialization
 *                          include/ORBmatcher.h:69, src/ORBmatcher.cc:405-520
 *                          (+ Frame::AssignFeaturesToGrid/GetFeaturesInArea
 *                          src/Frame.cc:229-244,326-391)
 *   orbm_search_by_bow     ORBmatcher::SearchByBoW(KeyFrame*, Frame&, ...)
 *                          include/ORBmatcher.h:65, src/ORBmatcher.cc:159-288;
 *                          kf_vs_kf=1: SearchByBoW(KeyFrame*, KeyFrame*, ...)
 *                          include/ORBmatcher.h:66, src/ORBmatcher.cc:522-655
 *   orbm_hamming_top2      the best/second Hamming inner loop shared by every
 *                          matcher (dense, device-resident, batched)
 *   orbm_compute_stereo_matches  Frame::ComputeStereoMatches (mvuRight, mvDepth)
 *                          include/Frame.h:82, src/Frame.cc:465-639
 *   orbm_stereo_frame      the stereo Frame constructor's two ExtractORB
 *                          threads + ComputeStereoMatches, src/Frame.cc:77-89
 *   orbx_undistort_points  cv::undistortPoints(src, dst, K, dist, Mat(), K) as
 *                          Frame calls it (OpenCV 3.x, five fixed iterations)
 *   orbx_undistort_keypoints / orbx_frame_tail_batch  Frame::UndistortKeyPoints
 *                          src/Frame.cc:403-433 (+ ComputeStereoFromRGBD :642-663
 *                          with the convertTo of src/Tracking.cc:276-277)
 *   orbx_image_bounds      Frame::ComputeImageBounds  src/Frame.cc:435-463
 *   orbx_rgbd_frame        the RGB-D Frame constructor's ExtractORB +
 *                          UndistortKeyPoints + ComputeStereoFromRGBD,
 *                          src/Frame.cc:134-144 (no depth: the monocular
 *                          constructor's :189-197)
 *   orbx_rectify_maps      cv::initUndistortRectifyMap(K, D, R, P.rowRange(0,3)
 *                          .colRange(0,3), size, CV_32F, M1, M2)
 *                          Examples/Stereo/stereo_euroc.cc:97-98,
 *                          Examples/ROS/ROS_WS/src/stereo/src/ros_stereo.cc:106-107
 *   orbx_remap_host / orbx_rectify_create / orbx_rectify_batch / orbx_set_rectify
 *                          cv::remap(im, imRect, M1, M2, cv::INTER_LINEAR) on the
 *                          left and the right image before TrackStereo,
 *                          stereo_euroc.cc:136-137, ros_stereo.cc:161-162
 *   orbm_search_by_projection  ORBmatcher::SearchByProjection(Frame&,
 *                          const vector<MapPoint*>&, th)  include/ORBmatcher.h:48,
 *                          src/ORBmatcher.cc:45-126 (Tracking::SearchLocalPoints)
 *   orbm_search_by_projection_last_frame  ORBmatcher::SearchByProjection(
 *                          Frame& CurrentFrame, const Frame& LastFrame, th,
 *                          bMono)  include/ORBmatcher.h:52, src/ORBmatcher.cc:1328-1470
 *                          (Tracking::TrackWithMotionModel)
 *   orbm_search_by_projection_keyframe  ORBmatcher::SearchByProjection(
 *                          Frame&, KeyFrame*, const set<MapPoint*>&, th,
 *                          ORBdist)  include/ORBmatcher.h:56,
 *                          src/ORBmatcher.cc:1472-1599 (Tracking::Relocalization)
 *   orbm_search_by_projection_sim3  ORBmatcher::SearchByProjection(KeyFrame*,
 *                          cv::Mat Scw, const vector<MapPoint*>&,
 *                          vector<MapPoint*>&, th)  include/ORBmatcher.h:60,
 *                          src/ORBmatcher.cc:290-403 (LoopClosing::ComputeSim3)
 *   orbm_fuse / orbm_fuse_sim3  ORBmatcher::Fuse(KeyFrame*, vector<MapPoint*>,
 *                          th) / Fuse(KeyFrame*, Scw, vpPoints, th,
 *                          vpReplacePoint)  include/ORBmatcher.h:80,83,
 *                          src/ORBmatcher.cc:825-975, 977-1100 (matching part)
 *   orbm_search_by_sim3    ORBmatcher::SearchBySim3  include/ORBmatcher.h:77,
 *                          src/ORBmatcher.cc:1102-1326
 *   orbm_search_by_projection_pose_batch  all of the above, batched on device
 *   orbm_search_for_triangulation  ORBmatcher::SearchForTriangulation
 *                          include/ORBmatcher.h:72, src/ORBmatcher.cc:657-823
 *   orbm_pose_optimization / _batch / _host  Optimizer::PoseOptimization(Frame*)
 *                          include/Optimizer.h:53, src/Optimizer.cc:334-543
 *   orbm_sim3_ransac / _batch / _host  Sim3Solver (ctor, SetRansacParameters,
 *                          iterate / find)  include/Sim3Solver.h, src/Sim3Solver.cc:37-423
 *   orbm_optimize_sim3 / _batch / _host  Optimizer::OptimizeSim3  include/Optimizer.h:57,
 *                          src/Optimizer.cc:1190-1385 (LoopClosing::ComputeSim3)
 *   orbm_create_new_map_points / _batch / _host  the loop over vMatchedIndices of
 *                          LocalMapping::CreateNewMapPoints  src/LocalMapping.cc:317-464
 *   orbm_compute_f12       LocalMapping::ComputeF12  src/LocalMapping.cc:572-589
 *   orbm_initialize / _batch / _host  Initializer::Initialize and everything under
 *                          it  include/Initializer.h, src/Initializer.cc:44-929
 *                          (Tracking::MonocularInitialization src/Tracking.cc:638-700)
 *   orbv_load_text / orbv_create  ORBVocabulary::loadFromTextFile
 *                          (DBoW2 TemplatedVocabulary, include/ORBVocabulary.h:30,
 *                          Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1338-1418)
 *   orbv_transform         Frame::ComputeBoW  src/Frame.cc:394-401 ->
 *                          TemplatedVocabulary::transform(features, BowVector,
 *                          FeatureVector, levelsup)  TemplatedVocabulary.h:1127-1256
 *   orbv_score             ORBVocabulary::score(v1, v2) (LoopClosing::DetectLoop
 *                          src/LoopClosing.cc:160), the six DBoW2 scorings
 *                          Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-311
 *   orbdb_add / orbdb_add_batch / orbdb_erase / orbdb_clear  KeyFrameDatabase::
 *                          add / erase / clear  src/KeyFrameDatabase.cc:76-109
 *   orbdb_query + orbdb_select_candidates  KeyFrameDatabase::DetectLoopCandidates
 *                          (:112-233, LoopClosing::DetectLoop src/LoopClosing.cc:173)
 *                          and DetectRelocalizationCandidates (:235-345,
 *                          Tracking::Relocalization src/Tracking.cc:1436)
 *   orbdb_query_batch      their counting and scoring, batched on device
 *   orbdb_score_slots      the score loop over covisibles src/LoopClosing.cc:147-165
 *
 * Error behaviour: every call returns ORBX_OK or a negative code; the
 * message of the last failure on the calling thread is orbx_last_error().
 * The C++ shim (include/orb_slam2/ORBextractor.h) turns codes into
 * std::runtime_error, as the reference's NVXIO_SAFE_CALL does
 * (nvxio/include/OVX/UtilityOVX.hpp:129-137).
 *
 * Threading: handles are independent and may be used concurrently from
 * different threads (the reference runs two extractors at once for stereo,
 * src/Frame.cc:77-80). One handle is not reentrant.
 */
#ifndef ORBX_C_H
#define ORBX_C_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORBX_OK 0
#define ORBX_EINVAL (-1)    /* bad argument / unsupported configuration   */
#define ORBX_EDEVICE (-2)   /* HIP runtime error or no gfx950 device       */
#define ORBX_ECAPACITY (-3) /* caller buffer or internal capacity too small */
#define ORBX_ENOMEM (-4)    /* device allocation failed                    */

/* Binary-identical to cv::KeyPoint: pt.x, pt.y, size, angle, response
 * (float), octave, class_id (int) = 28 bytes. class_id is always -1. */
typedef struct orbx_kp {
  float x, y, size, angle, response;
  int32_t octave, class_id;
} orbx_kp;

/* Parity-mode switches. */
#define ORBX_SCALE_U 0        /* level geometry from scaleFactor^l (default)   */
#define ORBX_SCALE_F 1        /* fork: VX ORB pyramid sizes override scales    */
#define ORBX_PATTERN_FORK 0   /* bit_pattern_31_[96] = VX_FAILURE-2 = -3 (default) */
#define ORBX_PATTERN_UPSTREAM 1 /* upstream ORB-SLAM2 table (-2)              */

typedef struct orbx_config {
  int nfeatures;      /* ORBextractor.nFeatures                  */
  float scale_factor; /* ORBextractor.scaleFactor                */
  int nlevels;        /* ORBextractor.nLevels (1..16)            */
  int ini_th_fast;    /* ORBextractor.iniThFAST                  */
  int min_th_fast;    /* ORBextractor.minThFAST                  */
  int width, height;  /* frame size (Camera.width / Camera.height); 0 x 0 in
                       * mode U = unknown until the first orbx_extract, as
                       * Tracking passes for the mono yamls that lack the keys
                       * (src/Tracking.cc:124-133): the plan is then built on
                       * the first image (mode F needs the size: EINVAL) */
  int device;         /* HIP device ordinal                       */
  int max_batch;      /* frames per orbx_extract_batch call (>=1); the
                       * pyramid planes of levels >= 1 of all max_batch
                       * frames must stay below 2 GiB (FAST's cell records
                       * hold 32-bit plane offsets): about 316 frames at
                       * 1920x1080 with 8 levels x 1.2, 39 at 4096x4096;
                       * orbx_create returns EINVAL past it */
  int scale_mode;     /* ORBX_SCALE_*                             */
  int pattern_mode;   /* ORBX_PATTERN_*                           */
  int reserved[5];    /* must be zero                             */
} orbx_config;

typedef struct orbx_extractor* orbx_handle;

const char* orbx_last_error(void);
const char* orbx_version(void);

int orbx_create(const orbx_config* cfg, orbx_handle* out);
int orbx_destroy(orbx_handle h);

/* Maximum keypoints one frame can produce (sizes per-frame output slots);
 * 0 while a handle created with width/height 0 has seen no image. */
int orbx_frame_capacity(orbx_handle h);

/* ORBextractor::operator(): host image in, host keypoints/descriptors out.
 * Synchronous. Empty image (w==0||h==0) -> *n = 0, ORBX_OK (reference
 * returns with outputs untouched, src/ORBextractor.cc:1542-1543). */
int orbx_extract(orbx_handle h, const uint8_t* img, int w, int h_, size_t stride,
                 orbx_kp* kps, int cap, uint8_t* desc, int* n);

/* Batched, device-resident, asynchronous on `stream` (hipStream_t; NULL =
 * the default stream).
 * d_frames: batch frames of (height x width) u8, row stride `row_stride`,
 * frame i at d_frames + i*frame_pitch. The kernels read each row in 16-byte
 * chunks: every row, the last row of the last frame included, must be
 * readable up to ceil16(width) bytes from its start (a 64-byte pitch, as
 * bench.py uses, always is). Outputs: frame i's keypoints at
 * d_kps + i*cap, descriptors at d_desc + i*cap*32, count in d_counts[i],
 * where cap = orbx_frame_capacity(h). Level-major order as the reference.
 * Calls on one handle from several threads are serialised by the handle's
 * lock (a synchronous orbx_extract holds it until its own work finished). */
int orbx_extract_batch(orbx_handle h, const uint8_t* d_frames, int batch,
                       size_t frame_pitch, size_t row_stride, orbx_kp* d_kps,
                       uint8_t* d_desc, int* d_counts, void* stream);

int orbx_get_scales(orbx_handle h, float* scale, float* inv_scale,
                    float* sigma2, float* inv_sigma2);
int orbx_get_levels_info(orbx_handle h, int* nlevels, int* level_w,
                         int* level_h, int* nfeatures_per_level);
/* Copy pyramid level `level` of frame `frame` of the last extraction to host
 * (mvImagePyramid). `blurred`=1 returns the 7x7 Gaussian-blurred level used
 * for the descriptors instead (stage probe). Waits for the handle's own last
 * launch only (not the device); served from the host pyramid below when that
 * holds the level. */
int orbx_get_level(orbx_handle h, int frame, int level, int blurred,
                   uint8_t* out, size_t out_stride);
/* Host pyramid: the reference's public mvImagePyramid (include/ORBextractor.h:116),
 * filled in place by ComputePyramid (src/ORBextractor.cc:1837-1863) and read
 * by Frame::ComputeStereoMatches (src/Frame.cc:472,562,579). With enable != 0
 * every later orbx_extract also leaves its frame's pyramid in handle-owned
 * pinned host memory: the levels >= 1 are copied on a branch of the call's
 * graph forked right after the pyramid kernel (the copy overlaps FAST ..
 * BRIEF), level 0 is the call's own pinned input staging. Off by default. */
int orbx_set_host_pyramid(orbx_handle h, int enable);
/* The host pyramid of the last orbx_extract: levels[l] / pitches[l] (bytes
 * between rows) for l < nlevels, valid until the next extraction on the
 * handle (as the reference's buffers are until its next operator() call).
 * ORBX_EINVAL when it is off or the last extraction was a batch call. */
int orbx_get_host_pyramid(orbx_handle h, const uint8_t** levels, size_t* pitches,
                          int cap_levels);
/* Stage probe: FAST + per-cell NMS candidates of (frame, level) of the last
 * extraction, in reference order, as keypoints (x,y relative to the border
 * box, response = FAST score). */
int orbx_get_fast_candidates(orbx_handle h, int frame, int level, orbx_kp* out,
                             int cap, int* n);
/* Quadtree tie-rule exposure of frames [frame0, frame0 +
 * nframes) of the last extraction: per (frame, level) three ints {events,
 * group nodes, kept keypoints}. DistributeOctTree's sorted rounds split nodes
 * in (size, heap-pointer) order (src/ORBextractor.cc:1041-1042) and stop at N;
 * an event is a cut-off inside a group of equal-size nodes, where the
 * reference's choice depends on its allocator and this library's on node
 * creation order (the oracle's rule). `kept keypoints` counts the outputs
 * that come from that group. Synchronous (waits for the device). */
int orbx_get_tie_stats(orbx_handle h, int frame0, int nframes, int* out);
/* Which DistributeOctTree implementation ran per (frame, level) of frames
 * [frame0, frame0 + nframes) of the last extraction: 1 = the sorted-key path
 * (node = contiguous range of keys binned by quadtree path code), 0 = the
 * legacy rounds (levels with more keys than the workgroup's registers hold,
 * a node to split below the bins' depth, or ORBX_QT_SORTED=0). Both give the
 * reference's output; this is a diagnostic for tests and profiles.
 * Synchronous (waits for the device). */
int orbx_get_quadtree_paths(orbx_handle h, int frame0, int nframes, int* out);
/* Device status word of the handle's kernels since the last call (0 = ok;
 * bit 1: quadtree round limit, bit 2: quadtree output over capacity, bit 3:
 * a quadtree node without keys, an internal invariant, never expected).
 * Waits for the device; `reset` != 0 clears it. orbx_extract checks and clears
 * it itself; batch callers (orbx_extract_batch) poll it here. */
int orbx_get_status(orbx_handle h, int reset, int* status);
/* The rBRIEF test table the kernels use (bit_pattern_31_,
 * src/ORBextractor.cc:236-494): 1024 ints in the reference's flat order
 * (test i = entries 4i..4i+3 = x0, y0, x1, y1), for pattern_mode
 * ORBX_PATTERN_FORK (entry 96 = VX_FAILURE-2 = -3, :261-262) or
 * ORBX_PATTERN_UPSTREAM (-2). Host only, no device needed. */
int orbx_get_pattern(int pattern_mode, int* out1024);
/* Per-stage device time (ms) of the last extraction, in launch order
 * (orbx_get_stage_order), stage names as the reference's GetTime labels
 * (src/ORBextractor.cc:1131,1331,1737,1753,1841). Filled only when the handle
 * was created with timing enabled (ORBX_TIMING=1 in the environment). */
int orbx_get_stage_times(orbx_handle h, float* ms, const char** names, int cap,
                         int* n);
/* The extraction stages' launch order of handle h (NULL: the default) as 5
 * letters + NUL into out[6]: p pyramid, b Gaussian blur, f FAST + grid, q
 * quadtree, o angle + descriptor (default "pfqbo", or ORBX_EXTRACT_ORDER).
 * Host only. */
int orbx_get_stage_order(orbx_handle h, char* out);
/* Set a handle's stage launch order for its later extractions: the pyramid
 * first, orient+BRIEF last, FAST before the quadtree ("pfqbo", "pbfqo",
 * "pfbqo"). Results do not depend on it; how the launches interleave with a
 * caller's other streams does (a pipeline that overlaps ComputeBoW and
 * SearchByBoW with the next extraction runs faster with "pbfqo", DESIGN.md
 * section 6). ORBX_EINVAL for any other string. */
int orbx_set_stage_order(orbx_handle h, const char* order);
/* Record caller-owned HIP events (ORBX_STAGE_EVENTS of them, hipEvent_t as
 * void*) between the stages of the NEXT orbx_extract_batch call on its
 * stream: ev[0] before the first stage, ev[i + 1] after the i-th stage
 * launched (orbx_get_stage_order). Lets a caller time every kernel of every
 * call without a host synchronisation. One-shot. */
#define ORBX_STAGE_EVENTS 6
int orbx_set_stage_events(orbx_handle h, void** events);

/* The descriptor rotation's sin/cos (src/ORBextractor.cc:199-200: glibc
 * sinf/cosf on a float argument) exactly as the kernels compute it, on the
 * host: s[i] = sinf(x[i]), c[i] = cosf(x[i]) for |x| < 120. For checking the
 * restatement against a host libm. */
int orbx_sincosf_glibc(const float* x, int n, float* s, float* c);

/* ------------------------------------------------------------- matcher */
typedef struct orbx_matcher* orbm_handle;

const char* orbm_last_error(void);

/* Workspace for batched matching of up to max_pairs frame pairs with up to
 * max_kps keypoints per frame. */
int orbm_create(int device, int max_pairs, int max_kps, orbm_handle* out);
int orbm_destroy(orbm_handle m);

/* Device status word of the matcher's batched kernels since the last call
 * (0 = ok; bit 16: orbm_hamming_top2 input over its limits, nA[p] > a_cap
 * or nB[p] > 65535, the excess rows / candidates were not searched; bit 32:
 * orbm_search_by_bow_batch saw a count above kp_pitch or a FeatureVector
 * index outside [0, n), which was skipped; bit 64:
 * orbm_search_local_points_batch found more than 8192 map points in view in
 * a frame, the points in view after the first 8192 were not searched; bit
 * 128: orbm_refresh_map_points_batch / orbm_refresh_map_points skipped a
 * point whose list names a keyframe, descriptor row or octave out of range;
 * bit 256: orbm_pose_optimization_batch / orbm_pose_optimization left out a
 * keypoint whose octave or map point row is out of range; bit 512:
 * orbm_sim3_ransac_batch / orbm_sim3_ransac treated an entry as unmatched
 * because its match12 or kp_index1 value is at or above the keyframe's
 * count, its keypoint's octave is outside [0, nlevels), or the gathered
 * list would not fit the pitch; bit 1024: orbm_create_new_map_points_batch /
 * orbm_create_new_map_points rejected a match whose idx2 is at or above n2,
 * whose keypoint's octave is outside [0, nlevels), or whose stereo keypoint
 * has mvDepth <= 0 where UnprojectStereo needs it; bit 2048: the same calls
 * found more new points than `capacity` and dropped the excess; bit 4096:
 * orbm_initialize_batch / orbm_initialize left a match out whose matches12
 * value is at or above n2; bit 8192: orbm_optimize_sim3_batch /
 * orbm_optimize_sim3 left an entry out whose match12, found12 or found21
 * value is at or above the other keyframe's count or whose keypoint's octave
 * is outside [0, nlevels)).
 * SearchForInitialization keeps no
 * candidate lists (8 smallest keys per query) and never sets it. Waits for
 * the matcher's own launches that may set it (on whatever streams they ran),
 * not for the device; `reset` != 0 clears it. The synchronous entry points
 * check and clear it themselves.
 *
 * Device workspaces (candidate lists, stereo SAD, pose picks, the compacted
 * points in view of SearchLocalPoints, SearchByBoW row records and
 * histograms) belong to the
 * handle: batched calls on different streams are ordered by the library
 * (each waits for the previous user of the workspace), so they never
 * overlap on it. The same holds for an extractor handle's plan buffers, and
 * orbm_compute_stereo_matches_batch orders itself after and before the two
 * extractors whose pyramids it reads. */
int orbm_get_status(orbm_handle m, int reset, int* status);

/* Hamming distance of two 32-byte descriptors (host, exact). */
int orbm_descriptor_distance(const uint8_t* a, const uint8_t* b);

/* Dense best/second search, device-resident, batched over `pairs`:
 * for pair p, A = d_A + p*a_pitch (nA[p] rows of 32 B), B likewise.
 * Outputs per query row (stride a_cap): best index (-1 if none), best
 * distance and second-best distance (256 when absent), with SearchByBoW's
 * sequential semantics (strict '<', first index wins ties). nB[p] <= 65535
 * (the candidate index shares a 32-bit key with the distance). */
int orbm_hamming_top2(orbm_handle m, const uint8_t* d_A, size_t a_pitch,
                      const int* d_nA, int a_cap, const uint8_t* d_B,
                      size_t b_pitch, const int* d_nB, int pairs,
                      int* d_best_idx, int* d_best, int* d_second, void* stream);

/* Frame-side inputs of SearchForInitialization: mvKeysUn (orbx_kp) and
 * descriptors, plus the image bounds Frame uses for its 64x48 grid
 * (mnMinX, mnMaxX, mnMinY, mnMaxY). */
typedef struct orbm_grid_bounds {
  float min_x, max_x, min_y, max_y;
} orbm_grid_bounds;

/* ORBmatcher::SearchForInitialization on host buffers (synchronous).
 * prev_xy: 2*n1 floats, vbPrevMatched, updated in place. matches12: n1.
 * n1 / n2 are not bounded by the matcher's max_kps: only octave-0 keypoints
 * take part (compacted on the host; up to the batch call's bound below per
 * frame: 10,192 at the reference's 0.9, 8192 at 0.7), and the kernels keep no candidate lists, so any
 * window density is matched, never refused for want of scratch. */
int orbm_search_for_initialization(orbm_handle m, const orbx_kp* kp1,
                                   const uint8_t* desc1, int n1,
                                   const orbx_kp* kp2, const uint8_t* desc2,
                                   int n2, orbm_grid_bounds bounds,
                                   float* prev_xy, int window, float nnratio,
                                   int check_ori, int* matches12,
                                   int* nmatches);

/* Batched device-resident variant: pair p matches frame F1 = (d_kp1 +
 * p*kp_pitch, d_desc1 + p*kp_pitch*32, d_n1[p]) against F2 likewise.
 * d_prev_xy: pairs x kp_pitch x 2 floats (in/out), or NULL to centre the
 * windows on F1's own keypoints (the initial mvbPrevMatched of
 * Tracking::MonocularInitialization, src/Tracking.cc:645-647; nothing is
 * written back then); d_matches12: pairs x kp_pitch; d_nmatches: pairs.
 * kp_pitch <= min(max_kps, 10,192, 2^(20 - dbits)); any window density is
 * matched (the kernels keep each query's 8 smallest keys, kInitK, not its
 * candidate list). 10,192 is the resolve kernel's LDS; dbits depends on
 * nnratio: distances are clamped to 2^dbits - 1 with the smallest dbits in
 * 6..9 for which nnratio * (2^dbits - 1) > 50, so the bound is 10,192 for
 * nnratio > 0.794, 8192 above 0.394, 4096 above 0.196 and 2048 below.
 * ECAPACITY's message names the bound that applied. */
int orbm_search_for_initialization_batch(
    orbm_handle m, const orbx_kp* d_kp1, const uint8_t* d_desc1,
    const int* d_n1, const orbx_kp* d_kp2, const uint8_t* d_desc2,
    const int* d_n2, int kp_pitch, int pairs, orbm_grid_bounds bounds,
    float* d_prev_xy, int window, float nnratio, int check_ori,
    int* d_matches12, int* d_nmatches, void* stream);

/* The MapPoint fields ORBmatcher::SearchByProjection(Frame&, vector<MapPoint*>,
 * th) reads (filled by Frame::isInFrustum, src/Frame.cc:277-324):
 * mTrackProjX/Y/XR, mTrackViewCos, mnTrackScaleLevel; track_in_view =
 * mbTrackInView && !isBad(); obs_positive = Observations() > 0. 24 bytes. */
typedef struct orbm_map_point_proj {
  float proj_x, proj_y, proj_xr, view_cos;
  int32_t predicted_level;
  uint8_t track_in_view, obs_positive, pad[2];
} orbm_map_point_proj;

/* SearchByProjection(Frame&, vpMapPoints, th) on host buffers (synchronous).
 * Frame: mvKeysUn (kps), mDescriptors, N; uright = mvuRight (NULL for a
 * monocular frame); bounds = mnMinX/MaxX/MinY/MaxY; scale = mvScaleFactors
 * (nlevels); blocked[idx] = mvpMapPoints[idx] && Observations() > 0 on entry.
 * Map points in vpMapPoints order with their descriptors (GetDescriptor()).
 * out[idx] = index into vpMapPoints of the point assigned to keypoint idx by
 * this call (the shim stores vpMapPoints[out[idx]] into mvpMapPoints[idx]),
 * -1 where the keypoint was not assigned. Up to 8192 map points. */
int orbm_search_by_projection(orbm_handle m, const orbx_kp* kps, const uint8_t* desc,
                              int n, const float* uright, orbm_grid_bounds bounds,
                              const float* scale, int nlevels, const uint8_t* blocked,
                              const orbm_map_point_proj* mps, const uint8_t* mpdesc,
                              int nmp, float th, float nnratio, int* out,
                              int* nmatches);

/* Batched device-resident variant: frame f's keypoints at d_kps + f*kp_pitch
 * (d_n[f] of them; descriptors, uright (or NULL), blocked and out likewise at
 * kp_pitch), its map points at d_mps + f*mp_pitch (d_nmp[f]; descriptors
 * likewise). All frames share the grid bounds and scale factors. */
int orbm_search_by_projection_batch(
    orbm_handle m, const orbx_kp* d_kps, const uint8_t* d_desc, const int* d_n,
    int kp_pitch, const float* d_uright, orbm_grid_bounds bounds,
    const float* scale, int nlevels, const uint8_t* d_blocked,
    const orbm_map_point_proj* d_mps, const uint8_t* d_mpdesc, const int* d_nmp,
    int mp_pitch, int frames, float th, float nnratio, int* d_out,
    int* d_nmatches, void* stream);

/* ---------------------------------------- pose-projection search overloads
 * The SearchByProjection overloads that project MapPoint world positions
 * with a pose inside the matcher. Frame/KeyFrame camera fields: fx, fy, cx,
 * cy, mb, mbf and rows 0..2 of mTcw, row-major (the Sim3 overload passes
 * Scw rows 0..2 here). */
typedef struct orbm_camera {
  float fx, fy, cx, cy, mb, mbf;
  float Tcw[12];
} orbm_camera;

/* A MapPoint as these overloads read it: GetWorldPos(), GetNormal() (Sim3
 * overload), mfMinDistance / mfMaxDistance (GetMin/MaxDistanceInvariance
 * scale them by 0.8f / 1.2f; PredictScale reads mfMaxDistance), the angle
 * and octave of the keypoint that holds the point in the source frame
 * (LastFrame.mvKeysUn[i].angle / mvKeys[i].octave; pKF->mvKeysUn[i].angle),
 * valid = the point is searched (LastFrame: pMP && !mvbOutlier[i]; KeyFrame:
 * pMP && !isBad() && !sAlreadyFound.count(pMP); Sim3: !isBad() && not in
 * vpMatched), obs_positive = Observations() > 0. 48 bytes. */
typedef struct orbm_map_point_world {
  float pos[3], normal[3];
  float min_distance, max_distance, angle;
  int32_t octave;
  uint8_t valid, obs_positive, pad[6];
} orbm_map_point_world;

#define ORBM_PROJ_LAST_FRAME 1 /* SearchByProjection  src/ORBmatcher.cc:1328-1470 */
#define ORBM_PROJ_KEYFRAME 2   /* SearchByProjection  src/ORBmatcher.cc:1472-1599 */
#define ORBM_PROJ_SIM3 3       /* SearchByProjection  src/ORBmatcher.cc:290-403   */
#define ORBM_PROJ_FUSE 4       /* Fuse(pKF, vpMapPoints, th)  :825-975            */
#define ORBM_PROJ_FUSE_SIM3 5  /* Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) :977-1100 */
#define ORBM_PROJ_SIM3_MATCH 6 /* SearchBySim3, one direction  :1102-1326       */

/* Per-frame projection prepared on the host from a camera (the scalar
 * cv::Mat work each overload does once per call): Rt = the 3x4 transform
 * applied to world points (Sim3: sRcw/scw | tcw/scw), Ow = -R^T t (camera
 * centre), level_mode (last-frame overload: 0 = levels lo-1..lo+1,
 * 1 = bForward: lo.., 2 = bBackward: 0..lo), Rt2 = the second transform of
 * SearchBySim3 (camera A to camera B: [sR21 | t21] or [sR12 | t12]).
 * 132 bytes. */
typedef struct orbm_pose {
  float Rt[12];
  float Ow[3];
  float fx, fy, cx, cy, mbf;
  int32_t level_mode;
  float Rt2[12];
} orbm_pose;

/* Fill *out for `mode` (LAST_FRAME, KEYFRAME, SIM3, FUSE, FUSE_SIM3; for
 * SIM3 and FUSE_SIM3 cam->Tcw = Scw). Tlw: LastFrame.mTcw rows 0..2
 * (ORBM_PROJ_LAST_FRAME only, else NULL); mono = bMono. Host only. */
int orbm_prepare_pose(int mode, const orbm_camera* cam, const float* Tlw, int mono,
                      orbm_pose* out);

/* The two directions of SearchBySim3 (src/ORBmatcher.cc:1114-1124):
 * out[0] projects pKF1's points into pKF2 (Rt = T1w, Rt2 = [sR21 | t21]),
 * out[1] pKF2's into pKF1 (Rt = T2w, Rt2 = [sR12 | t12]); both use cam1's
 * fx, fy, cx, cy as the reference does. R12 row-major 3x3. Host only. */
int orbm_prepare_sim3_match(const orbm_camera* cam1, const float* T1w, const float* T2w,
                            float s12, const float* R12, const float* t12, orbm_pose* out);

/* MapPoint::PredictScale(dist, Frame* or KeyFrame*) (src/MapPoint.cc:390-422)
 * as the kernels evaluate it: the level is the number of thresholds
 * thr[0..nlevels-2] the ratio mfMaxDistance/dist reaches, thr[k-1] = the
 * least float ratio with ceil(logf(ratio)/logf(scale_factor)) >= k, found
 * on the host with the host's logf. Host only. */
int orbm_predict_scale_thresholds(float scale_factor, int nlevels, float* thr);
int orbm_predict_scale(float max_distance, float dist, float scale_factor, int nlevels);

/* SearchByProjection(CurrentFrame, LastFrame, th, bMono), host buffers,
 * synchronous. Current frame as for orbm_search_by_projection (uright NULL
 * for monocular); blocked[i2] = mvpMapPoints[i2] && Observations() > 0 on
 * entry; cur = CurrentFrame camera and pose; Tlw = LastFrame.mTcw rows 0..2;
 * one map point record + descriptor per LastFrame keypoint. out[i2] = index
 * of the LastFrame keypoint whose point this call stored in
 * CurrentFrame.mvpMapPoints[i2]; -1 = not touched; -2 = stored and then
 * cleared (NULL) by the rotation consistency check. */
int orbm_search_by_projection_last_frame(
    orbm_handle m, const orbx_kp* kps, const uint8_t* desc, int n, const float* uright,
    orbm_grid_bounds bounds, const float* scale, int nlevels, const uint8_t* blocked,
    const orbm_camera* cur, const float* Tlw, const orbm_map_point_world* mps,
    const uint8_t* mpdesc, int nmp, float th, int mono, int check_ori, int* out,
    int* nmatches);

/* SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist):
 * has_mp[i2] = CurrentFrame.mvpMapPoints[i2] != NULL on entry; one record
 * per pKF->GetMapPointMatches() entry; scale_factor = mfScaleFactor (for
 * PredictScale). out as above. */
int orbm_search_by_projection_keyframe(
    orbm_handle m, const orbx_kp* kps, const uint8_t* desc, int n, orbm_grid_bounds bounds,
    const float* scale, int nlevels, float scale_factor, const uint8_t* has_mp,
    const orbm_camera* cur, const orbm_map_point_world* mps, const uint8_t* mpdesc, int nmp,
    float th, int orb_dist, int check_ori, int* out, int* nmatches);

/* SearchByProjection(pKF, Scw, vpPoints, vpMatched, th): pKF's keypoints,
 * grid bounds, mvScaleFactors and mfScaleFactor; kf->Tcw = Scw rows 0..2;
 * matched[idx] >= 0 where vpMatched[idx] is set on entry (NULL: none).
 * out[idx] = index into vpPoints stored in vpMatched[idx] by this call, -1
 * otherwise. */
int orbm_search_by_projection_sim3(
    orbm_handle m, const orbx_kp* kps, const uint8_t* desc, int n, orbm_grid_bounds bounds,
    const float* scale, int nlevels, float scale_factor, const orbm_camera* kf,
    const orbm_map_point_world* mps, const uint8_t* mpdesc, int nmp, int th,
    const int* matched, int* out, int* nmatches);

/* Fuse(pKF, vpMapPoints, th), the matching part (src/ORBmatcher.cc:825-930):
 * pKF's keypoints, descriptors, mvuRight (NULL = all monocular), grid bounds,
 * mvScaleFactors, mvInvLevelSigma2, mfScaleFactor, camera (fx, fy, cx, cy,
 * mbf, Tcw); one record per point (valid = pMP && !isBad() &&
 * !IsInKeyFrame(pKF)). out[i] = keypoint index the point fuses into
 * (bestDist <= TH_LOW), -1 otherwise; *nfused = their count. The caller
 * applies the reference's side effects in point order (:932-957: Replace
 * when the keypoint holds a MapPoint, else AddObservation + AddMapPoint),
 * re-checking isBad() at each point's turn. */
int orbm_fuse(orbm_handle m, const orbx_kp* kps, const uint8_t* desc, int n, const float* uright,
              orbm_grid_bounds bounds, const float* scale, const float* inv_sigma2, int nlevels,
              float scale_factor, const orbm_camera* kf, const orbm_map_point_world* mps,
              const uint8_t* mpdesc, int nmp, float th, int* out, int* nfused);

/* Fuse(pKF, Scw, vpPoints, th, vpReplacePoint), the matching part
 * (:977-1081): kf->Tcw = Scw rows 0..2; valid = !isBad() && not in
 * pKF->GetMapPoints(). out[i] = bestIdx (<= TH_LOW) or -1. The caller's
 * in-order tail (:1083-1097): GetMapPoint(bestIdx) ? vpReplacePoint[i] =
 * it (if !isBad()) : AddObservation + AddMapPoint. */
int orbm_fuse_sim3(orbm_handle m, const orbx_kp* kps, const uint8_t* desc, int n,
                   orbm_grid_bounds bounds, const float* scale, int nlevels, float scale_factor,
                   const orbm_camera* kf, const orbm_map_point_world* mps, const uint8_t* mpdesc,
                   int nmp, float th, int* out, int* nfused);

/* SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (:1102-1326).
 * Per keyframe: keypoints, descriptors, grid bounds, mvScaleFactors, Tcw
 * rows 0..2 and one record per keypoint for GetMapPointMatches() (valid =
 * pMP && !vbAlreadyMatched && !isBad()). cam1: pKF1's fx, fy, cx, cy.
 * match12[i1] = idx2 for every new mutual match (the shim stores
 * vpMapPoints2[idx2] into vpMatches12[i1]), -1 otherwise; *nfound. */
int orbm_search_by_sim3(orbm_handle m, const orbx_kp* kps1, const uint8_t* desc1, int n1,
                        orbm_grid_bounds bounds1, const float* T1w,
                        const orbm_map_point_world* mps1, const uint8_t* mpdesc1,
                        const orbx_kp* kps2, const uint8_t* desc2, int n2,
                        orbm_grid_bounds bounds2, const float* T2w,
                        const orbm_map_point_world* mps2, const uint8_t* mpdesc2,
                        const float* scale, int nlevels, float scale_factor,
                        const orbm_camera* cam1, float s12, const float* R12, const float* t12,
                        float th, int* match12, int* nfound);

/* Batched device-resident variant of every pose mode: frame f's keypoints
 * at d_kps + f*kp_pitch (d_n[f]; descriptors, d_uright (LAST_FRAME, FUSE,
 * or NULL) and d_blocked likewise), its points at d_mps + f*mp_pitch
 * (d_nmp[f]; descriptors likewise), d_poses[f] from orbm_prepare_pose /
 * orbm_prepare_sim3_match. d_blocked: the blocking state on entry of the
 * mode (LAST_FRAME: a point with observations; KEYFRAME: any point; SIM3:
 * vpMatched set; ignored by FUSE, FUSE_SIM3, SIM3_MATCH). dist_th: TH_HIGH
 * (100) / ORBdist / TH_LOW (50); th: the window factor. inv_sigma2
 * (FUSE): mvInvLevelSigma2, nlevels floats (host), else NULL. d_out: per keypoint at
 * kp_pitch (LAST_FRAME, KEYFRAME, SIM3) or per point at mp_pitch (FUSE,
 * FUSE_SIM3, SIM3_MATCH: the keypoint each point matched, -1). All frames
 * share grid bounds, scale factors and scale_factor. */
int orbm_search_by_projection_pose_batch(
    orbm_handle m, int mode, const orbx_kp* d_kps, const uint8_t* d_desc, const int* d_n,
    int kp_pitch, const float* d_uright, orbm_grid_bounds bounds, const float* scale,
    int nlevels, float scale_factor, const uint8_t* d_blocked, const orbm_pose* d_poses,
    const orbm_map_point_world* d_mps, const uint8_t* d_mpdesc, const int* d_nmp,
    int mp_pitch, int frames, float th, int dist_th, int check_ori,
    const float* inv_sigma2, int* d_out, int* d_nmatches, void* stream);

/* ------------------------- Frame::isInFrustum, Tracking::SearchLocalPoints
 * Frame::isInFrustum(pMP, viewingCosLimit) (src/Frame.cc:268-324) for every
 * point of a local map, with the reference's float / double arithmetic
 * operation by operation. pose: the frame's orbm_pose from
 * orbm_prepare_pose(ORBM_PROJ_KEYFRAME, cam, NULL, 0, &pose), which holds
 * Rt = mTcw, Ow = -Rcw^T tcw as Frame::UpdatePoseMatrices computes it, and
 * fx, fy, cx, cy, mbf: isInFrustum needs nothing else, so it has no mode
 * constant of its own. bounds = mnMinX/MaxX/MinY/MaxY (inclusive here);
 * scale_factor, nlevels = mfScaleFactor, mnScaleLevels (PredictScale).
 * Input records: pos, normal, min/max_distance, obs_positive, and valid =
 * the point is tested at all, !isBad() && mnLastFrameSeen !=
 * mCurrentFrame.mnId (src/Tracking.cc:1256-1259); angle and octave are
 * ignored. Output record j: track_in_view and the mTrackProj* / view cosine /
 * predicted level the reference leaves on the MapPoint; a point that is not
 * valid or not in view gets an all-zero record (the reference leaves stale
 * fields there), obs_positive apart, which is copied from the input.
 * *n_in_view = the number of records with track_in_view. Host only: runs
 * without a device. */
int orbm_is_in_frustum(const orbm_pose* pose, orbm_grid_bounds bounds, float scale_factor,
                       int nlevels, float viewing_cos_limit, const orbm_map_point_world* mps,
                       int nmp, orbm_map_point_proj* out, int* n_in_view);

/* The same on the device, asynchronous on `stream`: frame f's points at
 * d_mps + f*mp_pitch (d_nmp[f] of them, 16-byte aligned), its pose
 * d_poses[f], its records to d_out + f*mp_pitch (slots from d_nmp[f] on are
 * left untouched), its count to d_n_in_view[f]. mp_pitch <= 65536. The
 * records equal orbm_is_in_frustum's byte for byte. */
int orbm_is_in_frustum_batch(orbm_handle m, const orbm_pose* d_poses, orbm_grid_bounds bounds,
                             float scale_factor, int nlevels, float viewing_cos_limit,
                             const orbm_map_point_world* d_mps, const int* d_nmp, int mp_pitch,
                             int frames, orbm_map_point_proj* d_out, int* d_n_in_view,
                             void* stream);

/* Tracking::SearchLocalPoints' device part (src/Tracking.cc:1254-1278) in one
 * round trip: isInFrustum on every point, then SearchByProjection(F,
 * vpMapPoints, th) over the points in view. Frame arguments as for
 * orbm_search_by_projection; cur = the frame's camera and pose; records as
 * for orbm_is_in_frustum, mpdesc their descriptors. out[idx] = index into
 * the caller's point list (all nmp of them) of the point assigned to keypoint
 * idx, -1 where nothing was assigned. proj (nmp records, or NULL) and
 * *n_in_view give the caller which points get IncreaseVisible() and nToMatch
 * (:1261-1265); with nothing in view the search is skipped (:1268): out is
 * all -1 and *nmatches 0. nmp <= 65536; the points are compacted to those in
 * view, in order, before the search, whose limit of 8192 points therefore
 * applies to the points in view: more gives ORBX_ECAPACITY (the message
 * names the count; proj and *n_in_view are still filled). */
int orbm_search_local_points(orbm_handle m, const orbx_kp* kps, const uint8_t* desc, int n,
                             const float* uright, orbm_grid_bounds bounds, const float* scale,
                             int nlevels, float scale_factor, const uint8_t* blocked,
                             const orbm_camera* cur, const orbm_map_point_world* mps,
                             const uint8_t* mpdesc, int nmp, float viewing_cos_limit, float th,
                             float nnratio, int* out, int* nmatches, orbm_map_point_proj* proj,
                             int* n_in_view);

/* Batched device-resident variant, asynchronous on `stream`: the frame side
 * as for orbm_search_by_projection_batch, the points as for
 * orbm_is_in_frustum_batch with their descriptors at d_mpdesc + f*mp_pitch*32
 * (16-byte aligned). d_proj: frames x mp_pitch records, or NULL to keep them
 * in the handle's workspace; d_n_in_view: frames counts. A frame with more
 * than 8192 points in view has only the first 8192 of them searched and sets
 * status bit 64 (orbm_get_status). */
int orbm_search_local_points_batch(
    orbm_handle m, const orbx_kp* d_kps, const uint8_t* d_desc, const int* d_n, int kp_pitch,
    const float* d_uright, orbm_grid_bounds bounds, const float* scale, int nlevels,
    float scale_factor, const uint8_t* d_blocked, const orbm_pose* d_poses,
    const orbm_map_point_world* d_mps, const uint8_t* d_mpdesc, const int* d_nmp, int mp_pitch,
    int frames, float viewing_cos_limit, float th, float nnratio, int* d_out, int* d_nmatches,
    orbm_map_point_proj* d_proj, int* d_n_in_view, void* stream);

/* ------ MapPoint::ComputeDistinctiveDescriptors, MapPoint::UpdateNormalAndDepth
 * The two functions local mapping, Fuse / MapPoint::Replace, the monocular
 * initialisation and loop closing call after a point's observations change
 * (mostly together). They produce the fields the searches above read:
 * orbm_map_point_world.normal / min_distance / max_distance and the point's
 * 32-byte descriptor.
 *
 * orbm_observation: one entry of mObservations, kf = index into the
 * keyframe table of the call, desc_row = row of pKF->mDescriptors.row(idx) in
 * the descriptor arena. orbm_keyframe_ref: GetCameraCenter() and isBad() of a
 * keyframe. orbm_point_refkf: mpRefKF as a keyframe index and
 * mpRefKF->mvKeysUn[mObservations[mpRefKF]].octave. */
typedef struct orbm_observation {
  uint32_t kf, desc_row;
} orbm_observation; /* 8 B */
typedef struct orbm_keyframe_ref {
  float Ow[3];
  uint32_t bad;
} orbm_keyframe_ref; /* 16 B */
typedef struct orbm_point_refkf {
  uint32_t kf;
  int32_t octave;
} orbm_point_refkf; /* 8 B */

/* MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:277-306) on n
 * gathered descriptors (32-byte rows, in std::map order, bad keyframes
 * already left out): *best = the first row with the least median distance
 * to all n rows (itself included; the median is element (n-1)/2 of the sorted
 * row, a value in 0..256), *median (may be NULL) that median. n = 0: *best =
 * *median = -1 (the reference returns with the descriptor untouched,
 * :261-262, :274-275). Host only: runs without a device. */
int orbm_distinctive_descriptor(const uint8_t* desc, int n, int* best, int* median);

/* MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:353-375) for one point:
 * pos = mWorldPos, Ow_list = n camera centres (3 floats each) in std::map
 * order (no isBad() test here: every observation counts), Ow_ref =
 * mpRefKF->GetCameraCenter(), ref_scale = mvScaleFactors[level of the point's
 * keypoint in mpRefKF], last_scale = mvScaleFactors[nLevels-1]. Writes
 * mNormalVector, mfMinDistance, mfMaxDistance with the reference's float /
 * double arithmetic operation by operation. n = 0 writes nothing
 * (:350-351). Host only. */
int orbm_update_normal_and_depth(const float* pos, const float* Ow_list, int n, const float* Ow_ref,
                                 float ref_scale, float last_scale, float* normal_out,
                                 float* min_distance, float* max_distance);

/* Both, for `points` map points in place on the device, asynchronous on
 * `stream`; nothing is read back. Point p of the call owns the observations
 * d_obs[d_obs_off[p] .. d_obs_off[p+1]) (d_obs_off: points + 1 ascending
 * entries; the list order is the caller's std::map order) and refreshes record
 * q = d_point_ids ? d_point_ids[p] : p; an id repeated within one call is the
 * caller's error. d_kfs: n_kfs keyframes; d_desc: one arena of desc_rows
 * 32-byte rows, 16-byte aligned (an orbx_extract_batch output at its
 * frame_capacity pitch: desc_row = frame*cap + idx); d_ref[p]: the point's
 * reference keyframe and octave; scale: mvScaleFactors, nlevels <= 16 floats
 * on the host.
 * Written: d_mps[q].normal, .min_distance, .max_distance and no other byte of
 * the record (pos is read); d_mpdesc[32*q .. 32*q+31] (16-byte aligned) =
 * the winning row; d_best[p] = the winner's position among the point's kept
 * observations (those whose keyframe is not bad) and d_median[p] its median,
 * when these pointers are given. A point whose keyframes are all bad keeps
 * its descriptor and gets d_best[p] = d_median[p] = -1, its normal and depth
 * are still refreshed (:355 has no isBad() test). A point without observations
 * gets d_best[p] = d_median[p] = -1 and nothing else.
 * d_mps and d_ref NULL: descriptors only. d_mpdesc NULL: normal and depth
 * only (d_best / d_median are still filled when given). d_point_ids NULL:
 * q = p.
 * A point with an observation whose kf >= n_kfs or desc_row >= desc_rows, or
 * (with d_mps) whose d_ref[p].kf >= n_kfs or octave is outside [0, nlevels),
 * is skipped as a whole: its record and descriptor stay untouched, d_best[p] =
 * d_median[p] = -1, and status bit 128 is set (orbm_get_status). Any number
 * of observations per point is accepted.
 * The call's work lists live in the handle's workspace and are ordered like
 * the other batched calls' (orbm_get_status). */
int orbm_refresh_map_points_batch(
    orbm_handle m, const orbm_observation* d_obs, const uint32_t* d_obs_off,
    const uint32_t* d_point_ids, int points, const orbm_keyframe_ref* d_kfs, int n_kfs,
    const uint8_t* d_desc, uint32_t desc_rows, const orbm_point_refkf* d_ref, const float* scale,
    int nlevels, orbm_map_point_world* d_mps, uint8_t* d_mpdesc, int* d_best, int* d_median,
    void* stream);

/* The same on host arrays, synchronous, in one round trip: the arrays as
 * above; mps / mpdesc are tables of n_mps records / descriptors (every id <
 * n_mps, checked; n_mps >= points without ids) that are uploaded, refreshed
 * and copied back whole. A skipped point (see above) is reported through
 * status bit 128 here too; the call itself returns ORBX_OK. */
int orbm_refresh_map_points(orbm_handle m, const orbm_observation* obs, const uint32_t* obs_off,
                            const uint32_t* point_ids, int points, const orbm_keyframe_ref* kfs,
                            int n_kfs, const uint8_t* desc, uint32_t desc_rows,
                            const orbm_point_refkf* ref, const float* scale, int nlevels,
                            orbm_map_point_world* mps, uint8_t* mpdesc, int n_mps, int* best,
                            int* median);

/* ------------------------------------------- Optimizer::PoseOptimization
 * The per-frame pose solve of Tracking (src/Optimizer.cc:334-543) between
 * SearchByProjection and SearchLocalPoints: one SE3 vertex, a monocular
 * (mvuRight[i] < 0) or stereo reprojection edge per keypoint that holds a map
 * point, four rounds of at most ten Levenberg-Marquardt iterations with an
 * inlier / outlier classification after each. The arithmetic restates what
 * the reference makes g2o do, in double.
 *
 * Inputs, as the searches leave them: kps = mvKeysUn (x, y, octave are read),
 * uright = mvuRight (NULL: a monocular frame, every edge monocular),
 * assign[i] >= 0 = the row of keypoint i's map point in the table mps (the
 * out / d_out convention of the pose searches), < 0 = no point; mps: pos is
 * read, and obs_positive for n_inliers_with_obs; inv_sigma2 =
 * mvInvLevelSigma2 (nlevels <= 16 floats, host); cam = fx, fy, cx, cy, mbf
 * and the frame's mTcw on entry.
 * Outputs: Tcw = rows 0..2 of the new mTcw (the old one, bit for bit, when
 * the frame has fewer than 3 correspondences); pose = orbm_prepare_pose(
 * ORBM_PROJ_KEYFRAME, ...) of the camera with the new Tcw, byte for byte;
 * outlier[i] = mvbOutlier[i], written only where keypoint i has a
 * correspondence; *result below. Tcw, pose, outlier and result may each be
 * NULL. With ORBM_POSEOPT_DISCARD_OUTLIERS, assign[i] = -1 for every outlier
 * (src/Tracking.cc:983-988).
 * A keypoint whose octave is outside [0, nlevels) or whose row is outside
 * [0, nmp) is treated as one without a point and sets status bit 256. */
typedef struct orbm_poseopt_result {
  int32_t ret;                /* the function's return value: n_initial - n_bad, 0 below 3 correspondences */
  int32_t n_initial;          /* nInitialCorrespondences */
  int32_t n_bad;              /* nBad of the last round that ran */
  int32_t n_inliers_with_obs; /* inliers whose point has obs_positive: nmatchesMap (src/Tracking.cc:993),
                                 mnMatchesInliers (:1033) */
  int32_t rounds;             /* rounds run: 0 (below 3), 1 (below 10) or 4 */
  int32_t trials;             /* Levenberg-Marquardt trials of all rounds */
  int32_t rejected;           /* trials whose step was rejected */
  int32_t reserved;
} orbm_poseopt_result; /* 32 B */

#define ORBM_POSEOPT_DISCARD_OUTLIERS 1

/* Host only: runs without a device. Edges accumulate in keypoint order, as
 * g2o's do. *status (may be NULL) gets 0 or bit 256. n is not bounded. */
int orbm_pose_optimization_host(const orbx_kp* kps, int n, const float* uright, int* assign,
                                const orbm_map_point_world* mps, int nmp, const float* inv_sigma2,
                                int nlevels, const orbm_camera* cam, int flags, float* Tcw,
                                orbm_pose* pose, uint8_t* outlier, orbm_poseopt_result* result,
                                int* status);

/* The same on the device from host arrays, synchronous, one round trip.
 * n <= max_kps. Sums over the edges are reduced lane -> wave -> workgroup in a
 * fixed order, so Tcw may differ from the host function's by double rounding
 * (each float equal or adjacent); flags and counts are those of the same
 * arithmetic. Status bit 256 is left for orbm_get_status. */
int orbm_pose_optimization(orbm_handle m, const orbx_kp* kps, int n, const float* uright, int* assign,
                           const orbm_map_point_world* mps, int nmp, const float* inv_sigma2,
                           int nlevels, const orbm_camera* cam, int flags, float* Tcw,
                           orbm_pose* pose, uint8_t* outlier, orbm_poseopt_result* result);

/* Device-resident and asynchronous on `stream`, one workgroup per frame:
 * frame f's keypoints at d_kps + f*kp_pitch (d_n[f] of them; d_uright,
 * d_assign and d_outlier likewise at kp_pitch), its map points at d_mps +
 * f*mp_pitch (d_nmp[f] rows), its camera d_cams[f]; d_Tcw + 12*f, d_pose[f],
 * d_result[f]. Slots from d_n[f] on are not touched. Frames without
 * correspondences are valid anywhere in the batch. kp_pitch <= max_kps; a
 * frame's edges stay in LDS up to a pitch of 4096, above that in the handle's
 * workspace. The output bits of a frame do not depend on the batch size, its
 * slot or the run. */
int orbm_pose_optimization_batch(orbm_handle m, const orbx_kp* d_kps, const int* d_n, int kp_pitch,
                                 const float* d_uright, int* d_assign,
                                 const orbm_map_point_world* d_mps, const int* d_nmp, int mp_pitch,
                                 const float* inv_sigma2, int nlevels, const orbm_camera* d_cams,
                                 int frames, int flags, float* d_Tcw, orbm_pose* d_pose,
                                 uint8_t* d_outlier, orbm_poseopt_result* d_result, void* stream);

/* ------------------------------------------------------------ Sim3Solver
 * Loop closing's RANSAC between SearchByBoW and SearchBySim3
 * (src/LoopClosing.cc:313-340): the constructor's gather (src/Sim3Solver.cc:
 * 37-112), SetRansacParameters (:114-138), iterate / find (:140-213),
 * ComputeSim3 (:226-337) and CheckInliers (:340-423) as one call. All
 * hypotheses are computed; the reference's early exit is the first iteration
 * whose inlier count is > min_inliers and >= the best so far.
 *
 * Inputs per keyframe pair: kps1 / kps2 = mvKeysUn (only octave is read), n1 /
 * n2 their counts; mps1 / mps2 = one orbm_map_point_world per keypoint
 * (GetMapPointMatches(): pos is read, valid = pMP && !isBad()); cam1 / cam2 =
 * fx, fy, cx, cy, mbf of each keyframe with Tcw = rows 0..2 of its pose (T1w,
 * T2w); match12[i1] = the keypoint index in KF2 matched to keypoint i1 of KF1,
 * or < 0 (the d_out of orbm_search_by_bow_batch with kf_vs_kf = 1, the match12
 * of orbm_search_by_sim3); kp_index1 (may be NULL = identity) =
 * pMP1->GetIndexInKeyFrame(pKF1) of the point at i1, the keypoint whose octave
 * is read (a negative value leaves i1 out, as the reference's `continue`);
 * level_sigma2 = mvLevelSigma2 (nlevels <= 16 floats, host).
 * Entry i1 is a correspondence when match12[i1] >= 0, mps1[i1].valid and
 * mps2[match12[i1]].valid; the correspondences keep the order of i1.
 * rand3[max_iterations][3]: the raw rand() values of the three draws of each
 * iteration (orbm_sim3_rand_fill), not indices: the call applies
 * DUtils::Random::RandomInt and the draw without replacement itself, on the
 * count of correspondences it finds.
 * A match12 value >= n2, a kp_index1 value >= n1 or an octave outside
 * [0, nlevels) makes the entry unmatched and sets status bit 512.
 *
 * Outputs (each may be NULL): *result below; s12, R12[9] (row-major), t12[3] of
 * the accepted hypothesis, or of the running best when none is accepted, left
 * untouched when result.best_iteration < 0; pose[2] = orbm_prepare_sim3_match(
 * cam1, T1w, T2w, s12, R12, t12), byte for byte, written when s12 is;
 * inlier[i1] for every i1 < n1: 1 where vbInliers of the accepted hypothesis
 * is set, all 0 when none is accepted; hyp[h] for every hypothesis h that ran
 * (first_iteration <= h < result.max_its). Fewer than 3 correspondences are
 * treated as fewer than min_inliers. */
typedef struct orbm_sim3_params {
  double probability;      /* SetRansacParameters(probability, minInliers, maxIterations) */
  int32_t min_inliers;
  int32_t max_iterations;  /* 1 .. 1024 (orbm_sim3_limits) */
  int32_t fix_scale;       /* mbFixScale */
  int32_t first_iteration; /* 0-based; 0 on a fresh solver, result.iterations to resume */
  int32_t best_inliers;    /* mnBestInliers on entry: 0 on a fresh solver */
  int32_t reserved;
} orbm_sim3_params; /* 32 B */

typedef struct orbm_sim3_result {
  int32_t ret;            /* nInliers of the accepted hypothesis, else 0 */
  int32_t iterations;     /* mnIterations on return: accepted index + 1, or mRansacMaxIts */
  int32_t no_more;        /* bNoMore: nothing was accepted and no iteration is left */
  int32_t n_corr;         /* N */
  int32_t max_its;        /* mRansacMaxIts; 0 when N < min_inliers */
  int32_t best_inliers;   /* mnBestInliers on return */
  int32_t best_iteration; /* the iteration (0-based) that set it, ties to the later one; -1: none in this call */
  int32_t reserved;
} orbm_sim3_result; /* 32 B */

typedef struct orbm_sim3_hyp {
  int32_t idx[3]; /* the three draws, positions in the gathered list */
  int32_t count;  /* mnInliersi */
  float s, R[9], t[3];
} orbm_sim3_hyp; /* 68 B */

/* 3 x rand() per iteration, in order: the reference's stream. Host only. */
int orbm_sim3_rand_fill(uint32_t* out, int iterations);
/* The cap of max_iterations, the hypotheses per workgroup and the largest
 * pitch whose gathered list stays in LDS (each may be NULL). Host only. */
int orbm_sim3_limits(int* max_iterations, int* chunk, int* lds_pitch);
/* out[N] = mRansacMaxIts for N = 0 .. n_max correspondences (0 where N <
 * max(min_inliers, 3)): ceil(log(1 - p) / log(1 - pow((float)min_inliers / N,
 * 3))) with the host's libm, 1 when N == min_inliers, limited to [1,
 * max_iterations]. The device calls look their count up in this table.
 * Host only. */
int orbm_sim3_iteration_table(double probability, int min_inliers, int max_iterations, int n_max,
                              int* out);

/* Host only: runs without a device, n1 / n2 not bounded by a handle. *status
 * (may be NULL) gets 0 or bit 512. With hyp == NULL it stops at the first
 * accepted hypothesis, as the reference does; the outputs are the same. */
int orbm_sim3_ransac_host(const orbx_kp* kps1, int n1, const orbx_kp* kps2, int n2,
                          const orbm_map_point_world* mps1, const orbm_map_point_world* mps2,
                          const orbm_camera* cam1, const orbm_camera* cam2, const int* match12,
                          const int* kp_index1, const float* level_sigma2, int nlevels,
                          const orbm_sim3_params* params, const uint32_t* rand3,
                          orbm_sim3_result* result, float* s12, float* R12, float* t12,
                          orbm_pose* pose, uint8_t* inlier, orbm_sim3_hyp* hyp, int* status);

/* The same on the device from host arrays, synchronous, one round trip.
 * n1, n2 <= max_kps. Counts, flags and everything after a hypothesis's
 * (s, R, t) are those of the same arithmetic; (s, R, t) may differ from the
 * host form's where the device's atan2 / sin / cos round differently. Status
 * bit 512 is left for orbm_get_status. */
int orbm_sim3_ransac(orbm_handle m, const orbx_kp* kps1, int n1, const orbx_kp* kps2, int n2,
                     const orbm_map_point_world* mps1, const orbm_map_point_world* mps2,
                     const orbm_camera* cam1, const orbm_camera* cam2, const int* match12,
                     const int* kp_index1, const float* level_sigma2, int nlevels,
                     const orbm_sim3_params* params, const uint32_t* rand3,
                     orbm_sim3_result* result, float* s12, float* R12, float* t12, orbm_pose* pose,
                     uint8_t* inlier, orbm_sim3_hyp* hyp);

/* Device-resident and asynchronous on `stream`. Pair p's keypoints, match12,
 * kp_index1 and inlier at p*kp_pitch (d_n1[p] / d_n2[p] of them), its map
 * points at p*mp_pitch (one row per keypoint, mp_pitch >= kp_pitch), its
 * cameras d_cam1[p] / d_cam2[p], its draws at d_rand3 + p*3*max_iterations,
 * its diagnostics at d_hyp + p*max_iterations; d_result[p], d_s12[p], d_R12 +
 * 9*p, d_t12 + 3*p, d_pose + 2*p. params holds for every pair. inlier slots
 * from d_n1[p] on are not touched; empty pairs are valid anywhere in the
 * batch. kp_pitch <= max_kps; the gathered list stays in LDS up to a pitch of
 * 1024, above that in the handle's workspace. The output bits of a pair do
 * not depend on the batch size, its slot, the run or the pitch. */
int orbm_sim3_ransac_batch(orbm_handle m, const orbx_kp* d_kps1, const int* d_n1,
                           const orbx_kp* d_kps2, const int* d_n2, int kp_pitch,
                           const orbm_map_point_world* d_mps1, const orbm_map_point_world* d_mps2,
                           int mp_pitch, const orbm_camera* d_cam1, const orbm_camera* d_cam2,
                           const int* d_match12, const int* d_kp_index1, const float* level_sigma2,
                           int nlevels, const orbm_sim3_params* params, const uint32_t* d_rand3,
                           int pairs, orbm_sim3_result* d_result, float* d_s12, float* d_R12,
                           float* d_t12, orbm_pose* d_pose, uint8_t* d_inlier, orbm_sim3_hyp* d_hyp,
                           void* stream);

/* ------------------------------------------------- Optimizer::OptimizeSim3
 * The refinement of a loop candidate's Sim3 (src/Optimizer.cc:1190-1385,
 * called at src/LoopClosing.cc:365) between SearchBySim3 and
 * SearchByProjection(pKF, Scw, ...): one 7-DoF vertex, the two reprojection
 * edges x1 = S12*X2 and x2 = S21*X1 per match with Huber kernels, optimize(5),
 * the removal of pairs with a chi2 above th2, optimize(5 or 10) and a second
 * check. The arithmetic restates what the reference makes g2o do, in double,
 * with g2o's numeric Jacobian.
 *
 * Inputs per keyframe pair, as orbm_sim3_ransac takes them: kps1 / kps2 =
 * mvKeysUn (x, y, octave are read), mps1 / mps2 = one orbm_map_point_world per
 * keypoint (pos and valid are read), cam1 / cam2 with Tcw = T1w / T2w,
 * inv_sigma2 = mvInvLevelSigma2 (nlevels <= 16 floats, host), *s12, R12[9]
 * (row-major), t12[3] = the RANSAC's estimate, th2 (the reference passes 10),
 * fix_scale = mbFixScale.
 * vpMatches1 is built from match12 (the BoW matches), inlier (uint8 per i1, the
 * RANSAC's; NULL keeps every match) and found12 / found21 (both or neither:
 * the two ORBM_PROJ_SIM3_MATCH outputs, per point of KF1 the keypoint of KF2
 * it matched and the reverse): m[i1] = match12[i1] where that is >= 0 and the
 * inlier flag is set (src/LoopClosing.cc:352-357); otherwise found12[i1] when
 * i2 = found12[i1] is in [0, n2), is not the target of a kept match and
 * found21[i2] == i1 (src/ORBmatcher.cc:1295-1312); otherwise -1. Entry i1
 * gets an edge pair when m[i1] >= 0, mps1[i1].valid and mps2[m[i1]].valid, in
 * i1 order. A match12, found12 or found21 value at or above the other
 * keyframe's count makes m[i1] = -1, an octave outside [0, nlevels) leaves the
 * pair out; both set status bit 8192.
 *
 * Outputs (each may be NULL): match12_out[i1] = vpMatches1 as the function
 * leaves it: m[i1], or -1 where the first or the second check rejected the
 * pair (must not overlap the inputs); S12[8] = g2oS12 on return as (qx, qy,
 * qz, qw, tx, ty, tz, s), the input through Quaterniond(Matrix3d) when the
 * function returns 0 before the second optimisation; Scw[12] = rows 0..2 of
 * Converter::toCvMat(gScm * gSmw), gSmw = Sim3(R2w, t2w, 1.0)
 * (src/LoopClosing.cc:372-374); pose = orbm_prepare_pose(ORBM_PROJ_SIM3, cam1
 * with Tcw = Scw), byte for byte; *result below; lin[36] = the upper triangle
 * of H row by row (28), b (7) and the robust chi2 of the first linearisation
 * of the first optimize, zeros without an edge pair (a diagnostic). */
typedef struct orbm_optsim3_result {
  int32_t ret;             /* the function's return value: nIn, or 0 */
  int32_t n_corr;          /* nCorrespondences */
  int32_t n_bad;           /* nBad of the first check */
  int32_t rounds;          /* optimisations run: 1 or 2 */
  int32_t more_iterations; /* nMoreIterations: 10 when n_bad > 0, else 5 */
  int32_t trials;          /* Levenberg-Marquardt trials of both rounds */
  int32_t rejected;        /* trials whose step was rejected */
  int32_t reserved;
} orbm_optsim3_result; /* 32 B */

/* Host only: runs without a device, n1 / n2 not bounded by a handle. Edges
 * accumulate in i1 order, e12 before e21, as g2o's do. *status (may be NULL)
 * gets 0 or bit 8192. */
int orbm_optimize_sim3_host(const orbx_kp* kps1, int n1, const orbx_kp* kps2, int n2,
                            const orbm_map_point_world* mps1, const orbm_map_point_world* mps2,
                            const orbm_camera* cam1, const orbm_camera* cam2, const int* match12,
                            const uint8_t* inlier, const int* found12, const int* found21,
                            const float* inv_sigma2, int nlevels, const float* s12, const float* R12,
                            const float* t12, float th2, int fix_scale, int* match12_out, double* S12,
                            float* Scw, orbm_pose* pose, orbm_optsim3_result* result, double* lin,
                            int* status);

/* The same on the device from host arrays, synchronous, one round trip.
 * n1, n2 <= max_kps. Sums over the edges are reduced lane -> wave -> workgroup
 * in a fixed order and exp / sin / cos are the device's, so S12 differs from
 * the host form's as it does between two edge orders on the host (the 1e-9
 * difference quotient amplifies a last-place change of a sum; DESIGN.md gives
 * the measured spread); flags and counts are those of the same arithmetic.
 * Status bit 8192 is left for orbm_get_status. */
int orbm_optimize_sim3(orbm_handle m, const orbx_kp* kps1, int n1, const orbx_kp* kps2, int n2,
                       const orbm_map_point_world* mps1, const orbm_map_point_world* mps2,
                       const orbm_camera* cam1, const orbm_camera* cam2, const int* match12,
                       const uint8_t* inlier, const int* found12, const int* found21,
                       const float* inv_sigma2, int nlevels, const float* s12, const float* R12,
                       const float* t12, float th2, int fix_scale, int* match12_out, double* S12,
                       float* Scw, orbm_pose* pose, orbm_optsim3_result* result, double* lin);

/* Device-resident and asynchronous on `stream`, one workgroup per pair. The
 * pitches and per-pair counts are orbm_sim3_ransac_batch's, so that call's
 * buffers pass straight through: pair p's keypoints, match12, inlier, found12,
 * found21 and match12_out at p*kp_pitch (d_n1[p] / d_n2[p] of them), its map
 * points at p*mp_pitch (mp_pitch >= kp_pitch), d_cam1[p] / d_cam2[p], d_s12[p],
 * d_R12 + 9*p, d_t12 + 3*p; d_S12 + 8*p, d_Scw + 12*p, d_pose[p], d_result[p],
 * d_lin + 36*p. th2 and fix_scale hold for every pair. match12_out slots from
 * d_n1[p] on are not touched; empty pairs are valid anywhere in the batch.
 * kp_pitch <= max_kps; the edge pairs stay in LDS up to a pitch of 1024, above
 * that in the handle's workspace. The output bits of a pair do not depend on
 * the batch size, its slot, the run or the pitch. */
int orbm_optimize_sim3_batch(orbm_handle m, const orbx_kp* d_kps1, const int* d_n1,
                             const orbx_kp* d_kps2, const int* d_n2, int kp_pitch,
                             const orbm_map_point_world* d_mps1, const orbm_map_point_world* d_mps2,
                             int mp_pitch, const orbm_camera* d_cam1, const orbm_camera* d_cam2,
                             const int* d_match12, const uint8_t* d_inlier, const int* d_found12,
                             const int* d_found21, const float* inv_sigma2, int nlevels,
                             const float* d_s12, const float* d_R12, const float* d_t12, float th2,
                             int fix_scale, int pairs, int* d_match12_out, double* d_S12, float* d_Scw,
                             orbm_pose* d_pose, orbm_optsim3_result* d_result, double* d_lin,
                             void* stream);

/* ------------------------------------------------------------ Initializer
 * The monocular bootstrap between SearchForInitialization and
 * CreateInitialMapMonocular (src/Tracking.cc:638-700): Initializer::Initialize
 * (src/Initializer.cc:44-121) with the draws (:82-97), FindHomography (:124-172),
 * FindFundamental (:175-223), Normalize (:749-795), ComputeH21 / ComputeF21
 * (:226-303), CheckHomography / CheckFundamental (:305-468), ReconstructF
 * (:470-570), ReconstructH (:572-732), Triangulate (:734-747), CheckRT
 * (:798-907) and DecomposeE (:909-929) as one call.
 *
 * Inputs per pair: kps1 / kps2 = mvKeysUn of the reference and the current
 * frame (only x, y are read), n1 / n2 their counts; matches12[i1] = the index
 * in frame 2, or negative (what orbm_search_for_initialization[_batch] writes,
 * at the same pitch; the call counts the matches itself). The gathered list
 * (i1, matches12[i1]) keeps the order of i1; N is its length. A matches12
 * value >= n2 leaves the entry out and sets status bit 4096. cam: fx, fy, cx,
 * cy are read. rand8[max_iterations][8]: the raw rand() values of the eight
 * draws of each iteration (orbm_initializer_rand_fill), not indices: the call
 * applies DUtils::Random::RandomInt and the swap-with-back draw itself, on
 * the N it finds.
 *
 * Outputs (each may be NULL): *result below; R21[9] (row-major), t21[3], Tcw[12]
 * = [R21 | t21], written when result.ok; p3d[n1][3] = vP3D and triangulated[n1]
 * = vbTriangulated of the winning reconstruction when result.ok, zeros
 * otherwise; matches12_out[i1] = matches12[i1] where that is negative or the
 * entry is triangulated, else -1 (src/Tracking.cc:688-693); inlier_h[k] /
 * inlier_f[k] for k < N = vbMatchesInliers of the best homography / fundamental
 * matrix (zeros when there is none); T1[9], T2[9] of Normalize; H21[9], F21[9]
 * the best of each (written when result.best_h / best_f >= 0); hyp[h] =
 * homography hypothesis h, hyp[max_iterations + h] = fundamental hypothesis h,
 * for h < max_iterations; rt[8] = the candidate (R, t) of the reconstruction
 * that ran (4 for F, 8 for H, the rest zero; written when a model was chosen).
 * With N < 8 (undefined in the reference) only *result is written: ok = 0, code
 * = ORBM_INIT_TOO_FEW_MATCHES, n = N. */
#define ORBM_INIT_TOO_FEW_MATCHES 1 /* N < 8 */
#define ORBM_INIT_NO_SCORE 2        /* SH and SF both zero: the reference would pass an empty F on */
#define ORBM_INIT_DEGENERATE 3      /* ReconstructH: d1/d2 or d2/d3 < 1.00001 (:597) */
#define ORBM_INIT_NO_CLEAR_WINNER 4 /* nsimilar > 1 (:517); secondBestGood >= 0.75*bestGood (:721) */
#define ORBM_INIT_TOO_FEW_POINTS 5  /* maxGood < nMinGood (:517); bestGood <= minTriangulated or 0.9*N (:721) */
#define ORBM_INIT_LOW_PARALLAX 6    /* :525-567, :721 */
#define ORBM_INIT_ACCEPTED 7
#define ORBM_INIT_MODEL_H 1
#define ORBM_INIT_MODEL_F 2

typedef struct orbm_init_params {
  float sigma;              /* Initializer(ReferenceFrame, sigma = 1.0, iterations = 200) */
  int32_t max_iterations;   /* 1 .. 1024 (orbm_initializer_limits) */
  float min_parallax;       /* 1.0 (:116, :118) */
  int32_t min_triangulated; /* 50 */
} orbm_init_params; /* 16 B */

typedef struct orbm_init_result {
  int32_t ok;         /* Initialize's return value */
  int32_t code;       /* ORBM_INIT_* */
  int32_t n;          /* N */
  int32_t model;      /* 0, ORBM_INIT_MODEL_H or ORBM_INIT_MODEL_F */
  float SH, SF, RH;
  int32_t best_h;     /* the iteration whose homography was kept, -1: none scored above 0 */
  int32_t best_f;
  int32_t best_rt;    /* the candidate the acceptance rule looked at (maxGood's / bestSolutionIdx), -1: none */
  int32_t n_good[8];  /* CheckRT's return value per candidate */
  float parallax[8];
  int32_t n_inliers;  /* inliers of the chosen model (N of ReconstructF / ReconstructH) */
  int32_t reserved;
} orbm_init_result; /* 112 B */

typedef struct orbm_init_hyp {
  int32_t idx[8]; /* mvSets[it]: positions in the gathered list */
  float M[9];     /* H21i or F21i, row-major */
  float score;    /* currentScore */
} orbm_init_hyp; /* 72 B */

typedef struct orbm_init_rt {
  float R[9], t[3];
} orbm_init_rt; /* 48 B */

/* 8 x rand() per iteration, in order: the reference's stream (after srand(0),
 * DUtils::Random::SeedRandOnce(0), for the first Initializer of a process).
 * Host only. */
int orbm_initializer_rand_fill(uint32_t* out, int iterations);
/* The cap of max_iterations, the hypotheses per workgroup of the solve kernel
 * and the largest pitch whose gathered list stays in LDS (0: the lists are
 * always in the handle's workspace, no pitch takes another path). Each may be
 * NULL. Host only. */
int orbm_initializer_limits(int* max_iterations, int* chunk, int* lds_pitch);

/* Host only: runs without a device, n1 / n2 not bounded by a handle. *status
 * (may be NULL) gets 0 or bit 4096. acosf is the host libm's. */
int orbm_initialize_host(const orbx_kp* kps1, int n1, const orbx_kp* kps2, int n2,
                         const int* matches12, const orbm_camera* cam,
                         const orbm_init_params* params, const uint32_t* rand8,
                         orbm_init_result* result, float* R21, float* t21, float* Tcw, float* p3d,
                         uint8_t* triangulated, int* matches12_out, uint8_t* inlier_h,
                         uint8_t* inlier_f, float* T1, float* T2, float* H21, float* F21,
                         orbm_init_hyp* hyp, orbm_init_rt* rt, int* status);

/* The same on the device from host arrays, synchronous, one round trip. n1,
 * n2 <= max_kps. Every output is that of the same arithmetic; only the
 * parallax may differ from the host form's where the device's acosf rounds
 * differently. Status bit 4096 is left for orbm_get_status. */
int orbm_initialize(orbm_handle m, const orbx_kp* kps1, int n1, const orbx_kp* kps2, int n2,
                    const int* matches12, const orbm_camera* cam, const orbm_init_params* params,
                    const uint32_t* rand8, orbm_init_result* result, float* R21, float* t21,
                    float* Tcw, float* p3d, uint8_t* triangulated, int* matches12_out,
                    uint8_t* inlier_h, uint8_t* inlier_f, float* T1, float* T2, float* H21,
                    float* F21, orbm_init_hyp* hyp, orbm_init_rt* rt);

/* Device-resident and asynchronous on `stream`. Pair p's keypoints, matches12,
 * triangulated, matches12_out, inlier_h and inlier_f at p*kp_pitch (d_n1[p] /
 * d_n2[p] keypoints), p3d at 3*p*kp_pitch, its camera d_cam[p], its draws at
 * d_rand8 + p*8*max_iterations, d_hyp + p*2*max_iterations, d_rt + 8*p,
 * d_result[p], d_R21 + 9*p, d_t21 + 3*p, d_Tcw + 12*p, d_T1 / d_T2 / d_H21 /
 * d_F21 + 9*p. params holds for every pair. Per-keypoint slots from d_n1[p] on
 * are not touched; empty and too-small pairs are valid anywhere in the batch.
 * kp_pitch <= max_kps. The output bits of a pair do not depend on the batch
 * size, its slot, the run, the pitch or the split into chunks. */
int orbm_initialize_batch(orbm_handle m, const orbx_kp* d_kps1, const int* d_n1,
                          const orbx_kp* d_kps2, const int* d_n2, int kp_pitch,
                          const int* d_matches12, const orbm_camera* d_cam,
                          const orbm_init_params* params, const uint32_t* d_rand8, int pairs,
                          orbm_init_result* d_result, float* d_R21, float* d_t21, float* d_Tcw,
                          float* d_p3d, uint8_t* d_triangulated, int* d_matches12_out,
                          uint8_t* d_inlier_h, uint8_t* d_inlier_f, float* d_T1, float* d_T2,
                          float* d_H21, float* d_F21, orbm_init_hyp* d_hyp, orbm_init_rt* d_rt,
                          void* stream);

/* DBoW2::FeatureVector as CSR: nodes[k] ascending NodeIds; the feature
 * indices of node k are idx[off[k] .. off[k+1]). Each feature index appears
 * in at most one node (DBoW2 guarantees it; checked). */
typedef struct orbm_feature_vector {
  const uint32_t* nodes;
  const int* off;
  const int* idx;
  int n_nodes;
} orbm_feature_vector;

/* ORBmatcher::SearchByBoW on host buffers (synchronous).
 * A = KeyFrame (descriptors, mvKeysUn angles, MapPoint-valid mask = pMP &&
 * !pMP->isBad()). kf_vs_kf = 0: B = Frame (mp_validB ignored), out[nB] =
 * matched KF feature index per frame feature or -1 (vpMapPointMatches).
 * kf_vs_kf = 1: B = KeyFrame 2, out[nA] = idx2 or -1 (vpMatches12). */
int orbm_search_by_bow(orbm_handle m, const uint8_t* descA, const float* angleA,
                       const uint8_t* mp_validA, int nA,
                       orbm_feature_vector fvA, const uint8_t* descB,
                       const float* angleB, const uint8_t* mp_validB, int nB,
                       orbm_feature_vector fvB, float nnratio, int check_ori,
                       int kf_vs_kf, int* out, int* nmatches);

/* Batched device-resident SearchByBoW over `pairs` (A, B) pairs on `stream`,
 * one workgroup per pair (Tracking::TrackReferenceKeyFrame calls the KF-F
 * form once per frame, src/Tracking.cc:839-842; relocalisation once per
 * candidate, :1445). Pair p: keypoints (orbx_kp, angles read from them),
 * descriptors (32 B rows) and MapPoint masks at p*kp_pitch of each side
 * (d_mpA/d_mpB NULL = every feature has one; d_mpB is read for kf_vs_kf
 * only), counts d_nA[p]/d_nB[p]; FeatureVectors as CSR at p*node_pitch
 * (offsets at p*(node_pitch+1)), d_nnA[p]/d_nnB[p] nodes: exactly the layout
 * orbv_transform_batch writes (node_pitch = its cap). Output at p*kp_pitch:
 * kf_vs_kf = 0: out[iB] = matched A index or -1 (vpMapPointMatches);
 * kf_vs_kf = 1: out[iA] = matched B index or -1; d_nmatches[p]. */
int orbm_search_by_bow_batch(orbm_handle m, int pairs, int kp_pitch, int node_pitch,
                             const orbx_kp* d_kpA, const uint8_t* d_descA, const int* d_nA,
                             const uint8_t* d_mpA, const uint32_t* d_nodesA, const int* d_offA,
                             const int* d_idxA, const int* d_nnA, const orbx_kp* d_kpB,
                             const uint8_t* d_descB, const int* d_nB, const uint8_t* d_mpB,
                             const uint32_t* d_nodesB, const int* d_offB, const int* d_idxB,
                             const int* d_nnB, float nnratio, int check_ori, int kf_vs_kf,
                             int* d_out, int* d_nmatches, void* stream);

/* Frame::ComputeStereoMatches (src/Frame.cc:465-639) on host buffers
 * (synchronous). kpL/descL = mvKeys/mDescriptors of the left image, kpR/descR
 * = mvKeysRight/mDescriptorsRight; the SAD refinement reads mvImagePyramid of
 * the two extractors, i.e. the pyramid of frame 0 of each handle's last
 * extraction (`left` and `right` may be one handle only if it is re-run, as
 * each extraction replaces its pyramid). mb = baseline (m), mbf = baseline x
 * fx. Outputs uRight/depth (nL floats, -1 where no match: mvuRight, mvDepth)
 * and the number of kept matches. A block-match window reaching off the
 * pyramid level (an OpenCV range assertion in the reference) rejects that
 * keypoint. */
int orbm_compute_stereo_matches(orbm_handle m, orbx_handle left, orbx_handle right,
                                const orbx_kp* kpL, const uint8_t* descL, int nL,
                                const orbx_kp* kpR, const uint8_t* descR, int nR,
                                float mb, float mbf, float* uRight, float* depth,
                                int* nkept);
/* The same for the frames of the two handles' last orbx_extract calls, as the
 * stereo Frame constructor runs it right after its two extractions
 * (src/Frame.cc:77-89): keypoints and descriptors are read where those calls
 * left them on the device (no host-to-device copy). nL = the left call's
 * keypoint count (mvKeys.size()); outputs as above. ORBX_EINVAL when either
 * handle's last extraction was a batch call. An empty left or right image
 * (orbx_extract of 0 x 0) matches nothing: uRight = depth = -1, nkept = 0.
 * When the extractors' capacity passes the device path's limits (max_kps, or
 * the stereo kernel's LDS at very large nFeatures) the call copies both
 * extractions to the host and runs orbm_compute_stereo_matches on their
 * actual counts instead of failing. */
int orbm_compute_stereo_matches_last(orbm_handle m, orbx_handle left, orbx_handle right,
                                     float mb, float mbf, float* uRight, float* depth,
                                     int nL, int* nkept);
/* The stereo Frame constructor's extraction and matching steps
 * (src/Frame.cc:77-89: ExtractORB on threadLeft / threadRight, then
 * ComputeStereoMatches) from the calling thread with one device round trip.
 * Outputs equal orbx_extract(left, img_left ...), orbx_extract(right,
 * img_right ...) and orbm_compute_stereo_matches_last(m, left, right, mb, mbf,
 * uRight, depth, *n_left, nkept) made in that order; the two extraction chains
 * run concurrently on the handles' streams and the stereo kernel follows on
 * the device. Both images are w x h (their own row strides); uRight and depth
 * hold cap_left floats. `left` and `right` are two distinct handles. Empty
 * images (w or h 0) take the three calls' own path. */
int orbm_stereo_frame(orbm_handle m, orbx_handle left, orbx_handle right,
                      const uint8_t* img_left, size_t stride_left,
                      const uint8_t* img_right, size_t stride_right, int w, int h,
                      float mb, float mbf, orbx_kp* kps_left, int cap_left,
                      uint8_t* desc_left, int* n_left, orbx_kp* kps_right,
                      int cap_right, uint8_t* desc_right, int* n_right,
                      float* uRight, float* depth, int* nkept);

/* Batched device-resident variant: pair p = left frame (left_frame0 + p) of
 * `left`'s last orbx_extract_batch and right frame (right_frame0 + p) of
 * `right`'s (the same handle may hold both when one batch extracted left and
 * right frames together); keypoints/descriptors at d_kpL + p*kp_pitch,
 * d_descL + p*kp_pitch*32, d_nL[p] (right likewise). Outputs d_uRight /
 * d_depth: pairs x kp_pitch floats; d_nkept: pairs. Run it on the stream
 * that extracted (or after it) and before the next extraction on either
 * handle, which overwrites the pyramid. */
int orbm_compute_stereo_matches_batch(
    orbm_handle m, orbx_handle left, int left_frame0, orbx_handle right,
    int right_frame0, const orbx_kp* d_kpL, const uint8_t* d_descL,
    const int* d_nL, const orbx_kp* d_kpR, const uint8_t* d_descR,
    const int* d_nR, int kp_pitch, int pairs, float mb, float mbf,
    float* d_uRight, float* d_depth, int* d_nkept, void* stream);

/* ------------- the Frame constructors' tail: UndistortKeyPoints, RGB-D depth
 * Camera.fx .. Camera.k3 of the settings file as Tracking stores them in mK
 * and mDistCoef (floats; k3 = 0 when the file has none). 36 bytes. */
typedef struct orbx_calib {
  float fx, fy, cx, cy, k1, k2, p1, p2, k3;
} orbx_calib;

/* Element type of a raw depth image (imDepth before GrabImageRGBD's convertTo). */
#define ORBX_DEPTH_U16 0 /* CV_16U, TUM's png */
#define ORBX_DEPTH_F32 1 /* CV_32F            */

/* cv::undistortPoints(src, dst, K, dist, Mat(), K) for n points (xy: x, y
 * pairs), the OpenCV 3.x scalar loop in double: five fixed-point iterations,
 * no early exit, no icdist guard. The raw call: no k1 == 0 shortcut. Host
 * only; the kernels evaluate the same function. xy_out may be xy. */
int orbx_undistort_points(const orbx_calib* calib, const float* xy, int n, float* xy_out);

/* Frame::ComputeImageBounds (src/Frame.cc:435-463) for a w x h image: the
 * undistorted corners' extremes when k1 != 0, the image rectangle when
 * k1 == 0 (whatever the other coefficients are). Host only. */
int orbx_image_bounds(const orbx_calib* calib, int w, int h, orbm_grid_bounds* out);

/* Frame::UndistortKeyPoints (src/Frame.cc:403-433) on host buffers, computed
 * on the device (synchronous): kps_un[i] = kps[i] with pt undistorted; a
 * bitwise copy when k1 == 0 (:405-409). n = 0 is ORBX_OK. */
int orbx_undistort_keypoints(const orbx_calib* calib, const orbx_kp* kps, int n, orbx_kp* kps_un);

/* The same device-resident and batched, asynchronous on `stream`, in the
 * layout orbx_extract_batch writes: frame f's d_counts[f] keypoints at
 * d_kps + f*kp_pitch, outputs at the same pitch; slots from d_counts[f] on
 * are not written. With a depth image (frame f at d_depth_img +
 * f*depth_frame_pitch, rows of w elements of depth_type at depth_row_stride
 * bytes, both multiples of the element size) it is also
 * Frame::ComputeStereoFromRGBD (src/Frame.cc:642-663): d = the pixel under
 * the distorted keypoint ((int)y, (int)x), converted as GrabImageRGBD's
 * convertTo(CV_32F, depth_factor) does ((float)raw * depth_factor iff
 * |depth_factor - 1| > 1e-5 or the type is not F32; depth_factor is
 * mDepthMapFactor, the inverse of the settings file's value,
 * src/Tracking.cc:150-154); d > 0: d_depth = d, d_uRight = x_undistorted -
 * mbf / d; otherwise both -1. A keypoint outside the image (undefined in the
 * reference) gets -1. d_depth_img == NULL: undistortion only, d_uRight and
 * d_depth are not touched and may be NULL. */
int orbx_frame_tail_batch(const orbx_calib* calib, const orbx_kp* d_kps, const int* d_counts, int kp_pitch,
                          int batch, const void* d_depth_img, int depth_type, size_t depth_frame_pitch,
                          size_t depth_row_stride, int w, int h, float depth_factor, float mbf,
                          orbx_kp* d_kps_un, float* d_uRight, float* d_depth, void* stream);

/* The RGB-D Frame constructor's ExtractORB, UndistortKeyPoints and
 * ComputeStereoFromRGBD (src/Frame.cc:134-144) with one device round trip:
 * the raw depth image is staged and uploaded while the gray image's
 * extraction runs, the tail kernel follows the extraction's last kernel on
 * the handle's stream and all outputs come back in the same wait. kps / desc / *n equal orbx_extract's
 * on the same image; kps_un, uRight, depth: cap entries, *n written.
 * depth_img == NULL: the monocular constructor (:189-197), uRight and depth
 * (when not NULL) are filled with -1. An empty image (w or h_ 0): *n = 0.
 * ORBX_EINVAL: a null calib, an unknown depth_type, depth_stride < w *
 * element size, cap below orbx_frame_capacity(h), or a handle planned for
 * another size than w x h_ (orbx_extract re-plans, this call does not). */
int orbx_rgbd_frame(orbx_handle h, const uint8_t* img, size_t stride, const void* depth_img, int depth_type,
                    size_t depth_stride, int w, int h_, const orbx_calib* calib, float depth_factor, float mbf,
                    orbx_kp* kps, int cap, uint8_t* desc, int* n, orbx_kp* kps_un, float* uRight, float* depth);

/* ------------------------------------- stereo rectification ahead of ExtractORB
 * What the stereo examples do to every camera pair before TrackStereo
 * (Examples/Stereo/stereo_euroc.cc:97-98,136-137; Examples/ROS/ROS_WS/src/
 * stereo/src/ros_stereo.cc:106-107,161-162): two pairs of float maps from
 * cv::initUndistortRectifyMap once, then cv::remap(im, imRect, M1, M2,
 * cv::INTER_LINEAR) on the left and the right image of every frame. Both are
 * restated here; no side of a source or destination
 * image may exceed 32766 (ORBX_EINVAL). */

/* cv::initUndistortRectifyMap(K, D, R, P.rowRange(0,3).colRange(0,3),
 * cv::Size(w, h), CV_32F, M1, M2) (stereo_euroc.cc:97-98, ros_stereo.cc:
 * 106-107) of OpenCV 3.x, in double: K, R row-major 3x3 (LEFT.K, LEFT.R), D =
 * k1 k2 p1 p2 k3 (LEFT.D), P row-major 3x4 of which columns 0..2 are used
 * (LEFT.P); map1 (x) and map2 (y): w*h floats each, rows of w. Host only. */
int orbx_rectify_maps(const double K[9], const double D[5], const double R[9], const double P[12], int w, int h,
                      float* map1, float* map2);

/* cv::remap(src, dst, map1, map2, cv::INTER_LINEAR) (stereo_euroc.cc:136-137,
 * ros_stereo.cc:161-162) for an 8-bit single-channel image, CV_32FC1 maps of
 * dst_w x dst_h (rows of dst_w floats) and BORDER_CONSTANT 0, on the host: the
 * function the kernels evaluate. Host only. */
int orbx_remap_host(const uint8_t* src, int src_w, int src_h, size_t src_stride, const float* map1,
                    const float* map2, int dst_w, int dst_h, uint8_t* dst, size_t dst_stride);

/* One camera's remap (the M1, M2 pair of stereo_euroc.cc:97-98), prepared
 * once on `device` from host maps of dst_w x dst_h for sources of src_w x
 * src_h: the per-frame kernel reads 4 bytes per output pixel (8 when a source
 * side exceeds 2046) instead of the two float maps. Synchronous. */
typedef struct orbx_rectifier* orbx_rectify_handle;
int orbx_rectify_create(int device, const float* map1, const float* map2, int dst_w, int dst_h, int src_w,
                        int src_h, orbx_rectify_handle* out);
/* Not while an extractor still has it set (orbx_set_rectify) or a batch call
 * on it is in flight. */
int orbx_rectify_destroy(orbx_rectify_handle r);

/* cv::remap (stereo_euroc.cc:136-137) for `batch` device-resident frames,
 * asynchronous on `stream`: frame i of src_w x src_h at d_src +
 * i*src_frame_pitch with rows src_stride apart, its rectification of dst_w x
 * dst_h to d_dst + i*dst_frame_pitch with rows dst_stride apart: the layout
 * orbx_extract_batch reads. Only bytes [0, src_w) of a source row are read and
 * only bytes [0, dst_w) of a destination row written. Equal to
 * orbx_remap_host byte for byte. */
int orbx_rectify_batch(orbx_rectify_handle r, const uint8_t* d_src, size_t src_stride, size_t src_frame_pitch,
                       uint8_t* d_dst, size_t dst_stride, size_t dst_frame_pitch, int batch, void* stream);

/* While r is set on h (NULL clears it), every host-image call on h
 * (orbx_extract, orbx_rgbd_frame, h's side of orbm_stereo_frame) takes `img`
 * as the raw camera image and extracts from its rectification, as
 * stereo_euroc.cc:136-137 does with cv::remap before TrackStereo: the raw
 * image is uploaded to a second device buffer, the remap kernel writes the
 * handle's frame buffer and the extraction follows, on the handle's stream
 * and inside the call's captured graph (still one linear chain). The
 * rectifier's source and destination size must both equal the call's w x h
 * (ORBX_EINVAL from that call otherwise) and r must live on h's device.
 * orbx_get_level(h, 0, 0, 0, ...) after such a call returns the rectified
 * image, and so does level 0 of the host pyramid. orbx_extract_batch is not
 * affected (rectify its frames with orbx_rectify_batch). The caller keeps r
 * alive while it is set. */
int orbx_set_rectify(orbx_handle h, orbx_rectify_handle r);

/* ------------------------------------------------------ vocabulary (DBoW2) */
typedef struct orbv_vocabulary* orbv_handle;

const char* orbv_last_error(void);

/* TemplatedVocabulary::loadFromTextFile: header "k L scoring weighting", then
 * one line per node "parent isLeaf d0..d31 weight" (node ids in line order,
 * the root is node 0). Lines without tokens are skipped. The tree is kept on
 * `device`. */
int orbv_load_text(const char* path, int device, orbv_handle* out);

/* The same from arrays in file order (node 0 = root; parent[i] < i for i > 0;
 * is_leaf marks words, numbered in node order; desc n_nodes x 32 bytes;
 * weight per node). scoring: L1 0, L2 1, CHI_SQUARE 2, KL 3, BHATTACHARYYA 4,
 * DOT_PRODUCT 5; weighting: TF_IDF 0, TF 1, IDF 2, BINARY 3. */
int orbv_create(int k, int L, int scoring, int weighting, int n_nodes,
                const int* parent, const uint8_t* is_leaf, const uint8_t* desc,
                const double* weight, int device, orbv_handle* out);
int orbv_destroy(orbv_handle v);
int orbv_info(orbv_handle v, int* k, int* L, int* scoring, int* weighting,
              int* n_nodes, int* n_words);

/* transform(features, BowVector, FeatureVector, levelsup) on host buffers
 * (synchronous), n <= 8192 descriptors of 32 bytes. BowVector: bow_n words
 * ascending with their values (capacity n). FeatureVector as CSR: fv_n node
 * ids ascending (file node ids), fv_off[fv_n + 1], fv_idx feature indices
 * (capacity n each; fv_off capacity n + 1). word_ids / node_ids / weights:
 * optional per-feature outputs (NULL to skip). */
int orbv_transform(orbv_handle v, const uint8_t* desc, int n, int levelsup,
                   uint32_t* bow_words, double* bow_values, int* bow_n,
                   uint32_t* fv_nodes, int* fv_off, int* fv_idx, int* fv_n,
                   uint32_t* word_ids, uint32_t* node_ids, double* weights);

/* Batched device-resident variant: frame f's descriptors at d_desc +
 * f*desc_pitch, d_n[f] of them (<= cap <= 8192). Outputs per frame at pitch
 * cap (fv_off: cap + 1): d_bow_words/d_bow_values/d_bow_n,
 * d_fv_nodes/d_fv_off/d_fv_idx/d_fv_n; per-feature d_word_ids/d_node_ids/
 * d_weights (frames x cap) or all three NULL to use an internal workspace. */
int orbv_transform_batch(orbv_handle v, const uint8_t* d_desc, size_t desc_pitch,
                         const int* d_n, int frames, int cap, int levelsup,
                         uint32_t* d_bow_words, double* d_bow_values, int* d_bow_n,
                         uint32_t* d_fv_nodes, int* d_fv_off, int* d_fv_idx,
                         int* d_fv_n, uint32_t* d_word_ids, uint32_t* d_node_ids,
                         double* d_weights, void* stream);

/* TemplatedVocabulary::score(v1, v2) = GeneralScoring::score of the
 * vocabulary's scoring type (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-311)
 * for two BowVectors given as ascending words with their values. `scoring`
 * as for orbv_create; all six are covered. The doubles are the reference
 * loops' bit for bit: terms are added in the order of the walk, L1 ends with
 * score = -score/2.0, KL uses LOG_EPS = log(DBL_EPSILON) and its asymmetric
 * walk (:175-221: every word of v1 counts, v2's only where shared). Host
 * only: no device, no handle. The message of a failure is orbdb_last_error(). */
int orbv_score(int scoring, const uint32_t* w1, const double* v1, int n1,
               const uint32_t* w2, const double* v2, int n2, double* out);

/* ------------------------------------------- keyframe database (BoW scores)
 * KeyFrameDatabase (src/KeyFrameDatabase.cc) with the keyframes' BowVectors
 * resident on the device: one row of up to word_pitch (word, value) pairs per
 * slot, words and values in separate arrays. A keyframe is named by its slot.
 * The reference's inverted file is not kept: a query intersects its sorted
 * words with every live row. scoring must be L1 (0), the scoring of
 * ORBvoc.txt; any other returns ORBX_EINVAL with a message naming it.
 *
 * Ordering: mutations and queries of one handle are ordered by the library
 * across streams (each waits for the previous user of the storage, as the
 * matcher's workspaces do). A handle is not reentrant. The message of the
 * last failure on the calling thread is orbdb_last_error(). */
typedef struct orbdb_database* orbdb_handle;

const char* orbdb_last_error(void);

/* max_keyframes slots of word_pitch pairs (1 .. 8192, the cap of
 * orbv_transform) on `device`: 12 bytes per pair of device memory. */
int orbdb_create(int device, int max_keyframes, int word_pitch, int scoring, orbdb_handle* out);
int orbdb_destroy(orbdb_handle db);
/* KeyFrameDatabase::clear (:105-109): every slot dead. The add sequence
 * counter goes on counting. Synchronous. */
int orbdb_clear(orbdb_handle db);
/* *live = entries in the database, *slots_high_water = one past the highest
 * slot ever used since the last clear (either may be NULL). Host only. */
int orbdb_size(orbdb_handle db, int* live, int* slots_high_water);

/* KeyFrameDatabase::add (:76-82) of a BowVector on the host (ascending words,
 * checked; synchronous). The entry takes the lowest free slot (*slot) and the
 * next value of the handle's 32-bit add sequence counter, which never
 * repeats within a handle and orders the entries as the reference's
 * per-word lists do (insertion order). n = 0 is a legal entry that shares no
 * word with anything. ORBX_ECAPACITY: max_keyframes entries are live already,
 * or n > word_pitch. The slot's relocalisation score (below) is set to 0. */
int orbdb_add(orbdb_handle db, const uint32_t* words, const double* values, int n, int* slot);

/* The same for `frames` BowVectors where orbv_transform_batch left them on
 * the device (its layout at pitch = its cap): frame f's d_bow_n[f] pairs at
 * f*pitch. slots (host, `frames` ints) receives their slots, assigned in
 * frame order. d_bow_n is needed on the host to validate (a count above
 * word_pitch is ORBX_ECAPACITY, and then nothing is added): the call copies
 * it back and waits for `stream` once before it enqueues the row copies,
 * which are asynchronous on `stream`. The rows are trusted to ascend. */
int orbdb_add_batch(orbdb_handle db, const uint32_t* d_bow_words, const double* d_bow_values,
                    const int* d_bow_n, int pitch, int frames, int* slots, void* stream);

/* KeyFrameDatabase::erase (:84-103). ORBX_EINVAL for a slot that is not
 * live. Synchronous. */
int orbdb_erase(orbdb_handle db, int slot);

/* What the two Detect functions compute per keyframe. 16 bytes. */
typedef struct orbdb_hit {
  int32_t common;      /* words shared with the query: mnLoopWords / mnRelocWords */
  uint32_t first_word; /* the smallest shared word id (0 when common == 0)       */
  double score;        /* L1 score where common > minCommon, else -1.0           */
} orbdb_hit;

/* `queries` BowVectors (device, the layout of orbv_transform_batch at
 * `pitch` <= 8192; a count above pitch is read as pitch) against every slot,
 * asynchronous on `stream`. d_hits: queries x max_keyframes records, query
 * q's slot s at q*max_keyframes + s; d_max_common: queries ints.
 * common = 0 for a dead slot, an empty entry and a slot in the query's
 * exclude list (d_exclude + q*exclude_pitch, d_n_exclude[q] slots: the
 * connected keyframes of DetectLoopCandidates :114,132; d_exclude NULL = none,
 * as for relocalisation). d_max_common[q] = the maximum of common over the
 * query's slots (maxCommonWords :149-154); minCommon = (int)(max * 0.8f) in
 * float (:156, :271). score is written where common > minCommon (:165, :282)
 * and equals orbv_score(0, query, keyframe) bit for bit: the terms of the
 * shared words are added one at a time in ascending word order from +0.0.
 * Elsewhere score is -1.0. */
int orbdb_query_batch(orbdb_handle db, const uint32_t* d_bow_words, const double* d_bow_values,
                      const int* d_bow_n, int pitch, int queries, const int* d_exclude,
                      const int* d_n_exclude, int exclude_pitch, orbdb_hit* d_hits,
                      int* d_max_common, void* stream);

/* mpORBVocabulary->score(CurrentBowVec, pKF->mBowVec) over entries of the
 * database (LoopClosing::DetectLoop's covisibles, src/LoopClosing.cc:147-165):
 * out[k] = orbv_score(0, query, entry slots[k]) bit for bit, by the device
 * code that scores the queries above. Synchronous. ORBX_EINVAL for a slot
 * that is not live. */
int orbdb_score_slots(orbdb_handle db, const uint32_t* words, const double* values, int n,
                      const int* slots, int nslots, double* out);

#define ORBDB_LOOP 0  /* DetectLoopCandidates            :112-233 */
#define ORBDB_RELOC 1 /* DetectRelocalizationCandidates  :235-345 */

/* The first half of a Detect function, one device round trip (synchronous):
 * lScoreAndMatch as (slot, si = (float)score) pairs in the reference's list
 * order, i.e. first encounter when the query's words are walked upwards with
 * each word's inverted list in insertion order = ascending (first_word, add
 * sequence). ORBDB_LOOP lists the entries with si >= min_score (:172) and
 * takes `exclude` (n_exclude slots) = pKF->GetConnectedKeyFrames();
 * ORBDB_RELOC lists every scored entry and ignores min_score. *ncand = their
 * number (ORBX_ECAPACITY when above cap; the first cap are written),
 * *min_common = minCommonWords (may be NULL). The ordering and everything
 * after the kernels run on the host over the copied-back hits. The handle
 * remembers, per mode, each slot's common, minCommon and score for
 * orbdb_select_candidates. Each call is a fresh query id: what the reference
 * does when one mnId queries twice (stale mnLoopQuery / mnRelocQuery marks)
 * is not reproduced. */
int orbdb_query(orbdb_handle db, int mode, const uint32_t* words, const double* values, int n,
                const int* exclude, int n_exclude, float min_score, int* cand_slots,
                float* cand_scores, int cap, int* ncand, int* min_common);

/* The second half (:180-232, :294-344) on the last orbdb_query of `mode`,
 * operation by operation: accScore a float sum over the candidate and its
 * counting neighbours, best score by strict >, bestAccScore starting at
 * min_score (loop) or 0 (relocalisation), retained where accScore >
 * 0.75f * bestAccScore, duplicates dropped in first-seen order. neigh: ncand
 * x 10 slots, candidate i's GetBestCovisibilityKeyFrames(10), -1 = none (the
 * library has no covisibility graph). A neighbour counts in loop mode if it
 * was listed by the query and its common > minCommon, in relocalisation mode
 * if it shares a word with the query; its mLoopScore / mRelocScore is added.
 * In relocalisation mode that score is stale when this query did not score
 * the neighbour: the handle keeps a per-slot relocalisation score across
 * queries, rewritten only when the slot is scored and set to 0.0f by add.
 * (Parity-unpinned: the reference reads a float that src/KeyFrame.cc:44
 * leaves uninitialised until the first scoring; 0 is this library's
 * definition.) out_slots: ncand ints; *nout = the candidates kept. Host
 * only. */
int orbdb_select_candidates(orbdb_handle db, int mode, const int* cand_slots,
                            const float* cand_scores, int ncand, const int* neigh,
                            float min_score, int* out_slots, int* nout);

/* ------------------------------------------------ SearchForTriangulation
 * Per pair: F12 (row-major 3x3, LocalMapping::ComputeF12) and the epipole
 * (ex, ey) of pKF1's camera centre in pKF2 (src/ORBmatcher.cc:664-670).
 * 44 bytes. */
typedef struct orbm_tri_pair {
  float F12[9];
  float ex, ey;
} orbm_tri_pair;

/* Fill *out from pKF1->GetCameraCenter() (cw1, 3 floats), pKF2's Tcw rows
 * 0..2 (T2w), pKF2's fx, fy, cx, cy (cam2) and F12. Host only. */
int orbm_prepare_triangulation(const float* cw1, const float* T2w, const float* cam2,
                               const float* F12, orbm_tri_pair* out);

/* SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo)
 * (src/ORBmatcher.cc:657-823), host buffers, synchronous. Per keyframe:
 * mvKeysUn, mDescriptors, mvuRight, has_mp[idx] = GetMapPoint(idx) != NULL,
 * mFeatVec (CSR). scale2 / sigma2: pKF2's mvScaleFactors / mvLevelSigma2.
 * matches12[idx1] = idx2 or -1 (vMatchedPairs = the pairs in idx1 order);
 * *nmatches = their count. */
int orbm_search_for_triangulation(
    orbm_handle m, const orbx_kp* kps1, const uint8_t* desc1, const float* uright1,
    const uint8_t* has_mp1, int n1, orbm_feature_vector fv1, const orbx_kp* kps2,
    const uint8_t* desc2, const float* uright2, const uint8_t* has_mp2, int n2,
    orbm_feature_vector fv2, const float* cw1, const float* T2w, const float* cam2,
    const float* scale2, const float* sigma2, int nlevels, const float* F12, int only_stereo,
    int check_ori, int* matches12, int* nmatches);

/* Batched device-resident variant: `pairs` keyframe pairs in one launch
 * (LocalMapping::CreateNewMapPoints: the new keyframe against each
 * neighbour). Side 1 arrays at kp_pitch1 / node_pitch1 per pair (0 and 0:
 * one pKF1 shared by every pair), side 2 at kp_pitch2 / node_pitch2.
 * d_off*: node_pitch + 1 ints per pair; d_nn*: node counts; d_n*: keypoint
 * counts. d_pairs from orbm_prepare_triangulation. scale2 / sigma2 are
 * host arrays shared by all pairs. d_matches12: pairs x out_pitch ints
 * (out_pitch >= n1); d_nmatches: pairs. */
int orbm_search_for_triangulation_batch(
    orbm_handle m, const orbx_kp* d_kps1, const uint8_t* d_desc1, const float* d_uright1,
    const uint8_t* d_has_mp1, const int* d_n1, const uint32_t* d_nodes1, const int* d_off1,
    const int* d_idx1, const int* d_nn1, int kp_pitch1, int node_pitch1,
    const orbx_kp* d_kps2, const uint8_t* d_desc2, const float* d_uright2,
    const uint8_t* d_has_mp2, const int* d_n2, const uint32_t* d_nodes2, const int* d_off2,
    const int* d_idx2, const int* d_nn2, int kp_pitch2, int node_pitch2,
    const orbm_tri_pair* d_pairs, const float* scale2, const float* sigma2, int nlevels,
    int pairs, int only_stereo, int check_ori, int* d_matches12, int out_pitch,
    int* d_nmatches, void* stream);

/* ------------------------------------ LocalMapping::CreateNewMapPoints
 * The loop over vMatchedIndices (src/LocalMapping.cc:317-483) between
 * SearchForTriangulation and the two refresh calls: the parallax test, the
 * linear triangulation (cv::SVD::compute of a 4x4), the two
 * KeyFrame::UnprojectStereo fallbacks (src/KeyFrame.cc:624-640) and the
 * depth, reprojection and scale-consistency gates, in the reference's float /
 * double arithmetic (UNPINNED). What stays with the
 * caller is `new MapPoint`, AddObservation and AddMapPoint.
 *
 * LocalMapping::ComputeF12 (:572-589) from two cameras (fx, fy, cx, cy and
 * Tcw are read): F12 row-major 3x3, for orbm_prepare_triangulation. Host
 * only. */
int orbm_compute_f12(const orbm_camera* cam1, const orbm_camera* cam2, float* F12);

/* One keyframe pair (current keyframe = 1, neighbour pKF2 = 2) as the loop
 * reads it: both cameras' intrinsics with invfx = 1.0f/fx as the Frame
 * constructor makes it, mb, the CURRENT keyframe's mbf (the reference uses it
 * for pKF2's stereo error too, :439), Tcw rows 0..2, Rwc, Twc rows 0..2 and
 * Ow as KeyFrame::SetPose computes them, ratio_factor = 1.5f*mfScaleFactor;
 * for the emitted observation lists the pair's keyframe indices, the
 * descriptor-arena row of each keyframe's keypoint 0, and kf2_first: whether
 * pKF2 precedes the current keyframe in the caller's std::map<KeyFrame*>
 * order (that order decides which descriptor wins the refresh's ties).
 * 376 bytes. */
typedef struct orbm_newpt_pair {
  float fx1, fy1, cx1, cy1, invfx1, invfy1, mb1, mbf1;
  float fx2, fy2, cx2, cy2, invfx2, invfy2, mb2, ratio_factor;
  float Tcw1[12], Tcw2[12];
  float Rwc1[9], Rwc2[9];
  float Twc1[12], Twc2[12];
  float Ow1[3], Ow2[3];
  uint32_t kf1, kf2, desc_base1, desc_base2;
  int32_t kf2_first, pad;
} orbm_newpt_pair;

/* Fill *out from the two cameras (fx, fy, cx, cy, mb, mbf, Tcw) and
 * mpCurrentKeyFrame->mfScaleFactor. Ow equals orbm_prepare_pose's. Host only. */
int orbm_prepare_new_points(const orbm_camera* cam1, const orbm_camera* cam2, float scale_factor,
                            uint32_t kf1, uint32_t kf2, uint32_t desc_base1, uint32_t desc_base2,
                            int kf2_first, orbm_newpt_pair* out);

/* reason[idx1]: what became of the match at idx1 */
#define ORBM_NEWPT_NONE 0          /* matches12[idx1] < 0                                  */
#define ORBM_NEWPT_TRIANGULATED 1  /* accepted, x3D from the SVD (:355-370)                */
#define ORBM_NEWPT_UNPROJECT1 2    /* accepted, mpCurrentKeyFrame->UnprojectStereo(idx1)   */
#define ORBM_NEWPT_UNPROJECT2 3    /* accepted, pKF2->UnprojectStereo(idx2)                */
#define ORBM_NEWPT_LOW_PARALLAX 4  /* :381-382, no stereo and very low parallax            */
#define ORBM_NEWPT_W_ZERO 5        /* x3D.at<float>(3) == 0 (:366)                         */
#define ORBM_NEWPT_STEREO_DEPTH 6  /* UnprojectStereo of a keypoint with mvDepth <= 0: the
                                      reference dereferences an empty Mat; status bit 1024 */
#define ORBM_NEWPT_BEHIND1 7       /* z1 <= 0                                              */
#define ORBM_NEWPT_BEHIND2 8       /* z2 <= 0                                              */
#define ORBM_NEWPT_REPROJ1 9       /* reprojection error in the current keyframe           */
#define ORBM_NEWPT_REPROJ2 10      /* reprojection error in pKF2                           */
#define ORBM_NEWPT_DIST_ZERO 11    /* dist1 == 0 || dist2 == 0                             */
#define ORBM_NEWPT_RATIO_LOW 12    /* ratioDist*ratioFactor < ratioOctave                  */
#define ORBM_NEWPT_RATIO_HIGH 13   /* ratioDist > ratioOctave*ratioFactor                  */
#define ORBM_NEWPT_DUPLICATE 14    /* accepted, but idx1 got its point from an earlier pair */
#define ORBM_NEWPT_BAD 15          /* idx2 >= n2 or an octave outside [0, nlevels); status
                                      bit 1024                                             */

/* The loop for one pair on host arrays, without a device. Per keyframe: kps =
 * mvKeysUn, kps_raw = mvKeys (UnprojectStereo reads the distorted keypoint;
 * NULL = the same as kps, which holds for rectified stereo), uright = mvuRight,
 * depth = mvDepth. level_sigma2 / scale_factors: mvLevelSigma2 /
 * mvScaleFactors (one set, as every keyframe of a map shares them).
 * matches12[idx1] = idx2 or -1 as orbm_search_for_triangulation writes it.
 * pos: n1 x 3 floats, x3D where reason[idx1] is 1..3, zeros elsewhere;
 * *nnew: the accepted matches; *status (may be NULL): 0 or 1024. */
int orbm_create_new_map_points_host(const orbm_newpt_pair* pair, const orbx_kp* kps1, const orbx_kp* kps_raw1,
                                    const float* uright1, const float* depth1, int n1, const orbx_kp* kps2,
                                    const orbx_kp* kps_raw2, const float* uright2, const float* depth2, int n2,
                                    const float* level_sigma2, const float* scale_factors, int nlevels,
                                    const int* matches12, float* pos, uint8_t* reason, int* nnew, int* status);

/* The same in one round trip through the device (synchronous). Status bit
 * 1024 is left for orbm_get_status. */
int orbm_create_new_map_points(orbm_handle m, const orbm_newpt_pair* pair, const orbx_kp* kps1,
                               const orbx_kp* kps_raw1, const float* uright1, const float* depth1, int n1,
                               const orbx_kp* kps2, const orbx_kp* kps_raw2, const float* uright2,
                               const float* depth2, int n2, const float* level_sigma2,
                               const float* scale_factors, int nlevels, const int* matches12, float* pos,
                               uint8_t* reason, int* nnew);

/* One accepted match, in the reference's creation order. 28 bytes. */
typedef struct orbm_new_point {
  float pos[3];
  int32_t pair, idx1, idx2, kind; /* kind: ORBM_NEWPT_TRIANGULATED / UNPROJECT1 / UNPROJECT2 */
} orbm_new_point;

/* Where the batch appends its points for the calls that follow (device
 * pointers, the struct itself is read on the host). New point k goes to row
 * q = point_base + k of d_mps: pos, valid = 1 and obs_positive = 1 are
 * written, the other fields stay. d_obs[2k], d_obs[2k+1]: its two
 * observations, pKF2's first when the pair's kf2_first is set, desc_row =
 * desc_base + idx; d_obs_off[k] = 2*min(k, nnew) for all capacity + 1
 * entries and d_point_ids[k] = point_base + k, d_ref[k] = {kf1, kp1.octave}
 * ({pair 0's kf1, 0} past the count) for all `capacity` slots, so
 * orbm_refresh_map_points_batch over `capacity` points is correct without
 * reading the count back: the slots past it have empty lists. */
typedef struct orbm_newpt_emit {
  orbm_map_point_world* d_mps;
  orbm_observation* d_obs;   /* 2 * capacity */
  uint32_t* d_obs_off;       /* capacity + 1 */
  uint32_t* d_point_ids;     /* capacity */
  orbm_point_refkf* d_ref;   /* capacity */
  uint32_t point_base;
  uint32_t pad;
} orbm_newpt_emit;

/* Batched device-resident variant, asynchronous on `stream`: `pairs` pairs
 * with the side and pitch conventions of orbm_search_for_triangulation_batch
 * (kp_pitch1 == 0: one current keyframe shared by every pair, d_n1 has one
 * entry); d_kps_raw1 / d_kps_raw2 may be NULL. d_matches12 / out_pitch exactly
 * as that call writes them; d_pairs from orbm_prepare_new_points;
 * level_sigma2 / scale_factors are host arrays.
 * Written: d_pos (pairs x out_pitch x 3 floats) and d_reason (pairs x
 * out_pitch) for idx1 < n1, the tail of each row stays untouched;
 * d_nnew_pair[p] = the matches of pair p that are accepted (after dedup);
 * d_new[0 .. *d_nnew) = those matches of all pairs compacted in the
 * reference's creation order (pair ascending, then idx1 ascending; found by a
 * scan, the same order in every run), *d_nnew = their number, at most
 * `capacity`. More than `capacity`: the excess is dropped whole (no record, no
 * emitted row, no has_mp update; d_reason keeps its code), and status bit 2048
 * is set. d_new may be NULL (capacity still bounds the emitted rows).
 * dedup != 0 with a shared side 1 applies the reference's sequential rule: a
 * keypoint idx1 accepted in several pairs keeps the lowest pair, the later
 * ones get ORBM_NEWPT_DUPLICATE and zero positions. This equals the
 * reference's loop, which sets the map point at idx1 before the next
 * neighbour's search skips it, because that search runs with
 * mbCheckOrientation = false (ORBmatcher matcher(0.6,false), :248) and its
 * per-idx1 searches are independent (vbMatched2 is never set). With
 * check_ori = 1 in the search the rotation histogram couples the idx1, and
 * the equivalence does NOT hold.
 * emit (may be NULL): see orbm_newpt_emit. d_has_mp1 / d_has_mp2 (may be
 * NULL; laid out like the search's): set to 1 at the idx1 / idx2 of every
 * point written, so that a following search or Fuse sees the new points.
 * A bad entry (see ORBM_NEWPT_BAD, ORBM_NEWPT_STEREO_DEPTH) sets status bit
 * 1024. */
int orbm_create_new_map_points_batch(
    orbm_handle m, const orbx_kp* d_kps1, const orbx_kp* d_kps_raw1, const float* d_uright1,
    const float* d_depth1, const int* d_n1, int kp_pitch1, const orbx_kp* d_kps2,
    const orbx_kp* d_kps_raw2, const float* d_uright2, const float* d_depth2, const int* d_n2,
    int kp_pitch2, const orbm_newpt_pair* d_pairs, const float* level_sigma2,
    const float* scale_factors, int nlevels, int pairs, const int* d_matches12, int out_pitch, int dedup,
    float* d_pos, uint8_t* d_reason, orbm_new_point* d_new, int capacity, int* d_nnew, int* d_nnew_pair,
    const orbm_newpt_emit* emit, uint8_t* d_has_mp1, uint8_t* d_has_mp2, void* stream);

/* --------------------------------------------- device plumbing for hosts
 * Thin wrappers so a host without its own HIP binding (ctypes, cgo, JNI)
 * can stage buffers for the batched entry points. */
int orbx_device_count(int* n);
int orbx_set_device(int device);
int orbx_malloc(void** p, size_t bytes);
int orbx_free(void* p);
int orbx_memcpy_htod(void* dst, const void* src, size_t bytes);
int orbx_memcpy_dtoh(void* dst, const void* src, size_t bytes);
int orbx_memset(void* dst, int value, size_t bytes);
int orbx_memcpy_dtod_async(void* dst, const void* src, size_t bytes, void* stream);
/* Pinned (page-locked) host memory and asynchronous host<->device copies on
 * a stream: host-streamed input (frames uploaded per batch) and read-back. */
int orbx_host_alloc(void** p, size_t bytes);
int orbx_host_free(void* p);
int orbx_memcpy_htod_async(void* dst, const void* src, size_t bytes, void* stream);
int orbx_memcpy_dtoh_async(void* dst, const void* src, size_t bytes, void* stream);
/* Rows of `width` bytes from a host image with row stride `spitch` into device
 * rows of stride `dpitch` (the extractor's padded pitch), one DMA rectangle
 * copy: frames cross the link unpadded. */
int orbx_memcpy2d_htod_async(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width,
                             size_t rows, void* stream);
/* The same rectangle copy done by a kernel of `blocks` 256-thread workgroups
 * reading pinned host memory (orbx_host_alloc) over the link directly, in
 * 16-byte loads, instead of by the DMA engines. */
int orbx_copy2d_kernel_async(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width,
                             size_t rows, int blocks, void* stream);
int orbx_stream_create(void** stream);
/* A stream whose work the dispatcher prefers (high = 1) or defers (high = 0)
 * when both compete for compute units (hipStreamCreateWithPriority). */
int orbx_stream_create_priority(void** stream, int high);
/* A stream whose kernels run only on the compute units whose bits are set in
 * mask[0 .. nwords) (hipExtStreamCreateWithCUMask; bit i = CU i in the
 * runtime's order): partitions the chip between concurrent pipelines
 * (bench.py --match-cus). */
int orbx_stream_create_cumask(void** stream, const uint32_t* mask, int nwords);
int orbx_stream_destroy(void* stream);
int orbx_stream_synchronize(void* stream);
int orbx_event_create(void** ev);
int orbx_event_destroy(void* ev);
int orbx_event_record(void* ev, void* stream);
/* Make `stream` wait (on the device) for the work recorded in `ev`, so a
 * host can pipeline extraction and matching on two streams. */
int orbx_stream_wait_event(void* stream, void* ev);
int orbx_event_elapsed_ms(void* start, void* stop, float* ms);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_C_H */
