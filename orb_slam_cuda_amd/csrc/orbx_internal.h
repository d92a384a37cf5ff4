// orbx_internal.h — device/host shared layout of the MI355X ORB front-end.
//
// Memory layout in HBM (one extractor handle, B = max_batch frames):
//   level 0          : the caller's frames (read in place, never copied)
//   pyramid levels>=1: level-major planes  [l][B][h_l][pitch_l]   u8
//   blurred levels   : level-major planes  [l][B][h_l][pitch_l]   u8
//   FAST key slots   : [B][slots_per_frame]  u32 packed (x|y<<12|score<<24),
//                      one fixed slot range per grid cell (cap = NMS bound)
//   cell counts      : [B][ncells_total]     i32
//   quadtree keys    : [B][kp_per_frame]     u32 packed, level-major slots
//   quadtree counts  : [B][L]                i32
//   outputs          : caller's [B][cap] orbx_kp + [B][cap][32] u8 + [B] i32
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <functional>

#include "../../include/orbx_c.h"

namespace orbx {

constexpr int kMaxLevels = 16;
constexpr int kEdgeThreshold = 19;      // EDGE_THRESHOLD  src/ORBextractor.cc:97
constexpr int kPatchSize = 31;          // PATCH_SIZE      src/ORBextractor.cc:95
constexpr int kHalfPatch = 15;          // HALF_PATCH_SIZE src/ORBextractor.cc:96
constexpr int kGridW = 30;              // W               src/ORBextractor.cc:1126
constexpr int kMaxRoi = 66;             // largest FAST cell ROI side (+6 halo)
constexpr int kMaxLevelDim = 4096;      // packed key coordinates are 12 bits
#ifndef ORBX_QT_THREADS
#define ORBX_QT_THREADS 512
#endif
constexpr int kQtThreads = ORBX_QT_THREADS;  // quadtree workgroup size

struct LevelGeom {
  int w, h, pitch;
  long long plane;   // bytes of one frame's plane (h * pitch)
  long long off;     // byte offset of this level's planes in the pyramid / blur buffers
  // INTER_LINEAR resize from level l-1 (l >= 1): offsets into the resize table
  int xtab, ytab, xmax, area2x;
  // FAST grid (ComputeKeyPointsOctTree src/ORBextractor.cc:1133-1147)
  int minBX, minBY, maxBX, maxBY;
  int nCols, nRows, wCell, hCell;
  int cell0, ncells;     // range in the cell table
  int slot0, nslots;     // key-slot range of this level inside a frame's slots
  int slot_stride;       // cell c of the level: slots slot0 + c * slot_stride .. (+ its cap)
  // DistributeOctTree (src/ORBextractor.cc:889-898)
  int N, nIni, boxW, boxH;
  float hX;
  int kcap, kbase;       // quadtree output slots of this level inside a frame
  float scale;           // mvScaleFactor[l]
  float size;            // (float)(int)(PATCH_SIZE * mvScaleFactor[l])
  int xtab2;             // band pyramid column table: {sx, a0 | a1 << 16}, replicate folded in
  // sorted-key quadtree (orbx_quadtree.hip): path-code tables of this level
  // in the resize table (u32 units: x codes, then y codes), their lengths
  // (tw | th << 16) and the code layout (bin shift | Dh << 8 | log2 bins << 16);
  // qt_tab < 0: the level's codes do not separate every position (legacy rounds)
  int qt_tab, qt_dims, qt_bits;
};

// keypoint slots per orient+BRIEF workgroup; every level's slot range starts
// at a multiple of it (orbx_plan.hip)
constexpr int kKpGroup = 8;

struct CellGeom {
  int16_t c0, r0, c1, r1;  // ROI [c0,c1) x [r0,r1) in level coordinates
  int slot_off;            // first key slot (frame-relative)
  int16_t cap, level;      // slot capacity (0 = cell skipped by the reference)
  // FAST staging, precomputed at plan time so that a wave needs no
  // level-indexed parameter after its one record load (orbx_fast.hip).
  // Levels >= 1 live in the plan's pyramid buffer; level 0 is the caller's
  // frames, whose row stride the kernel applies (pitch == 0 marks level 0).
  int row_off;   // levels >= 1: byte offset of the ROI's row r0 in frame 0's plane (from the pyramid buffer); level 0: r0
  int pitch;     // levels >= 1: the level's row pitch; 0 for level 0
  int fstride;   // levels >= 1: bytes between two frames' planes
  int geo;       // (h - 1 - r0) | ceil16(w) << 16: the buffer range's rows below r0 and last readable column
};
static_assert(sizeof(CellGeom) == 32, "one 32-byte scalar load per FAST wave");

struct ExtractParams {
  int L, B;
  int t_low, t_ini, t_min;
  int slots_per_frame, ncells_total;
  unsigned ncells_magic;       // ceil(2^32 / ncells_total) when frame = mulhi(id, magic) is exact for every id of the plan's batch, else 0
  int kp_per_frame;            // == output capacity per frame
  int maxnodes, sortn;         // quadtree node-table size, bitonic size (pow2)
  int max_cells_level;         // largest ncells of any level
  int kcap_lds;                // quadtree keys kept in LDS up to this count
  int qt_lean;                 // quadtree: lean rounds (packed 16-bit key nodes, maxnodes < 16384), else the generic ones
  int qt_big;                  // quadtree: node tables past 64 KB of LDS: 1024-thread blocks, a whole CU's LDS each
  int qt_sorted;               // quadtree: the sorted-key path first (levels with code tables, K <= threads x 8, maxnodes <= 2 x threads)
  int qt_tabmax, qt_nbmax;     // largest code-table length (tw + th) and bin count of any level
  int qt_ownmax;               // sorted path: most keys of a level (spill mode past threads x 8: keys in global scratch)
  int fast_rh_max;             // largest FAST cell ROI height
  int fast_bw_max, fast_bh_max;  // largest FAST detection band
  int pattern_upstream;
  // band pyramid (orbx_pyramid.hip): one workgroup per (frame, band of rows, column tile)
  int pyr_fused;               // 0 = one launch per level instead
  int pyr_nbands;              // bands per frame
  int pyr_bands;               // int2 offset in the resize table: per (band, level) {comp_lo, comp_hi}, {own_lo, own_hi};
                               // level 0's second entry: {int2 offset of the band's staged row entries, their count}
  int pyr_nct;                 // column tiles per band
  int pyr_ctiles;              // int2 offset: per (tile, level) {comp_lo, comp_hi}, {own_lo, own_hi}, {LDS pitch, LDS origin},
                               // {int2 offset of the level's column records (orbx_plan.hip plan_band_pyramid), 0}
  int pyr_lds_a, pyr_lds_b;    // LDS bytes of the even-level and odd-level row buffers
  int pyr_lds_y;               // LDS bytes of the band's staged row coefficients
  // alternative tilings, one picked per launch (launch_pyramid): the
  // workgroup count nbands x nct x batch against the resident workgroups per CU
  struct PyrPlan {
    int nbands, nct, bands, ctiles, lds_a, lds_b, lds_y;
    int cost;  // largest per-tile pixel count over the levels (level 0 staged + computed rows x columns)
    int occ;   // resident workgroups per CU at this plan's LDS (occupancy API, set at plan time)
  } pyr_plan[8];
  int pyr_nplans;
  int gauss[7];                // 7-tap Gaussian fixed-point kernel (sum 257)
  // blur work lists (orbx_blur.hip), [0] long / [1] short segments: per frame,
  // blur_ntiles entries of the resize table from blur_tiles on, one per wave:
  // {level | x0 << 4 | y0 << 16, rows}; four waves to a workgroup, whose frame
  // is a multiply-high of its id with blur_magic when exact (else 0)
  int blur_tiles[2], blur_ntiles[2];
  unsigned blur_magic[2];
  LevelGeom lv[kMaxLevels];
  // single-frame calls: the device status word copied to status_dst by the
  // last stage (orient_brief_kernel), so the output block carries it and one
  // read-back serves both (null otherwise)
  const int* status_src;
  int* status_dst;
};

inline void select_pyr_plan(ExtractParams& P, int i) {
  const ExtractParams::PyrPlan& q = P.pyr_plan[i];
  P.pyr_nbands = q.nbands;
  P.pyr_bands = q.bands;
  P.pyr_nct = q.nct;
  P.pyr_ctiles = q.ctiles;
  P.pyr_lds_a = q.lds_a;
  P.pyr_lds_b = q.lds_b;
  P.pyr_lds_y = q.lds_y;
}

// Estimated launch time of a tiling: the largest tile's pixel count times
// the workgroups the busiest CU runs (wpc = ceil(workgroups / CUs)), less
// 13 % per co-resident one (occ per CU: LDS and registers). Measured on
// gfx950 (tools/pyr_plans.py, 32 KITTI frames alone): a CU's second resident
// band workgroup adds ~87 % of the first's time, a third ~80 %.
inline long long pyr_plan_time(long long cost, long long wgs, int cus, int occ) {
  const long long wpc = (wgs + cus - 1) / cus;
  const long long res = std::min<long long>(wpc, std::max(1, occ));
  return cost * (100 * wpc - 13 * (res - 1));
}

// The band plan for a launch of `batch` frames. The one-tile plans compete
// by (rounds of resident workgroups) x (largest tile's pixel count), the
// rule measured best over band heights for 32-frame launches; a column-tiled
// plan replaces that pick when pyr_plan_time puts it at least 15 % faster
// (the estimate's error on the measured plans: tools/pyr_plans.py). A single
// frame then spreads over many small tiles (KITTI: 53 bands x 4, one per
// CU), a 32-frame KITTI batch over 4 x 4 large ones (less halo recompute).
inline int pick_pyr_plan(const ExtractParams::PyrPlan* plans, int n, int batch, int cus) {
  int i1 = -1, i2 = -1;
  long long t1 = -1, t2 = -1;
  for (int i = 0; i < n; ++i) {
    const ExtractParams::PyrPlan& q = plans[i];
    const long long wgs = (long long)q.nbands * q.nct * batch;
    if (q.nct == 1) {
      const long long slots = (long long)cus * std::max(1, q.occ);
      const long long t = ((wgs + slots - 1) / slots) * (long long)q.cost;
      if (t1 < 0 || t < t1) i1 = i, t1 = t;
    }
    const long long t = pyr_plan_time(q.cost, wgs, cus, q.occ);
    if (t2 < 0 || t < t2) i2 = i, t2 = t;
  }
  if (i1 < 0) return i2 < 0 ? 0 : i2;
  const ExtractParams::PyrPlan& q1 = plans[i1];
  const long long t1m = pyr_plan_time(q1.cost, (long long)q1.nbands * batch, cus, q1.occ);
  return (plans[i2].nct > 1 && t2 * 115 < t1m * 100) ? i2 : i1;
}
inline int pick_pyr_plan(const ExtractParams& P, int batch, int cus) {
  return pick_pyr_plan(P.pyr_plan, P.pyr_nplans, batch, cus);
}

// Pointers to level data for one launch. Level 0 is the caller's frames.
struct LevelPtrs {
  const uint8_t* base[kMaxLevels];
  long long fstride[kMaxLevels];  // bytes between frames
  int pitch[kMaxLevels];          // bytes between rows
  int aligned16[kMaxLevels];      // base, pitch and frame stride all 16-byte aligned
};
// both travel as kernel arguments of every extraction kernel (4 KB limit)
static_assert(sizeof(ExtractParams) + sizeof(LevelPtrs) + 128 <= 4096, "kernel arguments over 4 KB");

__host__ __device__ inline uint32_t pack_key(int x, int y, int score) {
  return (uint32_t)x | ((uint32_t)y << 12) | ((uint32_t)score << 24);
}
__host__ __device__ inline int key_x(uint32_t k) { return (int)(k & 0xFFFu); }
__host__ __device__ inline int key_y(uint32_t k) { return (int)((k >> 12) & 0xFFFu); }
__host__ __device__ inline int key_score(uint32_t k) { return (int)(k >> 24); }

// ------------------------------------------------------------ launchers
// (implemented in orbx_extract.hip; all asynchronous on `stream`)
struct ExtractBuffers {
  uint8_t* pyr;        // levels >= 1
  uint8_t* blur;       // all levels
  const int2* rtab;    // resize tables
  const CellGeom* cells;
  const int* umax;     // 16 ints
  uint32_t* slots;
  int* cell_counts;
  uint32_t* qkeys;
  int* qcounts;
  int* qties;          // [B][L][4] tie-straddle events, group nodes, kept keys (quadtree)
  uint32_t* qscratch;  // global fallback for quadtree keys (K > kcap_lds)
  uint16_t* qnode_scratch;
  long long qscratch_per_fl;  // entries per (frame, level)
  int* err;            // device error word
};

// orbx_extract.hip: the stages' default launch order, one letter each (p
// pyramid, b blur, f FAST, q quadtree, o orient+BRIEF), and the check of one
const char* extract_stage_order();
bool valid_stage_order(const char* order);
// pyr_event (optional): recorded on `stream` right after the pyramid stage, so
// a caller can fork work that only needs the pyramid (orbx_extract's host copy)
int launch_extract(const ExtractParams& P, const ExtractBuffers& X, const uint8_t* d_frames,
                   int batch, size_t frame_pitch, size_t row_stride, orbx_kp* d_kps,
                   uint8_t* d_desc, int* d_counts, void* stream, void** stage_events,
                   void* pyr_event = nullptr, int* status_dst = nullptr, const char* stage_order = nullptr);
// What the plan and the extractor handle ask the stage kernels' files: LDS
// bytes of a launch (host arithmetic on the plan), the kernels whose
// dynamic-LDS limit the handle raises, and the band kernel's occupancy
size_t quadtree_lds_bytes(const ExtractParams& P);  // orbx_quadtree.hip
size_t quadtree_legacy_lds_bytes(const ExtractParams& P);
size_t quadtree_sorted_lds_bytes(const ExtractParams& P, int big);
int quadtree_sorted_ownmax(const ExtractParams& P, int big, size_t budget);
const void* quadtree_kernel_ptr(const ExtractParams& P);
size_t pyr_band_lds_bytes(const ExtractParams& P);  // orbx_pyramid.hip
const void* pyr_band_kernel_ptr();
int pyr_band_occupancy(size_t lds);
void blur_strip_dims(int small, int* strip, int* rows);  // orbx_blur.hip

// orbx_top2.hip — dense Hamming best/second search
int launch_hamming_top2(const uint8_t* A, size_t a_pitch, const int* nA, int a_cap,
                        const uint8_t* B, size_t b_pitch, const int* nB, int pairs, int* best_idx,
                        int* best, int* second, int* err, void* stream);
// orbx_bow.hip — SearchByBoW over a batch of pairs; one side of the pairs:
struct BowSide {
  const uint8_t* desc;  // pair p: desc + p * kp_pitch * 32
  const float* angle;   // keypoint i's angle at angle[p * kp_pitch * angle_stride + i * angle_stride]
  int angle_stride;     // 1 for an angle array, 7 for orbx_kp records
  const uint8_t* mp;    // has a (good) MapPoint, or null = all
  const int* n;         // features per pair
  const uint32_t* nodes;  // FeatureVector CSR: pair p at p * node_pitch (off: p * (node_pitch + 1))
  const int* off;
  const int* idx;
  const int* nn;        // nodes per pair
  long long kp_pitch, node_pitch;
};
int launch_search_bow(const BowSide& A, const BowSide& B, int pairs, float nnratio, int check_ori, int kf_vs_kf,
                      int* out, long long out_pitch, int* nmatches, int* rec_scratch, size_t rec_ints,
                      int* hist_scratch, size_t hist_ints, bool* clean, int* err, void* stream);
// the Frame / KeyFrame keypoint grid (FRAME_GRID_COLS / ROWS include/Frame.h:37-38)
constexpr int kGridCols = 64, kGridRows = 48;

// orbx_stereo.hip — Frame::ComputeStereoMatches over a batch of rectified pairs.
// Pyramid pointers address pair 0; pair p's level l is at base[l] + p * fstride[l].
struct StereoParams {
  LevelPtrs pl, pr;
  int lw[kMaxLevels], lh[kMaxLevels];
  float scale[kMaxLevels], inv_scale[kMaxLevels];
  int L, nrows;        // levels; rows of level 0 (the row table's size)
  int kp_pitch, groups;
  int jobs_cap;        // SAD jobs a workgroup can hold: its share of left keypoints
  float mb, mbf;
  int stop;            // diagnostics: 1 = return after the row table, 2 = after the Hamming search
};
size_t stereo_lds_bytes(int nrows, int kp_pitch, int jobs_cap);
int launch_stereo(const StereoParams& P, const orbx_kp* kpL, const uint8_t* descL, const int* nL,
                  const orbx_kp* kpR, const uint8_t* descR, const int* nR, int pairs, float* uRight,
                  float* depth, int* sad, int* nkept, void* stream);
// orbx_init.hip — SearchForInitialization: prep, key and resolve launches per batch of pairs
struct InitParams {
  float minX, maxX, minY, maxY, invW, invH;  // F2 grid bounds
  float r;                                   // windowSize
  float nnratio;
  int check_ori;
  int kp_pitch;
  long long ws_ints;  // per-pair workspace stride in ints (set by the launcher)
  int dshift, obits, dclamp;  // key layout (set by the launcher from nnratio)
  uint32_t omask;
  long long* prof;  // diagnostics (ORBX_INIT_PROF=1): resolve-kernel phase clocks per pair, or null
};
constexpr size_t kInitLdsBudget = 160 * 1024 - 512;
size_t init_ws_bytes_per_pair(int kp_pitch);
int search_init_max_pitch(float nnratio);  // kp_pitch bound of launch_search_init at this ratio
int launch_search_init(const InitParams& P, const orbx_kp* kp1, const uint8_t* desc1, const int* n1,
                       const orbx_kp* kp2, const uint8_t* desc2, const int* n2, float* prev, int* ws,
                       int* matches12, int* nmatches, int pairs, void* stream);
// orbx_project.hip — SearchByProjection(Frame&, vector<MapPoint*>, th), one frame per workgroup
struct ProjParams {
  float minX, maxX, minY, maxY, invW, invH;  // Frame grid bounds, FRAME_GRID_COLS/ROWS over their extent
  float scale[kMaxLevels];                   // mvScaleFactors
  float th, nnratio;
  int kp_pitch, mp_pitch, has_uright;
  int max_rounds;                            // fixed-point rounds before the sequential pass
  long long* prof;                           // diagnostics: per-frame phase clocks, or null
};
size_t proj_lds_bytes(int kp_pitch);
int launch_search_proj(const ProjParams& P, const orbx_kp* kps, const uint8_t* desc, const int* n,
                       const float* uright, const uint8_t* blocked, const orbm_map_point_proj* mps,
                       const uint8_t* mpdesc, const int* nmp, int frames, int* out, int* nmatches, void* stream);
// orbx_project_pose.hip — the pose-projection SearchByProjection overloads, one frame per workgroup
struct PoseParams {
  int mode;                                  // ORBM_PROJ_LAST_FRAME / KEYFRAME / SIM3
  float minX, maxX, minY, maxY, invW, invH;  // grid bounds (image bounds of IsInImage / the u, v tests)
  float scale[kMaxLevels];                   // mvScaleFactors
  float pred_thr[kMaxLevels];                // PredictScale thresholds (orbm_predict_scale_thresholds)
  float inv_sigma2[kMaxLevels];              // mvInvLevelSigma2 (FUSE reprojection test)
  int L;                                     // mnScaleLevels
  float th;                                  // window factor
  int dist_th;                               // TH_HIGH / ORBdist / TH_LOW
  int check_ori;
  int kp_pitch, mp_pitch, has_uright;
  int max_rounds;                            // fixed-point rounds before the sequential pass
};
size_t pose_lds_bytes(int kp_pitch);
int launch_search_pose(const PoseParams& P, const orbx_kp* kps, const uint8_t* desc, const int* n,
                       const float* uright, const uint8_t* blocked, const orbm_pose* poses,
                       const orbm_map_point_world* mps, const uint8_t* mpdesc, const int* nmp, int frames, int* picks,
                       int* out, int* nmatches, void* stream);
// orbx_frustum.hip — Frame::isInFrustum per point, the stable compaction of the
// points in view and the index map back (Tracking::SearchLocalPoints)
struct FrustumParams {
  float minX, maxX, minY, maxY;  // mnMinX .. mnMaxY
  float pred_thr[kMaxLevels];    // PredictScale thresholds (orbm_predict_scale_thresholds)
  int L;                         // mnScaleLevels
  float cos_limit;               // viewingCosLimit
  int mp_pitch;
};
constexpr int kFrustumMaxView = 8192;  // points in view search_proj_kernel takes per frame (its kProjMaxMp)
constexpr int kStatusViewOverflow = 64;  // matcher status bit: more than kFrustumMaxView points in view
int launch_frustum(const FrustumParams& P, const orbm_pose* poses, const orbm_map_point_world* mps, const int* nmp,
                   int frames, orbm_map_point_proj* out, int* n_in_view, void* stream);
// c_*: per frame c_pitch compacted records, descriptors and original indices, c_nmp[f] of them
// (<= kFrustumMaxView); err: the status word for kStatusViewOverflow, or null
int launch_compact_in_view(const orbm_map_point_proj* proj, const uint8_t* mpdesc, const int* nmp, int mp_pitch,
                           int frames, orbm_map_point_proj* c_proj, uint8_t* c_desc, int* c_map, int* c_nmp,
                           int c_pitch, int* err, void* stream);
int launch_remap_out(int* out, const int* n, int kp_pitch, const int* c_map, int c_pitch, int frames, void* stream);
// orbx_mappoint.hip — MapPoint::ComputeDistinctiveDescriptors and UpdateNormalAndDepth
// for a list of points, in place on the device
constexpr int kStatusRefreshSkipped = 128;  // matcher status bit: a point with an out-of-range kf, desc_row or octave
constexpr int kRefreshClasses = 5;          // observation counts <= 8, <= 16, <= 32, <= 64, more
struct RefreshArgs {
  const orbm_observation* obs;
  const uint32_t* off;  // points + 1
  const uint32_t* ids;  // or null
  int points;
  const orbm_keyframe_ref* kfs;
  uint32_t n_kfs;
  const uint8_t* desc;
  uint32_t desc_rows;
  const orbm_point_refkf* ref;  // null with mps
  float scale[kMaxLevels];
  int nlevels;
  orbm_map_point_world* mps;  // or null
  uint8_t* mpdesc;            // or null
  int* best;                  // or null
  int* median;                // or null
  int* err;                   // the handle's status word
  int* counts;                // workspace: kRefreshClasses counters (8 ints)
  int* lists;                 // workspace: kRefreshClasses x points point indices
};
size_t refresh_ws_bytes(int points);
int launch_refresh_map_points(const RefreshArgs& A, void* stream);
// orbx_poseopt.hip — Optimizer::PoseOptimization, one frame per workgroup (the
// arithmetic and status bit 256 are in orbx_poseopt.cuh)
constexpr int kPoLdsEdges = 4096;  // frame pitches up to this keep their edge records in LDS (32 bytes each)
struct PoseOptArgs {
  const orbx_kp* kps;
  const int* n;
  int kp_pitch;
  const float* uright;  // or null
  int* assign;
  const orbm_map_point_world* mps;
  const int* nmp;
  int mp_pitch;
  const float* inv_sigma2;  // host, nlevels
  int nlevels;
  const orbm_camera* cams;
  int frames, flags;
  float* Tcw;                   // or null
  orbm_pose* pose;              // or null
  uint8_t* outlier;             // or null
  orbm_poseopt_result* result;  // or null
  int* err;                     // the handle's status word
};
size_t poseopt_spill_bytes(int kp_pitch, int frames);  // workspace of a launch (0 up to kPoLdsEdges)
int launch_pose_optimization(const PoseOptArgs& P, void* spill, void* stream);
// orbx_sim3.hip — Sim3Solver: the RANSAC of one keyframe pair per grid row (the
// arithmetic, the limits and status bit 512 are in orbx_sim3.cuh)
struct Sim3LaunchArgs {
  const orbx_kp *kps1, *kps2;
  const int *n1, *n2;
  int kp_pitch, mp_pitch;
  const orbm_map_point_world *mps1, *mps2;
  const orbm_camera *cam1, *cam2;
  const int* match12;
  const int* kp_index1;       // or null
  const float* level_sigma2;  // host, nlevels
  int nlevels;
  orbm_sim3_params params;
  const int* its_tab;  // device: mRansacMaxIts per count 0..kp_pitch (sim3_iterations)
  const uint32_t* rand3;
  int pairs;
  orbm_sim3_result* result;  // every output or null
  float *s12, *R12, *t12;
  orbm_pose* pose;
  uint8_t* inlier;
  orbm_sim3_hyp* hyp;
  int* err;  // the handle's status word
};
// workspace of a launch: the hypotheses' records, then the gathered lists of pitches above kSim3LdsCorr (else 0)
void sim3_ws_bytes(int kp_pitch, int pairs, int max_iterations, size_t* hyp_bytes, size_t* rec_bytes);
int launch_sim3_ransac(const Sim3LaunchArgs& P, void* ws, void* stream);
int sim3_iterations(double probability, int min_inliers, int max_iterations, int N);
int sim3_ransac_host(const orbx_kp* kps1, int n1, const orbx_kp* kps2, int n2, const orbm_map_point_world* mps1,
                     const orbm_map_point_world* mps2, const orbm_camera* cam1, const orbm_camera* cam2,
                     const int* match12, const int* kp_index1, const float* level_sigma2, int nlevels,
                     const orbm_sim3_params* params, const uint32_t* rand3, orbm_sim3_result* result, float* s12,
                     float* R12, float* t12, orbm_pose* pose, uint8_t* inlier, orbm_sim3_hyp* hyp, int* status);
// orbx_optsim3.hip — Optimizer::OptimizeSim3, one keyframe pair per workgroup
// (the arithmetic, the LDS limit and status bit 8192 are in orbx_optsim3.cuh)
struct OptSim3Args {
  const orbx_kp *kps1, *kps2;
  const int *n1, *n2;
  int kp_pitch, mp_pitch;
  const orbm_map_point_world *mps1, *mps2;
  const orbm_camera *cam1, *cam2;
  const int* match12;
  const uint8_t* inlier;           // or null
  const int *found12, *found21;    // both or null
  const float* inv_sigma2;         // host, nlevels
  int nlevels;
  const float *s12, *R12, *t12;
  float th2;
  int fix_scale, pairs;
  int* match12_out;             // every output or null
  double* S12;
  float* Scw;
  orbm_pose* pose;
  orbm_optsim3_result* result;
  double* lin;
  int* err;  // the handle's status word
};
size_t optsim3_ws_bytes(int kp_pitch, int pairs);  // workspace of a launch (0 up to kOs3LdsCorr)
int launch_optimize_sim3(const OptSim3Args& P, void* ws, void* stream);
int optimize_sim3_host(const OptSim3Args& P, int n1, int n2, int* status);  // pair 0 of host arrays
// orbx_initializer.hip — Initializer: the two-view H / F RANSAC and reconstruction
// of one frame pair per grid row (the arithmetic, the limits and status bit
// 4096 are in orbx_initializer.cuh)
struct InitzLaunchArgs {
  const orbx_kp *kps1, *kps2;
  const int *n1, *n2;
  int kp_pitch;
  const int* matches12;
  const orbm_camera* cam;
  orbm_init_params params;
  const uint32_t* rand8;
  int pairs;
  orbm_init_result* result;  // every output or null
  float *R21, *t21, *Tcw, *p3d;
  uint8_t* triangulated;
  int* matches12_out;
  uint8_t *inlier_h, *inlier_f;
  float *T1, *T2, *H21, *F21;
  orbm_init_hyp* hyp;
  orbm_init_rt* rt;
  int* err;  // the handle's status word
};
// workspace of a launch: headers, gathered lists, hypotheses, flags and cosine keys
size_t initializer_ws_bytes(int kp_pitch, int pairs, int max_iterations);
int launch_initialize(const InitzLaunchArgs& P, void* ws, void* stream);
int initialize_host(const orbx_kp* kps1, int n1, const orbx_kp* kps2, int n2, const int* matches12,
                    const orbm_camera* cam, const orbm_init_params* params, const uint32_t* rand8,
                    orbm_init_result* result, float* R21, float* t21, float* Tcw, float* p3d, uint8_t* triangulated,
                    int* matches12_out, uint8_t* inlier_h, uint8_t* inlier_f, float* T1, float* T2, float* H21,
                    float* F21, orbm_init_hyp* hyp, orbm_init_rt* rt, int* status);
// orbx_triangulate.hip — SearchForTriangulation, one keyframe pair per workgroup
struct TriSide {  // one side of the pairs; pitches of 0 share one keyframe across pairs
  const orbx_kp* kps;
  const uint8_t* desc;
  const float* uright;
  const uint8_t* has_mp;
  const int* n;
  const uint32_t* nodes;
  const int* off;  // node_pitch + 1 entries per pair
  const int* idx;
  const int* nn;
  int kp_pitch, node_pitch;
};
struct TriParams {
  float scale2[kMaxLevels], sigma2[kMaxLevels];  // pKF2->mvScaleFactors, mvLevelSigma2
  int only_stereo, check_ori, out_pitch;
};
int launch_search_tri(const TriParams& P, const TriSide& A, const TriSide& B, const orbm_tri_pair* pairs, int npairs,
                      int* matches12, int* nmatches, void* stream);
// orbx_newpoints.hip — LocalMapping::CreateNewMapPoints' loop over the search's
// pairs: one lane per (pair, idx1), then the first-pair rule and the ordered
// compaction (the arithmetic and status bits 1024 / 2048 are in orbx_newpoints.cuh)
struct NewPtArgs {  // passed to the kernels by value
  const orbx_kp *kps1, *raw1;  // raw: mvKeys, or null for "the same as kps"
  const float *ur1, *dp1;
  const int* n1;
  int kp_pitch1;  // 0: one keyframe shared by every pair
  const orbx_kp *kps2, *raw2;
  const float *ur2, *dp2;
  const int* n2;
  int kp_pitch2;
  float sigma2[kMaxLevels], scale[kMaxLevels];  // mvLevelSigma2, mvScaleFactors
  int nlevels, npairs;
  const int* matches12;
  int out_pitch, dedup;
  float* pos;
  uint8_t* reason;
  orbm_new_point* out_new;  // or null
  int capacity;
  int *nnew, *nnew_pair;
  orbm_newpt_emit emit;  // read when has_emit
  int has_emit;
  uint8_t *has_mp1, *has_mp2;  // or null
  int* err;                    // the handle's status word
};
// hipSuccess (0) or the launch's hipError_t
int launch_new_points(const NewPtArgs& A, const orbm_newpt_pair* d_pairs, void* stream);
int create_new_map_points_host(const orbm_newpt_pair& P, const orbx_kp* kps1, const orbx_kp* raw1, const float* ur1,
                               const float* dp1, int n1, const orbx_kp* kps2, const orbx_kp* raw2, const float* ur2,
                               const float* dp2, int n2, const float* sigma2, const float* scale, int nlevels,
                               const int* matches12, float* pos, uint8_t* reason, int* nnew, int* status);
void compute_f12_host(const orbm_camera& c1, const orbm_camera& c2, float* F12);
// Stream order of a handle's device workspace: a launch that uses it first
// waits for the last launch that used it (on whatever stream that was), so
// calls of one handle on different streams never overlap on its scratch.
struct WsOrder {
  hipEvent_t ev = nullptr;
  bool used = false;
  int before(hipStream_t s) {
    return used && hipStreamWaitEvent(s, ev, 0) != hipSuccess ? ORBX_EDEVICE : ORBX_OK;
  }
  // the same, but no wait when the last use has already finished (a
  // cross-stream wait is a barrier packet the next launch pays for); for the
  // synchronous entry points, which wait for their own work before returning
  // and so record no event after it
  int before_pending(hipStream_t s) {
    if (!used || hipEventQuery(ev) == hipSuccess) return ORBX_OK;
    return hipStreamWaitEvent(s, ev, 0) != hipSuccess ? ORBX_EDEVICE : ORBX_OK;
  }
  int after(hipStream_t s) {
    if (!ev && hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return ORBX_EDEVICE;
    if (hipEventRecord(ev, s) != hipSuccess) return ORBX_EDEVICE;
    used = true;
    return ORBX_OK;
  }
  void release() {
    if (ev) (void)hipEventDestroy(ev);
    ev = nullptr;
    used = false;
  }
};
// The streams a handle's status-word writers last ran on, each with an event
// recorded after its last such launch: a status poll waits for these events,
// not for the device (other handles' and threads' work goes on).
struct StreamMarks {
  static constexpr int kMax = 16;
  hipStream_t s[kMax] = {};
  hipEvent_t ev[kMax] = {};
  int n = 0;
  int mark(hipStream_t st) {
    int i = 0;
    while (i < n && s[i] != st) ++i;
    if (i == n) {
      if (n == kMax) {  // forget the oldest stream after waiting for it
        if (hipEventSynchronize(ev[0]) != hipSuccess) return ORBX_EDEVICE;
        hipEvent_t e0 = ev[0];
        for (int k = 1; k < n; ++k) { s[k - 1] = s[k]; ev[k - 1] = ev[k]; }
        ev[n - 1] = e0;
        i = n - 1;
      } else {
        if (!ev[i] && hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) != hipSuccess) return ORBX_EDEVICE;
        ++n;
      }
      s[i] = st;
    }
    return hipEventRecord(ev[i], st) == hipSuccess ? ORBX_OK : ORBX_EDEVICE;
  }
  int wait() {
    for (int i = 0; i < n; ++i)
      if (hipEventSynchronize(ev[i]) != hipSuccess) return ORBX_EDEVICE;
    return ORBX_OK;
  }
  void release() {
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
    for (auto& e : ev) e = nullptr;
    n = 0;
  }
};
// orbx_extractor.hip: the workspace order of an extractor (its pyramid is read by
// the stereo matcher)
WsOrder* extractor_ws(orbx_handle h);
// orbx_extractor.hip: where the handle's last orbx_extract left its frame's
// outputs on the device (count, keypoints at a pitch of `cap`, descriptors);
// an empty image leaves cap = 0 and null pointers (no keypoints);
// ORBX_EINVAL when the last extraction was not an orbx_extract call
int extractor_last_output(orbx_handle h, const int** d_count, const orbx_kp** d_kps, const uint8_t** d_desc,
                          int* cap);
// orbx_runtime.hip: raise a kernel's dynamic-LDS limit on the current device to at
// least `bytes` (never lowers it; process-wide, thread-safe)
int raise_lds_limit(const void* fn, size_t bytes);
// orbx_extractor.hip: the pyramid of frames [frame0, frame0 + n) of an extractor's last extraction
int extractor_pyramid(orbx_handle h, int frame0, int n, LevelPtrs* lp, int* w, int* hgt, float* scale,
                      float* inv_scale, int* L);
// orbx_runtime.hip: `bytes` from device memory to pinned host memory by a copy
// kernel on `stream` (a blit launch, as a graph's memcpy node runs, instead of
// a copy-engine transfer and its start-up latency)
int copy_to_host_async(void* host_dst, const void* dev_src, size_t bytes, hipStream_t stream);
// orbx_extractor.hip: the stereo Frame's two extractions (src/Frame.cc:77-80) as two
// orbx_extract calls make them, from one thread and with one wait: left staged
// and launched on its handle's stream, right on its own (the two run
// concurrently), then `between(right's stream)` enqueues the work that reads
// both outputs on the device (ComputeStereoMatches; the left chain, started
// first, has normally finished by then, so its wait costs nothing on the
// critical path), then both streams are waited for and the outputs copied
// out. Two distinct handles, non-empty images of one size.
int extract_pair(orbx_handle L, orbx_handle R, const uint8_t* imL, size_t strideL, const uint8_t* imR,
                 size_t strideR, int w, int h, const std::function<int(hipStream_t)>& between, orbx_kp* kpsL,
                 int capL, uint8_t* descL, int* nL, orbx_kp* kpsR, int capR, uint8_t* descR, int* nR,
                 double* stamps = nullptr);  // diagnostics: host clock after each of its 7 phases

// orbx_frametail.hip: the Frame constructors' tail after ExtractORB
// (UndistortKeyPoints, ComputeStereoFromRGBD). Uniform per launch; passed to
// the kernel by value.
struct FrameTailParams {
  orbx_calib calib;
  int kp_pitch;        // keypoint slots per frame (input and outputs)
  int depth_type;      // ORBX_DEPTH_*
  int convert;         // the sampled pixel is multiplied by `factor` (depth_converts)
  int w, h;            // depth image size
  float factor, mbf;
  size_t depth_frame_pitch, depth_row_stride;  // bytes
};
size_t depth_elem_size(int depth_type);  // bytes of an ORBX_DEPTH_* element, 0 for an unknown type
FrameTailParams tail_params(const orbx_calib& c, int kp_pitch, int depth_type, size_t frame_pitch, size_t row_stride,
                            int w, int h, float factor, float mbf);
// frame f: counts[f] keypoints at kps + f*kp_pitch -> kps_un (+ uright, depth
// when depth_img is not null); slots from counts[f] on are not written
int launch_frame_tail(const FrameTailParams& P, const orbx_kp* kps, const int* counts, int batch,
                      const void* depth_img, orbx_kp* kps_un, float* uright, float* depth, void* stream);
// cv::undistortPoints for n host points (x, y pairs); Frame::ComputeImageBounds
void undistort_points_host(const orbx_calib& c, const float* xy, int n, float* xy_out);
void image_bounds_host(const orbx_calib& c, int w, int h, orbm_grid_bounds* out);

// orbx_rectify.hip: cv::initUndistortRectifyMap and cv::remap (INTER_LINEAR,
// BORDER_CONSTANT 0, 8-bit) on the host, a rectifier's prepared map and the
// per-frame kernel: frame f of `batch` from src + f*src_fpitch (src_w x src_h,
// rows src_stride apart) to dst + f*dst_fpitch (dst_w x dst_h)
void rectify_maps_host(const double* K, const double* D, const double* R, const double* P, int w, int h, float* map1,
                       float* map2);
void remap_host(const uint8_t* src, int src_w, int src_h, size_t src_stride, const float* map1, const float* map2,
                int dst_w, int dst_h, uint8_t* dst, size_t dst_stride);
int rectifier_create(int device, const float* map1, const float* map2, int dst_w, int dst_h, int src_w, int src_h,
                     orbx_rectifier** out);
void rectifier_destroy(orbx_rectifier* r);
int launch_rectify(const orbx_rectifier& r, const uint8_t* src, size_t src_stride, size_t src_fpitch, uint8_t* dst,
                   size_t dst_stride, size_t dst_fpitch, int batch, hipStream_t stream);

}  // namespace orbx

// One camera's rectification (orbx_rectify_create): the prepared map on the
// device, `mpitch` records of rec_bytes (4 or 8) per destination row.
struct orbx_rectifier {
  int device;
  int dst_w, dst_h, src_w, src_h;
  int rec_bytes, mpitch;
  void* recs;
};
