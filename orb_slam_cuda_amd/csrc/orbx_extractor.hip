// orbx_extractor.hip — the extractor handle of include/orbx_c.h: its plan's
// device buffers (the plan itself is orbx_plan.hip), the batch entry point,
// the single-frame path (pinned staging, one captured graph per image size),
// the stereo pair and RGB-D calls built on it, and the handle's getters.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

#include "orbx_hostutil.h"
#include "orbx_plan.h"

using namespace orbx;

// offset of the descriptors in orbx_extract's output block (16-byte aligned
// for orient_brief's 16-byte stores)
static size_t out_desc_off(int cap_frame) { return (16 + (size_t)cap_frame * sizeof(orbx_kp) + 15) & ~(size_t)15; }
// row pitch of the single-frame staging (pinned and device) for a w-byte row
static size_t frame_pitch(size_t w) { return (w + 63) & ~(size_t)63; }

namespace {
struct Plan : HostPlan {
  DeviceBuf pyr, blur, rtab_d, cells_d, umax_d, slots, cell_counts, qkeys, qcounts, qties, qscratch, qnscratch,
      err;
};
}  // namespace

struct orbx_extractor {
  orbx_config cfg{};
  ScaleTables tab;
  Plan plan;
  hipStream_t stream = nullptr;
  // staging for the synchronous API: device buffers, pinned host staging and
  // the captured H2D -> 5 kernels -> D2H chain of a one-frame call
  // orbx_extract's device output block, laid out as h_out so that one copy
  // brings back the count, the keypoints and the descriptors (out_desc_off)
  DeviceBuf d_in, d_out;
  PinnedBuf h_in;   // the image, rows at the device pitch
  PinnedBuf h_out;  // {count, status, -, -} + cap keypoints + (16-B aligned) cap descriptors
  hipGraphExec_t graph = nullptr;
  int graph_w = 0, graph_h = 0;
  bool graph_hp = false;  // the graph holds the host-pyramid copy branch
  bool last_single = false;  // the last extraction was orbx_extract (outputs in d_out)
  bool last_empty = false;   // ... of an empty image (no outputs, src/ORBextractor.cc:1542-1543)
  int warm_w = 0, warm_h = 0;  // size of the last plain (uncaptured) call: capture from the next one
  int last_batch = 0;
  const uint8_t* last_frames = nullptr;
  size_t last_fpitch = 0, last_rstride = 0;
  bool timing = false;
  hipEvent_t ev[6] = {};
  void* user_ev[ORBX_STAGE_EVENTS] = {};
  bool has_user_ev = false;
  WsOrder ws;  // stream order of the plan buffers (pyramid, blur, slots, quadtree)
  // host pyramid (orbx_set_host_pyramid): orbx_extract also copies levels >= 1
  // of its frame into pinned memory, on a graph branch forked right after the
  // pyramid stage and joined at the end of the call (the copy overlaps FAST ..
  // BRIEF); level 0 is the pinned input staging itself
  bool host_pyr = false;
  bool host_pyr_valid = false;  // h_pyr holds the last orbx_extract's levels
  PinnedBuf h_pyr;
  long long h_pyr_off[kMaxLevels] = {};  // level l's offset in h_pyr (l >= 1)
  hipStream_t pstream = nullptr;         // the copy branch's stream (capture fork)
  hipEvent_t pev[2] = {};                // pyramid done, copy done
  // orbx_rgbd_frame: the raw depth image (pinned staging and its device copy,
  // rows at a 64-byte pitch; uploaded on dstream beside the extraction, joined
  // by dev) and the tail kernel's outputs {cap keypoints, cap uRight, cap
  // depth}, which the kernel stores straight into pinned host memory
  DeviceBuf d_depth;
  PinnedBuf h_depth, h_tail;
  hipStream_t dstream = nullptr;
  hipEvent_t dev = nullptr;  // depth upload done
  // orbx_set_rectify: while set, the staged image is the raw camera image; it
  // is uploaded to d_raw and the remap kernel writes d_in ahead of the pyramid
  orbx_rectifier* rect = nullptr;
  DeviceBuf d_raw;
  // ORBX_EXTRACT_PROF=1 (diagnostics): orbx_extract's host phases per call
  // (s), their medians printed by orbx_destroy: staging copy, issue, wait, copy-out
  std::vector<float> prof_t[4];
  char order[6] = {};  // the stages' launch order (orbx_set_stage_order; default extract_stage_order())
  std::mutex mu;
};

WsOrder* orbx::extractor_ws(orbx_handle h) { return h ? &h->ws : nullptr; }

// the single-frame graph was captured for a setting or a buffer that changes
static void drop_graph(orbx_extractor* h) {
  if (h->graph) (void)hipGraphExecDestroy(h->graph);
  h->graph = nullptr;
}

// The plan for W x Hh frames (orbx_plan.hip) and its device half: buffers,
// table uploads, the kernels' LDS limits and the band plans' occupancy.
static int build_plan(orbx_extractor* h, int W, int Hh, int B) {
  int rc;
  Plan& pl = h->plan;
  if ((rc = build_plan_host(h->cfg, h->tab, W, Hh, B, pl))) return rc;
  const ExtractParams& P = pl.P;
  const int L = P.L, slot = P.slots_per_frame;
  const long long lvl_off = pl.level_bytes;
  // device buffers (the pyramid's level-0 planes stay unused: level 0 is the caller's frames)
  if ((rc = device_alloc(pl.pyr, (size_t)lvl_off))) return rc;
  if ((rc = device_alloc(pl.blur, (size_t)lvl_off))) return rc;
  if ((rc = device_alloc(pl.rtab_d, std::max<size_t>(pl.rtab.size(), 1) * sizeof(int2)))) return rc;
  if ((rc = device_alloc(pl.cells_d, pl.cells.size() * sizeof(CellGeom)))) return rc;
  if ((rc = device_alloc(pl.umax_d, 16 * sizeof(int)))) return rc;
  if ((rc = device_alloc(pl.slots, (size_t)B * slot * 4 + 4 + 4 * 96))) return rc;  // + the quadtree's prefetch overrun
  if ((rc = device_alloc(pl.cell_counts, (size_t)B * P.ncells_total * 4))) return rc;
  if ((rc = device_alloc(pl.qkeys, (size_t)B * P.kp_per_frame * 4))) return rc;
  if ((rc = device_alloc(pl.qcounts, (size_t)B * L * 4 + 4 * kMaxLevels))) return rc;  // orient_brief reads kMaxLevels counts per frame
  if ((rc = device_alloc(pl.qties, (size_t)B * L * 16))) return rc;
  if ((rc = device_alloc(pl.qscratch, (size_t)B * slot * 4 + 4))) return rc;
  if ((rc = device_alloc(pl.qnscratch, (size_t)B * slot * 2 + 4))) return rc;
  if ((rc = device_alloc(pl.err, 16))) return rc;
  HIP_OK(g_err, hipMemcpy(pl.rtab_d.p, pl.rtab.data(), pl.rtab.size() * sizeof(int2), hipMemcpyHostToDevice));
  HIP_OK(g_err, hipMemcpy(pl.cells_d.p, pl.cells.data(), pl.cells.size() * sizeof(CellGeom), hipMemcpyHostToDevice));
  HIP_OK(g_err, hipMemcpy(pl.umax_d.p, h->tab.umax, 16 * sizeof(int), hipMemcpyHostToDevice));
  HIP_OK(g_err, hipMemset(pl.err.p, 0, 16));
  if (P.pyr_fused && getenv("ORBX_PYR_PROF") && getenv("ORBX_PYR_PROF")[0] == '1')
    for (int i = 0; i < P.pyr_nplans; ++i)
      fprintf(stderr, "pyr plan %d: %d bands x %d column tiles, lds %d + %d + %d, cost %d\n", i,
              P.pyr_plan[i].nbands, P.pyr_plan[i].nct, P.pyr_plan[i].lds_a, P.pyr_plan[i].lds_b, P.pyr_plan[i].lds_y,
              P.pyr_plan[i].cost);
  if (P.pyr_fused) {
    size_t mx = 0;
    for (int i = 0; i < P.pyr_nplans; ++i) {
      ExtractParams Q = P;
      select_pyr_plan(Q, i);
      mx = std::max(mx, pyr_band_lds_bytes(Q));
    }
    if (raise_lds_limit(pyr_band_kernel_ptr(), mx))
      return g_err.fail(ORBX_EDEVICE, "LDS limit of pyr_band_kernel: %s", hipGetErrorString(hipGetLastError()));
    for (int i = 0; i < P.pyr_nplans; ++i) {
      ExtractParams Q = P;
      select_pyr_plan(Q, i);
      pl.P.pyr_plan[i].occ = pyr_band_occupancy(pyr_band_lds_bytes(Q));
      if (getenv("ORBX_PYR_PROF") && getenv("ORBX_PYR_PROF")[0] == '1')
        fprintf(stderr, "pyr plan %d: %d workgroups per CU\n", i, pl.P.pyr_plan[i].occ);
    }
  }
  if (raise_lds_limit(quadtree_kernel_ptr(P), quadtree_lds_bytes(P)))
    return g_err.fail(ORBX_EDEVICE, "LDS limit of quadtree_kernel: %s", hipGetErrorString(hipGetLastError()));
  return ORBX_OK;
}

static ExtractBuffers buffers_of(const Plan& pl) {
  ExtractBuffers X;
  X.pyr = pl.pyr.as<uint8_t>();
  X.blur = pl.blur.as<uint8_t>();
  X.rtab = pl.rtab_d.as<int2>();
  X.cells = pl.cells_d.as<CellGeom>();
  X.umax = pl.umax_d.as<int>();
  X.slots = pl.slots.as<uint32_t>();
  X.cell_counts = pl.cell_counts.as<int>();
  X.qkeys = pl.qkeys.as<uint32_t>();
  X.qcounts = pl.qcounts.as<int>();
  X.qties = pl.qties.as<int>();
  X.qscratch = pl.qscratch.as<uint32_t>();
  X.qnode_scratch = pl.qnscratch.as<uint16_t>();
  X.qscratch_per_fl = 0;
  X.err = pl.err.as<int>();
  return X;
}

// The device pyramid (mvImagePyramid) of frames [frame0, frame0 + n) of the
// last extraction: level 0 is the caller's frames, levels >= 1 the plan's planes.
int orbx::extractor_pyramid(orbx_handle h, int frame0, int n, LevelPtrs* lp, int* w, int* hgt, float* scale,
                            float* inv_scale, int* L) {
  if (!h) return g_err.fail(ORBX_EINVAL, "null extractor handle");
  if (frame0 < 0 || n < 1 || frame0 + n > h->last_batch || !h->last_frames)
    return g_err.fail(ORBX_EINVAL, "frames [%d, %d) not in the extractor's last extraction (%d frames)", frame0,
                frame0 + n, h->last_batch);
  const ExtractParams& P = h->plan.P;
  const ExtractBuffers X = buffers_of(h->plan);
  *L = P.L;
  for (int l = 0; l < P.L; ++l) {
    const LevelGeom& g = P.lv[l];
    if (l == 0) {
      lp->base[0] = h->last_frames + (long long)frame0 * h->last_fpitch;
      lp->fstride[0] = (long long)h->last_fpitch;
      lp->pitch[0] = (int)h->last_rstride;
    } else {
      lp->base[l] = X.pyr + g.off + (long long)frame0 * g.plane;
      lp->fstride[l] = g.plane;
      lp->pitch[l] = g.pitch;
    }
    lp->aligned16[l] = 0;
    w[l] = g.w;
    hgt[l] = g.h;
    scale[l] = h->tab.scale[l];
    inv_scale[l] = h->tab.inv_scale[l];
  }
  return ORBX_OK;
}

int orbx::extractor_last_output(orbx_handle h, const int** d_count, const orbx_kp** d_kps, const uint8_t** d_desc,
                                int* cap) {
  if (!h) return g_err.fail(ORBX_EINVAL, "null extractor handle");
  if (h->last_empty) {  // an empty image: no keypoints
    *d_count = nullptr;
    *d_kps = nullptr;
    *d_desc = nullptr;
    *cap = 0;
    return ORBX_OK;
  }
  if (!h->last_single || !h->d_out.p)
    return g_err.fail(ORBX_EINVAL, "the extractor's last extraction was not an orbx_extract call");
  const int c = h->plan.P.kp_per_frame;
  uint8_t* d = h->d_out.as<uint8_t>();
  *d_count = (const int*)d;
  *d_kps = (const orbx_kp*)(d + 16);
  *d_desc = d + out_desc_off(c);
  *cap = c;
  return ORBX_OK;
}

// ------------------------------------------------------------ C ABI
extern "C" {

int orbx_create(const orbx_config* cfg, orbx_handle* out) {
  if (!cfg || !out) return g_err.fail(ORBX_EINVAL, "null argument");
  *out = nullptr;
  const orbx_config& c = *cfg;
  if (c.nlevels < 1 || c.nlevels > kMaxLevels) return g_err.fail(ORBX_EINVAL, "nlevels must be 1..%d", kMaxLevels);
  if (c.nfeatures < 0) return g_err.fail(ORBX_EINVAL, "nfeatures < 0");
  if (!(c.scale_factor > 1.0f)) return g_err.fail(ORBX_EINVAL, "scaleFactor must be > 1");
  // Camera.width/height absent from the yaml (the reference's mono KITTI /
  // EuRoC settings, src/Tracking.cc:124-133) arrive as 0: mode U's tables do
  // not depend on the size, so the plan waits for the first image; mode F's
  // scale override is computed from the width (src/ORBextractor.cc:674-680)
  const bool deferred = c.width == 0 && c.height == 0 && c.scale_mode == ORBX_SCALE_U;
  if (!deferred && (c.width <= 0 || c.height <= 0))
    return g_err.fail(ORBX_EINVAL, c.scale_mode == ORBX_SCALE_F && c.width == 0 && c.height == 0
                                 ? "scale mode F needs width/height (Camera.width/height)"
                                 : "width/height must be > 0, or both 0 in scale mode U (Camera.width/height)");
  if (c.max_batch < 1) return g_err.fail(ORBX_EINVAL, "max_batch must be >= 1");
  if (c.scale_mode != ORBX_SCALE_U && c.scale_mode != ORBX_SCALE_F) return g_err.fail(ORBX_EINVAL, "bad scale_mode");
  if (c.pattern_mode != ORBX_PATTERN_FORK && c.pattern_mode != ORBX_PATTERN_UPSTREAM)
    return g_err.fail(ORBX_EINVAL, "bad pattern_mode");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return g_err.fail(ORBX_EDEVICE, "no HIP device");
  if (c.device < 0 || c.device >= ndev) return g_err.fail(ORBX_EINVAL, "device %d out of range", c.device);
  HIP_OK(g_err, hipSetDevice(c.device));
  hipDeviceProp_t prop;
  HIP_OK(g_err, hipGetDeviceProperties(&prop, c.device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return g_err.fail(ORBX_EDEVICE, "device %d is %s; liborbx is built for gfx950 only", c.device, prop.gcnArchName);
  orbx_extractor* h = new orbx_extractor();
  h->cfg = c;
  memcpy(h->order, extract_stage_order(), 6);
  compute_scales(c, h->tab);
  h->plan.B = c.max_batch;
  int rc = deferred ? ORBX_OK : build_plan(h, c.width, c.height, c.max_batch);
  if (rc) { delete h; return rc; }
  // h->stream (the synchronous API's stream) is created on first use: an idle
  // stream would still take one of the process's few hardware queues, and a
  // host that pipelines on its own streams wants those on distinct queues
  const char* t = getenv("ORBX_TIMING");
  h->timing = t && t[0] == '1';
  if (h->timing)
    for (auto& e : h->ev) (void)hipEventCreate(&e);
  *out = h;
  return ORBX_OK;
}

int orbx_destroy(orbx_handle h) {
  if (!h) return ORBX_OK;
  (void)hipSetDevice(h->cfg.device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  for (auto& e : h->ev)
    if (e) (void)hipEventDestroy(e);
  if (h->ws.ev) (void)hipEventSynchronize(h->ws.ev);
  h->ws.release();
  drop_graph(h);
  if (h->pstream) (void)hipStreamSynchronize(h->pstream);
  if (h->prof_t[0].size() > 20) {
    // medians over the calls after the first 20 (plan, capture, warm-up)
    double med[4];
    for (int k = 0; k < 4; ++k) {
      std::vector<float> v(h->prof_t[k].begin() + 20, h->prof_t[k].end());
      std::nth_element(v.begin(), v.begin() + v.size() / 2, v.end());
      med[k] = v[v.size() / 2] * 1e6;
    }
    fprintf(stderr, "orbx_extract host phases, median of %zu calls (us): stage %.1f issue %.1f wait %.1f out %.1f\n",
            h->prof_t[0].size() - 20, med[0], med[1], med[2], med[3]);
  }
  // the pinned buffers go before their streams (the device ones with the handle, as ever)
  h->h_in.release();
  h->h_out.release();
  h->h_pyr.release();
  if (h->dstream) (void)hipStreamSynchronize(h->dstream);
  h->h_depth.release();
  h->h_tail.release();
  if (h->dev) (void)hipEventDestroy(h->dev);
  if (h->dstream) (void)hipStreamDestroy(h->dstream);
  for (auto& e : h->pev)
    if (e) (void)hipEventDestroy(e);
  if (h->pstream) (void)hipStreamDestroy(h->pstream);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
  return ORBX_OK;
}

int orbx_frame_capacity(orbx_handle h) { return h ? h->plan.P.kp_per_frame : 0; }

int orbx_extract_batch(orbx_handle h, const uint8_t* d_frames, int batch, size_t frame_pitch, size_t row_stride,
                       orbx_kp* d_kps, uint8_t* d_desc, int* d_counts, void* stream) {
  if (!h || !d_frames || !d_kps || !d_desc || !d_counts) return g_err.fail(ORBX_EINVAL, "null argument");
  // one call of a handle at a time: a synchronous orbx_extract in flight on
  // another thread holds the lock until its chain has finished (it records
  // no workspace event for a batch call to wait on), and it may re-plan the
  // handle for a new image size, so the plan is checked under the lock
  std::lock_guard<std::mutex> lk(h->mu);
  if (batch < 1 || batch > h->plan.B) return g_err.fail(ORBX_EINVAL, "batch %d not in 1..max_batch(%d)", batch, h->plan.B);
  if (h->plan.W == 0)
    return g_err.fail(ORBX_EINVAL, "no frame size yet: the handle was created with width/height 0 and has seen no orbx_extract");
  if (row_stride < (size_t)h->plan.W) return g_err.fail(ORBX_EINVAL, "row_stride < width");
  HIP_OK(g_err, hipSetDevice(h->cfg.device));
  void** ev = h->has_user_ev ? h->user_ev : (h->timing ? (void**)h->ev : nullptr);
  h->has_user_ev = false;
  if (h->ws.before((hipStream_t)stream)) return g_err.fail(ORBX_EDEVICE, "stream wait on the handle's last use failed");
  const int rc = launch_extract(h->plan.P, buffers_of(h->plan), d_frames, batch, frame_pitch, row_stride, d_kps,
                                d_desc, d_counts, stream, ev, nullptr, nullptr, h->order);
  if (!rc && h->ws.after((hipStream_t)stream)) return g_err.fail(ORBX_EDEVICE, "event record failed");
  h->last_batch = batch;
  h->last_frames = d_frames;
  h->last_fpitch = frame_pitch;
  h->last_rstride = row_stride;
  h->host_pyr_valid = false;  // the pinned host pyramid is of an earlier orbx_extract
  h->last_single = false;
  h->last_empty = false;
  if (rc) return g_err.fail(rc, "kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
  return ORBX_OK;
}

// ORBextractor::operator() on one host image (the call Tracking makes per
// frame, src/Frame.cc:246-252 -> src/ORBextractor.cc:1538). The image is
// staged in a pinned buffer; the H2D copy, the five extraction launches and
// one D2H copy of {count, status, keypoints, descriptors} (full capacity, so
// no second round trip) run as one captured hipGraph replayed per call, and
// the call synchronises once. ORBX_EXTRACT_GRAPH=0 issues the same chain as
// plain stream operations (A/B); ORBX_TIMING=1 implies that path.

// Host-pyramid layout: frame 0's levels 1..L-1 packed at their device pitches.
// With max_batch 1 the device planes of levels >= 1 are one contiguous block
// (level-major [l][B][h][pitch]), so the copy is one linear D2H.
static size_t host_pyr_layout(orbx_extractor* h) {
  const ExtractParams& P = h->plan.P;
  size_t off = 0;
  for (int l = 1; l < P.L; ++l) {
    h->h_pyr_off[l] = (long long)off;
    off += (size_t)P.lv[l].plane;
  }
  return off;
}

static int issue_one_frame(orbx_extractor* h, size_t pitch, int hh, int cap_frame) {
  hipStream_t s = h->stream;
  const ExtractParams& P = h->plan.P;
  if (h->rect) {
    // the raw image to its own buffer, its rectification into the frame buffer
    HIP_OK(g_err, hipMemcpyAsync(h->d_raw.p, h->h_in.p, pitch * hh, hipMemcpyHostToDevice, s));
    if (launch_rectify(*h->rect, h->d_raw.as<uint8_t>(), pitch, pitch * hh, h->d_in.as<uint8_t>(), pitch, pitch * hh, 1,
                       s))
      return g_err.fail(ORBX_EDEVICE, "remap launch failed: %s", hipGetErrorString(hipGetLastError()));
  } else {
    HIP_OK(g_err, hipMemcpyAsync(h->d_in.p, h->h_in.p, pitch * hh, hipMemcpyHostToDevice, s));
  }
  uint8_t* d = h->d_out.as<uint8_t>();
  const size_t doff = out_desc_off(cap_frame);
  const bool hp = h->host_pyr && P.L > 1;
  // level 0 of the host pyramid is the pinned staging: with a rectifier the
  // rectified image is copied back over the raw one (uploaded by then)
  const bool hp0 = h->host_pyr && h->rect;
  const int rc = launch_extract(P, buffers_of(h->plan), h->d_in.as<uint8_t>(), 1, pitch * hh, pitch,
                                (orbx_kp*)(d + 16), d + doff, (int*)d, s, h->timing ? (void**)h->ev : nullptr,
                                hp ? (void*)h->pev[0] : nullptr, (int*)d + 1, h->order);
  if (rc) return g_err.fail(rc, "kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
  if (hp) {
    // fork: the pyramid levels go to pinned host memory beside FAST .. BRIEF
    HIP_OK(g_err, hipStreamWaitEvent(h->pstream, h->pev[0], 0));
    const uint8_t* pyr = h->plan.pyr.as<uint8_t>();
    uint8_t* hpyr = (uint8_t*)h->h_pyr.p;
    if (h->plan.B == 1) {
      const size_t bytes = (size_t)(P.lv[P.L - 1].off + P.lv[P.L - 1].plane - P.lv[1].off);
      HIP_OK(g_err, hipMemcpyAsync(hpyr, pyr + P.lv[1].off, bytes, hipMemcpyDeviceToHost, h->pstream));
    } else {
      for (int l = 1; l < P.L; ++l)
        HIP_OK(g_err, hipMemcpyAsync(hpyr + h->h_pyr_off[l], pyr + P.lv[l].off, (size_t)P.lv[l].plane,
                              hipMemcpyDeviceToHost, h->pstream));
    }
    if (hp0) HIP_OK(g_err, hipMemcpyAsync(h->h_in.p, h->d_in.p, pitch * hh, hipMemcpyDeviceToHost, h->pstream));
    HIP_OK(g_err, hipEventRecord(h->pev[1], h->pstream));
  } else if (hp0) {
    HIP_OK(g_err, hipMemcpyAsync(h->h_in.p, h->d_in.p, pitch * hh, hipMemcpyDeviceToHost, s));
  }
  // count, status word (bytes 4..7 of the block's header, written there by
  // the last stage), keypoints and descriptors in one copy
  uint8_t* o = (uint8_t*)h->h_out.p;
  HIP_OK(g_err, hipMemcpyAsync(o, d, doff + (size_t)cap_frame * 32, hipMemcpyDeviceToHost, s));
  if (hp) HIP_OK(g_err, hipStreamWaitEvent(s, h->pev[1], 0));  // join
  return ORBX_OK;
}

// orbx_extract's halves. extract_submit: the image staged in the handle's
// pinned buffer and the call's chain (H2D, the five launches, one D2H of
// {count, status, keypoints, descriptors}) issued on its stream; the handle's
// lock is held, the image is not empty. extract_finish: after that stream was
// waited for, the outputs copied out of the pinned block.
// extract_submit = extract_prepare (plan and buffers for the image size),
// extract_stage (the copy into the pinned staging; no HIP call, so another
// thread may run it) and extract_issue (the chain on the handle's stream).
static int extract_prepare(orbx_extractor* h, const uint8_t* img, int w, int hh, size_t stride) {
  h->last_empty = false;
  if (!img || w < 0 || hh < 0 || stride < (size_t)w) return g_err.fail(ORBX_EINVAL, "bad image");
  if (const orbx_rectifier* r = h->rect)
    if (r->src_w != w || r->src_h != hh || r->dst_w != w || r->dst_h != hh)
      return g_err.fail(ORBX_EINVAL, "the handle's rectifier maps %d x %d to %d x %d, the image is %d x %d", r->src_w, r->src_h,
                  r->dst_w, r->dst_h, w, hh);
  HIP_OK(g_err, hipSetDevice(h->cfg.device));
  if (w != h->plan.W || hh != h->plan.H) {
    // the reference accepts any image size per call: re-plan for it (after
    // every launch that uses the current plan's buffers)
    if (h->ws.ev) (void)hipEventSynchronize(h->ws.ev);
    drop_graph(h);
    const int rc = build_plan(h, w, hh, h->plan.B);
    if (rc) return rc;
    h->d_in.release();
  }
  const int cap_frame = h->plan.P.kp_per_frame;
  const size_t pitch = frame_pitch(w);
  const size_t out_bytes = out_desc_off(cap_frame) + (size_t)cap_frame * 32;
  int rc;
  // a buffer that grows takes the graph captured on the old one with it
  auto grow = [h](DeviceBuf& b, size_t bytes) {
    if (b.n >= bytes) return (int)ORBX_OK;
    drop_graph(h);
    return device_alloc(b, bytes);
  };
  if ((rc = grow(h->d_in, pitch * hh)) || (rc = grow(h->d_out, out_bytes)) ||
      (h->rect && (rc = grow(h->d_raw, pitch * hh))))
    return rc;
  if (h->h_in.n < pitch * hh || h->h_out.n < out_bytes) drop_graph(h);
  if ((rc = pinned_reserve(h->h_in, pitch * hh)) || (rc = pinned_reserve(h->h_out, out_bytes))) return rc;
  if (!h->stream) HIP_OK(g_err, hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  h->host_pyr_valid = false;
  if (h->graph && h->graph_hp != h->host_pyr) drop_graph(h);  // captured with / without the copy branch
  if (h->host_pyr) {
    const size_t pb = host_pyr_layout(h);
    if (h->h_pyr.n < pb) drop_graph(h);
    if ((rc = pinned_reserve(h->h_pyr, std::max<size_t>(pb, 64)))) return rc;
    if (!h->pstream) HIP_OK(g_err, hipStreamCreateWithFlags(&h->pstream, hipStreamNonBlocking));
    for (auto& e : h->pev)
      if (!e) HIP_OK(g_err, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  return ORBX_OK;
}

static void extract_stage(orbx_extractor* h, const uint8_t* img, int w, int hh, size_t stride) {
  // the pinned staging buffer is free: every call waits for its chain before it returns
  // (plain stores: streaming ones that skip the destination's read-for-ownership
  // measured slower, 0.108 vs 0.100 ms per call: the copy engine then reads DRAM
  // instead of lines still in the host's caches)
  const size_t pitch = frame_pitch(w);
  if (stride == pitch) {
    memcpy(h->h_in.p, img, pitch * hh);
  } else {
    for (int y = 0; y < hh; ++y) memcpy((uint8_t*)h->h_in.p + (size_t)y * pitch, img + (size_t)y * stride, w);
  }
}

// mark: record the handle's workspace event after the chain (for work another
// stream orders after it: the stereo pair's left chain); the synchronous
// callers wait for the chain themselves, so later users find it finished
static int extract_issue(orbx_extractor* h, int w, int hh, bool mark) {
  const int cap_frame = h->plan.P.kp_per_frame;
  const size_t pitch = frame_pitch(w);
  int rc;
  // the plan buffers may still be in use by a batch call on another stream
  if (h->ws.before_pending(h->stream)) return g_err.fail(ORBX_EDEVICE, "stream wait on the handle's last use failed");
  static const bool use_graph = !(getenv("ORBX_EXTRACT_GRAPH") && getenv("ORBX_EXTRACT_GRAPH")[0] == '0');
  // the first call of a size runs plain (one-time uploads and attribute
  // queries of the launchers happen outside any capture); later ones replay
  if (h->graph && (h->graph_w != w || h->graph_h != hh)) drop_graph(h);
  if (use_graph && !h->timing && (h->graph || (h->warm_w == w && h->warm_h == hh))) {
    if (!h->graph) {
      hipGraph_t g = nullptr;
      HIP_OK(g_err, hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
      rc = issue_one_frame(h, pitch, hh, cap_frame);
      const hipError_t ec = hipStreamEndCapture(h->stream, &g);
      if (rc) {
        if (g) (void)hipGraphDestroy(g);
        return rc;
      }
      if (ec != hipSuccess) return g_err.fail(ORBX_EDEVICE, "hipStreamEndCapture: %s", hipGetErrorString(ec));
      const hipError_t ei = hipGraphInstantiate(&h->graph, g, nullptr, nullptr, 0);
      (void)hipGraphDestroy(g);
      if (ei != hipSuccess) {
        h->graph = nullptr;
        return g_err.fail(ORBX_EDEVICE, "hipGraphInstantiate: %s", hipGetErrorString(ei));
      }
      h->graph_w = w;
      h->graph_h = hh;
      h->graph_hp = h->host_pyr;
    }
    HIP_OK(g_err, hipGraphLaunch(h->graph, h->stream));
  } else {
    if ((rc = issue_one_frame(h, pitch, hh, cap_frame))) return rc;
    h->warm_w = w;
    h->warm_h = hh;
  }
  if (mark && h->ws.after(h->stream)) return g_err.fail(ORBX_EDEVICE, "event record failed");
  h->last_batch = 1;
  h->last_single = true;
  h->last_frames = h->d_in.as<uint8_t>();
  h->last_fpitch = pitch * hh;
  h->last_rstride = pitch;
  return ORBX_OK;
}

static int extract_submit(orbx_extractor* h, const uint8_t* img, int w, int hh, size_t stride, double* t_staged) {
  const int rc = extract_prepare(h, img, w, hh, stride);
  if (rc) return rc;
  extract_stage(h, img, w, hh, stride);
  if (t_staged) *t_staged = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
  return extract_issue(h, w, hh, false);
}

static int extract_finish(orbx_extractor* h, orbx_kp* kps, int cap, uint8_t* desc, int* n) {
  h->host_pyr_valid = h->host_pyr;
  const int cap_frame = h->plan.P.kp_per_frame;
  const int* head = (const int*)h->h_out.p;
  const int cnt = head[0], err = head[1];
  if (err) {
    // reported once, not on every later call: cleared in the handle's stream
    // order (after any batch call still using the plan, before the next one)
    if (h->ws.before(h->stream)) return g_err.fail(ORBX_EDEVICE, "stream wait on the handle's last use failed");
    HIP_OK(g_err, hipMemsetAsync(h->plan.err.p, 0, 16, h->stream));
    if (h->ws.after(h->stream)) return g_err.fail(ORBX_EDEVICE, "event record failed");
    HIP_OK(g_err, hipStreamSynchronize(h->stream));
    return g_err.fail(ORBX_ECAPACITY, "device error word 0x%x", err);
  }
  *n = cnt;
  if (cnt > cap) return g_err.fail(ORBX_ECAPACITY, "%d keypoints do not fit cap %d", cnt, cap);
  const uint8_t* o = (const uint8_t*)h->h_out.p + 16;
  if (kps) memcpy(kps, o, (size_t)cnt * sizeof(orbx_kp));
  if (desc) memcpy(desc, (const uint8_t*)h->h_out.p + out_desc_off(cap_frame), (size_t)cnt * 32);
  return ORBX_OK;
}

static void extract_empty(orbx_extractor* h) {
  // src/ORBextractor.cc:1542-1543: no outputs. Later readers of "the last
  // extraction" (the stereo matcher on the device outputs, the host pyramid)
  // see an empty one, as the reference's Frame sees empty mvKeysRight
  h->last_single = false;
  h->last_empty = true;
  h->host_pyr_valid = false;
  h->last_batch = 0;
}

int orbx_extract(orbx_handle h, const uint8_t* img, int w, int hh, size_t stride, orbx_kp* kps, int cap,
                 uint8_t* desc, int* n) {
  if (!h || !n) return g_err.fail(ORBX_EINVAL, "null argument");
  std::lock_guard<std::mutex> lk(h->mu);
  *n = 0;
  if (w == 0 || hh == 0) {
    extract_empty(h);
    return ORBX_OK;
  }
  static const bool prof = getenv("ORBX_EXTRACT_PROF") && getenv("ORBX_EXTRACT_PROF")[0] == '1';
  auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t0 = prof ? now() : 0;
  double t1 = 0;
  int rc = extract_submit(h, img, w, hh, stride, prof ? &t1 : nullptr);
  if (rc) return rc;
  const double t2 = prof ? now() : 0;
  HIP_OK(g_err, hipStreamSynchronize(h->stream));
  const double t3 = prof ? now() : 0;
  if ((rc = extract_finish(h, kps, cap, desc, n))) return rc;
  if (prof) {
    const double t4 = now();
    h->prof_t[0].push_back((float)(t1 - t0));
    h->prof_t[1].push_back((float)(t2 - t1));
    h->prof_t[2].push_back((float)(t3 - t2));
    h->prof_t[3].push_back((float)(t4 - t3));
  }
  return ORBX_OK;
}

// orbx_extract and the Frame constructor's tail (orbx_frametail.hip) in one device round trip
int orbx_rgbd_frame(orbx_handle h, const uint8_t* img, size_t stride, const void* depth_img, int depth_type,
                    size_t depth_stride, int w, int hh, const orbx_calib* calib, float depth_factor, float mbf,
                    orbx_kp* kps, int cap, uint8_t* desc, int* n, orbx_kp* kps_un, float* uRight, float* depth) {
  if (!h || !n) return g_err.fail(ORBX_EINVAL, "null argument");
  if (!calib) return g_err.fail(ORBX_EINVAL, "orbx_rgbd_frame: null calib");
  const size_t es = depth_elem_size(depth_type);
  if (!es) return g_err.fail(ORBX_EINVAL, "orbx_rgbd_frame: unknown depth_type %d", depth_type);
  std::lock_guard<std::mutex> lk(h->mu);
  *n = 0;
  if (w == 0 || hh == 0) {
    extract_empty(h);
    return ORBX_OK;
  }
  if (w < 0 || hh < 0) return g_err.fail(ORBX_EINVAL, "bad image");
  if (depth_img && depth_stride < (size_t)w * es)
    return g_err.fail(ORBX_EINVAL, "orbx_rgbd_frame: depth_stride %zu below %d elements of %zu bytes", depth_stride, w, es);
  if (w != h->plan.W || hh != h->plan.H)
    return g_err.fail(ORBX_EINVAL, "orbx_rgbd_frame: the handle is planned for %d x %d, not %d x %d", h->plan.W, h->plan.H,
                w, hh);
  const int cap_frame = h->plan.P.kp_per_frame;
  if (cap < cap_frame) return g_err.fail(ORBX_EINVAL, "orbx_rgbd_frame: cap %d below the handle's capacity %d", cap, cap_frame);
  if (!kps_un || (depth_img && (!uRight || !depth))) return g_err.fail(ORBX_EINVAL, "orbx_rgbd_frame: null output");
  int rc = extract_prepare(h, img, w, hh, stride);
  if (rc) return rc;
  // the tail's outputs: cap keypoints, cap uRight, cap depth, in pinned host memory
  const size_t ur_off = (size_t)cap_frame * sizeof(orbx_kp), dp_off = ur_off + (size_t)cap_frame * 4;
  const size_t tail_bytes = depth_img ? dp_off + (size_t)cap_frame * 4 : ur_off;
  const size_t dpitch = frame_pitch((size_t)w * es);
  if ((rc = pinned_reserve(h->h_tail, tail_bytes))) return rc;
  void* tail_dev = nullptr;
  HIP_OK(g_err, hipHostGetDevicePointer(&tail_dev, h->h_tail.p, 0));
  if (depth_img) {
    if (h->d_depth.n < dpitch * hh && (rc = device_alloc(h->d_depth, dpitch * hh))) return rc;
    if ((rc = pinned_reserve(h->h_depth, dpitch * hh))) return rc;
    if (!h->dstream) HIP_OK(g_err, hipStreamCreateWithFlags(&h->dstream, hipStreamNonBlocking));
    if (!h->dev) HIP_OK(g_err, hipEventCreateWithFlags(&h->dev, hipEventDisableTiming));
  }
  extract_stage(h, img, w, hh, stride);
  if ((rc = extract_issue(h, w, hh, false))) return rc;
  // from here on the device is extracting: a failure waits for it before it returns
  auto issue_tail = [&]() -> int {
    if (depth_img) {
      // the depth image is staged while the extraction runs and uploaded on its
      // own stream; the handle's stream waits for it before the tail kernel
      for (int y = 0; y < hh; ++y)
        memcpy((uint8_t*)h->h_depth.p + (size_t)y * dpitch, (const uint8_t*)depth_img + (size_t)y * depth_stride,
               (size_t)w * es);
      HIP_OK(g_err, hipMemcpyAsync(h->d_depth.p, h->h_depth.p, dpitch * hh, hipMemcpyHostToDevice, h->dstream));
      HIP_OK(g_err, hipEventRecord(h->dev, h->dstream));
      HIP_OK(g_err, hipStreamWaitEvent(h->stream, h->dev, 0));
    }
    // after the extraction's last kernel, on its stream: a plain launch on the
    // count and keypoints where the chain left them
    uint8_t* d = h->d_out.as<uint8_t>();
    uint8_t* t = (uint8_t*)tail_dev;
    const FrameTailParams P = tail_params(*calib, cap_frame, depth_type, dpitch * hh, dpitch, w, hh, depth_factor, mbf);
    if (launch_frame_tail(P, (const orbx_kp*)(d + 16), (const int*)d, 1, depth_img ? h->d_depth.p : nullptr,
                          (orbx_kp*)t, (float*)(t + ur_off), (float*)(t + dp_off), h->stream))
      return g_err.fail(ORBX_EDEVICE, "frame tail launch failed: %s", hipGetErrorString(hipGetLastError()));
    return ORBX_OK;
  };
  rc = issue_tail();
  if (rc) {
    if (h->dstream) (void)hipStreamSynchronize(h->dstream);
    (void)hipStreamSynchronize(h->stream);
    return rc;
  }
  HIP_OK(g_err, hipStreamSynchronize(h->stream));
  if ((rc = extract_finish(h, kps, cap, desc, n))) return rc;
  const size_t cnt = (size_t)*n;
  const uint8_t* o = (const uint8_t*)h->h_tail.p;
  memcpy(kps_un, o, cnt * sizeof(orbx_kp));
  if (depth_img) {
    memcpy(uRight, o + ur_off, cnt * 4);
    memcpy(depth, o + dp_off, cnt * 4);
  } else {  // the monocular constructor: no stereo information (src/Frame.cc:200-201)
    if (uRight) std::fill(uRight, uRight + cnt, -1.f);
    if (depth) std::fill(depth, depth + cnt, -1.f);
  }
  return ORBX_OK;
}

int orbx_set_rectify(orbx_handle h, orbx_rectify_handle r) {
  if (!h) return g_err.fail(ORBX_EINVAL, "null handle");
  if (r && r->device != h->cfg.device)
    return g_err.fail(ORBX_EINVAL, "orbx_set_rectify: the rectifier is on device %d, the extractor on %d", r->device,
                h->cfg.device);
  std::lock_guard<std::mutex> lk(h->mu);
  if (h->rect == r) return ORBX_OK;
  // the single-frame graph was captured with the old setting (the calls that
  // replay it have all returned); the next call runs plain, the one after captures
  if (h->ws.ev) (void)hipEventSynchronize(h->ws.ev);
  drop_graph(h);
  h->warm_w = h->warm_h = 0;
  h->rect = r;
  return ORBX_OK;
}

int orbx_get_scales(orbx_handle h, float* s, float* is, float* s2, float* is2) {
  if (!h) return g_err.fail(ORBX_EINVAL, "null handle");
  const int L = h->cfg.nlevels;
  for (int l = 0; l < L; ++l) {
    if (s) s[l] = h->tab.scale[l];
    if (is) is[l] = h->tab.inv_scale[l];
    if (s2) s2[l] = h->tab.sigma2[l];
    if (is2) is2[l] = h->tab.inv_sigma2[l];
  }
  return ORBX_OK;
}

int orbx_get_levels_info(orbx_handle h, int* nlevels, int* lw, int* lh, int* nf) {
  if (!h) return g_err.fail(ORBX_EINVAL, "null handle");
  const ExtractParams& P = h->plan.P;
  const int L = h->cfg.nlevels;  // also before a deferred plan (sizes 0 until the first image)
  if (nlevels) *nlevels = L;
  for (int l = 0; l < L; ++l) {
    if (lw) lw[l] = P.L ? P.lv[l].w : 0;
    if (lh) lh[l] = P.L ? P.lv[l].h : 0;
    if (nf) nf[l] = h->tab.nfeat[l];
  }
  return ORBX_OK;
}

// Synchronous reads of a handle's buffers wait for the handle's own last
// launch (its workspace event, recorded on whatever stream that launch used),
// never for the whole device: another handle's work (the other extractor of a
// stereo pair, on another thread) goes on. The copies run on the handle's stream.
static int handle_quiesce(orbx_extractor* h) {
  HIP_OK(g_err, hipSetDevice(h->cfg.device));
  if (h->ws.used) HIP_OK(g_err, hipEventSynchronize(h->ws.ev));
  if (!h->stream) HIP_OK(g_err, hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  return ORBX_OK;
}
static int handle_d2h(orbx_extractor* h, void* dst, const void* src, size_t bytes) {
  HIP_OK(g_err, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
  HIP_OK(g_err, hipStreamSynchronize(h->stream));
  return ORBX_OK;
}

int orbx_set_host_pyramid(orbx_handle h, int enable) {
  if (!h) return g_err.fail(ORBX_EINVAL, "null handle");
  std::lock_guard<std::mutex> lk(h->mu);
  h->host_pyr = enable != 0;
  h->host_pyr_valid = false;
  return ORBX_OK;
}

int orbx_get_host_pyramid(orbx_handle h, const uint8_t** levels, size_t* pitches, int cap_levels) {
  if (!h || !levels || !pitches) return g_err.fail(ORBX_EINVAL, "null argument");
  const ExtractParams& P = h->plan.P;
  if (cap_levels < P.L) return g_err.fail(ORBX_ECAPACITY, "%d levels do not fit %d entries", P.L, cap_levels);
  if (!h->host_pyr_valid)
    return g_err.fail(ORBX_EINVAL, "no host pyramid: enable it (orbx_set_host_pyramid) before an orbx_extract call");
  const size_t pitch0 = frame_pitch(P.lv[0].w);  // orbx_extract's staging pitch
  levels[0] = (const uint8_t*)h->h_in.p;
  pitches[0] = pitch0;
  for (int l = 1; l < P.L; ++l) {
    levels[l] = (const uint8_t*)h->h_pyr.p + h->h_pyr_off[l];
    pitches[l] = (size_t)P.lv[l].pitch;
  }
  return ORBX_OK;
}

int orbx_get_level(orbx_handle h, int frame, int level, int blurred, uint8_t* out, size_t out_stride) {
  if (!h || !out) return g_err.fail(ORBX_EINVAL, "null argument");
  const Plan& pl = h->plan;
  if (level < 0 || level >= pl.P.L || frame < 0 || frame >= h->last_batch)
    return g_err.fail(ORBX_EINVAL, "no such frame/level");
  const LevelGeom& g = pl.P.lv[level];
  if (h->host_pyr_valid && !blurred && frame == 0) {
    // the pinned copy orbx_extract already made
    const uint8_t* lv[kMaxLevels];
    size_t lp[kMaxLevels];
    if (int rc = orbx_get_host_pyramid(h, lv, lp, kMaxLevels)) return rc;
    for (int y = 0; y < g.h; ++y) memcpy(out + (size_t)y * out_stride, lv[level] + (size_t)y * lp[level], g.w);
    return ORBX_OK;
  }
  if (int rc = handle_quiesce(h)) return rc;
  const ExtractBuffers X = buffers_of(pl);
  const uint8_t* src;
  size_t spitch;
  if (blurred) {
    src = X.blur + g.off + (long long)frame * g.plane;
    spitch = g.pitch;
  } else if (level == 0) {
    src = h->last_frames + (long long)frame * h->last_fpitch;
    spitch = h->last_rstride;
  } else {
    src = X.pyr + g.off + (long long)frame * g.plane;
    spitch = g.pitch;
  }
  HIP_OK(g_err, hipMemcpy2DAsync(out, out_stride, src, spitch, g.w, g.h, hipMemcpyDeviceToHost, h->stream));
  HIP_OK(g_err, hipStreamSynchronize(h->stream));
  return ORBX_OK;
}

int orbx_get_fast_candidates(orbx_handle h, int frame, int level, orbx_kp* out, int cap, int* n) {
  if (!h || !n) return g_err.fail(ORBX_EINVAL, "null argument");
  const Plan& pl = h->plan;
  if (level < 0 || level >= pl.P.L || frame < 0 || frame >= h->last_batch)
    return g_err.fail(ORBX_EINVAL, "no such frame/level");
  if (int rc = handle_quiesce(h)) return rc;
  const LevelGeom& g = pl.P.lv[level];
  std::vector<int> cnt(g.ncells);
  std::vector<uint32_t> slots(std::max(g.nslots, 1));
  if (int rc = handle_d2h(h, cnt.data(), pl.cell_counts.as<int>() + (size_t)frame * pl.P.ncells_total + g.cell0,
                          g.ncells * 4))
    return rc;
  if (int rc = handle_d2h(h, slots.data(), pl.slots.as<uint32_t>() + (size_t)frame * pl.P.slots_per_frame + g.slot0,
                          (size_t)g.nslots * 4))
    return rc;
  int k = 0;
  for (int c = 0; c < g.ncells; ++c) {
    const CellGeom& cg = pl.cells[g.cell0 + c];
    for (int i = 0; i < cnt[c]; ++i, ++k) {
      if (k >= cap || !out) continue;
      const uint32_t key = slots[cg.slot_off - g.slot0 + i];
      orbx_kp kp{(float)key_x(key), (float)key_y(key), 7.f, -1.f, (float)key_score(key), 0, -1};
      out[k] = kp;
    }
  }
  *n = k;
  return k > cap ? g_err.fail(ORBX_ECAPACITY, "cap too small") : ORBX_OK;
}

int orbx_get_status(orbx_handle h, int reset, int* status) {
  if (!h || !status) return g_err.fail(ORBX_EINVAL, "null argument");
  if (int rc = handle_quiesce(h)) return rc;
  int e = 0;
  if (int rc = handle_d2h(h, &e, h->plan.err.p, 4)) return rc;
  // cleared on the handle's stream, ordered after the batches that set it
  if (reset && e) {
    HIP_OK(g_err, hipMemsetAsync(h->plan.err.p, 0, 16, h->stream));
    if (h->ws.after(h->stream)) return g_err.fail(ORBX_EDEVICE, "event record failed");
    HIP_OK(g_err, hipStreamSynchronize(h->stream));
  }
  *status = e;
  return ORBX_OK;
}


// the quadtree's four statistics per (frame, level) of frames [frame0, frame0 + nframes) of the last extraction
static int read_qties(orbx_extractor* h, int frame0, int nframes, const void* out, std::vector<int>& t) {
  if (!h || !out) return g_err.fail(ORBX_EINVAL, "null argument");
  const Plan& pl = h->plan;
  if (frame0 < 0 || nframes < 1 || frame0 + nframes > h->last_batch)
    return g_err.fail(ORBX_EINVAL, "frames [%d, %d) not in the last extraction (%d frames)", frame0, frame0 + nframes,
                      h->last_batch);
  if (int rc = handle_quiesce(h)) return rc;
  const int L = pl.P.L;
  t.resize((size_t)nframes * L * 4);
  return handle_d2h(h, t.data(), pl.qties.as<int>() + (size_t)frame0 * L * 4, t.size() * 4);
}

int orbx_get_quadtree_paths(orbx_handle h, int frame0, int nframes, int* out) {
  std::vector<int> t;
  if (int rc = read_qties(h, frame0, nframes, out, t)) return rc;
  for (size_t i = 0; i < t.size() / 4; ++i) out[i] = t[i * 4 + 3];
  return ORBX_OK;
}

int orbx_get_tie_stats(orbx_handle h, int frame0, int nframes, int* out) {
  std::vector<int> t;
  if (int rc = read_qties(h, frame0, nframes, out, t)) return rc;
  for (size_t i = 0; i < t.size() / 4; ++i)
    for (int k = 0; k < 3; ++k) out[i * 3 + k] = t[i * 4 + k];
  return ORBX_OK;
}

int orbx_get_stage_order(orbx_handle h, char* out) {
  if (!out) return g_err.fail(ORBX_EINVAL, "null argument");
  memcpy(out, h ? h->order : extract_stage_order(), 6);
  return ORBX_OK;
}

int orbx_set_stage_order(orbx_handle h, const char* order) {
  if (!h) return g_err.fail(ORBX_EINVAL, "null handle");
  if (!valid_stage_order(order))
    return g_err.fail(ORBX_EINVAL, "stage order must be 5 letters of p b f q o: p first, o last, f before q");
  std::lock_guard<std::mutex> lk(h->mu);
  if (memcmp(h->order, order, 5) == 0) return ORBX_OK;
  // the single-frame graph was captured with the old order (after the launches using it)
  if (h->ws.ev) (void)hipEventSynchronize(h->ws.ev);
  drop_graph(h);
  memcpy(h->order, order, 6);
  return ORBX_OK;
}

int orbx_get_stage_times(orbx_handle h, float* ms, const char** names, int cap, int* n) {
  auto name_of = [](char c) -> const char* {
    switch (c) {
      case 'p': return "Pyramid/Resize";
      case 'b': return "Gaussian Blur";
      case 'f': return "FAST+Grid";
      case 'q': return "Make quadtree";
      default: return "Compute angle+ORB descriptor+scale";
    }
  };
  if (!h || !n) return g_err.fail(ORBX_EINVAL, "null argument");
  *n = 0;
  if (!h->timing) return ORBX_OK;
  HIP_OK(g_err, hipEventSynchronize(h->ev[5]));
  for (int i = 0; i < 5 && i < cap; ++i) {
    float t = 0;
    HIP_OK(g_err, hipEventElapsedTime(&t, h->ev[i], h->ev[i + 1]));
    if (ms) ms[i] = t;
    if (names) names[i] = name_of(h->order[i]);
    *n = i + 1;
  }
  return ORBX_OK;
}

int orbx_set_stage_events(orbx_handle h, void** events) {
  if (!h || !events) return g_err.fail(ORBX_EINVAL, "null argument");
  for (int i = 0; i < ORBX_STAGE_EVENTS; ++i) h->user_ev[i] = events[i];
  h->has_user_ev = true;
  return ORBX_OK;
}

}  // extern "C"

// A process-wide helper thread for orbm_stereo_frame: it copies the right
// image into its handle's pinned staging while the calling thread stages and
// issues the left one, so the two copies take two host cores as the
// reference's two extraction threads do, without spawning threads per frame.
// One job at a time: a caller that finds it busy copies inline. The worker
// makes no HIP call. ORBX_STAGE_THREAD=0: both copies on the calling thread.
namespace {
class StageHelper {
 public:
  static StageHelper& get() {
    static StageHelper s;
    return s;
  }
  bool try_post(orbx_extractor* h, const uint8_t* img, int w, int hh, size_t stride) {
    if (busy_.test_and_set(std::memory_order_acquire)) return false;
    {
      std::lock_guard<std::mutex> lk(mu_);
      if (!th_.joinable()) th_ = std::thread([this] { loop(); });
      h_ = h;
      img_ = img;
      w_ = w;
      hh_ = hh;
      stride_ = stride;
      state_.store(1, std::memory_order_relaxed);
    }
    cv_.notify_one();
    return true;
  }
  void wait() {  // the posted copy is done (spin briefly, then yield)
    for (int i = 0; state_.load(std::memory_order_acquire) != 2; ++i) {
      if (i < 2000) __builtin_ia32_pause();
      else std::this_thread::yield();
    }
    state_.store(0, std::memory_order_relaxed);
    busy_.clear(std::memory_order_release);
  }
  ~StageHelper() {
    {
      std::lock_guard<std::mutex> lk(mu_);
      quit_ = true;
    }
    cv_.notify_one();
    if (th_.joinable()) th_.join();
  }

 private:
  void loop() {
    std::unique_lock<std::mutex> lk(mu_);
    for (;;) {
      cv_.wait(lk, [this] { return quit_ || state_.load(std::memory_order_relaxed) == 1; });
      if (quit_) return;
      lk.unlock();
      extract_stage(h_, img_, w_, hh_, stride_);
      state_.store(2, std::memory_order_release);
      lk.lock();
    }
  }
  std::thread th_;
  std::mutex mu_;
  std::condition_variable cv_;
  std::atomic_flag busy_ = ATOMIC_FLAG_INIT;
  std::atomic<int> state_{0};  // 0 idle, 1 posted, 2 done
  bool quit_ = false;
  orbx_extractor* h_ = nullptr;
  const uint8_t* img_ = nullptr;
  int w_ = 0, hh_ = 0;
  size_t stride_ = 0;
};
}  // namespace

int orbx::extract_pair(orbx_handle L, orbx_handle R, const uint8_t* imL, size_t strideL, const uint8_t* imR,
                       size_t strideR, int w, int hh, const std::function<int(hipStream_t)>& between,
                       orbx_kp* kpsL, int capL, uint8_t* descL, int* nL, orbx_kp* kpsR, int capR, uint8_t* descR,
                       int* nR, double* stamps) {
  auto stamp = [stamps](int i) {
    if (stamps) stamps[i] = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
  };
  if (!L || !R || !nL || !nR) return g_err.fail(ORBX_EINVAL, "null argument");
  if (L == R) return g_err.fail(ORBX_EINVAL, "left and right need two extractor handles");
  if (w <= 0 || hh <= 0) return g_err.fail(ORBX_EINVAL, "empty image");
  if (L->cfg.device != R->cfg.device) return g_err.fail(ORBX_EINVAL, "left and right extractors on different devices");
  std::unique_lock<std::mutex> lkL(L->mu, std::defer_lock), lkR(R->mu, std::defer_lock);
  std::lock(lkL, lkR);
  *nL = *nR = 0;
  // left first: its chain runs while the right image is staged
  int rc;
  if ((rc = extract_prepare(L, imL, w, hh, strideL)) || (rc = extract_prepare(R, imR, w, hh, strideR))) return rc;
  static const bool use_helper = !(getenv("ORBX_STAGE_THREAD") && getenv("ORBX_STAGE_THREAD")[0] == '0');
  const bool posted = use_helper && StageHelper::get().try_post(R, imR, w, hh, strideR);
  extract_stage(L, imL, w, hh, strideL);
  stamp(0);
  if ((rc = extract_issue(L, w, hh, true))) {
    if (posted) StageHelper::get().wait();
    return rc;
  }
  stamp(1);
  if (posted) StageHelper::get().wait();
  else extract_stage(R, imR, w, hh, strideR);
  stamp(2);
  if ((rc = extract_issue(R, w, hh, false))) return rc;
  stamp(3);
  const int rb = between(R->stream);
  stamp(4);
  // both streams: `between` may have failed before it ordered anything after the right chain
  HIP_OK(g_err, hipStreamSynchronize(L->stream));
  HIP_OK(g_err, hipStreamSynchronize(R->stream));
  stamp(5);
  if ((rc = extract_finish(L, kpsL, capL, descL, nL)) || (rc = extract_finish(R, kpsR, capR, descR, nR))) return rc;
  stamp(6);
  return rb;
}
