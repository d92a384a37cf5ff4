// orbx_frustum.hip — the device half of Tracking::SearchLocalPoints
// (src/Tracking.cc:1229-1279) that runs before ORBmatcher::SearchByProjection(F,
// vpMapPoints, th): Frame::isInFrustum (src/Frame.cc:268-324) on every local
// map point, and the hand-over of the points in view to search_proj_kernel
// (orbx_project.hip).
//
//   frustum_kernel          frames x chunks of points, one point per lane: the
//                           48-byte orbm_map_point_world record in, the 24-byte
//                           orbm_map_point_proj record out (frustum_point,
//                           orbx_posemath.cuh), the in-view count per frame.
//   compact_in_view_kernel  one workgroup per frame: the records in view, their
//                           descriptors and their original indices, in order.
//                           search_proj_kernel resolves the reference's
//                           sequential blocking by point index and reports the
//                           last writer; a stable compaction maps indices
//                           monotonically, so the search over the compacted
//                           list is the search over the full list with the
//                           indices mapped back. The limit of 8192 points the
//                           search keeps in registers then applies to the
//                           points in view, not to the local map's size.
//   remap_out_kernel        out[i] >= 0 through the index map.
#include "orbx_posemath.cuh"
#include "orbx_wave.cuh"

namespace orbx {

constexpr int kFrustumThreads = 256;
constexpr int kCompactThreads = 1024;

static_assert(sizeof(orbm_map_point_world) == 48 && sizeof(orbm_map_point_proj) == 24, "record layouts");

__global__ __launch_bounds__(kFrustumThreads) void frustum_kernel(FrustumParams P,
                                                                  const orbm_pose* __restrict__ poses,
                                                                  const orbm_map_point_world* __restrict__ mps,
                                                                  const int* __restrict__ d_nmp,
                                                                  orbm_map_point_proj* __restrict__ out,
                                                                  int* __restrict__ n_in_view) {
  const int f = blockIdx.y, lane = threadIdx.x & 63;
  const int nmp = min(d_nmp[f], P.mp_pitch);
  if ((int)(blockIdx.x * kFrustumThreads) >= nmp) return;  // the whole workgroup
  const int j = blockIdx.x * kFrustumThreads + threadIdx.x;
  int in = 0;
  if (j < nmp) {
    const size_t at = (size_t)f * P.mp_pitch + j;
    union {
      uint4 q[3];
      orbm_map_point_world r;
    } a;
    const uint4* src = (const uint4*)(mps + at);  // 48-byte records from a 16-byte aligned base
    a.q[0] = src[0];
    a.q[1] = src[1];
    a.q[2] = src[2];
    union {
      uint2 q[3];
      orbm_map_point_proj r;
    } o;
    in = frustum_point(P, poses[f], a.r, &o.r) ? 1 : 0;
    uint2* dst = (uint2*)(out + at);  // 24-byte records: 8-byte aligned
    dst[0] = o.q[0];
    dst[1] = o.q[1];
    dst[2] = o.q[2];
  }
  in = wave_sum_dpp(in);  // every lane of the wave is here
  if (lane == 0 && in) atomicAdd(&n_in_view[f], in);
}

__global__ __launch_bounds__(kCompactThreads) void compact_in_view_kernel(
    const orbm_map_point_proj* __restrict__ proj, const uint8_t* __restrict__ mpdesc, const int* __restrict__ d_nmp,
    int mp_pitch, orbm_map_point_proj* __restrict__ c_proj, uint8_t* __restrict__ c_desc, int* __restrict__ c_map,
    int* __restrict__ c_nmp, int c_pitch, int* __restrict__ err) {
  constexpr int kWaves = kCompactThreads / 64;
  __shared__ int s_w[kWaves];
  const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int nmp = min(d_nmp[f], mp_pitch);
  const uint2* MP = (const uint2*)(proj + (size_t)f * mp_pitch);
  const uint4* MD = (const uint4*)(mpdesc + (size_t)f * mp_pitch * 32);
  uint2* CP = (uint2*)(c_proj + (size_t)f * c_pitch);
  uint4* CD = (uint4*)(c_desc + (size_t)f * c_pitch * 32);
  int* CM = c_map + (size_t)f * c_pitch;
  int run = 0;  // points in view before this chunk
  for (int base = 0; base < nmp; base += kCompactThreads) {
    const int j = base + tid;
    uint2 r0{}, r1{}, r2{};
    bool in = false;
    if (j < nmp) {
      r0 = MP[3 * j];
      r1 = MP[3 * j + 1];
      r2 = MP[3 * j + 2];
      in = (r2.y & 0xffu) != 0;  // track_in_view
    }
    const uint64_t b = __ballot(in);
    if (lane == 0) s_w[w] = __popcll(b);
    __syncthreads();
    int off = run, tot = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
      const int c = s_w[k];
      off += k < w ? c : 0;
      tot += c;
    }
    const int pos = off + mbcnt64(b);
    if (in && pos < c_pitch) {
      CP[3 * pos] = r0;
      CP[3 * pos + 1] = r1;
      CP[3 * pos + 2] = r2;
      CD[2 * pos] = MD[2 * j];
      CD[2 * pos + 1] = MD[2 * j + 1];
      CM[pos] = j;
    }
    run += tot;
    __syncthreads();
  }
  if (tid == 0) {
    c_nmp[f] = min(run, c_pitch);
    if (run > c_pitch && err) atomicOr(err, kStatusViewOverflow);
  }
}

__global__ __launch_bounds__(256) void remap_out_kernel(int* __restrict__ out, const int* __restrict__ d_n,
                                                        int kp_pitch, const int* __restrict__ c_map, int c_pitch) {
  const int f = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= min(d_n[f], kp_pitch)) return;
  int* o = out + (size_t)f * kp_pitch + i;
  const int v = *o;
  if (v >= 0 && v < c_pitch) *o = c_map[(size_t)f * c_pitch + v];
}

int launch_frustum(const FrustumParams& P, const orbm_pose* poses, const orbm_map_point_world* mps, const int* nmp,
                   int frames, orbm_map_point_proj* out, int* n_in_view, void* stream) {
  const dim3 grid((P.mp_pitch + kFrustumThreads - 1) / kFrustumThreads, frames);
  hipLaunchKernelGGL(frustum_kernel, grid, dim3(kFrustumThreads), 0, (hipStream_t)stream, P, poses, mps, nmp, out,
                     n_in_view);
  return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_EDEVICE;
}

int launch_compact_in_view(const orbm_map_point_proj* proj, const uint8_t* mpdesc, const int* nmp, int mp_pitch,
                           int frames, orbm_map_point_proj* c_proj, uint8_t* c_desc, int* c_map, int* c_nmp,
                           int c_pitch, int* err, void* stream) {
  hipLaunchKernelGGL(compact_in_view_kernel, dim3(frames), dim3(kCompactThreads), 0, (hipStream_t)stream, proj, mpdesc,
                     nmp, mp_pitch, c_proj, c_desc, c_map, c_nmp, c_pitch, err);
  return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_EDEVICE;
}

int launch_remap_out(int* out, const int* n, int kp_pitch, const int* c_map, int c_pitch, int frames, void* stream) {
  hipLaunchKernelGGL(remap_out_kernel, dim3((kp_pitch + 255) / 256, frames), dim3(256), 0, (hipStream_t)stream, out, n,
                     kp_pitch, c_map, c_pitch);
  return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_EDEVICE;
}

}  // namespace orbx
