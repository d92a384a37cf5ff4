// Where does `buffer_load_dword ... lds` put a wave's dwords? One wave, three
// loads into a sentinel-filled LDS array, the array copied out and described:
//   A: all 64 lanes, lane j reading source dword 63 - j (so the slot shows the
//      lane and not the address), LDS base 256;
//   B: lanes 0..54 only (the others masked off by EXEC), LDS base 1024;
//   C: all lanes through a descriptor of 40 bytes, so lanes 10.. are out of
//      range, LDS base 2048.
// Expected by the ISA text (measured for FAST's ROI staging, DESIGN "FAST: 16-byte
// score-map clear, one-maximum NMS", which in the end kept its register staging):
// lane j's dword at base + 4 j; masked-off lanes write nothing; out-of-range
// lanes write 0.
//   hipcc --offload-arch=gfx950 -O2 tools/lds_dword_probe.hip -o lds_dword_probe && ./lds_dword_probe
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <vector>

#define LDSP __attribute__((address_space(3)))
constexpr int kWords = 1024;
constexpr uint32_t kSentinel = 0xDEADBEEFu;

__global__ __launch_bounds__(64) void probe(const uint32_t* src, uint32_t* out) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kWords];
  const int lane = threadIdx.x;
  for (int i = lane; i < kWords; i += 64) lds[i] = kSentinel;
  __syncthreads();
  LDSP unsigned char* base = (LDSP unsigned char*)lds;
  typedef LDSP void lds_void;
  const __amdgpu_buffer_rsrc_t all = __builtin_amdgcn_make_buffer_rsrc((void*)src, (short)0, 64 * 4, 0x00020000);
  const __amdgpu_buffer_rsrc_t tenw = __builtin_amdgcn_make_buffer_rsrc((void*)src, (short)0, 10 * 4, 0x00020000);
  __builtin_amdgcn_raw_ptr_buffer_load_lds(all, (lds_void*)(base + 256), 4, 4 * (63 - lane), 0, 0, 0);
  if (lane < 55) __builtin_amdgcn_raw_ptr_buffer_load_lds(all, (lds_void*)(base + 1024), 4, 4 * lane, 0, 0, 0);
  __builtin_amdgcn_raw_ptr_buffer_load_lds(tenw, (lds_void*)(base + 2048), 4, 4 * lane, 0, 0, 0);
  __builtin_amdgcn_s_waitcnt(0);  // vmcnt(0): the loads' LDS writes have landed
  __syncthreads();
  for (int i = lane; i < kWords; i += 64) out[i] = lds[i];
}

#define CK(x)                                                              \
  do {                                                                     \
    hipError_t e_ = (x);                                                   \
    if (e_ != hipSuccess) {                                                \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));              \
      return 2;                                                            \
    }                                                                      \
  } while (0)

int main() {
  std::vector<uint32_t> h(64), o(kWords);
  for (int i = 0; i < 64; ++i) h[i] = 0x1000u + i;
  uint32_t *src = nullptr, *out = nullptr;
  CK(hipMalloc(&src, 64 * 4));
  CK(hipMalloc(&out, kWords * 4));
  CK(hipMemcpy(src, h.data(), 64 * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, src, out);
  CK(hipDeviceSynchronize());
  CK(hipMemcpy(o.data(), out, kWords * 4, hipMemcpyDeviceToHost));
  int bad = 0, written = 0;
  for (int i = 0; i < kWords; ++i) {
    uint32_t want = kSentinel;
    if (i >= 64 && i < 128) want = 0x1000u + (63 - (i - 64));           // A: slot = lane
    if (i >= 256 && i < 256 + 55) want = 0x1000u + (i - 256);           // B: lanes 0..54, nothing from 55..63
    if (i >= 512 && i < 576) want = i - 512 < 10 ? 0x1000u + (i - 512) : 0u;  // C: zeros out of range
    written += o[i] != kSentinel;
    if (o[i] != want) {
      if (bad++ < 16) printf("dword %d: 0x%08x, expected 0x%08x\n", i, o[i], want);
    }
  }
  printf("A (64 lanes, base 256): dwords 64..127 %s lane j -> base + 4 j\n", bad ? "NOT" : "are");
  printf("B (lanes 0..54, base 1024): dwords 256..310 written, 311..319 = 0x%08x .. 0x%08x (sentinel: masked lanes write nothing)\n",
         o[311], o[319]);
  printf("C (40-byte descriptor, base 2048): dword 521 = 0x%08x, dword 522 = 0x%08x .. dword 575 = 0x%08x (out of range: 0 written)\n",
         o[521], o[522], o[575]);
  printf("%d dwords written in all (expected 64 + 55 + 64 = 183), %d mismatches\n", written, bad);
  CK(hipFree(src));
  CK(hipFree(out));
  return bad ? 1 : 0;
}
