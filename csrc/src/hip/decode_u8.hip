// Byte image -> float image: y[i] = fmaf(float(x[i]), sc[i % C], of[i % C]) (cpu::decode_u8 is the definition).
//
// The input of every Conv1 path that does not read bytes itself (the band + GEMM Winograd form, conv2d_mfma,
// the direct oracle, K != 96, conv1_fused = 0, conv1_u8 = 0) passes through here. The source may start at any
// byte address (an image slice of a byte tensor does) and hold any number of elements: the bytes before the
// first 16-B boundary and after the last whole 16-B unit are single-byte loads, the body one 16-B load and
// four 16-B stores per thread (scalar stores where the destination is not 16-B aligned behind the head).
//
// The reference has no byte input: its programs fill float arrays (v1_serial/src/main.cpp:18-43).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "anx/ops.hpp"

namespace anx::hip {
namespace {

using u32x4 = __attribute__((ext_vector_type(4))) unsigned;
using f32x4 = __attribute__((ext_vector_type(4))) float;

// head: elements before the body; units: 16-element body units; n: all elements
template <bool ALIGNED_DST>
__global__ void __launch_bounds__(256) decode_u8_kernel(const uint8_t* __restrict__ x, float* __restrict__ y,
                                                        unsigned head, size_t units, size_t n, U8Norm nm) {
  __shared__ float so[2 * kU8MaxC];  // scale, offset: indexed by a run-time channel
  if (threadIdx.x < static_cast<unsigned>(nm.C)) {
    so[threadIdx.x] = nm.sc[threadIdx.x];
    so[kU8MaxC + threadIdx.x] = nm.of[threadIdx.x];
  }
  __syncthreads();
  const int C = nm.C;
  const size_t gid = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t k = gid; k < units; k += stride) {
    const size_t e0 = head + 16 * k;
    const u32x4 v = *reinterpret_cast<const u32x4*>(x + e0);  // 16-B aligned: head ends on a boundary
    int c = static_cast<int>(e0 % static_cast<size_t>(C));
    float f[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const unsigned b = (v[j >> 2] >> (8 * (j & 3))) & 0xffu;
      f[j] = __builtin_fmaf(static_cast<float>(b), so[c], so[kU8MaxC + c]);
      c = c + 1 == C ? 0 : c + 1;
    }
    if constexpr (ALIGNED_DST) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        *reinterpret_cast<f32x4*>(y + e0 + 4 * q) = f32x4{f[4 * q], f[4 * q + 1], f[4 * q + 2], f[4 * q + 3]};
    } else {
#pragma unroll
      for (int j = 0; j < 16; ++j) y[e0 + j] = f[j];
    }
  }
  // head and tail (at most 15 elements each): one byte per thread, the first threads of the grid
  const size_t t0 = head + 16 * units;
  if (gid < head) {
    const int c = static_cast<int>(gid % static_cast<size_t>(C));
    y[gid] = __builtin_fmaf(static_cast<float>(x[gid]), so[c], so[kU8MaxC + c]);
  }
  if (gid < n - t0) {
    const size_t e = t0 + gid;
    const int c = static_cast<int>(e % static_cast<size_t>(C));
    y[e] = __builtin_fmaf(static_cast<float>(x[e]), so[c], so[kU8MaxC + c]);
  }
}

}  // namespace

hipError_t decode_u8(const uint8_t* x, float* y, size_t n, const U8Norm& nm, hipStream_t s) {
  if (nm.C < 1 || nm.C > kU8MaxC) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  const size_t to_boundary = (16 - reinterpret_cast<uintptr_t>(x) % 16) % 16;
  const unsigned head = static_cast<unsigned>(to_boundary < n ? to_boundary : n);
  const size_t units = (n - head) / 16;
  const size_t want = (units + 255) / 256;
  const unsigned grid = static_cast<unsigned>(want < 1 ? 1 : want > 4096 ? 4096 : want);  // grid-stride above 1 M units
  if (reinterpret_cast<uintptr_t>(y + head) % 16 == 0)
    decode_u8_kernel<true><<<grid, 256, 0, s>>>(x, y, head, units, n, nm);
  else
    decode_u8_kernel<false><<<grid, 256, 0, s>>>(x, y, head, units, n, nm);
  return hipGetLastError();
}

}  // namespace anx::hip
