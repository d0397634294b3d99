// What the two classifier-head kernels (softmax_topk.hip, softmax_topk_views.hip) must agree on to give the same
// bits and the same order: the workgroup shape, the vector type of the row loads, the ranking rule and the alignment
// test that picks the load width. One copy, so the rule cannot drift between them.
// The evaluation head (softmax_eval.hip) is the third kernel on it: its pred and rank are these two kernels' order.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace anx::hip::head {

using f32x4 = __attribute__((ext_vector_type(4))) float;
constexpr unsigned kThreads = 256, kWaves = kThreads / 64;

// a NaN ranks with -inf, which keeps the order total: a row of any values yields k distinct indices
__device__ inline float rank_key(float v) { return v != v ? -INFINITY : v; }
// (va, ia) ranks before (vb, ib): value descending, then index ascending; float comparison, so -0.0 and +0.0 tie
__device__ inline bool ranks_before(float va, int ia, float vb, int ib) { return va > vb || (va == vb && ia < ib); }

// The sum of one int per thread over the workgroup, the same value in every thread: wave butterfly, then the four
// wave values through `slots` (kWaves ints of LDS nobody else reads or writes until the caller's next barrier).
// Integer adds, so the order cannot show.
__device__ inline int workgroup_sum(int v, int* slots) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63u) == 0) slots[threadIdx.x >> 6] = v;
  __syncthreads();
  return (slots[0] + slots[1]) + (slots[2] + slots[3]);
}

inline bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace anx::hip::head
