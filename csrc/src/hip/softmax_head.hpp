// The phases of the classifier-head kernels (softmax_topk.hip, softmax_topk_views.hip, softmax_eval.hip), each written
// once: the three kernels are sequences of these calls plus a tail of their own, so the bits and the order they must
// agree on (evaluate's pred and rank are the other two heads' indices) come from one expression each.
//
// One 256-thread workgroup owns a row of K floats at a time, in LDS (or, for softmax_topk's long rows, in global
// memory). In the order a kernel calls them:
//   reduce_row   z = bias + slab 0 + slab 1 + ... in splitk_reduce_kernel's order (conv_bf16.hip): 16-B loads where
//                vec_loads() allows them, scalar loads otherwise, the same bits either way; optionally a copy to the
//                caller's logits.
//   row_max      per-thread strided walk, wave butterfly, four wave values through LDS.
//   row_expsum   sum of expf(z - max), the same way (butterfly adds: every lane ends with the same bits).
//   add_view     acc[c] (+)= expf(z[c] - max) / sum on the thread's own strided elements: thread t owns elements
//   mean_views   t, t + 256, ... of every view, so the running sum needs no atomics and adds in view order; then the
//                division by float(V).
//   next_best    one round of the (value, index) argmax, value descending then index ascending: the best element that
//                ranks strictly after the previous round's winner, so nothing is marked or rewritten. Float comparison
//                makes -0.0 and +0.0 tie, and a NaN ranks with -inf, which keeps the order total: a row of any values
//                yields k distinct indices.
// Everything after reduce_row reads the row in one fixed pattern whatever reduce_row's load width was, so a result
// depends only on the bits of z, on K and on V.
//
// The functions take plain float* and are force-inlined: the compiler then sees which rows are LDS and which are
// global, and no access goes through a generic address.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace anx::hip::head {

using f32x4 = __attribute__((ext_vector_type(4))) float;
constexpr unsigned kThreads = 256, kWaves = kThreads / 64;

// ---- the dynamic LDS of a head kernel: `rows` rows of K floats, then 2 x kWaves (value, index) reduction slots ----

// floats of one LDS row: K rounded up to a 16-B unit, so the second row and the slots stay aligned
constexpr unsigned row_floats(unsigned K) { return (K + 3u) & ~3u; }

// bytes of the region: at the limits (one row of 15360 floats, two of 7680) 61440 + 64
inline size_t lds_bytes(unsigned rows, int K) {
  return (rows * static_cast<size_t>(row_floats(static_cast<unsigned>(K))) + 4 * kWaves) * sizeof(float);
}

struct Slots {
  float (*v)[kWaves];  // [2][kWaves]
  int (*i)[kWaves];    // [2][kWaves]
};
struct Lds {
  float* z;    // the row at hand
  float* acc;  // the running sum of the views' probabilities (rows == 2); z otherwise
  Slots red;
};

// `lds` is the kernel's whole `extern __shared__` region (16-B aligned), rows 0 (the row lives elsewhere), 1 or 2
__device__ __forceinline__ Lds carve(float* lds, unsigned Ku, unsigned rows) {
  float* slots = lds + rows * row_floats(Ku);
  return {lds, rows == 2 ? lds + row_floats(Ku) : lds,
          {reinterpret_cast<float(*)[kWaves]>(slots), reinterpret_cast<int(*)[kWaves]>(slots + 2 * kWaves)}};
}

// ---- the load width (host) ----

inline bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// 16-B loads and stores in reduce_row: every row starts at a multiple of K floats from its base, so K % 4 == 0 keeps
// the rows as aligned as the bases are
inline bool vec_loads(const float* src, int ksplit, size_t slab_stride, const float* bias, int K,
                      const float* logits_out) {
  return K % 4 == 0 && (ksplit == 1 || slab_stride % 4 == 0) && aligned16(src) && aligned16(bias) &&
         aligned16(logits_out);
}

// ---- the ranking rule ----

// a NaN ranks with -inf, which keeps the order total: a row of any values yields k distinct indices
__device__ inline float rank_key(float v) { return v != v ? -INFINITY : v; }
// (va, ia) ranks before (vb, ib): value descending, then index ascending; float comparison, so -0.0 and +0.0 tie
__device__ inline bool ranks_before(float va, int ia, float vb, int ib) { return va > vb || (va == vb && ia < ib); }

// ---- the phases ----

// z = bias + slab 0 + slab 1 + ... of the row x (slab s at x + s * slab_stride), also into lo unless null; ends
// with the barrier that makes z readable by the whole workgroup
template <bool VEC>
__device__ __forceinline__ void reduce_row(const float* x, int ksplit, size_t slab_stride, const float* bias,
                                           unsigned Ku, float* z, float* lo) {
  if constexpr (VEC) {
    for (unsigned q = threadIdx.x; q < Ku / 4; q += kThreads) {
      f32x4 v;
      int s = 0;
      if (bias) {
        v = reinterpret_cast<const f32x4*>(bias)[q];
      } else {
        v = reinterpret_cast<const f32x4*>(x)[q];
        s = 1;
      }
      for (; s < ksplit; ++s) v += *reinterpret_cast<const f32x4*>(x + s * slab_stride + 4 * static_cast<size_t>(q));
      reinterpret_cast<f32x4*>(z)[q] = v;
      if (lo) reinterpret_cast<f32x4*>(lo)[q] = v;
    }
  } else {
    for (unsigned c = threadIdx.x; c < Ku; c += kThreads) {
      float v;
      int s = 0;
      if (bias) {
        v = bias[c];
      } else {
        v = x[c];
        s = 1;
      }
      for (; s < ksplit; ++s) v += x[s * slab_stride + c];
      z[c] = v;
      if (lo) lo[c] = v;
    }
  }
  __syncthreads();
}

// the maximum of the row, the same value in every thread; `slot` is kWaves floats of LDS
__device__ __forceinline__ float row_max(const float* z, unsigned Ku, float* slot) {
  float m = -INFINITY;
  for (unsigned c = threadIdx.x; c < Ku; c += kThreads) m = fmaxf(m, z[c]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
  if ((threadIdx.x & 63u) == 0) slot[threadIdx.x >> 6] = m;
  __syncthreads();
  return fmaxf(fmaxf(slot[0], slot[1]), fmaxf(slot[2], slot[3]));
}

// the sum of expf(z - m) over the row, the same bits in every thread; `slot` is kWaves floats of LDS other than
// row_max's, whose readers may not have passed a barrier yet
__device__ __forceinline__ float row_expsum(const float* z, unsigned Ku, float m, float* slot) {
  float sum = 0.f;
  for (unsigned c = threadIdx.x; c < Ku; c += kThreads) sum += expf(z[c] - m);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
  if ((threadIdx.x & 63u) == 0) slot[threadIdx.x >> 6] = sum;
  __syncthreads();
  return (slot[0] + slot[1]) + (slot[2] + slot[3]);
}

// a view's probabilities onto the thread's own elements of the running sum (`first`: the view that starts it); ends
// with the barrier behind which z and both slots are free for the next view
__device__ __forceinline__ void add_view(const float* z, float* acc, unsigned Ku, float m, float sum, bool first) {
  for (unsigned c = threadIdx.x; c < Ku; c += kThreads) {
    const float p = expf(z[c] - m) / sum;
    acc[c] = first ? p : acc[c] + p;
  }
  __syncthreads();
}

// the mean of V views, still on the thread's own elements, also into out unless null; ends with the barrier that
// makes acc readable by the whole workgroup
__device__ __forceinline__ void mean_views(float* acc, unsigned Ku, int V, float* out) {
  const float fv = static_cast<float>(V);
  for (unsigned c = threadIdx.x; c < Ku; c += kThreads) {
    const float p = acc[c] / fv;
    acc[c] = p;
    if (out) out[c] = p;
  }
  __syncthreads();
}

// Round j of the argmax on the score row r: (pv, pi) is the previous round's winner on entry ((+inf, -1) before
// round 0, which every element ranks after) and this round's on return, the same in every thread. The two slot
// pairs alternate with j, so the one barrier in here is enough: pair j & 1 is rewritten two rounds later, behind
// the barrier every reader of it has passed.
__device__ __forceinline__ void next_best(const float* r, int K, float& pv, int& pi, int j, Slots red) {
  const unsigned t = threadIdx.x, Ku = static_cast<unsigned>(K);
  float bv = -INFINITY;
  int bi = INT_MAX;  // "none": ranks after every real element
  for (unsigned c = t; c < Ku; c += kThreads) {
    const float v = rank_key(r[c]);
    const int ci = static_cast<int>(c);
    if ((v < pv || (v == pv && ci > pi)) && ranks_before(v, ci, bv, bi)) bv = v, bi = ci;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(bv, off, 64);
    const int oi = __shfl_xor(bi, off, 64);
    if (ranks_before(ov, oi, bv, bi)) bv = ov, bi = oi;
  }
  const int b = j & 1;
  if ((t & 63u) == 0) red.v[b][t >> 6] = bv, red.i[b][t >> 6] = bi;
  __syncthreads();
  bv = red.v[b][0], bi = red.i[b][0];
#pragma unroll
  for (unsigned w = 1; w < kWaves; ++w)
    if (ranks_before(red.v[b][w], red.i[b][w], bv, bi)) bv = red.v[b][w], bi = red.i[b][w];
  pv = bv;
  pi = bi < K ? bi : K - 1;  // rounds <= K leave a candidate in every round; never index past the row
}

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

}  // namespace anx::hip::head
