// The classifier head: top-k class indices and softmax probabilities of M rows of K logits
// (cpu::softmax_topk is the definition). The rows arrive as split-K slabs (+ bias), which this kernel reduces in
// splitk_reduce_kernel's order (conv_bf16.hip), or as logits (ksplit 1, no bias).
//
// One 256-thread workgroup per row, four phases with the row on chip:
//   1. one pass over the slabs: z = bias + slab 0 + slab 1 + ... (16-B loads where everything is 16-B aligned and
//      K % 4 == 0, scalar loads otherwise) into LDS, and into logits_out when the caller wants the logits;
//   2. max over the row: per-thread strided walk, wave butterfly, four wave values through LDS;
//   3. sum of exp(z - max), the same way (butterfly adds: every lane ends with the same bits);
//   4. k rounds of an (value, index) argmax, value descending then index ascending. A round takes the best element
//      that ranks strictly after the previous round's winner, so nothing is marked or rewritten; float comparison
//      makes -0.0 and +0.0 tie, and a NaN ranks with -inf, which keeps the order total: a row of any values yields
//      k distinct indices.
// Phases 2-4 read the row in one fixed pattern whatever phase 1's load width was, so a row's result depends only on
// the bits of z and on K. A row longer than kSoftmaxTopkLdsRow floats is staged in its logits_out row instead of
// LDS (written in phase 1, read back by the same workgroup behind the barrier).
//
// The reference ends at Block 2's LRN and has no classifier head.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

#include "anx/ops.hpp"
#include "softmax_head.hpp"

namespace anx::hip {
namespace {

using namespace head;  // the workgroup shape, f32x4, rank_key, ranks_before, aligned16: shared with the view head

template <bool VEC, bool STAGED>
__global__ void __launch_bounds__(kThreads) softmax_topk_kernel(const float* src, int ksplit, size_t slab_stride,
                                                                const float* bias, int K, int k, int* idx, float* prob,
                                                                float* logits_out) {
  extern __shared__ __attribute__((aligned(16))) float zs[];
  __shared__ float red_v[2][kWaves];
  __shared__ int red_i[2][kWaves];
  const unsigned t = threadIdx.x, lane = t & 63u, wave = t >> 6, Ku = static_cast<unsigned>(K);
  const size_t row = blockIdx.x;
  const float* x = src + row * Ku;
  float* lo = logits_out ? logits_out + row * Ku : nullptr;
  float* z = STAGED ? lo : zs;

  // 1. the reduced row
  if constexpr (VEC) {
    for (unsigned q = t; q < Ku / 4; q += kThreads) {
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
      if (!STAGED && lo) reinterpret_cast<f32x4*>(lo)[q] = v;
    }
  } else {
    for (unsigned c = t; c < Ku; c += kThreads) {
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
      if (!STAGED && lo) lo[c] = v;
    }
  }
  __syncthreads();

  // 2. max
  float m = -INFINITY;
  for (unsigned c = t; c < Ku; c += kThreads) m = fmaxf(m, z[c]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
  if (lane == 0) red_v[0][wave] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red_v[0][0], red_v[0][1]), fmaxf(red_v[0][2], red_v[0][3]));

  // 3. sum of exp(z - max)
  float sum = 0.f;
  for (unsigned c = t; c < Ku; c += kThreads) sum += expf(z[c] - m);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
  if (lane == 0) red_v[1][wave] = sum;
  __syncthreads();
  sum = (red_v[1][0] + red_v[1][1]) + (red_v[1][2] + red_v[1][3]);

  // 4. k rounds; (pv, pi) is the previous winner. The two red_* slots alternate, so one barrier per round is
  // enough: slot b is rewritten two rounds later, behind the barrier every reader of it has passed.
  float pv = INFINITY;
  int pi = -1;
  for (int j = 0; j < k; ++j) {
    float bv = -INFINITY;
    int bi = INT_MAX;  // "none": ranks after every real element
    for (unsigned c = t; c < Ku; c += kThreads) {
      const float v = rank_key(z[c]);
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
    if (lane == 0) red_v[b][wave] = bv, red_i[b][wave] = bi;
    __syncthreads();
    bv = red_v[b][0], bi = red_i[b][0];
#pragma unroll
    for (unsigned w = 1; w < kWaves; ++w)
      if (ranks_before(red_v[b][w], red_i[b][w], bv, bi)) bv = red_v[b][w], bi = red_i[b][w];
    pv = bv;
    pi = bi < K ? bi : K - 1;  // k <= K leaves a candidate in every round; never index past the row
    if (t == 0) {
      idx[row * static_cast<size_t>(k) + j] = pi;
      prob[row * static_cast<size_t>(k) + j] = expf(z[pi] - m) / sum;
    }
  }
}

}  // namespace

hipError_t softmax_topk(const float* src, int ksplit, size_t slab_stride, const float* bias, int M, int K, int k,
                        int* idx, float* prob, float* logits_out, hipStream_t s) {
  if (K < 1 || k < 1 || k > cpu::kMaxTopK || k > K || ksplit < 1 || M < 0) return hipErrorInvalidValue;
  if (M == 0) return hipSuccess;
  if (!src || !idx || !prob) return hipErrorInvalidValue;
  const bool staged = K > kSoftmaxTopkLdsRow;
  if (staged && !logits_out) return hipErrorInvalidValue;
  const bool vec = K % 4 == 0 && (ksplit == 1 || slab_stride % 4 == 0) && aligned16(src) && aligned16(bias) &&
                   aligned16(logits_out);
  const size_t lds = staged ? 0 : (static_cast<size_t>(K) * 4 + 15) / 16 * 16;
  const dim3 grid(static_cast<unsigned>(M));
#define ANX_HEAD(V, S) \
  softmax_topk_kernel<V, S><<<grid, kThreads, lds, s>>>(src, ksplit, slab_stride, bias, K, k, idx, prob, logits_out)
  if (vec && staged)
    ANX_HEAD(true, true);
  else if (vec)
    ANX_HEAD(true, false);
  else if (staged)
    ANX_HEAD(false, true);
  else
    ANX_HEAD(false, false);
#undef ANX_HEAD
  return hipGetLastError();
}

}  // namespace anx::hip
