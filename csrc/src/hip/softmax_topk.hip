// The classifier head: top-k class indices and softmax probabilities of M rows of K logits
// (cpu::softmax_topk is the definition). The rows arrive as split-K slabs (+ bias) or as logits (ksplit 1, no bias).
//
// One workgroup per row, the phases of softmax_head.hpp: reduce, max, sum, then k rounds; thread 0 writes each
// round's index and expf(z - max) / sum there. A row longer than kSoftmaxTopkLdsRow floats is staged in its
// logits_out row instead of LDS (written by reduce_row, read back by the same workgroup behind its barrier).
//
// The reference ends at Block 2's LRN and has no classifier head.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "anx/ops.hpp"
#include "softmax_head.hpp"

namespace anx::hip {
namespace {

using namespace head;

template <bool VEC, bool STAGED>
__global__ void __launch_bounds__(kThreads) softmax_topk_kernel(const float* src, int ksplit, size_t slab_stride,
                                                                const float* bias, int K, int k, int* idx, float* prob,
                                                                float* logits_out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const unsigned Ku = static_cast<unsigned>(K);
  const Lds l = carve(lds, Ku, STAGED ? 0 : 1);
  const size_t row = blockIdx.x;
  float* lo = logits_out ? logits_out + row * Ku : nullptr;
  float* z = STAGED ? lo : l.z;

  reduce_row<VEC>(src + row * Ku, ksplit, slab_stride, bias, Ku, z, STAGED ? nullptr : lo);
  const float m = row_max(z, Ku, l.red.v[0]);
  const float sum = row_expsum(z, Ku, m, l.red.v[1]);

  float pv = INFINITY;
  int pi = -1;
  for (int j = 0; j < k; ++j) {
    next_best(z, K, pv, pi, j, l.red);
    if (threadIdx.x == 0) {
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
  const bool vec = vec_loads(src, ksplit, slab_stride, bias, K, logits_out);
  const size_t lds = lds_bytes(staged ? 0 : 1, K);
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
