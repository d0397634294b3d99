// The view-averaging classifier head: N images of V views each, rows [N * V][K] image-major; per image the mean of
// the views' softmax rows, and the k best classes of that mean (cpu::softmax_topk_views is the definition). The
// evaluation protocol AlexNet is known by takes ten views per image (four corner crops, the centre crop and their
// mirror images) and ranks the average of the ten softmax outputs; here neither the [N * V][K] logits nor the
// probabilities leave the chip.
//
// One workgroup per image, two rows in LDS, the phases of softmax_head.hpp: for each view in order reduce, max, sum
// and accumulate; then the mean (also into probs_out) and k rounds on it; thread 0 writes each round's index and the
// mean there.
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

template <bool VEC>
__global__ void __launch_bounds__(kThreads) softmax_topk_views_kernel(const float* src, int ksplit, size_t slab_stride,
                                                                      const float* bias, int V, int K, int k, int* idx,
                                                                      float* prob, float* probs_out, float* logits_out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const unsigned Ku = static_cast<unsigned>(K);
  const Lds l = carve(lds, Ku, 2);
  const size_t img = blockIdx.x;

  for (int v = 0; v < V; ++v) {
    const size_t row = img * static_cast<size_t>(V) + static_cast<size_t>(v);
    reduce_row<VEC>(src + row * Ku, ksplit, slab_stride, bias, Ku, l.z, logits_out ? logits_out + row * Ku : nullptr);
    const float m = row_max(l.z, Ku, l.red.v[0]);
    const float sum = row_expsum(l.z, Ku, m, l.red.v[1]);
    add_view(l.z, l.acc, Ku, m, sum, v == 0);
  }
  mean_views(l.acc, Ku, V, probs_out ? probs_out + img * Ku : nullptr);

  float pv = INFINITY;
  int pi = -1;
  for (int j = 0; j < k; ++j) {
    next_best(l.acc, K, pv, pi, j, l.red);
    if (threadIdx.x == 0) {
      idx[img * static_cast<size_t>(k) + j] = pi;
      prob[img * static_cast<size_t>(k) + j] = l.acc[pi];
    }
  }
}

}  // namespace

hipError_t softmax_topk_views(const float* src, int ksplit, size_t slab_stride, const float* bias, int N, int V, int K,
                              int k, int* idx, float* prob, float* probs_out, float* logits_out, hipStream_t s) {
  if (K < 1 || K > kSoftmaxViewsMaxK || V < 1 || V > cpu::kMaxViews || k < 1 || k > cpu::kMaxTopK || k > K ||
      ksplit < 1 || N < 0)
    return hipErrorInvalidValue;
  if (N == 0) return hipSuccess;
  if (!src || !idx || !prob) return hipErrorInvalidValue;
  const bool vec = vec_loads(src, ksplit, slab_stride, bias, K, logits_out);
  const size_t lds = lds_bytes(2, K);
  const dim3 grid(static_cast<unsigned>(N));
  if (vec)
    softmax_topk_views_kernel<true><<<grid, kThreads, lds, s>>>(src, ksplit, slab_stride, bias, V, K, k, idx, prob,
                                                                 probs_out, logits_out);
  else
    softmax_topk_views_kernel<false><<<grid, kThreads, lds, s>>>(src, ksplit, slab_stride, bias, V, K, k, idx, prob,
                                                                  probs_out, logits_out);
  return hipGetLastError();
}

}  // namespace anx::hip
