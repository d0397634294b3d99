// The view-averaging classifier head: N images of V views each, rows [N * V][K] image-major; per image the mean of
// the views' softmax rows, and the k best classes of that mean (cpu::softmax_topk_views is the definition). The
// evaluation protocol AlexNet is known by takes ten views per image (four corner crops, the centre crop and their
// mirror images) and ranks the average of the ten softmax outputs; here neither the [N * V][K] logits nor the
// probabilities leave the chip.
//
// One 256-thread workgroup per image. Two rows live in LDS: z (the view at hand) and acc (the running sum of the
// views' probabilities). For each view, in order:
//   1. z = bias + slab 0 + slab 1 + ... as in softmax_topk.hip (16-B loads where everything is 16-B aligned and
//      K % 4 == 0, scalar loads otherwise; the same bits either way), and into logits_out when the caller wants it;
//   2. max over the row, 3. sum of expf(z - max): per-thread strided walk, wave butterfly, four wave values
//      through LDS (every thread ends with the same bits);
//   4. acc[c] += expf(z[c] - max) / sum on the thread's own strided elements: thread t owns elements t, t + 256, ...
//      in every view, so the running sum needs neither atomics nor a barrier of its own, and adds in view order.
// After the last view each thread divides its elements by float(V) (and writes them to probs_out); then the k
// rounds of softmax_topk.hip's (value, index) argmax run on acc. Phases 2-4 and the rounds read LDS in one fixed
// pattern whatever phase 1's load width was, so an image's result depends only on the bits of its rows' z, V and K.
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

using namespace head;  // the workgroup shape, f32x4, rank_key, ranks_before, aligned16: shared with softmax_topk.hip

// floats of one LDS row: K rounded up to a 16-B unit, so the second row and the reduction slots stay aligned
constexpr unsigned row_floats(unsigned K) { return (K + 3u) & ~3u; }

template <bool VEC>
__global__ void __launch_bounds__(kThreads) softmax_topk_views_kernel(const float* src, int ksplit, size_t slab_stride,
                                                                      const float* bias, int V, int K, int k, int* idx,
                                                                      float* prob, float* probs_out, float* logits_out) {
  // all of it dynamic, so the base of the rows is the 16-B aligned base of the region
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const unsigned t = threadIdx.x, lane = t & 63u, wave = t >> 6, Ku = static_cast<unsigned>(K);
  float* z = lds;
  float* acc = z + row_floats(Ku);
  float(*red_v)[kWaves] = reinterpret_cast<float(*)[kWaves]>(acc + row_floats(Ku));  // [2][kWaves]
  int(*red_i)[kWaves] = reinterpret_cast<int(*)[kWaves]>(red_v + 2);                  // [2][kWaves]
  const size_t img = blockIdx.x;

  for (int v = 0; v < V; ++v) {
    const size_t row = img * static_cast<size_t>(V) + static_cast<size_t>(v);
    const float* x = src + row * Ku;
    float* lo = logits_out ? logits_out + row * Ku : nullptr;

    // 1. the view's reduced row
    if constexpr (VEC) {
      for (unsigned q = t; q < Ku / 4; q += kThreads) {
        f32x4 a;
        int s = 0;
        if (bias) {
          a = reinterpret_cast<const f32x4*>(bias)[q];
        } else {
          a = reinterpret_cast<const f32x4*>(x)[q];
          s = 1;
        }
        for (; s < ksplit; ++s) a += *reinterpret_cast<const f32x4*>(x + s * slab_stride + 4 * static_cast<size_t>(q));
        reinterpret_cast<f32x4*>(z)[q] = a;
        if (lo) reinterpret_cast<f32x4*>(lo)[q] = a;
      }
    } else {
      for (unsigned c = t; c < Ku; c += kThreads) {
        float a;
        int s = 0;
        if (bias) {
          a = bias[c];
        } else {
          a = x[c];
          s = 1;
        }
        for (; s < ksplit; ++s) a += x[s * slab_stride + c];
        z[c] = a;
        if (lo) lo[c] = a;
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

    // 4. this view's probabilities onto the thread's own elements of the running sum
    for (unsigned c = t; c < Ku; c += kThreads) {
      const float p = expf(z[c] - m) / sum;
      acc[c] = v ? acc[c] + p : p;
    }
    __syncthreads();  // z and both red_v slots are free for the next view
  }

  // the mean, still on the thread's own elements
  const float fv = static_cast<float>(V);
  float* po = probs_out ? probs_out + img * Ku : nullptr;
  for (unsigned c = t; c < Ku; c += kThreads) {
    const float p = acc[c] / fv;
    acc[c] = p;
    if (po) po[c] = p;
  }
  __syncthreads();

  // k rounds on the mean row; (pv, pi) is the previous winner. The two red_* slots alternate, so one barrier per
  // round is enough: slot b is rewritten two rounds later, behind the barrier every reader of it has passed.
  float pv = INFINITY;
  int pi = -1;
  for (int j = 0; j < k; ++j) {
    float bv = -INFINITY;
    int bi = INT_MAX;  // "none": ranks after every real element
    for (unsigned c = t; c < Ku; c += kThreads) {
      const float val = rank_key(acc[c]);
      const int ci = static_cast<int>(c);
      if ((val < pv || (val == pv && ci > pi)) && ranks_before(val, ci, bv, bi)) bv = val, bi = ci;
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
      idx[img * static_cast<size_t>(k) + j] = pi;
      prob[img * static_cast<size_t>(k) + j] = acc[pi];
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
  // every row starts at a multiple of K floats from src, so K % 4 == 0 keeps the rows aligned with the base
  const bool vec = K % 4 == 0 && (ksplit == 1 || slab_stride % 4 == 0) && aligned16(src) && aligned16(bias) &&
                   aligned16(logits_out);
  // two rows and the 2 x 4 (value, index) slots of the reductions: at K = 7680, 61440 + 64 bytes
  const size_t lds = (2 * static_cast<size_t>(row_floats(static_cast<unsigned>(K))) + 4 * kWaves) * sizeof(float);
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
