// The evaluation head: the model held to labels (cpu::softmax_eval is the definition). Per image the rank of the
// true class under the heads' own order, the negative log-likelihood and the top-1 prediction, and each image added
// into running device counters (images, top-1 hits, top-k hits, a fixed-point loss sum, optionally a confusion
// matrix), so a whole validation set runs without a host synchronisation and neither logits nor probabilities leave
// the chip.
//
// One 256-thread workgroup per image, the score row in LDS.
//   V == 0 (one row per image, ranked by logit):
//     1. z = bias + slab 0 + slab 1 + ... as in softmax_topk.hip (16-B loads where everything is 16-B aligned and
//        K % 4 == 0, scalar loads otherwise; the same bits either way), and into logits_out when the caller wants it;
//     2. max, 3. sum of expf(z - max): per-thread strided walk, wave butterfly, four wave values through LDS;
//   V >= 1 (views, ranked by mean probability): softmax_topk_views.hip's loop over the image's rows, z the view at
//     hand and acc the running sum on each thread's own elements, then the division by float(V).
//   Then on the score row r (z, or acc):
//     4. one round of the other heads' (value, index) argmax: pred;
//     5. one counting pass: each thread counts, over its strided elements, the classes that rank before the label
//        (head::ranks_before on head::rank_key), and an integer wave and workgroup sum gives rank.
//   Thread 0 writes rank, nll (logf(sum) - (z[y] - max), or -logf(acc[y]) with views) and pred, and adds the image
//   into stats / confusion with integer atomicAdd. There are no float atomics: integer sums do not depend on the
//   order workgroups, chunks and lanes arrive in, so the totals are the same bits from run to run.
// A label outside 0 .. K-1 is decided here (the labels live on the device): rank -1, nll 0, pred, nothing counted.
// No top-k rounds and no per-class outputs: this head does less per image than softmax_topk.hip.
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

using namespace head;  // the workgroup shape, f32x4, rank_key, ranks_before, aligned16: shared with the other heads

// floats of one LDS row: K rounded up to a 16-B unit, so the second row and the reduction slots stay aligned
constexpr unsigned row_floats(unsigned K) { return (K + 3u) & ~3u; }

struct EvalOut {
  int* rank;
  float* nll;
  int* pred;
  unsigned long long* stats;
  unsigned* confusion;
};

template <bool VEC, bool VIEWS>
__global__ void __launch_bounds__(kThreads) softmax_eval_kernel(const float* src, int ksplit, size_t slab_stride,
                                                                const float* bias, int V, int K, int k,
                                                                const int* labels, EvalOut o, float* logits_out) {
  // all of it dynamic, so the base of the rows is the 16-B aligned base of the region
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const unsigned t = threadIdx.x, lane = t & 63u, wave = t >> 6, Ku = static_cast<unsigned>(K);
  float* z = lds;
  float* acc = VIEWS ? z + row_floats(Ku) : z;  // the score row
  float(*red_v)[kWaves] = reinterpret_cast<float(*)[kWaves]>(acc + row_floats(Ku));  // [2][kWaves]
  int(*red_i)[kWaves] = reinterpret_cast<int(*)[kWaves]>(red_v + 2);                  // [2][kWaves]
  const size_t img = blockIdx.x;
  const int rows = VIEWS ? V : 1;
  float m = -INFINITY, sum = 0.f;

  for (int v = 0; v < rows; ++v) {
    const size_t row = img * static_cast<size_t>(rows) + static_cast<size_t>(v);
    const float* x = src + row * Ku;
    float* lo = logits_out ? logits_out + row * Ku : nullptr;

    // 1. the reduced row
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
    m = -INFINITY;
    for (unsigned c = t; c < Ku; c += kThreads) m = fmaxf(m, z[c]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if (lane == 0) red_v[0][wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red_v[0][0], red_v[0][1]), fmaxf(red_v[0][2], red_v[0][3]));

    // 3. sum of exp(z - max)
    sum = 0.f;
    for (unsigned c = t; c < Ku; c += kThreads) sum += expf(z[c] - m);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
    if (lane == 0) red_v[1][wave] = sum;
    __syncthreads();
    sum = (red_v[1][0] + red_v[1][1]) + (red_v[1][2] + red_v[1][3]);

    if constexpr (VIEWS) {
      // this view's probabilities onto the thread's own elements of the running sum (softmax_topk_views.hip, 4.)
      for (unsigned c = t; c < Ku; c += kThreads) {
        const float p = expf(z[c] - m) / sum;
        acc[c] = v ? acc[c] + p : p;
      }
      __syncthreads();  // z and both red_v slots are free for the next view
    }
  }

  if constexpr (VIEWS) {  // the mean, still on the thread's own elements
    const float fv = static_cast<float>(V);
    for (unsigned c = t; c < Ku; c += kThreads) acc[c] = acc[c] / fv;
    __syncthreads();
  }
  const float* r = acc;

  // 4. the first class: round 0 of the other heads' argmax. Slot 0 of red_* is free: every thread read the maximum
  // out of it before the barrier that followed the sum's write.
  float bv = -INFINITY;
  int bi = INT_MAX;  // "none": ranks after every real element
  for (unsigned c = t; c < Ku; c += kThreads) {
    const float val = rank_key(r[c]);
    const int ci = static_cast<int>(c);
    if (ranks_before(val, ci, bv, bi)) bv = val, bi = ci;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(bv, off, 64);
    const int oi = __shfl_xor(bi, off, 64);
    if (ranks_before(ov, oi, bv, bi)) bv = ov, bi = oi;
  }
  if (lane == 0) red_v[0][wave] = bv, red_i[0][wave] = bi;
  __syncthreads();
  bv = red_v[0][0], bi = red_i[0][0];
#pragma unroll
  for (unsigned w = 1; w < kWaves; ++w)
    if (ranks_before(red_v[0][w], red_i[0][w], bv, bi)) bv = red_v[0][w], bi = red_i[0][w];
  const int first = bi < K ? bi : K - 1;  // K >= 1 leaves a candidate; never index past the row

  // 5. the label's rank. y is one value for the whole workgroup, so the branch (and the barrier in it) is uniform.
  const int y = labels[img];
  const bool counted = static_cast<unsigned>(y) < Ku;
  int before = -1;
  float loss = 0.f;
  if (counted) {
    const float ky = rank_key(r[y]);  // one address for every lane: a broadcast
    int n = 0;
    for (unsigned c = t; c < Ku; c += kThreads) n += ranks_before(rank_key(r[c]), static_cast<int>(c), ky, y) ? 1 : 0;
    before = workgroup_sum(n, red_i[1]);  // slot 1 of red_i: nothing has used it
    if (t == 0) loss = VIEWS ? -logf(r[y]) : logf(sum) - (z[y] - m);
  }

  if (t == 0) {
    if (o.pred) o.pred[img] = first;
    if (o.rank) o.rank[img] = before;
    if (o.nll) o.nll[img] = loss;
    if (counted && o.stats) {
      atomicAdd(o.stats + cpu::kEvalCount, 1ull);
      if (before == 0) atomicAdd(o.stats + cpu::kEvalTop1, 1ull);
      if (before < k) atomicAdd(o.stats + cpu::kEvalTopK, 1ull);
      atomicAdd(o.stats + cpu::kEvalNll, static_cast<unsigned long long>(cpu::eval_nll_q32(loss)));
    }
    if (counted && o.confusion) atomicAdd(o.confusion + static_cast<size_t>(y) * Ku + static_cast<unsigned>(first), 1u);
  }
}

}  // namespace

hipError_t softmax_eval(const float* src, int ksplit, size_t slab_stride, const float* bias, int N, int V, int K, int k,
                        const int* labels, int* rank, float* nll, int* pred, uint64_t* stats, uint32_t* confusion,
                        float* logits_out, hipStream_t s) {
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t) && sizeof(unsigned) == sizeof(uint32_t), "the counters");
  if (K < 1 || V < 0 || V > cpu::kMaxViews || K > (V ? kSoftmaxViewsMaxK : kSoftmaxEvalMaxK) || k < 1 ||
      k > cpu::kMaxTopK || k > K || ksplit < 1 || N < 0)
    return hipErrorInvalidValue;
  if (N == 0) return hipSuccess;
  if (!src || !labels) return hipErrorInvalidValue;
  // every row starts at a multiple of K floats from src, so K % 4 == 0 keeps the rows aligned with the base
  const bool vec = K % 4 == 0 && (ksplit == 1 || slab_stride % 4 == 0) && aligned16(src) && aligned16(bias) &&
                   aligned16(logits_out);
  // one row (two with views) and the 2 x 4 (value, index) slots of the reductions: 61440 + 64 bytes at the limits
  const size_t lds = ((V ? 2 : 1) * static_cast<size_t>(row_floats(static_cast<unsigned>(K))) + 4 * kWaves) * sizeof(float);
  const dim3 grid(static_cast<unsigned>(N));
  const EvalOut o{rank, nll, pred, reinterpret_cast<unsigned long long*>(stats), reinterpret_cast<unsigned*>(confusion)};
#define ANX_EVAL(VEC, VIEWS) \
  softmax_eval_kernel<VEC, VIEWS><<<grid, kThreads, lds, s>>>(src, ksplit, slab_stride, bias, V, K, k, labels, o, logits_out)
  if (vec && V)
    ANX_EVAL(true, true);
  else if (vec)
    ANX_EVAL(true, false);
  else if (V)
    ANX_EVAL(false, true);
  else
    ANX_EVAL(false, false);
#undef ANX_EVAL
  return hipGetLastError();
}

}  // namespace anx::hip
