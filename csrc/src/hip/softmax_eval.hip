// The evaluation head: the model held to labels (cpu::softmax_eval is the definition). Per image the rank of the
// true class under the heads' own order, the negative log-likelihood and the top-1 prediction, and each image added
// into running device counters (images, top-1 hits, top-k hits, a fixed-point loss sum, optionally a confusion
// matrix), so a whole validation set runs without a host synchronisation and neither logits nor probabilities leave
// the chip.
//
// One workgroup per image, the phases of softmax_head.hpp.
//   V == 0 (one row per image, ranked by logit): reduce, max, sum; the score row r is z.
//   V >= 1 (views, ranked by mean probability): softmax_topk_views.hip's sequence, for each view reduce, max, sum and
//     accumulate, then the mean; the score row r is acc.
//   Then round 0 of the other heads' argmax gives pred, and one counting pass gives rank: each thread counts, over its
//   strided elements, the classes that rank before the label (head::ranks_before on head::rank_key), and an integer
//   wave and workgroup sum adds them up.
//   Thread 0 writes rank, nll (logf(sum) - (z[y] - max), or -logf(acc[y]) with views) and pred, and adds the image
//   into stats / confusion with integer atomicAdd. There are no float atomics: integer sums do not depend on the
//   order workgroups, chunks and lanes arrive in, so the totals are the same bits from run to run.
// A label outside 0 .. K-1 is decided here (the labels live on the device): rank -1, nll 0, pred, nothing counted.
// No top-k rounds and no per-class outputs: this head does less per image than softmax_topk.hip.
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
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const unsigned t = threadIdx.x, Ku = static_cast<unsigned>(K);
  const Lds l = carve(lds, Ku, VIEWS ? 2 : 1);
  const size_t img = blockIdx.x;
  const int rows = VIEWS ? V : 1;
  float m = -INFINITY, sum = 0.f;

  for (int v = 0; v < rows; ++v) {
    const size_t row = img * static_cast<size_t>(rows) + static_cast<size_t>(v);
    reduce_row<VEC>(src + row * Ku, ksplit, slab_stride, bias, Ku, l.z, logits_out ? logits_out + row * Ku : nullptr);
    m = row_max(l.z, Ku, l.red.v[0]);
    sum = row_expsum(l.z, Ku, m, l.red.v[1]);
    if constexpr (VIEWS) add_view(l.z, l.acc, Ku, m, sum, v == 0);
  }
  if constexpr (VIEWS) mean_views(l.acc, Ku, V, nullptr);
  const float *z = l.z, *r = l.acc;  // the score row: z without views

  // the first class: round 0. Its slot pair is free: every thread read the maximum out of it before the barrier
  // that followed the sum's write.
  float pv = INFINITY;
  int first = -1;
  next_best(r, K, pv, first, 0, l.red);

  // the label's rank. y is one value for the whole workgroup, so the branch (and the barrier in it) is uniform.
  const int y = labels[img];
  const bool counted = static_cast<unsigned>(y) < Ku;
  int before = -1;
  float loss = 0.f;
  if (counted) {
    const float ky = rank_key(r[y]);  // one address for every lane: a broadcast
    int n = 0;
    for (unsigned c = t; c < Ku; c += kThreads) n += ranks_before(rank_key(r[c]), static_cast<int>(c), ky, y) ? 1 : 0;
    before = workgroup_sum(n, l.red.i[1]);  // the other pair's index slots: nothing has used them
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
  const bool vec = vec_loads(src, ksplit, slab_stride, bias, K, logits_out);
  const size_t lds = lds_bytes(V ? 2 : 1, K);
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
