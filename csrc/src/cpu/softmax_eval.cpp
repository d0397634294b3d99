// cpu::softmax_eval — the definition of the evaluation head (anx/ops.hpp): rank of the true class, negative
// log-likelihood and top-1 prediction per image, and the running counters. The row reduction, the softmax and the
// view mean are cpu::softmax_topk's and cpu::softmax_topk_views' expressions (ref_layers.cpp), so pred and rank agree
// with the indices those two return, bit for bit on the score row.
//
// The reference ends at Block 2's LRN and has no classifier head.
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "anx/ops.hpp"
#include "pairwise_sum.hpp"

namespace anx::cpu {

void softmax_eval(const float* src, int ksplit, size_t slab_stride, const float* bias, int N, int V, int K, int k,
                  const int* labels, int* rank, float* nll, int* pred, uint64_t* stats, uint32_t* confusion,
                  float* logits_out) {
  const float inf = std::numeric_limits<float>::infinity();
  const size_t Kz = static_cast<size_t>(K);
  const int views = V ? V : 1;
  std::vector<float> z(Kz), e(Kz), acc(V ? Kz : 0);
  for (int i = 0; i < N; ++i) {
    float mx = -inf, sum = 0.f;
    for (int v = 0; v < views; ++v) {
      const size_t row = static_cast<size_t>(i) * views + v;
      const float* x = src + row * Kz;
      for (int c = 0; c < K; ++c) {  // softmax_topk's reduction, max, exponentials and sum
        float a;
        int s = 0;
        if (bias) {
          a = bias[c];
        } else {
          a = x[c];
          s = 1;
        }
        for (; s < ksplit; ++s) a = a + x[s * slab_stride + c];
        z[c] = a;
      }
      if (logits_out) std::copy(z.begin(), z.end(), logits_out + row * Kz);
      mx = -inf;
      for (int c = 0; c < K; ++c)
        if (z[c] > mx) mx = z[c];
      for (int c = 0; c < K; ++c) e[c] = std::exp(z[c] - mx);
      sum = pairwise_sum(e.data(), e.size());
      if (V)
        for (int c = 0; c < K; ++c) {
          const float p = e[c] / sum;
          acc[c] = v ? acc[c] + p : p;
        }
    }
    if (V) {
      const float fv = static_cast<float>(V);
      for (int c = 0; c < K; ++c) acc[c] = acc[c] / fv;
    }
    const float* r = V ? acc.data() : z.data();  // the score row
    auto key = [&](int c) { return r[c] != r[c] ? -inf : r[c]; };
    int first = 0;  // value descending, then index ascending: a later class wins only with a greater value
    for (int c = 1; c < K; ++c)
      if (key(c) > key(first)) first = c;
    const int y = labels[i];
    const bool counted = y >= 0 && y < K;
    int before = -1;
    float loss = 0.f;
    if (counted) {
      const float ky = key(y);
      before = 0;
      for (int c = 0; c < K; ++c) before += key(c) > ky || (key(c) == ky && c < y);
      loss = V ? -std::log(acc[y]) : std::log(sum) - (z[y] - mx);
    }
    if (pred) pred[i] = first;
    if (rank) rank[i] = before;
    if (nll) nll[i] = loss;
    if (counted && stats) {
      stats[kEvalCount] += 1;
      stats[kEvalTop1] += before == 0;
      stats[kEvalTopK] += before < k;
      stats[kEvalNll] += eval_nll_q32(loss);
    }
    if (counted && confusion) confusion[static_cast<size_t>(y) * Kz + first] += 1;
  }
}

}  // namespace anx::cpu
