// The host heads' sum of a row's exponentials (cpu::softmax_topk, softmax_topk_views, softmax_eval): one copy, so
// the three definitions sum in one order and give one another's bits.
#pragma once
#include <cstddef>

namespace anx::cpu {

// fp32 pairwise sum: the error grows with log2(n) roundings, not n
inline float pairwise_sum(const float* v, size_t n) {
  if (n <= 8) {
    float s = 0.f;
    for (size_t i = 0; i < n; ++i) s += v[i];
    return s;
  }
  const size_t h = n / 2;
  return pairwise_sum(v, h) + pairwise_sum(v + h, n - h);
}

}  // namespace anx::cpu
