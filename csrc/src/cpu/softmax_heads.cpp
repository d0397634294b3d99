// cpu::softmax_topk, cpu::softmax_topk_views and cpu::softmax_eval — the definitions of the three classifier heads
// (anx/ops.hpp). The row reduction, the softmax, the view mean and the ranking rounds are written once below, so the
// three sum in one order and give one another's bits: softmax_eval's pred and rank agree with the indices the other
// two return, bit for bit on the score row.
//
// The reference ends at Block 2's LRN and has no classifier head.
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "anx/ops.hpp"

namespace anx::cpu {
namespace {

constexpr float inf = std::numeric_limits<float>::infinity();

// fp32 pairwise sum: the error grows with log2(n) roundings, not n
float pairwise_sum(const float* v, size_t n) {
  if (n <= 8) {
    float s = 0.f;
    for (size_t i = 0; i < n; ++i) s += v[i];
    return s;
  }
  const size_t h = n / 2;
  return pairwise_sum(v, h) + pairwise_sum(v + h, n - h);
}

// z = bias + slab 0 + slab 1 + ... of the row x (slab s at x + s * slab_stride), also into lo unless null
void reduce_row(const float* x, int ksplit, size_t slab_stride, const float* bias, int K, float* z, float* lo) {
  for (int c = 0; c < K; ++c) {
    float v;
    int s = 0;
    if (bias) {
      v = bias[c];
    } else {
      v = x[c];
      s = 1;
    }
    for (; s < ksplit; ++s) v = v + x[s * slab_stride + c];
    z[c] = v;
  }
  if (lo) std::copy(z, z + K, lo);
}

// the row's maximum, e[c] = exp(z[c] - max) and their sum
struct Softmax {
  float mx, sum;
};
Softmax softmax_row(const float* z, int K, float* e) {
  float mx = -inf;
  for (int c = 0; c < K; ++c)
    if (z[c] > mx) mx = z[c];
  for (int c = 0; c < K; ++c) e[c] = std::exp(z[c] - mx);
  return {mx, pairwise_sum(e, static_cast<size_t>(K))};
}

// a view's probabilities e / sum onto the running sum (`first`: the view that starts it), adding in view order
void add_view(const float* e, float sum, int K, float* acc, bool first) {
  for (int c = 0; c < K; ++c) {
    const float p = e[c] / sum;
    acc[c] = first ? p : acc[c] + p;
  }
}

void mean_views(float* acc, int K, int V) {
  const float fv = static_cast<float>(V);
  for (int c = 0; c < K; ++c) acc[c] = acc[c] / fv;
}

// a NaN ranks with -inf, so the order (value descending, then index ascending) is total
float rank_key(float v) { return v != v ? -inf : v; }

// the k classes of the score row r that rank first, in order. Round j takes the best element ranking strictly after
// round j-1's winner, so nothing is marked or rewritten.
void top_rounds(const float* r, int K, int k, int* idx) {
  float pv = inf;
  int pi = -1;
  for (int j = 0; j < k; ++j) {
    float bv = -inf;
    int bi = K;
    for (int c = 0; c < K; ++c) {
      const float v = rank_key(r[c]);
      if ((v < pv || (v == pv && c > pi)) && (bi == K || v > bv)) bv = v, bi = c;
    }
    pv = bv;
    pi = bi;
    idx[j] = bi;
  }
}

}  // namespace

void softmax_topk(const float* src, int ksplit, size_t slab_stride, const float* bias, int M, int K, int k, int* idx,
                  float* prob, float* logits_out) {
  const size_t Kz = static_cast<size_t>(K);
  std::vector<float> z(Kz), e(Kz);
  for (int m = 0; m < M; ++m) {
    const size_t row = static_cast<size_t>(m);
    reduce_row(src + row * Kz, ksplit, slab_stride, bias, K, z.data(), logits_out ? logits_out + row * Kz : nullptr);
    const Softmax s = softmax_row(z.data(), K, e.data());
    top_rounds(z.data(), K, k, idx + row * k);
    for (int j = 0; j < k; ++j) prob[row * k + j] = std::exp(z[idx[row * k + j]] - s.mx) / s.sum;
  }
}

void softmax_topk_views(const float* src, int ksplit, size_t slab_stride, const float* bias, int N, int V, int K, int k,
                        int* idx, float* prob, float* probs_out, float* logits_out) {
  const size_t Kz = static_cast<size_t>(K);
  std::vector<float> z(Kz), e(Kz), acc(Kz);
  for (int i = 0; i < N; ++i) {
    const size_t img = static_cast<size_t>(i);
    for (int v = 0; v < V; ++v) {
      const size_t row = img * V + v;
      reduce_row(src + row * Kz, ksplit, slab_stride, bias, K, z.data(), logits_out ? logits_out + row * Kz : nullptr);
      const Softmax s = softmax_row(z.data(), K, e.data());
      add_view(e.data(), s.sum, K, acc.data(), v == 0);
    }
    mean_views(acc.data(), K, V);
    if (probs_out) std::copy(acc.begin(), acc.end(), probs_out + img * Kz);
    top_rounds(acc.data(), K, k, idx + img * k);
    for (int j = 0; j < k; ++j) prob[img * k + j] = acc[idx[img * k + j]];
  }
}

void softmax_eval(const float* src, int ksplit, size_t slab_stride, const float* bias, int N, int V, int K, int k,
                  const int* labels, int* rank, float* nll, int* pred, uint64_t* stats, uint32_t* confusion,
                  float* logits_out) {
  const size_t Kz = static_cast<size_t>(K);
  const int views = V ? V : 1;
  std::vector<float> z(Kz), e(Kz), acc(V ? Kz : 0);
  for (int i = 0; i < N; ++i) {
    Softmax s{-inf, 0.f};
    for (int v = 0; v < views; ++v) {
      const size_t row = static_cast<size_t>(i) * views + v;
      reduce_row(src + row * Kz, ksplit, slab_stride, bias, K, z.data(), logits_out ? logits_out + row * Kz : nullptr);
      s = softmax_row(z.data(), K, e.data());
      if (V) add_view(e.data(), s.sum, K, acc.data(), v == 0);
    }
    if (V) mean_views(acc.data(), K, V);
    const float* r = V ? acc.data() : z.data();  // the score row
    int first = 0;
    top_rounds(r, K, 1, &first);
    const int y = labels[i];
    const bool counted = y >= 0 && y < K;
    int before = -1;
    float loss = 0.f;
    if (counted) {
      const float ky = rank_key(r[y]);
      before = 0;
      for (int c = 0; c < K; ++c) before += rank_key(r[c]) > ky || (rank_key(r[c]) == ky && c < y);
      loss = V ? -std::log(acc[y]) : std::log(s.sum) - (z[y] - s.mx);
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
