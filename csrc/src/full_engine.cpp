// Full AlexNet engine (bf16 extension, see anx/bf16_ops.hpp). Weights are packed to bf16 once and
// stay resident; every activation between layers lives in a persistent bf16 workspace, with the
// padded layers' inputs kept as zero-bordered windows that the producing kernel writes into.
#include <algorithm>
#include <cstdlib>
#include <stdexcept>
#include <string>

#include "anx/bf16_ops.hpp"
#include "anx/upload.hpp"

namespace anx {

namespace {
// C, K, F, S per layer (groups filled in per instance for conv2)
constexpr int kGeom[8][4] = {{3, 96, 11, 4},      {96, 256, 5, 1},    {256, 384, 3, 1},   {384, 384, 3, 1},
                             {384, 256, 3, 1},    {9216, 4096, 1, 1}, {4096, 4096, 1, 1}, {4096, 0, 1, 1}};
}  // namespace

// xb_ holds the raw image as bf16 (taps8) or its polyphase form [57,57,48], the larger and the one tap() reports
const FullEngine::ActSpec FullEngine::kActs[FullEngine::kNumActs] = {
    {55 * 55 * 96, false},  {31 * 31 * 96, true},   {27 * 27 * 256, false}, {15 * 15 * 256, true},
    {15 * 15 * 384, true},  {15 * 15 * 384, true},  {13 * 13 * 256, false}, {9216, false},
    {4096, false},          {4096, false},          {std::max(227 * 227 * 3, 57 * 57 * 48), false}};

void full_weight_shapes(int classes, int groups2, size_t wn[8], size_t bn[8]) {
  for (int i = 0; i < 8; ++i) {
    const int C = kGeom[i][0], K = i == 7 ? classes : kGeom[i][1], F = kGeom[i][2];
    const int g = i == 1 ? groups2 : 1;
    wn[i] = static_cast<size_t>(K) * (C / g) * F * F;
    bn[i] = static_cast<size_t>(K);
  }
}

FullEngine::FullEngine(const FullWeights& w, int classes, int max_batch, int groups2, LrnMode lrn, const Knobs& kn)
    : k_(kn), classes_(classes), max_batch_(max_batch), lrn_(lrn) {
  size_t wn[8], bn[8];
  full_weight_shapes(classes, groups2, wn, bn);
  for (int i = 0; i < 8; ++i) {
    if (w.w[i].size() != wn[i] || w.b[i].size() != bn[i])
      throw std::invalid_argument("full AlexNet: weight " + std::to_string(i) + " has the wrong size");
    Layer& L = L_[i];
    L.C = kGeom[i][0];
    L.K = i == 7 ? classes : kGeom[i][1];
    L.F = kGeom[i][2];
    L.S = kGeom[i][3];
    L.groups = i == 1 ? groups2 : 1;
    L.host = w.w[i];
    L.bias = DevBuf<float>::upload(w.b[i], 16);
  }
  // Conv1 polyphase (the fp32 Winograd Conv1's rewrite, conv1_wino.hip): space-to-depth by the stride
  // turns 11x11/4 over 3 channels into 3x3/1 over 48, so the implicit GEMM's A gathers are aligned
  // 16-B channel runs instead of taps8's 2-byte-aligned 11-tap rows. Exact: W'[k][(rh*4+rw)*3+c][qh][qw]
  // = w[k][c][4qh+rh][4qw+rw], 0 past the 11x11 window. ANX_FULL_CONV1=taps8 keeps the direct form.
  {
    const char* e = std::getenv("ANX_FULL_CONV1");
    poly1_ = !(e && std::string(e) == "taps8");
  }
  if (poly1_) {
    Layer& L = L_[0];
    std::vector<float> wp(static_cast<size_t>(L.K) * 48 * 9, 0.f);
    for (int k = 0; k < L.K; ++k)
      for (int rh = 0; rh < 4; ++rh)
        for (int rw = 0; rw < 4; ++rw)
          for (int c = 0; c < 3; ++c)
            for (int qh = 0; qh < 3; ++qh)
              for (int qw = 0; qw < 3; ++qw) {
                const int fh = 4 * qh + rh, fw = 4 * qw + rw;
                if (fh < 11 && fw < 11)
                  wp[((static_cast<size_t>(k) * 48 + (rh * 4 + rw) * 3 + c) * 3 + qh) * 3 + qw] =
                      L.host[((static_cast<size_t>(k) * 3 + c) * 11 + fh) * 11 + fw];
              }
    L.host = std::move(wp);
    L.C = 48;
    L.F = 3;
    L.S = 1;
    std::vector<uint16_t> rp;
    hip::pack_conv1_ring_weights(L.host.data(), rp);
    w1ring_ = DevBuf<uint16_t>::upload(rp, 16);
  }
  {
    int dev = 0;
    hip_check(hipGetDevice(&dev), "hipGetDevice");
    hip_check(hipDeviceGetAttribute(&cus_, hipDeviceAttributeMultiprocessorCount, dev), "CU count");
  }
  chunk_ = std::max(1, std::min(max_batch, static_cast<int>(((1UL << 31) - 1) / (55UL * 55 * 96))));
  const size_t n = static_cast<size_t>(chunk_);
  for (int i = 0; i < kNumActs; ++i) act_[i] = DevBuf<uint16_t>(n * kActs[i].elems, 16);
  // zero borders of the padded windows once; kernels only ever write the interiors
  for (int i = 0; i < kNumActs; ++i)
    if (kActs[i].window) hip_check(hipMemset(act_[i].get(), 0, n * kActs[i].elems * 2), "memset");
  size_t ws = 0;  // largest split-K slab set over the FC layers and every batch the engine can see
  for (int i = 5; i < 8; ++i)
    for (int b = 1; b <= chunk_; ++b) {
      const hip::ConvPlanB p = hip::make_conv_plan_bf16(b, 1, 1, L_[i].C, L_[i].K, 1, 1, 1);
      const int ks = hip::fc_split_k(p);
      if (ks > 1) ws = std::max(ws, static_cast<size_t>(ks) * b * L_[i].K);
      for (int c = -1; c < hip::conv_bf16_big_cfgs(); ++c) {  // every config bf16_fc_cfg may force
        const hip::BigFc f = hip::pick_bf16_big_fc(p, cus_, c, 1);  // wide-tile FC slabs (ksplit 1 for fp32 logits)
        if (f.cfg >= 0) ws = std::max(ws, static_cast<size_t>(f.ksplit) * b * L_[i].K);
      }
    }
  if (ws) ws_ = DevBuf<float>(ws, 16);
  hlog_ = DevBuf<float>(n * static_cast<size_t>(classes), 16);  // classify without a caller's logits buffer
}

hipError_t FullEngine::conv(Layer& L, int N, int Hp, int Wp, const void* x, hip::OutViewB out, float* out_f32,
                            bool relu, hipStream_t s, const FullCall* head) {
  auto B = [](void* q) { return static_cast<__bf16*>(q); };
  const hip::ConvPlanB p = hip::make_conv_plan_bf16(N, Hp, Wp, L.C, L.K, L.F, L.S, L.groups);
  if (p.variant != L.key) {  // pack for this tile variant (first use / batch-size class change)
    std::vector<uint16_t> pk;
    std::vector<int> ko;
    hip::pack_conv_weights_bf16(p, L.host.data(), pk, ko);
    // both new buffers first, then commit them with the key: a failure leaves the layer as it was
    DevBuf<uint16_t> wp;
    DevBuf<int> koff;
    ANX_TRY(wp.try_alloc(pk.size()));
    ANX_TRY(koff.try_alloc(ko.size()));
    ANX_TRY(upload_h2d(wp.get(), pk.data(), pk.size() * 2));
    ANX_TRY(upload_h2d(koff.get(), ko.data(), ko.size() * 4));
    L.wp = std::move(wp);
    L.koff = std::move(koff);
    L.key = p.variant;
  }
  const bool fc = p.Hp == 1 && p.Wp == 1 && p.F == 1;
  // what ran (last_path): the launchers write id at their launch. Conv1 here is path_.conv1's "tiles" / "taps8".
  FullPathRecord::Gemm scratch, &rec = &L == &L_[0] ? scratch : path_.gemm[&L - &L_[1]];
  auto big = [&](int ksplit) {
    rec.kernel = "big";
    rec.splitk = ksplit;
    return &rec.id;
  };
  auto tile = [&](int ksplit, hipError_t e) {  // conv2d_bf16 wrote the slot count into rec.id
    rec.kernel = rec.id ? "glds" : "staged";
    if (!rec.id) rec.id = p.variant;
    rec.splitk = ksplit;
    return e;
  };
  // a call with a head and bf16_head: the head kernel reduces the slabs [ksplit][N][K] (+ bias) in place of the reduce
  auto reduce = [&](int ksplit) {
    if (head && k_.bf16_head) return run_head(*head, ws_.get(), ksplit, static_cast<size_t>(N) * L.K, L.bias.get(), s);
    return hip::splitk_reduce_bf16(ws_.get(), ksplit, N, L.K, L.bias.get(), relu, out, out_f32, s);
  };
  if (fc && k_.bf16_big != -2) {  // wide-tile FC: one 256-row tile of the batch, K split over the CUs
    hip::BigFc f = hip::pick_bf16_big_fc(p, cus_, k_.bf16_fc_cfg, k_.bf16_fc_minkt);
    if (f.cfg >= 0 && k_.bf16_big >= 0 && hip::conv_bf16_big_ok(p, k_.bf16_big, hip::OutViewB{B(ws_.get()), 1, 1, p.Kg, 0, 0, 0}))
      f.cfg = k_.bf16_big;
    if (f.cfg >= 0 && (f.ksplit > 1 || out_f32)) {
      ANX_TRY(hip::conv2d_bf16_big(p, f.cfg, x, L.wp.get(), L.koff.get(), L.bias.get(), hip::OutViewB{B(ws_.get()), 1, 1, p.Kg, 0, 0, 0}, relu,
                                   s, hip::SplitK{f.ksplit, ws_.get()}, big(f.ksplit)));
      return reduce(f.ksplit);
    }
    if (f.cfg >= 0) return hip::conv2d_bf16_big(p, f.cfg, x, L.wp.get(), L.koff.get(), L.bias.get(), out, relu, s, {}, big(1));
  }
  const int ks = hip::fc_split_k(p);
  if (ks > 1) {  // FC layer at a small batch: K split over ~one workgroup per CU, then a reduce
    ANX_TRY(tile(ks, hip::conv2d_bf16(p, x, L.wp.get(), L.koff.get(), L.bias.get(), out, out_f32, relu, s, hip::SplitK{ks, ws_.get()},
                                      k_.bf16_glds, &rec.id)));
    return reduce(ks);
  }
  if (!fc && !out_f32 && k_.bf16_big != -2) {  // wide-tile kernel: forced config if it applies, else the cost model
    const int cfg = k_.bf16_big >= 0 && hip::conv_bf16_big_ok(p, k_.bf16_big, out) ? k_.bf16_big
                                                                                    : hip::pick_bf16_big_cfg(p, out, cus_);
    if (cfg >= 0) return hip::conv2d_bf16_big(p, cfg, x, L.wp.get(), L.koff.get(), L.bias.get(), out, relu, s, {}, big(1));
  }
  return tile(1, hip::conv2d_bf16(p, x, L.wp.get(), L.koff.get(), L.bias.get(), out, out_f32, relu, s, {}, k_.bf16_glds, &rec.id));
}

void FullEngine::set_input_norm(const float* scale, const float* offset) {
  for (int c = 0; c < 3; ++c) norm_.sc[c] = scale[c], norm_.of[c] = offset[c];
}

const char* FullEngine::check_eval(const FullCall& c) {
  const bool outputs = c.rank || c.nll || c.pred || c.stats || c.confusion;
  if (!c.labels) return outputs ? "rank, nll, pred, stats and confusion go with labels" : nullptr;
  if (c.idx || c.prob) return "a call has one head: labels (the evaluation head) go without idx and prob";
  if (c.k == 0) return "labels need the top-k threshold (k > 0)";
  if (!outputs) return "no output (rank, nll, pred, stats, confusion)";
  return nullptr;
}

const char* FullEngine::check(const FullCall& c) const {
  static_assert(cpu::kMaxTopK == 16 && cpu::kMaxViews == 32 && hip::kSoftmaxViewsMaxK == 7680 &&
                    hip::kSoftmaxEvalMaxK == 15360,
                "the reasons spell them");
  if (const char* why = check_eval(c)) return why;  // null for every call without the evaluation head's fields
  if (c.rows < 0) return "rows < 0";
  if (c.k < 0 || c.k > cpu::kMaxTopK || c.k > classes_) return "k outside 0 .. min(classes, 16)";
  if (c.k == 0 && (c.idx || c.prob || c.views != 0)) return "idx, prob and views go with a head (k > 0)";
  if (c.rows > 0 && !c.x) return "no input (x)";
  if (c.rows > 0 && !c.labels && (c.k ? !c.idx || !c.prob : !c.logits))
    return c.k ? "no output (idx, prob)" : "no output (logits)";
  if (c.views < 0 || c.views > cpu::kMaxViews) return "views outside 0 .. 32";
  if (c.views && c.rows % c.views != 0) return "rows are no whole number of images of `views` views";
  if (c.views && chunk_ < c.views) return "the engine's launch chunk is smaller than one image's views";
  if (c.views && classes_ > hip::kSoftmaxViewsMaxK) return "the view-averaging head takes at most 7680 classes";
  if (c.labels && !c.views && classes_ > hip::kSoftmaxEvalMaxK)
    return "the evaluation head takes at most 15360 classes without views";
  return nullptr;
}

hipError_t FullEngine::run_head(const FullCall& ch, const float* src, int ksplit, size_t slab_stride, const float* bias,
                                hipStream_t s) {
  float* const z = ch.logits ? ch.logits : hlog_.get();  // where the chunk's logits are, or would be
  const bool slabs = src != z;                           // else they are written: nothing to write again
  if (ch.labels)
    ANX_TRY(hip::softmax_eval(src, ksplit, slab_stride, bias, ch.views ? ch.rows / ch.views : ch.rows, ch.views, classes_,
                              ch.k, ch.labels, ch.rank, ch.nll, ch.pred, ch.stats, ch.confusion,
                              slabs ? ch.logits : nullptr, s));
  else if (ch.views)
    ANX_TRY(hip::softmax_topk_views(src, ksplit, slab_stride, bias, ch.rows / ch.views, ch.views, classes_, ch.k, ch.idx,
                                    ch.prob, nullptr, slabs ? ch.logits : nullptr, s));
  else  // a row too long for the kernel's LDS is staged in z (written logits are read back from there)
    ANX_TRY(hip::softmax_topk(src, ksplit, slab_stride, bias, ch.rows, classes_, ch.k, ch.idx, ch.prob,
                              slabs && ch.logits ? ch.logits : classes_ > hip::kSoftmaxTopkLdsRow ? z : nullptr, s));
  head_ = slabs ? "slabs" : "logits";
  return hipSuccess;
}

hipError_t FullEngine::run(const FullCall& c, hipStream_t s) {
  if (check(c)) return hipErrorInvalidValue;
  const int N = c.rows, V = c.views;
  const float* const xf = c.u8 ? nullptr : static_cast<const float*>(c.x);
  const uint8_t* const xu = c.u8 ? static_cast<const uint8_t*>(c.x) : nullptr;
  const int step = V ? chunk_ / V * V : chunk_;  // views: whole images per launch chunk
  head_ = nullptr;
  if (c.mark && !mark_) ANX_TRY(mark_.try_create(hipEventDisableTiming));
  using hip::OutViewB;
  auto B = [](void* p) { return static_cast<__bf16*>(p); };
  constexpr size_t kImage = 227 * 227 * 3;
  void *const xb_ = a(kXb), *const c1_ = a(kC1), *const q2_ = a(kQ2), *const c2_ = a(kC2), *const q3_ = a(kQ3),
             *const q4_ = a(kQ4), *const q5_ = a(kQ5), *const c5_ = a(kC5), *const f6_ = a(kF6), *const f7_ = a(kF7),
             *const f8_ = a(kF8);
  // bytes straight into the row-band kernel, else decoded into the workspace first
  const bool u8_ring = xu && poly1_ && k_.bf16_conv1 == 2 && k_.bf16_u8 != 0;
  if (xu && !u8_ring && !xdec_) {
    // one launch chunk, once; a captured stream must not see the allocation
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) == hipSuccess && st != hipStreamCaptureStatusNone)
      return hipErrorStreamCaptureUnsupported;
    ANX_TRY(xdec_.try_alloc(static_cast<size_t>(chunk_) * kImage));
  }
  for (int n0 = 0; n0 < N; n0 += step) {
    const int n = std::min(step, N - n0);
    const float* xn = xf ? xf + static_cast<size_t>(n0) * kImage : xdec_.get();
    if (xu && !u8_ring) ANX_TRY(hip::decode_u8(xu + static_cast<size_t>(n0) * kImage, xdec_.get(), n * kImage, norm_, s));
    input_ = !xu ? "f32" : u8_ring ? "u8_ring" : "u8_decode";
    bool pooled = false;  // pool1 done with Conv1
    if (poly1_) {
      if (k_.bf16_conv1 == 2) {  // the image straight into the row-band kernel (no polyphase copy)
        const OutViewB q2v{B(q2_), 31, 31, 96, 2, 2, 0};
        const OutViewB c1v{B(c1_), 55, 55, 96, 0, 0, 0};
        hip::RingRan ran;
        if (u8_ring)
          ANX_TRY(hip::conv1_bf16_ring_u8(xu + static_cast<size_t>(n0) * kImage, norm_, n, w1ring_.get(), L_[0].bias.get(), c1v, true,
                                          s, cus_, k_.bf16_pool1 ? &q2v : nullptr, &ran));
        else
          ANX_TRY(hip::conv1_bf16_ring(xn, n, w1ring_.get(), L_[0].bias.get(), c1v, true, s, cus_, true,
                                       k_.bf16_pool1 ? &q2v : nullptr, &ran));
        pooled = k_.bf16_pool1 != 0;
        path_.conv1 = u8_ring ? (ran.pool ? "ring_u8_pool" : "ring_u8") : (ran.pool ? "ring_f32_pool" : "ring_f32");
        path_.conv1_segs = ran.segs;
      } else {
        ANX_TRY(hip::f32_to_bf16_s2d4(xn, xb_, n, 227, 227, s));
        if (k_.bf16_conv1 == 1) {
          hip::RingRan ran;
          ANX_TRY(hip::conv1_bf16_ring(xb_, n, w1ring_.get(), L_[0].bias.get(), OutViewB{B(c1_), 55, 55, 96, 0, 0, 0}, true, s, cus_,
                                       false, nullptr, &ran));
          path_.conv1 = "ring";
          path_.conv1_segs = ran.segs;
        } else {
          ANX_TRY(conv(L_[0], n, 57, 57, xb_, OutViewB{B(c1_), 55, 55, 96, 0, 0, 0}, nullptr, true, s));
          path_.conv1 = "tiles";
          path_.conv1_segs = 0;
        }
      }
    } else {
      ANX_TRY(hip::f32_to_bf16(xn, xb_, static_cast<size_t>(n) * 227 * 227 * 3, s));
      ANX_TRY(conv(L_[0], n, 227, 227, xb_, OutViewB{B(c1_), 55, 55, 96, 0, 0, 0}, nullptr, true, s));
      path_.conv1 = "taps8";
      path_.conv1_segs = 0;
    }
    if (!pooled) ANX_TRY(hip::maxpool_bf16(c1_, n, 55, 55, 96, 3, 2, OutViewB{B(q2_), 31, 31, 96, 2, 2, 0}, s));
    ANX_TRY(conv(L_[1], n, 31, 31, q2_, OutViewB{B(c2_), 27, 27, 256, 0, 0, 0}, nullptr, true, s));
    ANX_TRY(hip::maxpool_lrn_bf16(c2_, n, 27, 27, 256, 3, 2, 5, 1e-4f, 0.75f, 2.0f, lrn_,
                                  OutViewB{B(q3_), 15, 15, 256, 1, 1, 0}, s, k_.bf16_lrn_tile));
    if (c.mark && n0 == 0) ANX_TRY(hipEventRecord(mark_.get(), s));
    ANX_TRY(conv(L_[2], n, 15, 15, q3_, OutViewB{B(q4_), 15, 15, 384, 1, 1, 0}, nullptr, true, s));
    ANX_TRY(conv(L_[3], n, 15, 15, q4_, OutViewB{B(q5_), 15, 15, 384, 1, 1, 0}, nullptr, true, s));
    ANX_TRY(conv(L_[4], n, 15, 15, q5_, OutViewB{B(c5_), 13, 13, 256, 0, 0, 0}, nullptr, true, s));
    ANX_TRY(hip::maxpool_bf16(c5_, n, 13, 13, 256, 3, 2, OutViewB{B(f6_), 6, 6, 256, 0, 0, 0}, s));
    ANX_TRY(conv(L_[5], n, 1, 1, f6_, OutViewB{B(f7_), 1, 1, 4096, 0, 0, 0}, nullptr, true, s));
    ANX_TRY(conv(L_[6], n, 1, 1, f7_, OutViewB{B(f8_), 1, 1, 4096, 0, 0, 0}, nullptr, true, s));
    // FC8 and the head on this chunk: the call narrowed to its rows and outputs (one output row per image). Logits the
    // caller does not take go to the workspace.
    FullCall ch = c;
    ch.rows = n;
    if (c.logits) ch.logits = c.logits + static_cast<size_t>(n0) * classes_;
    if (c.labels) {  // the per-image arrays by the chunk's images; stats and confusion are every chunk's
      const size_t i0 = static_cast<size_t>(V ? n0 / V : n0);
      ch.labels = c.labels + i0;
      if (c.rank) ch.rank = c.rank + i0;
      if (c.nll) ch.nll = c.nll + i0;
      if (c.pred) ch.pred = c.pred + i0;
    } else if (c.k) {
      const size_t o0 = static_cast<size_t>(V ? n0 / V : n0) * c.k;
      ch.idx = c.idx + o0;
      ch.prob = c.prob + o0;
    }
    float* const z = ch.logits ? ch.logits : hlog_.get();
    head_ = nullptr;
    ANX_TRY(conv(L_[7], n, 1, 1, f8_, OutViewB{nullptr, 1, 1, classes_, 0, 0, 0}, z, false, s, c.k ? &ch : nullptr));
    if (c.k && !head_) ANX_TRY(run_head(ch, z, 1, 0, nullptr, s));  // FC8 wrote the logits: the head runs on those
  }
  return hipSuccess;
}

size_t FullEngine::tap(int i, int N, void* dst, hipStream_t s) const {
  if (i < 0 || i >= kNumActs || (i == kXb && !poly1_) || N < 1 || N > chunk_) return 0;
  if (hipMemcpyAsync(dst, act_[i].get(), kActs[i].elems * N * 2, hipMemcpyDeviceToDevice, s) != hipSuccess) return 0;
  return kActs[i].elems;
}

}  // namespace anx
