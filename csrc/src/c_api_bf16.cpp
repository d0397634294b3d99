// Flat C ABI of the bf16 full-AlexNet engine (anx/c_api.h, "full AlexNet bf16 engine"): libanx_bf16.so.
// Its own library so the fp32 programs (the anx CLI, the Blocks engine) never load the bf16 kernels'
// code objects: the V3 process's cold start pays only for what it runs. Errors go through libanx's
// thread-local message (anx_set_last_error / anx_last_error).
#include <exception>
#include <stdexcept>
#include <string>

#include "anx/bf16_ops.hpp"
#include "anx/c_api.h"
#include "anx/knobs.hpp"

namespace {
int fail(const std::string& m) {
  anx_set_last_error(m.c_str());
  return 1;
}
int hip_status(hipError_t e, const char* what) {
  if (e == hipSuccess) return 0;
  return fail(std::string(what) + ": " + hipGetErrorString(e));
}
template <class F>
int guarded(const char* what, F&& f) {
  try {
    return f();
  } catch (const std::exception& ex) {
    return fail(std::string(what) + ": " + ex.what());
  } catch (...) {
    return fail(std::string(what) + ": unknown exception");
  }
}
hipStream_t S(void* s) { return static_cast<hipStream_t>(s); }
}  // namespace

extern "C" {

int anx_full_weight_sizes(int classes, int groups2, size_t* wn, size_t* bn) {
  anx::full_weight_shapes(classes, groups2, wn, bn);
  return 0;
}

int anx_full_create(void** out, const float* const* weights, const float* const* biases, int classes,
                    int max_batch, int groups2, int lrn_mode) {
  return guarded("anx_full_create", [&] {
    size_t wn[8], bn[8];
    anx::full_weight_shapes(classes, groups2, wn, bn);
    anx::FullWeights w;
    for (int i = 0; i < 8; ++i) {
      w.w[i].assign(weights[i], weights[i] + wn[i]);
      w.b[i].assign(biases[i], biases[i] + bn[i]);
    }
    *out = new anx::FullEngine(w, classes, max_batch, groups2, static_cast<anx::LrnMode>(lrn_mode));
    return 0;
  });
}

int anx_full_destroy(void* e) {
  delete static_cast<anx::FullEngine*>(e);
  return 0;
}

int anx_full_forward(void* e, const float* x, int N, float* logits, void* stream) {
  return guarded("anx_full_forward", [&] {
    return hip_status(static_cast<anx::FullEngine*>(e)->forward(x, N, logits, S(stream)), "full forward");
  });
}

int anx_full_forward_mark(void* e, const float* x, int N, float* logits, void* stream) {
  return guarded("anx_full_forward_mark", [&] {
    return hip_status(static_cast<anx::FullEngine*>(e)->forward(x, N, logits, S(stream), true), "full forward");
  });
}

int anx_full_forward_u8(void* e, const uint8_t* x, int N, float* logits, void* stream) {
  return guarded("anx_full_forward_u8", [&] {
    if (!e) return fail("anx_full_forward_u8: no engine");
    if (N > 0 && (!x || !logits)) return fail("anx_full_forward_u8: no buffer");
    return hip_status(static_cast<anx::FullEngine*>(e)->forward_u8(x, N, logits, S(stream)), "full forward (bytes)");
  });
}

int anx_full_forward_mark_u8(void* e, const uint8_t* x, int N, float* logits, void* stream) {
  return guarded("anx_full_forward_mark_u8", [&] {
    if (!e) return fail("anx_full_forward_mark_u8: no engine");
    if (N > 0 && (!x || !logits)) return fail("anx_full_forward_mark_u8: no buffer");
    return hip_status(static_cast<anx::FullEngine*>(e)->forward_u8(x, N, logits, S(stream), true), "full forward (bytes)");
  });
}

int anx_full_set_input_norm(void* e, const float* scale, const float* offset) {
  return guarded("anx_full_set_input_norm", [&] {
    if (!e) return fail("anx_full_set_input_norm: no engine");
    if (!scale || !offset) return fail("anx_full_set_input_norm: 3 scale and 3 offset values");
    static_cast<anx::FullEngine*>(e)->set_input_norm(scale, offset);
    return 0;
  });
}

// How the last forward's input reached Conv1 ("" before the first). Host state only.
int anx_full_last_input(void* e, char* buf, size_t cap) {
  return guarded("anx_full_last_input", [&] {
    if (!e) return fail("anx_full_last_input: no engine");
    if (!buf || cap == 0) return fail("anx_full_last_input: no buffer");
    const char* v = static_cast<anx::FullEngine*>(e)->last_input();
    const std::string j = v ? v : "";
    if (j.size() + 1 > cap) return fail("anx_full_last_input: buffer too small");
    j.copy(buf, j.size());
    buf[j.size()] = 0;
    return 0;
  });
}

namespace {
// the argument checks of the two classify entries; 0 = fine
int classify_args(const std::string& fn, void* e, const void* x, int N, int k, const int* idx, const float* prob) {
  if (!e) return fail(fn + ": no engine");
  const int classes = static_cast<anx::FullEngine*>(e)->classes();
  if (k < 1 || k > anx::cpu::kMaxTopK || k > classes)
    return fail(fn + ": 1 <= k <= min(classes, 16), got k = " + std::to_string(k) + " for " + std::to_string(classes) +
                " classes");
  if (N > 0 && (!x || !idx || !prob)) return fail(fn + ": no buffer (x, idx, prob)");
  return 0;
}
}  // namespace

int anx_full_classify(void* e, const float* x, int N, int k, int* idx, float* prob, float* logits, void* stream,
                      int mark) {
  return guarded("anx_full_classify", [&] {
    if (classify_args("anx_full_classify", e, x, N, k, idx, prob)) return 1;
    return hip_status(static_cast<anx::FullEngine*>(e)->classify(x, N, k, idx, prob, logits, S(stream), mark != 0),
                      "anx_full_classify");
  });
}

int anx_full_classify_u8(void* e, const uint8_t* x, int N, int k, int* idx, float* prob, float* logits, void* stream,
                         int mark) {
  return guarded("anx_full_classify_u8", [&] {
    if (classify_args("anx_full_classify_u8", e, x, N, k, idx, prob)) return 1;
    return hip_status(static_cast<anx::FullEngine*>(e)->classify_u8(x, N, k, idx, prob, logits, S(stream), mark != 0),
                      "anx_full_classify_u8");
  });
}

namespace {
// what the two classify_views entries check beyond classify_args; 0 = fine
int views_args(const std::string& fn, void* e, int rows, int V) {
  if (V < 1 || V > anx::cpu::kMaxViews) return fail(fn + ": 1 <= V <= 32 views, got " + std::to_string(V));
  if (rows < 0 || rows % V != 0)
    return fail(fn + ": " + std::to_string(rows) + " rows are no whole number of images of " + std::to_string(V) + " views");
  if (static_cast<anx::FullEngine*>(e)->classes() > anx::hip::kSoftmaxViewsMaxK)
    return fail(fn + ": more than " + std::to_string(anx::hip::kSoftmaxViewsMaxK) + " classes");
  return 0;
}
}  // namespace

int anx_full_classify_views(void* e, const float* x, int rows, int V, int k, int* idx, float* prob, float* logits,
                            void* stream, int mark) {
  return guarded("anx_full_classify_views", [&] {
    if (classify_args("anx_full_classify_views", e, x, rows, k, idx, prob)) return 1;
    if (views_args("anx_full_classify_views", e, rows, V)) return 1;
    return hip_status(
        static_cast<anx::FullEngine*>(e)->classify_views(x, rows, V, k, idx, prob, logits, S(stream), mark != 0),
        "anx_full_classify_views");
  });
}

int anx_full_classify_views_u8(void* e, const uint8_t* x, int rows, int V, int k, int* idx, float* prob, float* logits,
                               void* stream, int mark) {
  return guarded("anx_full_classify_views_u8", [&] {
    if (classify_args("anx_full_classify_views_u8", e, x, rows, k, idx, prob)) return 1;
    if (views_args("anx_full_classify_views_u8", e, rows, V)) return 1;
    return hip_status(
        static_cast<anx::FullEngine*>(e)->classify_views_u8(x, rows, V, k, idx, prob, logits, S(stream), mark != 0),
        "anx_full_classify_views_u8");
  });
}

// What the head of the last call read ("" after a plain forward and before the first call). Host state only.
int anx_full_last_head(void* e, char* buf, size_t cap) {
  return guarded("anx_full_last_head", [&] {
    if (!e) return fail("anx_full_last_head: no engine");
    if (!buf || cap == 0) return fail("anx_full_last_head: no buffer");
    const char* v = static_cast<anx::FullEngine*>(e)->last_head();
    const std::string j = v ? v : "";
    if (j.size() + 1 > cap) return fail("anx_full_last_head: buffer too small");
    j.copy(buf, j.size());
    buf[j.size()] = 0;
    return 0;
  });
}

int anx_full_wait_mark(void* e, void* stream) {
  return guarded("anx_full_wait_mark", [&] {
    return hip_status(static_cast<anx::FullEngine*>(e)->wait_mark(S(stream)), "full wait mark");
  });
}

int anx_full_tap(void* e, int i, int N, void* dst, size_t* elems, void* stream) {
  *elems = static_cast<anx::FullEngine*>(e)->tap(i, N, dst, S(stream));
  return *elems ? 0 : fail("anx_full_tap: bad tap index or batch");
}
// The kernels the engine's last forward launched (anx::FullPathRecord) as one JSON object. Host state only.
int anx_full_last_path(void* e, char* buf, size_t cap) {
  return guarded("anx_full_last_path", [&] {
    if (!e) return fail("anx_full_last_path: no engine");
    if (!buf || cap == 0) return fail("anx_full_last_path: no buffer");
    const anx::FullPathRecord& p = static_cast<anx::FullEngine*>(e)->last_path();
    std::string j = "{\"conv1\": ";
    if (p.conv1)
      j += std::string("{\"form\": \"") + p.conv1 + "\", \"segs\": " +
           (p.conv1_segs ? std::to_string(p.conv1_segs) : std::string("null")) + "}";
    else
      j += "null";
    static const char* const names[7] = {"conv2", "conv3", "conv4", "conv5", "fc6", "fc7", "fc8"};
    for (int i = 0; i < 7; ++i) {
      const anx::FullPathRecord::Gemm& g = p.gemm[i];
      j += std::string(", \"") + names[i] + "\": ";
      if (g.kernel)
        j += std::string("{\"kernel\": \"") + g.kernel + "\", \"id\": " + std::to_string(g.id) +
             ", \"splitk\": " + std::to_string(g.splitk) + "}";
      else
        j += "null";
    }
    j += "}";
    if (j.size() + 1 > cap) return fail("anx_full_last_path: buffer too small (" + std::to_string(j.size() + 1) + " bytes)");
    j.copy(buf, j.size());
    buf[j.size()] = 0;
    return 0;
  });
}
int anx_full_set_knob(void* e, const char* name, int value) {
  if (anx::set_knob(static_cast<anx::FullEngine*>(e)->knobs(), name, value) != 0)
    return fail(std::string("bad knob or value: ") + (name ? name : "(null)"));
  return 0;
}
int anx_full_get_knob(void* e, const char* name, int* value) {
  if (anx::get_knob(static_cast<anx::FullEngine*>(e)->knobs(), name, value) != 0)
    return fail(std::string("unknown knob: ") + (name ? name : "(null)"));
  return 0;
}
}  // extern "C"
