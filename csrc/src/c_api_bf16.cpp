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
#include "capi_util.hpp"

namespace {
using namespace anx::capi;  // fail, hip_status, guarded, put_string
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

int anx_full_run(void* e, const anx_full_call* c, void* stream) {
  return guarded("anx_full_run", [&] {
    if (!c) return fail("anx_full_run: no call");
    if (c->size != sizeof(anx_full_call))
      return fail("anx_full_run: size is " + std::to_string(c->size) + ", sizeof(anx_full_call) is " +
                  std::to_string(sizeof(anx_full_call)));
    const anx::FullCall call{c->x,    c->u8 != 0, c->rows,   c->logits, c->mark != 0, c->k,     c->idx,      c->prob,
                             c->views, c->labels,  c->rank,   c->nll,    c->pred,      c->stats, c->confusion};
    // what the evaluation head's fields rule out among themselves needs no engine
    if (const char* why = anx::FullEngine::check_eval(call)) return fail(std::string("anx_full_run: ") + why);
    if (!e) return fail("anx_full_run: no engine");
    auto* eng = static_cast<anx::FullEngine*>(e);
    if (const char* why = eng->check(call)) return fail(std::string("anx_full_run: ") + why);
    return hip_status(eng->run(call, S(stream)), "anx_full_run");
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

// How the last call's input reached Conv1 ("" before the first). Host state only.
int anx_full_last_input(void* e, char* buf, size_t cap) {
  return guarded("anx_full_last_input", [&] {
    if (!e) return fail("anx_full_last_input: no engine");
    const char* v = static_cast<anx::FullEngine*>(e)->last_input();
    return put_string("anx_full_last_input", v ? v : "", buf, cap);
  });
}

// What the head of the last call read ("" after a plain forward and before the first call). Host state only.
int anx_full_last_head(void* e, char* buf, size_t cap) {
  return guarded("anx_full_last_head", [&] {
    if (!e) return fail("anx_full_last_head: no engine");
    const char* v = static_cast<anx::FullEngine*>(e)->last_head();
    return put_string("anx_full_last_head", v ? v : "", buf, cap);
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
    return put_string("anx_full_last_path", j + "}", buf, cap);
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
