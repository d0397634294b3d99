// The primitives behind the device owners (anx/device.hpp): the only host code of the project that creates or
// destroys device buffers, streams and events, so the counters below see every one of them.
#include "anx/device.hpp"

#include <atomic>
#include <mutex>
#include <unordered_map>

namespace anx {

namespace {
std::atomic<size_t> g_bufs{0}, g_bytes{0}, g_sync{0}, g_mallocs{0};
std::atomic<int> g_fail{0};  // device_fail_alloc: calls left until the failing one (0: disarmed)

// bytes of each live buffer (dev_free gets the pointer alone). Never destroyed: owners with static storage
// may free after this file's statics are gone.
struct Sizes {
  std::mutex m;
  std::unordered_map<void*, size_t> of;
};
Sizes& sizes() {
  static Sizes* const s = new Sizes;
  return *s;
}
}  // namespace

hipError_t dev_malloc(void** p, size_t bytes) noexcept {
  g_mallocs.fetch_add(1, std::memory_order_relaxed);
  if (g_fail.load(std::memory_order_relaxed) > 0 && g_fail.fetch_sub(1) == 1) return hipErrorOutOfMemory;
  const hipError_t e = hipMalloc(p, bytes);
  if (e != hipSuccess || *p == nullptr) return e;
  try {
    Sizes& s = sizes();
    std::lock_guard<std::mutex> g(s.m);
    s.of[*p] = bytes;
  } catch (...) {
    (void)hipFree(*p);
    *p = nullptr;
    return hipErrorOutOfMemory;
  }
  g_bufs.fetch_add(1, std::memory_order_relaxed);
  g_bytes.fetch_add(bytes, std::memory_order_relaxed);
  return hipSuccess;
}

void dev_free(void* p) noexcept {
  if (p == nullptr) return;
  {
    Sizes& s = sizes();
    std::lock_guard<std::mutex> g(s.m);
    const auto it = s.of.find(p);
    if (it != s.of.end()) {
      g_bufs.fetch_sub(1, std::memory_order_relaxed);
      g_bytes.fetch_sub(it->second, std::memory_order_relaxed);
      s.of.erase(it);
    }
  }
  (void)hipFree(p);
}

hipError_t stream_create(hipStream_t* s, unsigned flags) noexcept {
  const hipError_t e = hipStreamCreateWithFlags(s, flags);
  if (e == hipSuccess) g_sync.fetch_add(1, std::memory_order_relaxed);
  return e;
}

void stream_destroy(hipStream_t s) noexcept {
  g_sync.fetch_sub(1, std::memory_order_relaxed);
  (void)hipStreamDestroy(s);
}

hipError_t event_create(hipEvent_t* e, unsigned flags) noexcept {
  const hipError_t r = hipEventCreateWithFlags(e, flags);
  if (r == hipSuccess) g_sync.fetch_add(1, std::memory_order_relaxed);
  return r;
}

void event_destroy(hipEvent_t e) noexcept {
  g_sync.fetch_sub(1, std::memory_order_relaxed);
  (void)hipEventDestroy(e);
}

void ipc_event_close(hipEvent_t e) noexcept { (void)hipEventDestroy(e); }

void device_live(size_t out[4]) noexcept {
  out[0] = g_bufs.load();
  out[1] = g_bytes.load();
  out[2] = g_sync.load();
  out[3] = g_mallocs.load();
}

void device_fail_alloc(int nth) noexcept { g_fail.store(nth > 0 ? nth : 0); }

}  // namespace anx
