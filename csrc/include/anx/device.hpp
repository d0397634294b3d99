// anx/device.hpp — owners of device buffers, streams and events (Owned handles, anx/owned.hpp).
//
// Two forms of allocation: construction paths throw (DevBuf<T>(n), DevBuf<T>::upload), the paths that
// return hipError_t from a forward do not (try_alloc). Both go through dev_malloc, which lives in libanx
// (csrc/src/device.cpp) with stream / event creation, so every library and program of the project shares
// one set of counters and one failure hook (anx_device_live / anx_device_fail_alloc, anx/c_api.h).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <stdexcept>
#include <string>
#include <vector>

#include "anx/owned.hpp"
#include "anx/upload.hpp"

#define ANX_TRY(expr)                \
  do {                               \
    hipError_t _e = (expr);          \
    if (_e != hipSuccess) return _e; \
  } while (0)

namespace anx {

inline void hip_check(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

// The out-of-line primitives (hipMalloc / hipFree, hipStreamCreateWithFlags / hipStreamDestroy,
// hipEventCreateWithFlags / hipEventDestroy) behind the process-wide counters.
hipError_t dev_malloc(void** p, size_t bytes) noexcept;
void dev_free(void* p) noexcept;
hipError_t stream_create(hipStream_t* s, unsigned flags) noexcept;
void stream_destroy(hipStream_t s) noexcept;
hipError_t event_create(hipEvent_t* e, unsigned flags) noexcept;
void event_destroy(hipEvent_t e) noexcept;
// An event opened with hipIpcOpenEventHandle: another process's, so outside the counters.
void ipc_event_close(hipEvent_t e) noexcept;
// live device buffers, live device bytes, live streams + events, cumulative dev_malloc calls
void device_live(size_t out[4]) noexcept;
// Test hook: the nth next dev_malloc call (1-based) returns hipErrorOutOfMemory without calling HIP, then
// the hook disarms itself; 0 disarms.
void device_fail_alloc(int nth) noexcept;

struct DevFree {
  static void* null() noexcept { return nullptr; }
  static void free(void* p) noexcept { dev_free(p); }
};
struct StreamFree {
  static hipStream_t null() noexcept { return nullptr; }
  static void free(hipStream_t s) noexcept { stream_destroy(s); }
};
struct EventFree {
  static hipEvent_t null() noexcept { return nullptr; }
  static void free(hipEvent_t e) noexcept { event_destroy(e); }
};

// A typed device allocation of max(n * sizeof(T), min_bytes) bytes.
template <class T>
class DevBuf {
 public:
  DevBuf() noexcept = default;
  explicit DevBuf(size_t n, size_t min_bytes = sizeof(T)) { hip_check(try_alloc(n, min_bytes), "hipMalloc"); }
  // h in device memory, through the pinned staging buffer (anx/upload.hpp)
  static DevBuf upload(const std::vector<T>& h, size_t min_bytes = sizeof(T)) {
    DevBuf d(h.size(), min_bytes);
    hip_check(upload_h2d(d.get(), h.data(), h.size() * sizeof(T)), "upload H2D");
    return d;
  }
  // Throws nothing. The buffer held before is freed once the new one exists and is kept on failure.
  hipError_t try_alloc(size_t n, size_t min_bytes = sizeof(T)) noexcept {
    void* p = nullptr;
    const hipError_t e = dev_malloc(&p, std::max(n * sizeof(T), min_bytes));
    if (e == hipSuccess) p_.reset(p);
    return e;
  }
  T* get() const noexcept { return static_cast<T*>(p_.get()); }
  explicit operator bool() const noexcept { return static_cast<bool>(p_); }
  void reset() noexcept { p_.reset(); }

 private:
  Owned<void*, DevFree> p_;
};

// Streams are created non-blocking; events with the flags the call site passes.
class HipStream {
 public:
  HipStream() noexcept = default;
  static HipStream create() {
    HipStream s;
    hip_check(s.try_create(), "hipStreamCreate");
    return s;
  }
  hipError_t try_create() noexcept {
    hipStream_t s = nullptr;
    const hipError_t e = stream_create(&s, hipStreamNonBlocking);
    if (e == hipSuccess) s_.reset(s);
    return e;
  }
  hipStream_t get() const noexcept { return s_.get(); }
  operator hipStream_t() const noexcept { return s_.get(); }  // passes as the raw handle to HIP calls and launches
  explicit operator bool() const noexcept { return static_cast<bool>(s_); }
  void reset() noexcept { s_.reset(); }

 private:
  Owned<hipStream_t, StreamFree> s_;
};

class HipEvent {
 public:
  HipEvent() noexcept = default;
  static HipEvent create(unsigned flags, const char* what = "hipEventCreate") {
    HipEvent e;
    hip_check(e.try_create(flags), what);
    return e;
  }
  hipError_t try_create(unsigned flags) noexcept {
    hipEvent_t e = nullptr;
    const hipError_t r = event_create(&e, flags);
    if (r == hipSuccess) e_.reset(e);
    return r;
  }
  hipEvent_t get() const noexcept { return e_.get(); }
  operator hipEvent_t() const noexcept { return e_.get(); }
  explicit operator bool() const noexcept { return static_cast<bool>(e_); }
  void reset() noexcept { e_.reset(); }

 private:
  Owned<hipEvent_t, EventFree> e_;
};

}  // namespace anx
