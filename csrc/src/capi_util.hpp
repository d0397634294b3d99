// What the C-ABI translation units share (c_api.cpp, c_api_bf16.cpp, runtime/c_api_dist.cpp): failures become a
// nonzero status plus libanx's thread-local message (anx_set_last_error), so nothing unwinds across the ctypes
// boundary. Internal to csrc/src: not installed.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <exception>
#include <string>

#include "anx/c_api.h"

namespace anx {
namespace capi {

inline int fail(const std::string& m) {
  anx_set_last_error(m.c_str());
  return 1;
}
inline int hip_status(hipError_t e, const char* what) {
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
// s with its terminator into the caller's buffer of cap bytes; a buffer that cannot hold it all is refused
inline int put_string(const char* fn, const std::string& s, char* buf, size_t cap) {
  if (!buf || cap == 0) return fail(std::string(fn) + ": no buffer");
  if (s.size() + 1 > cap) return fail(std::string(fn) + ": buffer too small (" + std::to_string(s.size() + 1) + " bytes)");
  std::memcpy(buf, s.c_str(), s.size() + 1);
  return 0;
}

}  // namespace capi
}  // namespace anx
