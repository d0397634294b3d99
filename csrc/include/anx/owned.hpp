// anx/owned.hpp — a move-only handle over one value that must be freed exactly once.
//
// Traits::null() is the empty value; Traits::free(T) releases a non-null one and is noexcept. Nothing here
// allocates or shares: the typed owners (device buffers, streams, events: anx/device.hpp) build on it.
// No HIP include, so the handle's own rules are testable on any host.
#pragma once
#include <utility>

namespace anx {

template <class T, class Traits>
class Owned {
 public:
  Owned() noexcept : v_(Traits::null()) {}
  explicit Owned(T v) noexcept : v_(v) {}
  Owned(Owned&& o) noexcept : v_(o.release()) {}
  Owned& operator=(Owned&& o) noexcept {
    if (this != &o) reset(o.release());
    return *this;
  }
  Owned(const Owned&) = delete;
  Owned& operator=(const Owned&) = delete;
  ~Owned() { reset(); }

  T get() const noexcept { return v_; }
  explicit operator bool() const noexcept { return v_ != Traits::null(); }
  // Gives the value up without freeing it.
  T release() noexcept { return std::exchange(v_, Traits::null()); }
  // Frees the held value (if any) and takes v.
  void reset(T v = Traits::null()) noexcept {
    const T old = std::exchange(v_, v);
    if (old != Traits::null()) Traits::free(old);
  }

 private:
  T v_;
};

}  // namespace anx
