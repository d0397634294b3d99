// cpu::resize_crop_u8 — the definition of the antialiased resize + crop of byte images (anx/ops.hpp), and the
// limit check both the host function's and the kernel's callers run first. All integer: the tap weights come
// from anx/resize_taps.hpp, the one place they are computed for the host and the gfx950 kernel alike.
#include <cstdint>
#include <vector>

#include "anx/ops.hpp"
#include "anx/resize_taps.hpp"

namespace anx {

const char* resize_crop_check(const ImageDesc* d, int n, int OH, int OW) {
  if (OH < 1 || OW < 1 || OH > kResizeMaxOut || OW > kResizeMaxOut) return "output size outside 1 .. 512";
  if (n < 0 || (n > 0 && !d)) return "no descriptors";
  for (int i = 0; i < n; ++i) {
    const ImageDesc& e = d[i];
    if (!e.ptr) return "null image pointer";
    if (e.H < 1 || e.W < 1 || e.H > kResizeMaxIn || e.W > kResizeMaxIn) return "image size outside 1 .. 16384";
    if (e.pitch < 3 * static_cast<int64_t>(e.W)) return "row pitch below 3 W bytes";
    if (e.bh < 1 || e.bw < 1) return "empty box";
    // bh, bw <= 16384 first: the sums below then fit an int
    if (e.bh > e.H || e.bw > e.W || e.y0h < 0 || e.x0h < 0 || e.y0h > 2 * e.H || e.x0h > 2 * e.W ||
        e.y0h + 2 * e.bh > 2 * e.H || e.x0h + 2 * e.bw > 2 * e.W)
      return "box outside the image";
    if (e.bh > kResizeMaxScale * OH || e.bw > kResizeMaxScale * OW) return "box more than 16 times the output";
  }
  return nullptr;
}

namespace cpu {

namespace {
struct Axis {
  std::vector<int> j0, n;
  std::vector<uint16_t> q;  // [n_out][kResizeMaxTaps]
  Axis(int n_in, int n_out, int o0h, int b) : j0(n_out), n(n_out), q(static_cast<size_t>(n_out) * kResizeMaxTaps) {
    for (int o = 0; o < n_out; ++o)
      n[o] = resize_axis_taps(n_in, n_out, o0h, b, o, kResizeMaxTaps, &j0[o], &q[static_cast<size_t>(o) * kResizeMaxTaps]);
  }
};
}  // namespace

void resize_crop_u8(const ImageDesc* d, int n, uint8_t* out, int OH, int OW) {
  resize_crop_u8(d, nullptr, n, out, OH, OW);
}

void resize_crop_u8(const ImageDesc* d, const uint8_t* flip, int n, uint8_t* out, int OH, int OW) {
  const size_t row = static_cast<size_t>(OW) * 3;
  std::vector<uint16_t> h;
  for (int i = 0; i < n; ++i) {
    const ImageDesc& e = d[i];
    const Axis ax(e.W, OW, e.x0h, e.bw), ay(e.H, OH, e.y0h, e.bh);
    const int ya = ay.j0[0], yb = ay.j0[OH - 1] + ay.n[OH - 1];  // the source rows any output row reads
    h.assign(static_cast<size_t>(yb - ya) * row, 0);
    for (int y = ya; y < yb; ++y) {
      const uint8_t* src = e.ptr + static_cast<int64_t>(y) * e.pitch;
      uint16_t* hr = &h[static_cast<size_t>(y - ya) * row];
      for (int ox = 0; ox < OW; ++ox) {
        const uint16_t* q = &ax.q[static_cast<size_t>(ox) * kResizeMaxTaps];
        const uint8_t* p = src + 3 * static_cast<size_t>(ax.j0[ox]);
        uint32_t s0 = 0, s1 = 0, s2 = 0;
        for (int k = 0; k < ax.n[ox]; ++k) {
          s0 += q[k] * static_cast<uint32_t>(p[3 * k]);
          s1 += q[k] * static_cast<uint32_t>(p[3 * k + 1]);
          s2 += q[k] * static_cast<uint32_t>(p[3 * k + 2]);
        }
        hr[3 * ox] = static_cast<uint16_t>((s0 + 64) >> 7);
        hr[3 * ox + 1] = static_cast<uint16_t>((s1 + 64) >> 7);
        hr[3 * ox + 2] = static_cast<uint16_t>((s2 + 64) >> 7);
      }
    }
    uint8_t* o = out + static_cast<size_t>(i) * OH * row;
    const bool mirror = flip && flip[i];
    for (int oy = 0; oy < OH; ++oy) {
      const uint16_t* q = &ay.q[static_cast<size_t>(oy) * kResizeMaxTaps];
      const uint16_t* h0 = &h[static_cast<size_t>(ay.j0[oy] - ya) * row];
      for (size_t el = 0; el < row; ++el) {
        uint32_t s = 0;
        for (int k = 0; k < ay.n[oy]; ++k) s += q[k] * static_cast<uint32_t>(h0[k * row + el]);
        // a mirrored output: column OW - 1 - ox, same channel
        const size_t at = mirror ? row - 3 - 3 * (el / 3) + el % 3 : el;
        o[oy * row + at] = static_cast<uint8_t>((s + (1u << 22)) >> 23);
      }
    }
  }
}

}  // namespace cpu
}  // namespace anx
