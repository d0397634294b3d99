// anx/resize_taps.hpp — the integer tap weights of the antialiased resize + crop (cpu::resize_crop_u8 is the
// definition of the whole operation; this header is the one place its per-axis integers exist: the host function
// and the gfx950 kernel both call resize_axis_taps, which is why they agree bit for bit).
//
// One axis: n_in source pixels, n_out outputs, a box of b source pixels whose origin o0h is given in HALF pixels
// (0 <= o0h, o0h + 2b <= 2 n_in). For output o, in units of 1 / (2 n_out) source pixels:
//   S = 2 max(b, n_out)                      the triangle's half width (support 1 when enlarging, b / n_out when reducing)
//   c2 = n_out o0h + (2o + 1) b              the output's centre
//   D_j = 2 n_out j + n_out - c2             source pixel j's centre relative to it;  t_j = S - |D_j|
// The taps are the j in [0, n_in) with t_j > 0 (pixels outside the image are dropped, which renormalises the rest;
// pixels outside the box but inside the image are used). T = sum t_j, q_j = floor(t_j 2^15 / T), and the remainder
// 2^15 - sum q_j goes to the tap with the largest t_j (the lowest j among equals): sum q_j = 2^15 exactly.
// With real weights t_j / T this is torch's / PIL's antialiased bilinear filter (align_corners = false).
//
// Limits (resize_crop_check): n_in <= 16384, n_out <= 512, b <= 16 n_out. Then a tap row has at most
// ceil(2 max(b, n_out) / n_out) <= 32 entries (kResizeMaxTaps leaves room), and every product here fits 32 bits:
// n_out o0h <= 2^24, (2o + 1) b < 2^23, 2 n_out j < 2^24, t_j 2^15 <= 2^29.
#pragma once
#include <hip/hip_runtime.h>

namespace anx {

constexpr int kResizeMaxTaps = 34;
constexpr int kResizeMaxIn = 16384;  // source pixels per axis
constexpr int kResizeMaxOut = 512;   // outputs per axis
constexpr int kResizeMaxScale = 16;  // b <= kResizeMaxScale * n_out

// Upper bound of the taps of any output of an axis with box b (what a caller sizes a weight row with).
__host__ __device__ inline int resize_taps_bound(int n_out, int b) {
  const int m = b > n_out ? b : n_out;
  const int n = (2 * m + n_out - 1) / n_out + 1;
  return n < kResizeMaxTaps ? n : kResizeMaxTaps;
}

// The taps of output o: *j0 = the first source index, returns their number (>= 1 for a box inside the image).
__host__ __device__ inline int resize_tap_range(int n_in, int n_out, int o0h, int b, int o, int* j0) {
  const int S = 2 * (b > n_out ? b : n_out);
  const int c2 = n_out * o0h + (2 * o + 1) * b;
  const int d = 2 * n_out;
  // t_j > 0  <=>  lo < d j < hi
  const int lo = c2 - n_out - S, hi = c2 - n_out + S;  // hi >= 1 + n_out
  const int ja = lo < 0 ? 0 : lo / d + 1;
  int jb = (hi - 1) / d;
  if (jb > n_in - 1) jb = n_in - 1;
  *j0 = ja;
  return jb - ja + 1;
}

// The tap weights of output o into q[0 .. n) (any integer type holding 0 .. 32768), n <= cap taps; returns n.
template <class Q>
__host__ __device__ inline int resize_axis_taps(int n_in, int n_out, int o0h, int b, int o, int cap, int* j0, Q* q) {
  int n = resize_tap_range(n_in, n_out, o0h, b, o, j0);
  if (n > cap) n = cap;  // never for cap >= resize_taps_bound: keeps a caller's row in bounds whatever it passed
  const int S = 2 * (b > n_out ? b : n_out);
  const int d = 2 * n_out;
  const int D0 = d * *j0 + n_out - (n_out * o0h + (2 * o + 1) * b);
  unsigned T = 0;
  int best = 0, tbest = 0;
  for (int k = 0; k < n; ++k) {
    const int D = D0 + d * k;
    const int t = S - (D < 0 ? -D : D);
    T += static_cast<unsigned>(t);
    if (t > tbest) {
      tbest = t;
      best = k;
    }
  }
  if (n < 1 || T == 0) return 0;  // a box outside the image: rejected before any caller gets here
  unsigned sum = 0;
  for (int k = 0; k < n; ++k) {
    const int D = D0 + d * k;
    const unsigned t = static_cast<unsigned>(S - (D < 0 ? -D : D));
    const unsigned qk = (t << 15) / T;
    q[k] = static_cast<Q>(qk);
    sum += qk;
  }
  q[best] = static_cast<Q>(static_cast<unsigned>(q[best]) + (32768u - sum));
  return n;
}

}  // namespace anx
