// Antialiased resize + crop of byte images: a batch of images of different sizes, each with its own box, onto
// OH x OW x 3 byte outputs in one launch (cpu::resize_crop_u8 is the definition; this kernel writes the same
// bytes, because every tap weight comes from the same integer function, anx/resize_taps.hpp).
//
// One workgroup = one image x one band of R output rows. It computes its own tap weights into LDS (the OW
// horizontal rows and the band's R vertical rows; no table is uploaded), then STREAMS the band's source rows:
// G rows at a time are staged in LDS with 16-B loads (a source row starts at any byte address: the bytes before
// the first 16-B boundary and after the last whole unit are single-byte loads, as in decode_u8.hip; row g sits at
// its global address mod 16, so the LDS stores are aligned too), each thread resamples its NI output elements
// (ox, c) of a staged row horizontally in registers (16-bit intermediate) and adds the result, times the vertical
// weight, into the accumulators of the band rows that row feeds. The band's source-row span grows with the scale
// (about 290 rows for 16 output rows at 16x), which is why rows are streamed and the R x NI vertical accumulators
// live in registers: LDS holds only G source rows, whatever the scale. The band's output (R x 3 OW contiguous
// bytes, from any byte address) is assembled in the staging area and leaves as 16-B stores with a byte head / tail.
// A launch may carry one flag byte per output: a flagged output is mirrored (columns reversed), which only changes
// where its bytes land in that assembly; several outputs may name one source image (the ten views of an image).
//
// The reference has no resampling stage: its programs fill float arrays (v1_serial/src/main.cpp:18-43).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "anx/ops.hpp"
#include "anx/resize_taps.hpp"

namespace anx::hip {
namespace {

using u32x4 = __attribute__((ext_vector_type(4))) unsigned;
constexpr int kThreads = 256;
constexpr int kMaxStageRows = 8;              // G: source rows staged per step
constexpr unsigned kStageTarget = 16 * 1024;  // bytes of staged source rows aimed at (G = target / row pitch)
constexpr unsigned kMaxLds = 64 * 1024;
constexpr int kRegTaps = 4;  // horizontal tap rows of at most this many entries live in registers (boxes up to 1.5x)

constexpr unsigned up16(unsigned v) { return (v + 15u) & ~15u; }
// bytes of the tap tables behind the staging area: vq [R][kResizeMaxTaps] u16, vj0 [R], vn [R] int (76 R: a
// multiple of 16 for R = 8, 16), hq [OW][TS] u16, hj0 [OW] u16, hn [OW] u8
constexpr unsigned v_bytes(int R) { return static_cast<unsigned>(R) * (2 * kResizeMaxTaps + 8); }
unsigned table_bytes(int R, int OW, int TS) {
  return v_bytes(R) + static_cast<unsigned>(OW) * (2 * TS + 2) + up16(OW);
}

// Copy len bytes src -> dst, both at a0 mod 16 (one of them global memory, the other LDS placed to match): whole
// 16-B units as vectors, the rest as bytes. li / ls: this thread's index and the number of threads sharing the copy.
__device__ __forceinline__ void copy_bytes(uint8_t* dst, const uint8_t* src, unsigned a0, unsigned len, unsigned li,
                                           unsigned ls) {
  unsigned head = (16u - a0) & 15u;
  if (head > len) head = len;
  const unsigned units = (len - head) >> 4;
  for (unsigned u = li; u < units; u += ls)
    *reinterpret_cast<u32x4*>(dst + head + 16 * u) = *reinterpret_cast<const u32x4*>(src + head + 16 * u);
  const unsigned tail0 = head + 16 * units;
  if (li < head) dst[li] = src[li];
  if (li < len - tail0) dst[tail0 + li] = src[tail0 + li];  // at most 15 bytes each: ls >= 64 covers them
}

// NI: output elements (ox, c) per thread, element e = thread + i * kThreads; R: output rows per band.
// KT > 0: no horizontal tap row of the launch has more than KT entries (TS <= KT), so each thread keeps its elements'
// weights in registers, padded with zeros to KT, and the horizontal pass is KT independent loads and multiply-adds
// (a padded tap reads at most 9 bytes past its staged row, inside this workgroup's LDS, times zero); KT = 0: the
// weights stay in LDS and the pass loops over each element's own tap count.
// G source rows of LP bytes are staged per step; TS: entries per horizontal tap row; stage: bytes of the staging area.
// Flip: empty, or one `const uint8_t*`, the launch's flag bytes (flip[img] != 0: a mirrored output). With the pack
// empty the kernel has no such parameter and no code for it.
template <int NI, int R, int KT, class... Flip>
__global__ void __launch_bounds__(kThreads) resize_crop_u8_kernel(const ImageDesc* __restrict__ descs,
                                                                  uint8_t* __restrict__ out, int OH, int OW, int bands,
                                                                  int G, int LP, int TS, unsigned stage, Flip... flip) {
  static_assert(sizeof...(Flip) <= 1, "at most one flag array");
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  uint16_t* vq = reinterpret_cast<uint16_t*>(lds + stage);
  int* vj0 = reinterpret_cast<int*>(vq + R * kResizeMaxTaps);
  int* vn = vj0 + R;
  uint16_t* hq = reinterpret_cast<uint16_t*>(vn + R);
  uint16_t* hj0 = hq + OW * TS;
  uint8_t* hn = reinterpret_cast<uint8_t*>(hj0 + OW);

  const int t = threadIdx.x;
  const int img = blockIdx.x / bands, band = blockIdx.x - img * bands;
  const ImageDesc d = descs[img];
  const int OW3 = 3 * OW;
  const int oy0 = band * R;
  const int rows = OH - oy0 < R ? OH - oy0 : R;

  // tap weights: one output index per thread; the band's vertical rows on the last threads
  for (int o = t; o < OW; o += kThreads) {
    int j0 = 0;
    const int n = resize_axis_taps(d.W, OW, d.x0h, d.bw, o, TS, &j0, hq + o * TS);
    hj0[o] = static_cast<uint16_t>(j0);
    hn[o] = static_cast<uint8_t>(n);
  }
  if (t >= kThreads - R) {
    const int r = kThreads - 1 - t;
    int j0 = 0, n = 0;
    if (r < rows) n = resize_axis_taps(d.H, OH, d.y0h, d.bh, oy0 + r, kResizeMaxTaps, &j0, vq + r * kResizeMaxTaps);
    vj0[r] = j0;
    vn[r] = n;
  }
  __syncthreads();

  const int xa = hj0[0], xb = hj0[OW - 1] + hn[OW - 1];  // source columns any output reads
  const unsigned len = 3u * static_cast<unsigned>(xb - xa);
  // the launcher sized LP from the same function; a mismatch must not become an out-of-bounds LDS write
  if (xb <= xa || len + 15u > static_cast<unsigned>(LP)) return;

  int sj0[R], sn[R];  // wave-uniform: kept in scalar registers
#pragma unroll
  for (int r = 0; r < R; ++r) {
    sj0[r] = __builtin_amdgcn_readfirstlane(vj0[r]);
    sn[r] = __builtin_amdgcn_readfirstlane(vn[r]);
  }
  const int ya = sj0[0];
  int yb = ya;
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (r < rows) yb = sj0[r] + sn[r];

  int base[NI], nk[NI], qo[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int e = t + i * kThreads;
    const int ox = e < OW3 ? e / 3 : 0;
    base[i] = (hj0[ox] - xa) * 3 + (e - 3 * ox);
    nk[i] = e < OW3 ? hn[ox] : 0;
    qo[i] = ox * TS;
    if (e >= OW3) base[i] = 0;
  }
  unsigned wq[NI][KT > 0 ? KT : 1];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int k = 0; k < (KT > 0 ? KT : 1); ++k) wq[i][k] = KT > 0 && k < nk[i] ? hq[qo[i] + k] : 0u;
  unsigned acc[NI][R];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int r = 0; r < R; ++r) acc[i][r] = 0;

  const uint8_t* src0 = d.ptr + 3 * static_cast<int64_t>(xa);
  const bool per_wave = G >= 4;  // a wave per staged row, or (few wide rows) all threads on each row
  const unsigned li = per_wave ? (t & 63) : t, ls = per_wave ? 64 : kThreads;
  for (int y = ya; y < yb; y += G) {
    const int gc = yb - y < G ? yb - y : G;
    for (int g = per_wave ? (t >> 6) : 0; g < gc; g += per_wave ? 4 : 1) {
      const uint8_t* p = src0 + static_cast<int64_t>(y + g) * d.pitch;
      const unsigned a0 = static_cast<unsigned>(reinterpret_cast<uintptr_t>(p) & 15u);
      copy_bytes(lds + g * LP + a0, p, a0, len, li, ls);
    }
    __syncthreads();
    for (int g = 0; g < gc; ++g) {
      const int yy = y + g;
      const uint8_t* row = lds + g * LP + (reinterpret_cast<uintptr_t>(src0 + static_cast<int64_t>(yy) * d.pitch) & 15u);
      unsigned h[NI];
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        unsigned s = 0;
        if constexpr (KT > 0) {
#pragma unroll
          for (int k = 0; k < KT; ++k) s += wq[i][k] * row[base[i] + 3 * k];
        } else {
          for (int k = 0; k < nk[i]; ++k) s += static_cast<unsigned>(hq[qo[i] + k]) * row[base[i] + 3 * k];
        }
        h[i] = (s + 64u) >> 7;
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const unsigned dd = static_cast<unsigned>(yy - sj0[r]);
        if (dd < static_cast<unsigned>(sn[r])) {  // rows past the band have sn = 0
          const unsigned w = vq[r * kResizeMaxTaps + dd];
#pragma unroll
          for (int i = 0; i < NI; ++i) acc[i][r] += w * h[i];
        }
      }
    }
    __syncthreads();  // the staged rows are free again (and, after the last step, the staging area is)
  }

  // the band's bytes, assembled at their global address mod 16, then stored wide. A mirrored output (the flag is
  // uniform over the workgroup) differs only here: element (ox, c) lands at column OW - 1 - ox.
  uint8_t* op = out + (static_cast<size_t>(img) * OH + oy0) * OW3;
  const unsigned o0 = static_cast<unsigned>(reinterpret_cast<uintptr_t>(op) & 15u);
  uint8_t* so = lds + o0;
  if constexpr (sizeof...(Flip) == 0) {
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int e = t + i * kThreads;
      if (e < OW3) {
#pragma unroll
        for (int r = 0; r < R; ++r)
          if (r < rows) so[r * OW3 + e] = static_cast<uint8_t>((acc[i][r] + (1u << 22)) >> 23);
      }
    }
  } else {
    const uint8_t* const flags = (flip, ...);
    const bool mirror = flags[img] != 0;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int e = t + i * kThreads;
      if (e < OW3) {
        const int ox = e / 3;
        const int at = mirror ? 3 * (OW - 1 - ox) + (e - 3 * ox) : e;
#pragma unroll
        for (int r = 0; r < R; ++r)
          if (r < rows) so[r * OW3 + at] = static_cast<uint8_t>((acc[i][r] + (1u << 22)) >> 23);
      }
    }
  }
  __syncthreads();
  copy_bytes(op, so, o0, static_cast<unsigned>(rows * OW3), t, kThreads);
}

}  // namespace

hipError_t resize_crop_u8(const ImageDesc* dev, const ImageDesc* host, int n, uint8_t* out, int OH, int OW,
                          hipStream_t s) {
  return resize_crop_u8(dev, host, nullptr, nullptr, n, out, OH, OW, s);
}

hipError_t resize_crop_u8(const ImageDesc* dev, const ImageDesc* host, const uint8_t* flip_dev, const uint8_t* flip_host,
                          int n, uint8_t* out, int OH, int OW, hipStream_t s) {
  if (resize_crop_check(host, n, OH, OW)) return hipErrorInvalidValue;
  if ((flip_dev == nullptr) != (flip_host == nullptr)) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (!dev || !out) return hipErrorInvalidValue;
  const int OW3 = 3 * OW;
  const int ni = (OW3 + kThreads - 1) / kThreads;  // 1 .. 6
  const int R = ni <= 3 ? 16 : 8;
  int span = 1, bmax = 1;  // the widest source-column span of any image, the widest box
  for (int i = 0; i < n; ++i) {
    int ja = 0, jb = 0;
    resize_tap_range(host[i].W, OW, host[i].x0h, host[i].bw, 0, &ja);
    const int nb = resize_tap_range(host[i].W, OW, host[i].x0h, host[i].bw, OW - 1, &jb);
    if (jb + nb - ja > span) span = jb + nb - ja;
    if (host[i].bw > bmax) bmax = host[i].bw;
  }
  const int TS = resize_taps_bound(OW, bmax);
  const unsigned LP = up16(3u * span + 15u);
  unsigned G = kStageTarget / LP;
  G = G < 1 ? 1 : G > kMaxStageRows ? kMaxStageRows : G;
  const unsigned out_stage = up16(static_cast<unsigned>(R) * OW3 + 15u);
  const unsigned stage = G * LP > out_stage ? G * LP : out_stage;
  const unsigned lds = stage + table_bytes(R, OW, TS);
  // the limits bound it: at OW = 512 and a 16x box, one staged row of 3 (8192 + 33) + 15 bytes rounded up to 16
  // (24704) + v_bytes(8) (608) + 512 (2 * 33 + 2) + 512 = 60640 bytes
  if (lds > kMaxLds) return hipErrorInvalidValue;
  const int bands = (OH + R - 1) / R;
  const long long grid = static_cast<long long>(bands) * n;
  if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 g(static_cast<unsigned>(grid));
#define ANX_RC_KERNEL(NI_, R_, KT_)                                                                              \
  do {                                                                                                           \
    if (flip_dev)                                                                                                \
      resize_crop_u8_kernel<NI_, R_, KT_, const uint8_t*><<<g, kThreads, lds, s>>>(                              \
          dev, out, OH, OW, bands, static_cast<int>(G), static_cast<int>(LP), TS, stage, flip_dev);              \
    else                                                                                                         \
      resize_crop_u8_kernel<NI_, R_, KT_><<<g, kThreads, lds, s>>>(dev, out, OH, OW, bands, static_cast<int>(G), \
                                                                    static_cast<int>(LP), TS, stage);            \
  } while (0)
#define ANX_RC_LAUNCH(NI_, R_)          \
  do {                                  \
    if (TS <= kRegTaps)                 \
      ANX_RC_KERNEL(NI_, R_, kRegTaps); \
    else                                \
      ANX_RC_KERNEL(NI_, R_, 0);        \
  } while (0)
  if (ni <= 1)
    ANX_RC_LAUNCH(1, 16);
  else if (ni == 2)
    ANX_RC_LAUNCH(2, 16);
  else if (ni == 3)
    ANX_RC_LAUNCH(3, 16);
  else
    ANX_RC_LAUNCH(6, 8);
#undef ANX_RC_LAUNCH
#undef ANX_RC_KERNEL
  return hipGetLastError();
}

}  // namespace anx::hip
