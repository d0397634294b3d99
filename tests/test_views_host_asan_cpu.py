"""The two host definitions of the ten-view path under AddressSanitizer and UBSan: cpu::softmax_topk_views and the
flipped cpu::resize_crop_u8.

One stand-alone program with its own main, built from the two host sources (no device code, nothing loaded into
Python) with -fsanitize=address,undefined and run as its own process, as test_owned_cpu.py does. Every buffer has
exactly the size the functions may touch, so a read or write one element outside is a sanitizer report.
"""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else shutil.which("clang++")
ROCM_INCLUDE = "/opt/rocm/include"  # anx/ops.hpp declares the HIP launchers next to the host functions

PROGRAM = r"""
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "anx/ops.hpp"

static int g_fail = 0;
#define EXPECT(c)                                                        \
  do {                                                                   \
    if (!(c)) std::printf("FAIL line %d: %s\n", __LINE__, #c), ++g_fail; \
  } while (0)

static uint32_t g_state = 12345u;
static uint32_t next() { return g_state = g_state * 1664525u + 1013904223u; }

static void views(int N, int V, int K, int k, int ksplit, bool with_bias, bool with_outputs) {
  const size_t M = static_cast<size_t>(N) * V;
  std::vector<float> slabs(static_cast<size_t>(ksplit) * M * K), bias(with_bias ? K : 0);
  for (float& v : slabs) v = static_cast<float>(next() >> 8) / 16777216.0f * 8.0f - 4.0f;
  for (float& v : bias) v = static_cast<float>(next() >> 8) / 16777216.0f - 0.5f;
  std::vector<int> idx(static_cast<size_t>(N) * k, -1);
  std::vector<float> prob(static_cast<size_t>(N) * k, -1.f), probs(with_outputs ? static_cast<size_t>(N) * K : 0),
      logits(with_outputs ? M * K : 0);
  anx::cpu::softmax_topk_views(slabs.data(), ksplit, M * K, with_bias ? bias.data() : nullptr, N, V, K, k, idx.data(),
                               prob.data(), with_outputs ? probs.data() : nullptr, with_outputs ? logits.data() : nullptr);
  for (int i = 0; i < N; ++i) {
    for (int j = 0; j < k; ++j) {
      const int c = idx[static_cast<size_t>(i) * k + j];
      EXPECT(c >= 0 && c < K);
      for (int j2 = 0; j2 < j; ++j2) EXPECT(idx[static_cast<size_t>(i) * k + j2] != c);
      if (j) EXPECT(prob[static_cast<size_t>(i) * k + j] <= prob[static_cast<size_t>(i) * k + j - 1]);
      if (with_outputs) EXPECT(prob[static_cast<size_t>(i) * k + j] == probs[static_cast<size_t>(i) * K + c]);
    }
    if (with_outputs) {
      double sum = 0;
      for (int c = 0; c < K; ++c) sum += probs[static_cast<size_t>(i) * K + c];
      EXPECT(std::fabs(sum - 1.0) < 1e-4);
    }
  }
}

static void flipped(int H, int W, int OH, int OW, int y0h, int x0h, int bh, int bw, int pitch_extra) {
  const int64_t pitch = 3 * static_cast<int64_t>(W) + pitch_extra;
  // the last row ends at its last pixel: no slack behind the image
  std::vector<uint8_t> img(static_cast<size_t>(pitch) * (H - 1) + 3 * static_cast<size_t>(W));
  for (uint8_t& v : img) v = static_cast<uint8_t>(next() >> 24);
  const anx::ImageDesc d{img.data(), H, W, pitch, y0h, x0h, bh, bw};
  const anx::ImageDesc three[3] = {d, d, d};  // views of one source
  const uint8_t flags[3] = {1, 0, 7};         // any nonzero byte mirrors
  EXPECT(anx::resize_crop_check(three, 3, OH, OW) == nullptr);
  const size_t one = static_cast<size_t>(OH) * OW * 3;
  std::vector<uint8_t> out(3 * one, 0xAA), plain(3 * one, 0x55);
  anx::cpu::resize_crop_u8(three, flags, 3, out.data(), OH, OW);
  anx::cpu::resize_crop_u8(three, nullptr, 3, plain.data(), OH, OW);
  std::vector<uint8_t> old(3 * one, 0x11);
  anx::cpu::resize_crop_u8(three, 3, old.data(), OH, OW);
  EXPECT(old == plain);
  for (int oy = 0; oy < OH; ++oy)
    for (int ox = 0; ox < OW; ++ox)
      for (int c = 0; c < 3; ++c) {
        const size_t at = (static_cast<size_t>(oy) * OW + ox) * 3 + c;
        const size_t mirrored = (static_cast<size_t>(oy) * OW + (OW - 1 - ox)) * 3 + c;
        EXPECT(out[at] == plain[mirrored]);
        EXPECT(out[one + at] == plain[one + at]);
        EXPECT(out[2 * one + at] == plain[2 * one + mirrored]);
      }
}

int main() {
  views(2, 3, 37, 5, 2, true, true);
  views(1, 1, 1, 1, 1, false, true);
  views(3, 10, 1000, 16, 1, false, false);
  views(1, 32, 9000, 16, 3, true, true);  // more classes than the device form takes
  views(0, 4, 10, 3, 1, false, false);
  flipped(13, 17, 5, 7, 1, 3, 11, 14, 0);
  flipped(13, 17, 5, 1, 0, 2, 13, 16, 5);   // one column: its own mirror image
  flipped(9, 40, 3, 2, 2, 0, 8, 32, 1);     // a 16x box on two columns
  flipped(6, 5, 12, 11, 0, 0, 6, 5, 0);     // upsampling: taps clipped at the image's edges
  std::printf(g_fail ? "views host: FAILED\n" : "views host: OK\n");
  return g_fail ? 1 : 0;
}
"""


def test_view_head_and_flipped_resize_under_asan_ubsan(tmp_path):
    assert CXX, "no clang++ to build the stand-alone program with"
    assert os.path.isdir(ROCM_INCLUDE), "anx/ops.hpp needs the HIP headers"
    src = tmp_path / "views_host_main.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "views_host_main"
    cpu = os.path.join(ROOT, "csrc", "src", "cpu")
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
                        "-I", os.path.join(ROOT, "csrc", "include"), "-isystem", ROCM_INCLUDE, str(src),
                        os.path.join(cpu, "softmax_heads.cpp"), os.path.join(cpu, "resize_crop_u8.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    text = r.stdout + r.stderr
    assert "Sanitizer" not in text and "runtime error" not in text, text[-4000:]
    assert r.returncode == 0 and "views host: OK" in r.stdout, text[-3000:]
