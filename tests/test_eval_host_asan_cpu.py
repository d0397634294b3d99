"""The host definition of the evaluation head, cpu::softmax_eval, under AddressSanitizer and UBSan.

One stand-alone program with its own main, built from the host source (no device code, nothing loaded into Python)
with -fsanitize=address,undefined and run as its own process, as test_views_host_asan_cpu.py does. Every buffer has
exactly the size the function may touch, so a read or write one element outside is a sanitizer report; labels outside
the class range (INT_MIN among them) must index nothing.
"""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else shutil.which("clang++")
ROCM_INCLUDE = "/opt/rocm/include"  # anx/ops.hpp declares the HIP launchers next to the host functions

PROGRAM = r"""
#include <climits>
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

static uint32_t g_state = 4321u;
static uint32_t next() { return g_state = g_state * 1664525u + 1013904223u; }

// which: bit 0 rank, 1 nll, 2 pred, 3 stats, 4 confusion, 5 logits_out
static void eval(int N, int V, int K, int k, int ksplit, bool with_bias, int which) {
  const size_t M = static_cast<size_t>(N) * (V ? V : 1);
  std::vector<float> slabs(static_cast<size_t>(ksplit) * M * K), bias(with_bias ? K : 0);
  for (float& v : slabs) v = static_cast<float>(next() >> 8) / 16777216.0f * 8.0f - 4.0f;
  for (float& v : bias) v = static_cast<float>(next() >> 8) / 16777216.0f - 0.5f;
  std::vector<int> labels(N);
  for (int i = 0; i < N; ++i) labels[i] = static_cast<int>(next() >> 8) % K;
  if (N > 1) labels[1] = -1;
  if (N > 2) labels[2] = K;
  if (N > 3) labels[3] = INT_MIN;
  if (N > 4) labels[4] = INT_MAX;
  std::vector<int> rank(which & 1 ? N : 0, -7), pred(which & 4 ? N : 0, -7);
  std::vector<float> nll(which & 2 ? N : 0, -7.f), logits(which & 32 ? M * K : 0);
  std::vector<uint64_t> stats(which & 8 ? anx::cpu::kEvalStats : 0, 0);
  std::vector<uint32_t> conf(which & 16 ? static_cast<size_t>(K) * K : 0, 0);
  auto ptr = [](auto& v) { return v.empty() ? nullptr : v.data(); };
  anx::cpu::softmax_eval(slabs.data(), ksplit, M * K, with_bias ? bias.data() : nullptr, N, V, K, k, labels.data(),
                         ptr(rank), ptr(nll), ptr(pred), ptr(stats), ptr(conf), ptr(logits));
  int counted = 0;
  for (int i = 0; i < N; ++i) {
    const bool in = labels[i] >= 0 && labels[i] < K;
    counted += in;
    if (which & 1) EXPECT(in ? rank[i] >= 0 && rank[i] < K : rank[i] == -1);
    if (which & 2) EXPECT(in ? nll[i] >= 0.f : nll[i] == 0.f);
    if (which & 4) EXPECT(pred[i] >= 0 && pred[i] < K);
    if ((which & 5) == 5 && in) EXPECT((rank[i] == 0) == (pred[i] == labels[i]));
  }
  if (which & 8) {
    EXPECT(stats[anx::cpu::kEvalCount] == static_cast<uint64_t>(counted));
    EXPECT(stats[anx::cpu::kEvalTop1] <= stats[anx::cpu::kEvalTopK] && stats[anx::cpu::kEvalTopK] <= stats[0]);
    if (k == K) EXPECT(stats[anx::cpu::kEvalTopK] == stats[0]);
  }
  if (which & 16) {
    uint64_t sum = 0;
    for (uint32_t v : conf) sum += v;
    EXPECT(sum == static_cast<uint64_t>(counted));
  }
}

int main() {
  EXPECT(anx::cpu::eval_nll_q32(0.f) == 0 && anx::cpu::eval_nll_q32(1.f) == (1ull << 32));
  EXPECT(anx::cpu::eval_nll_q32(INFINITY) == (1ull << 42) && anx::cpu::eval_nll_q32(NAN) == (1ull << 42));
  EXPECT(anx::cpu::eval_nll_q32(-1.f) == 0 && anx::cpu::eval_nll_q32(-INFINITY) == 0);
  eval(6, 0, 37, 5, 2, true, 63);
  eval(6, 3, 37, 5, 2, true, 63);
  eval(1, 0, 1, 1, 1, false, 63);
  eval(1, 1, 1, 1, 1, false, 63);
  eval(7, 10, 1000, 16, 1, false, 1 | 8);     // rank and stats alone
  eval(7, 0, 1000, 16, 3, true, 2);           // the loss alone
  eval(5, 0, 16000, 16, 1, false, 4 | 32);    // more classes than the device form takes
  eval(2, 32, 9000, 5, 3, true, 63);
  eval(5, 2, 16, 16, 1, false, 8 | 16);       // k == K: every counted image is a top-k hit
  eval(0, 4, 10, 3, 1, false, 0);
  std::printf(g_fail ? "eval host: FAILED\n" : "eval host: OK\n");
  return g_fail ? 1 : 0;
}
"""


def test_evaluation_head_under_asan_ubsan(tmp_path):
    assert CXX, "no clang++ to build the stand-alone program with"
    assert os.path.isdir(ROCM_INCLUDE), "anx/ops.hpp needs the HIP headers"
    src = tmp_path / "eval_host_main.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "eval_host_main"
    cpu = os.path.join(ROOT, "csrc", "src", "cpu")
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
                        "-I", os.path.join(ROOT, "csrc", "include"), "-isystem", ROCM_INCLUDE, str(src),
                        os.path.join(cpu, "softmax_heads.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    text = r.stdout + r.stderr
    assert "Sanitizer" not in text and "runtime error" not in text, text[-4000:]
    assert r.returncode == 0 and "eval host: OK" in r.stdout, text[-3000:]
