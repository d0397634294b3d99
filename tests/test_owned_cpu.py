"""The move-only handle every device owner builds on (csrc/include/anx/owned.hpp), on the host alone.

One stand-alone program against anx/owned.hpp only (no HIP header), compiled with
-fsanitize=address,undefined and run as its own process: a counting fake Traits shows each rule of the
handle, and the sanitizers see the moves of a growing std::vector<Owned>.
"""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else shutil.which("clang++")

PROGRAM = r"""
#include <cstdio>
#include <utility>
#include <vector>

#include "anx/owned.hpp"

static int g_freed[64];  // frees per value
static int g_total = 0;
struct Fake {
  static int null() noexcept { return 0; }
  static void free(int v) noexcept { ++g_freed[v], ++g_total; }
};
using H = anx::Owned<int, Fake>;

static int g_fail = 0;
#define EXPECT(c)                                                  \
  do {                                                             \
    if (!(c)) std::printf("FAIL line %d: %s\n", __LINE__, #c), ++g_fail; \
  } while (0)

int main() {
  {  // default-empty: frees nothing
    H h;
    EXPECT(!h && h.get() == 0);
  }
  EXPECT(g_total == 0);
  {  // the destructor frees once
    H h(1);
    EXPECT(h && h.get() == 1);
  }
  EXPECT(g_freed[1] == 1 && g_total == 1);
  {  // a moved-from handle frees nothing
    H a(2);
    H b(std::move(a));
    EXPECT(!a && b.get() == 2 && g_freed[2] == 0);
  }
  EXPECT(g_freed[2] == 1 && g_total == 2);
  {  // move assignment over a live handle frees the old value exactly once
    H a(3), b(4);
    a = std::move(b);
    EXPECT(g_freed[3] == 1 && g_freed[4] == 0 && a.get() == 4 && !b);
  }
  EXPECT(g_freed[3] == 1 && g_freed[4] == 1 && g_total == 4);
  {  // self-move-assignment frees nothing and keeps the value
    H a(5);
    H& same = a;
    a = std::move(same);
    EXPECT(g_freed[5] == 0 && a.get() == 5);
  }
  EXPECT(g_freed[5] == 1 && g_total == 5);
  {  // release() frees nothing
    H a(6);
    EXPECT(a.release() == 6 && !a);
  }
  EXPECT(g_freed[6] == 0 && g_total == 5);
  {  // reset(v) frees the old value once; reset() empties
    H a(7);
    a.reset(8);
    EXPECT(g_freed[7] == 1 && g_freed[8] == 0 && a.get() == 8);
    a.reset();
    EXPECT(g_freed[8] == 1 && !a);
  }
  EXPECT(g_freed[7] == 1 && g_freed[8] == 1 && g_total == 7);
  {  // a vector that grows (reallocates, moving its handles) and is destroyed frees each value once
    std::vector<H> v;
    for (int i = 10; i < 50; ++i) v.emplace_back(i);
    EXPECT(g_total == 7);
    v.erase(v.begin());  // shifts the rest down by move assignment: 10 goes, once
    EXPECT(g_freed[10] == 1 && g_total == 8);
  }
  for (int i = 10; i < 50; ++i) EXPECT(g_freed[i] == 1);
  EXPECT(g_total == 7 + 40);
  std::printf(g_fail ? "owned: FAILED\n" : "owned: OK\n");
  return g_fail ? 1 : 0;
}
"""


def test_owned_handle_rules_under_asan_ubsan(tmp_path):
    assert CXX, "no clang++ to build the stand-alone program with"
    src = tmp_path / "owned_main.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "owned_main"
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-self-move",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "csrc", "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, env=env)
    text = r.stdout + r.stderr
    assert "Sanitizer" not in text and "runtime error" not in text, text[-4000:]
    assert r.returncode == 0 and "owned: OK" in r.stdout, text[-3000:]


def test_owned_header_needs_no_hip():
    text = open(os.path.join(ROOT, "csrc", "include", "anx", "owned.hpp")).read()
    assert "#include <hip" not in text and "hip_runtime" not in text
