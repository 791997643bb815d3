"""pptk_amd/csrc/host_plan.h on a CPU: tests/c/host_plan_check.cc, a program of
its own that includes the header and nothing of HIP, built with g++ and run
twice -- under ASan + UBSan, and under ThreadSanitizer (the worker pool's
generations and the staged parts' running totals).

What the program checks: a staged one-part chunk (lengths from 0 to 1500, a
frame without data, a frame over max_frame; offsets, bytes, zero padding,
with and without non-temporal gather) in exactly-sized heap staging; 8 192
frames over a pool of four against the one-thread run, 50 times; ring chunks'
uniformity at 64 frames on one thread and 16 384 over the pool (in order,
swapped, irregular pitch, one odd length, one frame, a stride that breaks at a
part's first frame and inside a part, a last part at twice the pitch) with the
descriptors written only when needed; the ring's bounds; and plan_transport's
truth table, each row written from the enqueue_chunk of the commit before the
split."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "pptk_amd", "csrc")
BASE = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g", "-pthread", "-I", CSRC]

TSAN_PROBE = """#include <thread>
int x;
int main() {
  std::thread t([] { x = 1; });
  t.join();
  return x - 1;
}
"""


def build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(BASE + flags + [os.path.join(ROOT, "tests", "c", "host_plan_check.cc"),
                                          "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "host_plan ok" in out.stdout, out.stdout + out.stderr


def test_header_is_plain_cxx():
    """host_plan.h alone, with no ROCm include path."""
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-x", "c++", "-include", os.path.join(CSRC, "host_plan.h"),
                           os.devnull])
    with open(os.path.join(CSRC, "host_plan.h")) as f:
        assert not re.search(r"\bhip[A-Z_]|<hip/|__device__|__global__", f.read())


def test_host_plan_asan_ubsan(tmp_path):
    build_and_run(tmp_path, "host_plan_asan",
                  ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                   "-static-libasan", "-static-libubsan"])


def test_host_plan_tsan(tmp_path):
    flags = ["-fsanitize=thread", "-static-libtsan"]
    src = tmp_path / "probe.cc"
    src.write_text(TSAN_PROBE)
    probe = str(tmp_path / "probe")
    subprocess.check_call(BASE + flags + [str(src), "-o", probe])
    p = subprocess.run([probe], capture_output=True, text=True, timeout=60)
    if p.returncode != 0:
        pytest.skip("ThreadSanitizer's runtime cannot start a threaded program here: "
                    + (p.stderr.strip().splitlines() or ["exit %d" % p.returncode])[0])
    build_and_run(tmp_path, "host_plan_tsan", flags)
