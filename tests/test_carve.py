"""pptk_amd/csrc/scratch_carve.h on a CPU: tests/c/carve_check.cc, a program of
its own that includes the header and nothing of HIP, built with g++ under
ASan + UBSan and run (in the manner of tests/test_host_plan.py).

What the program checks, for a mixed list of element sizes 1, 2, 4, 8, 16 and
32 with zero counts among them, at alignments 16 and 256: the walk without a
base and the walk over a real block give the same offsets and total; every
pointer is aligned; writing every array in full stays inside a heap block of
exactly total() bytes."""
import os
import re
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "pptk_amd", "csrc")


def test_header_is_plain_cxx():
    """scratch_carve.h alone, with no ROCm include path."""
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-x", "c++", "-include", os.path.join(CSRC, "scratch_carve.h"),
                           os.devnull])
    with open(os.path.join(CSRC, "scratch_carve.h")) as f:
        assert not re.search(r"\bhip[A-Z_]|<hip/|__device__|__global__", f.read())


def test_carve_asan_ubsan(tmp_path):
    exe = str(tmp_path / "carve_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g",
                           "-I", CSRC, "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan",
                           os.path.join(ROOT, "tests", "c", "carve_check.cc"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "carve ok" in out.stdout, out.stdout + out.stderr
