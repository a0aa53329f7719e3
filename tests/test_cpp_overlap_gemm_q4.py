"""wg_gemm_q4's aliasing rule under the host sanitizers: tests/cpp/overlap_gemm_q4_check.cpp links wgmath_amd/csrc/views_overlap.hip ALONE -- no device, nothing else of
the library -- and compares the three predicates the call asks (`out` against `m` in 1-byte units, against `scales`, against `x` in 2-byte units) with a brute-force
intersection of the byte sets on the layout tests/test_gpu_gemm_q4.py::test_aliasing uses."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "_build", "overlap_gemm_q4_check")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SAN = "-fsanitize=address,undefined"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")
def test_gemm_q4_predicates_alone_under_host_sanitizers():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    csrc = os.path.join(ROOT, "wgmath_amd", "csrc")
    # (host side only -- the unit has no kernel: the sanitizers are the host compiler's and nothing of this ever runs on a device)
    subprocess.run([HIPCC, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "--offload-arch=gfx950", "--cuda-host-only",
                    SAN, "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                    os.path.join(csrc, "views_overlap.hip"), os.path.join(ROOT, "tests", "cpp", "overlap_gemm_q4_check.cpp"), "-o", EXE], check=True)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OVERLAP GEMM Q4 OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
