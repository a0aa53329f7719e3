"""wg_gemm_q8a8's planner under the host sanitizers: tests/cpp/gemm_q8a8_plan_check.cpp links wgmath_amd/csrc/gemm_q8a8_plan.hip ALONE -- the planner needs nothing else of
the library, and no device -- with AddressSanitizer and UndefinedBehaviorSanitizer on the host side, and runs the invariant sweep of
tests/test_gemm_q8a8_plan_host.py on the CPU, sizes next to 2^32 included."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "_build", "gemm_q8a8_plan_check")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SAN = "-fsanitize=address,undefined,float-cast-overflow"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")
def test_planner_alone_under_host_sanitizers():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    csrc = os.path.join(ROOT, "wgmath_amd", "csrc")
    # (host side only -- the unit has no kernel: the sanitizers are the host compiler's and nothing of this ever runs on a device)
    subprocess.run([HIPCC, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "--offload-arch=gfx950", "--cuda-host-only",
                    SAN, "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                    os.path.join(csrc, "gemm_q8a8_plan.hip"), os.path.join(ROOT, "tests", "cpp", "gemm_q8a8_plan_check.cpp"), "-o", EXE], check=True)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "PLAN OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
