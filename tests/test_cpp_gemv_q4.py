"""The q4 GemvTr through the C++ facade (include/wgebra.hpp): tests/cpp/q4_facade.cpp builds with -Wall -Wextra -Werror and links like tests/cpp/q8_facade.cpp; it
references Gemv::dispatch_q4_tr / dispatch_q4_generic on GpuTensor<uint8_t>; on the GPU it checks them on exact integer operands."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "_build", "q4_facade")


def build():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    lib_dir = os.path.join(ROOT, "wgmath_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "q4_facade.cpp"), "-o", EXE, "-L", lib_dir, "-lwgebra_hip",
                    f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"], check=True)


def test_cpp_q4_facade_compiles_and_links():
    build()
    r = subprocess.run([EXE, "--host-only"], capture_output=True, text=True)
    assert r.returncode == 0 and "HOST OK" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_q4_gemv_on_gpu():
    build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr
