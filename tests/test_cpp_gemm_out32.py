"""The f32-output Gemm through the C++ facade (include/wgebra.hpp): tests/cpp/out32_facade.cpp builds and links like tests/cpp/mixed_facade.cpp, which instantiates
Gemm::dispatch_out32 / dispatch_out32_tr / dispatch_out32_generic for _Float16, wg::bf16 and float; an `out` that is not a view of float does not compile; on the
GPU it checks them on exact integer operands."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "_build", "out32_facade")


def compile_(extra=(), exe=EXE):
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    lib_dir = os.path.join(ROOT, "wgmath_amd")
    return subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "out32_facade.cpp"), "-o", exe, "-L", lib_dir, "-lwgebra_hip",
                           f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"], capture_output=True, text=True)


def build():
    r = compile_()
    assert r.returncode == 0, r.stderr


def test_cpp_out32_facade_compiles_and_links():
    build()
    r = subprocess.run([EXE, "--host-only"], capture_output=True, text=True)
    assert r.returncode == 0 and "HOST OK" in r.stdout, r.stdout + r.stderr


def test_cpp_out32_refuses_an_out_that_is_not_float():
    r = compile_(["-DWG_OUT32_OUT_NOT_FLOAT"], EXE + "_must_not_build")
    assert r.returncode != 0 and "out_not_float" in r.stderr and "GpuTensorView<float>" in r.stderr, r.stderr


@pytest.mark.gpu
def test_cpp_out32_gemm_on_gpu():
    build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr
