"""The q8a8 Gemm and the quantiser through the C++ facade (include/wgebra.hpp): tests/cpp/gemm_q8a8_facade.cpp builds with -Wall -Wextra -Werror and links like
tests/cpp/gemm_q8_facade.cpp; it takes the addresses of Gemm::dispatch_q8a8_tr / dispatch_q8a8_generic and instantiates QuantizeQ8::dispatch for float, f16 and bf16
sources, and checks at compile time which operand types they take."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "_build", "gemm_q8a8_facade")


def test_cpp_gemm_q8a8_facade_compiles_and_links():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    lib_dir = os.path.join(ROOT, "wgmath_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "gemm_q8a8_facade.cpp"), "-o", EXE, "-L", lib_dir, "-lwgebra_hip",
                    f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"], check=True)
    r = subprocess.run([EXE], capture_output=True, text=True)
    assert r.returncode == 0 and "HOST OK" in r.stdout, r.stdout + r.stderr
