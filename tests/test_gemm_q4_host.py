"""wg_gemm_q4 without a GPU: the symbols are declared, bound and exported, the ABI version and wg_dtype are what they were, a NULL context is refused with Gemm's
wording, the refusals that need a context are worded in the one place that produces them (tests/test_gpu_gemm_q4.py::test_status_codes reaches them on the device),
the Python operators check element types before any library call, and the C++ facade carries the mirror (tests/cpp/gemm_q4_facade.cpp)."""
import os
import subprocess

import numpy as np
import pytest

import wgmath_amd as wg
from wgmath_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_bound_and_exported():
    for name in ("wg_gemm_q4", "wg_debug_gemm_q4_plan"):
        assert name in _lib.declared_symbols() and name in _lib.lib._wg_signatures, name
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " T wg_gemm_q4\n" in exported and " T wg_debug_gemm_q4_plan\n" in exported
    S, c = _lib.ViewShapeC, _lib.ctypes
    assert _lib.lib.wg_gemm_q4.argtypes == [c.c_void_p, c.c_int, c.c_uint32, c.c_int] + [c.c_void_p, S] * 4
    assert _lib.lib.wg_abi_version() == _lib.ABI_VERSION == 5  # (added symbols, no bump)
    hdr = open(_lib.HEADER_PATH).read()
    assert "#define WGEBRA_HIP_ABI_VERSION 5 " in hdr
    assert "WG_F32 = 0" in hdr and "WG_BF16 = 2" in hdr and all(n not in hdr for n in ("WG_I8", "WG_INT8", "WG_U8", "WG_I4", "WG_Q4"))  # wg_dtype is not extended
    assert c.sizeof(_lib.GemmQ4QueryC) == 88 and c.sizeof(_lib.GemmQ4PlanC) == 192
    assert _lib.GEMM_Q4_LEAVES == ("nothing", "unsupported", "mfma", "any")
    for i, leaf in enumerate(("NOTHING", "UNSUPPORTED", "MFMA", "ANY")):
        assert f"WG_GEMM_Q4_{leaf} = {i}" in hdr, leaf
    facade = open(os.path.join(ROOT, "include", "wgebra.hpp")).read()
    for name in ("wg_gemm_q4(pass.ctx()", "GpuTensorView<float> out, GpuTensorView<uint8_t> m, GpuTensorView<float> scales,\n                             GpuTensorView<X> x, uint32_t group_rows, GemmVariant variant = GemmVariant::GemmTr"):
        assert name in facade, name


def test_null_context_is_refused_with_gemms_wording():
    S = _lib.ViewShapeC()
    for variant, g, dt in ((1, 32, _lib.WG_F16), (0, 0, _lib.WG_BF16), (7, 48, _lib.WG_F32), (1, 7, 9)):
        assert _lib.lib.wg_gemm_q4(None, variant, g, dt, None, S, None, S, None, S, None, S) == _lib.WG_ERR_INVALID_ARG
        assert _lib.lib.wg_last_error_string() == b"Gemm: ctx is NULL"
    assert _lib.lib.wg_gemm_q8(None, 1, 32, _lib.WG_F16, None, S, None, S, None, S, None, S) == _lib.WG_ERR_INVALID_ARG
    assert _lib.lib.wg_last_error_string() == b"Gemm: ctx is NULL"  # (wg_gemm_q8's wording)


def _body():
    api = open(os.path.join(ROOT, "wgmath_amd", "csrc", "api.hip")).read()
    a = api.index("int wg_gemm_q4(")
    return api[a:api.index("\nint wg_reduce(", a)]


def test_refusals_in_their_order():
    """Everything behind the NULL-context check needs a context, so no device-less call reaches it: the wording and the order are read from the function itself."""
    body = _body()
    marks = ['check_common("Gemm", ctx, x_dtype, bufs, 4)',  # NULL context, an unknown x_dtype (INVALID_ARG), NULL buffers
             'if (x_dtype == WG_F32)', 'WG_ERR_UNSUPPORTED, "Gemm: wg_gemm_q4 takes f16 or bf16 columns (f32 activations stay with wg_gemv_q4',
             'WG_ERR_INVALID_ARG, "Gemm: unknown variant %d"',
             'if (variant != WG_GEMM_TR && variant != WG_GEMM_TR_FAST)', 'WG_ERR_UNSUPPORTED, "Gemm: wg_gemm_q4 computes out = W^T x only (WG_GEMM_TR); wg_gemv_q8 computes out = W v',
             'const uint64_t k64 = 2ull * mm.rows;',
             'WG_ERR_DIM_MISMATCH, "Gemm: dimension mismatch. (out [%u,%u,%u], m1 [%u,%u,%u]^T packed: k %llu, m2 [%u,%u,%u])"',
             'if (group_rows == 0 || (group_rows % 32u != 0 && group_rows < k))',
             'WG_ERR_INVALID_ARG, "Gemm: group_rows %u is neither a positive multiple of 32 nor at least the %u logical rows of m"',
             'WG_ERR_DIM_MISMATCH, "Gemm: dimension mismatch. (m [%u,%u,%u] packed: k %u, group_rows %u, scales [%u,%u,%u], expected [%u,%u,%u])"',
             'return WG_OK;', 'check_bounds("Gemm", "out", o, out, WG_F32)', 'check_bounds_es("Gemm", "m", mm, m, 1)', 'check_bounds("Gemm", "scales", ss, scales, WG_F32)',
             'check_bounds("Gemm", "x", xx, x, x_dtype)', 'check_alias_f32_u8("Gemm", "out", o, out->ptr, "m", mm, m->ptr)',
             'check_alias("Gemm", WG_F32, "out", o, out->ptr, "scales", ss, scales->ptr)', 'check_alias_f32_u16("Gemm", "out", o, out->ptr, "x", xx, x->ptr)',
             'gemm_q4_plan(q)', 'wgk_gemm_q4(']
    at = -1
    for m in marks:
        nxt = body.find(m, at + 1)
        assert nxt > at, f"'{m}' is missing or out of order"
        at = nxt


def test_other_entry_points_are_untouched_by_the_new_one():
    """wg_gemm_q8 and wg_gemv_q4 keep their own checks and kernels: the new function shares helpers, not code paths."""
    body = _body()
    assert "wgk_gemv_q4" not in body and "wgk_gemm_q8" not in body and "gemm_q8_plan" not in body and "gemm_launch" not in body and "gemm_staged" not in body
    for dt in (np.int8, np.uint8):
        with pytest.raises(TypeError):
            wg.wgcore.wg_dtype(dt)


class _NoCtx:
    handle = None


class _NoPass:
    """A pass whose context must never be reached: the element-type checks come first."""

    @property
    def _ctx(self):
        raise AssertionError("the library was called")


def detached(shape, dtype):
    return wg.GpuTensor(_NoCtx(), 0, shape, np.dtype(dtype))


def _args(method, out, m, s, x, g=32):
    return (None, wg.ViewShapeBuffers(), _NoPass(), out, m, s, x, g) + ((wg.GemmVariant.GemmTr,) if method.endswith("generic") else ())


@pytest.mark.parametrize("method", ["dispatch_q4_tr", "dispatch_q4_generic"])
@pytest.mark.parametrize("m_dt,s_dt,x_dt,o_dt", [(np.int8, np.float32, np.float16, np.float32), (np.int16, np.float32, np.float16, np.float32),
                                                 (np.float16, np.float32, np.float16, np.float32), (np.uint8, np.float16, np.float16, np.float32),
                                                 (np.uint8, np.float32, np.float32, np.float32), (np.uint8, np.float32, np.uint8, np.float32),
                                                 (np.uint8, np.float32, np.float64, np.float32), (np.uint8, np.float32, np.float16, np.float16),
                                                 (np.uint8, np.float32, wg.bfloat16, wg.bfloat16), (np.uint8, np.uint8, np.float16, np.float32)])
def test_dispatch_q4_refuses_wrong_element_types(method, m_dt, s_dt, x_dt, o_dt):
    g = wg.Gemm.from_device(None)
    out, m, s, x = detached((32, 8), o_dt), detached((16, 32), m_dt), detached((1, 32), s_dt), detached((32, 8), x_dt)
    with pytest.raises(TypeError):
        getattr(g, method)(*_args(method, out, m, s, x))


@pytest.mark.parametrize("method", ["dispatch_q4_tr", "dispatch_q4_generic"])
@pytest.mark.parametrize("x_dt", [np.float16, wg.bfloat16])
def test_dispatch_q4_accepts_16_bit_columns_and_refuses_row_major(method, x_dt):
    """The checks pass and the call reaches the library (here: the stand-in pass, which says so)."""
    out, m, s, x = detached((32, 8), np.float32), detached((16, 32), np.uint8), detached((1, 32), np.float32), detached((32, 8), x_dt)
    with pytest.raises(AssertionError, match="the library was called"):
        getattr(wg.Gemm.from_device(None), method)(*_args(method, out, m, s, x))
    with pytest.raises(TypeError, match="row-major"):
        getattr(wg.Gemm.from_device(None, wg.row_major_shader_defs()), method)(*_args(method, out, m, s, x))


def test_gemv_q4_keeps_refusing_16_bit_vectors():
    out, m, s, v = detached((32,), np.float32), detached((16, 32), np.uint8), detached((1, 32), np.float32), detached((32,), np.float16)
    with pytest.raises(TypeError):
        wg.Gemv.from_device(None).dispatch_q4_tr(None, wg.ViewShapeBuffers(), _NoPass(), out, m, s, v, 32)


def test_cpp_gemm_q4_facade_compiles_and_links():
    """tests/cpp/gemm_q4_facade.cpp builds with -Wall -Wextra -Werror and links like tests/cpp/gemm_q8_facade.cpp; it instantiates Gemm::dispatch_q4_tr /
    dispatch_q4_generic for f16 and bf16 columns and checks at compile time which operand types they take."""
    exe = os.path.join(ROOT, "tests", "cpp", "_build", "gemm_q4_facade")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    lib_dir = os.path.join(ROOT, "wgmath_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "gemm_q4_facade.cpp"), "-o", exe, "-L", lib_dir, "-lwgebra_hip",
                    f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "HOST OK" in r.stdout, r.stdout + r.stderr
