"""wg_gemm_q8a8 without a GPU: the symbols are declared, bound and exported, the ABI version and wg_dtype are what they were, a NULL context is refused with Gemm's
wording, the refusals that need a context are worded in the one place that produces them and stand in the contract's order
(tests/test_gpu_gemm_q8a8.py::test_status_codes reaches them on the device), and the Python operators check element types before any library call."""
import os
import subprocess

import numpy as np
import pytest

import wgmath_amd as wg
from wgmath_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_bound_and_exported():
    for name in ("wg_gemm_q8a8", "wg_debug_gemm_q8a8_plan"):
        assert name in _lib.declared_symbols() and name in _lib.lib._wg_signatures, name
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " T wg_gemm_q8a8\n" in exported and " T wg_debug_gemm_q8a8_plan\n" in exported
    S, c = _lib.ViewShapeC, _lib.ctypes
    assert _lib.lib.wg_gemm_q8a8.argtypes == [c.c_void_p, c.c_int, c.c_uint32, c.c_uint32] + [c.c_void_p, S] * 5
    assert _lib.lib.wg_abi_version() == _lib.ABI_VERSION == 5  # (added symbols, no bump)
    hdr = open(_lib.HEADER_PATH).read()
    assert "#define WGEBRA_HIP_ABI_VERSION 5 " in hdr
    assert "WG_F32 = 0" in hdr and "WG_BF16 = 2" in hdr and "WG_I8" not in hdr and "WG_INT8" not in hdr  # wg_dtype is not extended
    assert c.sizeof(_lib.GemmQ8A8QueryC) == 104 and c.sizeof(_lib.GemmQ8A8PlanC) == c.sizeof(_lib.GemmQ8PlanC) == 184
    facade = open(os.path.join(ROOT, "include", "wgebra.hpp")).read()
    for name in ("wg_gemm_q8a8(pass.ctx()", "void dispatch_q8a8_tr(", "struct QuantizeQ8 {"):
        assert name in facade, name


def test_null_context_is_refused_with_gemms_wording():
    S = _lib.ViewShapeC()
    for variant, g, gx in ((1, 32, 32), (0, 0, 0), (7, 16, 48), (1, 7, 9)):
        assert _lib.lib.wg_gemm_q8a8(None, variant, g, gx, None, S, None, S, None, S, None, S, None, S) == _lib.WG_ERR_INVALID_ARG
        assert _lib.lib.wg_last_error_string() == b"Gemm: ctx is NULL"


def _body():
    api = open(os.path.join(ROOT, "wgmath_amd", "csrc", "api.hip")).read()
    a = api.index("int wg_gemm_q8a8(")
    return api[a:api.index("\nnamespace {", a)]


def test_refusals_in_their_order():
    """Everything behind the NULL-context check needs a context, so no device-less call reaches it: the wording and the order are read from the function itself."""
    body = _body()
    marks = ['check_common("Gemm", ctx, WG_F32, bufs, 5)',  # NULL context, NULL buffers
             'WG_ERR_INVALID_ARG, "Gemm: unknown variant %d"',
             'if (variant != WG_GEMM_TR && variant != WG_GEMM_TR_FAST)', 'WG_ERR_UNSUPPORTED, "Gemm: wg_gemm_q8a8 computes out = W^T x only (WG_GEMM_TR); wg_gemv_q8 computes out = W v',
             'mk(out_shape)',  # no dimension is looked at before the refusal
             'WG_ERR_DIM_MISMATCH, "Gemm: dimension mismatch. (out [%u,%u,%u], m1 [%u,%u,%u]^T, m2 [%u,%u,%u])"',
             'WG_ERR_INVALID_ARG, "Gemm: group_rows %u is neither a positive multiple of 16 nor at least the %u rows of m"',
             'WG_ERR_INVALID_ARG, "Gemm: x_group_rows %u is neither a positive multiple of 16 nor at least the %u rows of x"',
             'group_rows % x_group_rows != 0 && x_group_rows % group_rows != 0', 'neither divides the other',
             'WG_ERR_DIM_MISMATCH, "Gemm: dimension mismatch. (m [%u,%u,%u], group_rows %u, scales [%u,%u,%u], expected [%u,%u,%u])"',
             'WG_ERR_DIM_MISMATCH, "Gemm: dimension mismatch. (x [%u,%u,%u], x_group_rows %u, x_scales [%u,%u,%u], expected [%u,%u,%u])"',
             'return WG_OK;', 'check_bounds("Gemm", "out", o, out, WG_F32)', 'check_bounds_es("Gemm", "m", mm, m, 1)', 'check_bounds("Gemm", "scales", ss, scales, WG_F32)',
             'check_bounds_es("Gemm", "x", xx, x, 1)', 'check_bounds("Gemm", "x_scales", xs, x_scales, WG_F32)',
             'check_alias_f32_u8("Gemm", "out", o, out->ptr, "m", mm, m->ptr)', 'check_alias("Gemm", WG_F32, "out", o, out->ptr, "scales", ss, scales->ptr)',
             'check_alias_f32_u8("Gemm", "out", o, out->ptr, "x", xx, x->ptr)', 'check_alias("Gemm", WG_F32, "out", o, out->ptr, "x_scales", xs, x_scales->ptr)',
             'gemm_q8a8_plan(q)', 'wgk_gemm_q8a8(']
    at = -1
    for m in marks:
        nxt = body.find(m, at + 1)
        assert nxt > at, f"'{m}' is missing or out of order"
        at = nxt


def test_other_entry_points_are_untouched_by_the_new_one():
    """wg_gemm_q8 keeps its own checks and kernels: the new function shares helpers, not code paths. Its unit defines no combine kernel and launches no other family's
    kernels: the partials of a cut go through the quantized families' one combine pass (tests/test_quant_plan_parent.py and the bit-exact GPU tests hold what that
    sharing must not change)."""
    import re
    body = _body()
    assert "wgk_gemm_q8(" not in body and "gemm_q8_plan(" not in body and "gemm_launch" not in body
    unit = open(os.path.join(ROOT, "wgmath_amd", "csrc", "gemm_q8a8.hip")).read()
    kernels = re.findall(r"__global__[^;{]*?void\s+(\w+)\s*\(", unit)
    assert kernels and not [k for k in kernels if "combine" in k], kernels
    launched = set(re.findall(r"hipLaunchKernelGGL\(\(?(\w+)", unit))
    assert launched and launched <= set(kernels), launched - set(kernels)
    assert "wgk_q_combine(ctx, true, " in unit
    with pytest.raises(TypeError):
        wg.wgcore.wg_dtype(np.int8)


class _NoCtx:
    handle = None


class _NoPass:
    """A pass whose context must never be reached: the element-type checks come first."""

    @property
    def _ctx(self):
        raise AssertionError("the library was called")


def detached(shape, dtype):
    return wg.GpuTensor(_NoCtx(), 0, shape, np.dtype(dtype))


def _args(method, out, m, s, x, xs, g=32, gx=32):
    return (None, wg.ViewShapeBuffers(), _NoPass(), out, m, s, x, xs, g, gx) + ((wg.GemmVariant.GemmTr,) if method.endswith("generic") else ())


I8, F32, F16 = np.int8, np.float32, np.float16


@pytest.mark.parametrize("method", ["dispatch_q8a8_tr", "dispatch_q8a8_generic"])
@pytest.mark.parametrize("m_dt,s_dt,x_dt,xs_dt,o_dt", [(np.uint8, F32, I8, F32, F32), (F16, F32, I8, F32, F32), (I8, F16, I8, F32, F32), (I8, F32, F16, F32, F32),
                                                       (I8, F32, wg.bfloat16, F32, F32), (I8, F32, np.uint8, F32, F32), (I8, F32, F32, F32, F32),
                                                       (I8, F32, I8, F16, F32), (I8, F32, I8, I8, F32), (I8, F32, I8, F32, F16), (I8, I8, I8, F32, F32)])
def test_dispatch_q8a8_refuses_wrong_element_types(method, m_dt, s_dt, x_dt, xs_dt, o_dt):
    g = wg.Gemm.from_device(None)
    out, m, s, x, xs = detached((32, 8), o_dt), detached((32, 32), m_dt), detached((1, 32), s_dt), detached((32, 8), x_dt), detached((1, 8), xs_dt)
    with pytest.raises(TypeError):
        getattr(g, method)(*_args(method, out, m, s, x, xs))


@pytest.mark.parametrize("method", ["dispatch_q8a8_tr", "dispatch_q8a8_generic"])
def test_dispatch_q8a8_accepts_int8_columns_and_refuses_row_major(method):
    """The checks pass and the call reaches the library (here: the stand-in pass, which says so)."""
    out, m, s, x, xs = detached((32, 8), F32), detached((32, 32), I8), detached((1, 32), F32), detached((32, 8), I8), detached((1, 8), F32)
    with pytest.raises(AssertionError, match="the library was called"):
        getattr(wg.Gemm.from_device(None), method)(*_args(method, out, m, s, x, xs))
    with pytest.raises(TypeError, match="row-major"):
        getattr(wg.Gemm.from_device(None, wg.row_major_shader_defs()), method)(*_args(method, out, m, s, x, xs))


def test_gemm_q8_keeps_refusing_int8_columns():
    out, m, s, x = detached((32, 8), F32), detached((32, 32), I8), detached((1, 32), F32), detached((32, 8), I8)
    with pytest.raises(TypeError):
        wg.Gemm.from_device(None).dispatch_q8_tr(None, wg.ViewShapeBuffers(), _NoPass(), out, m, s, x, 32)
