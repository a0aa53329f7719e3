"""wg_gemv_q4 without a GPU: the symbols are declared, bound and exported, the ABI version and wg_dtype are what they were, a NULL context is refused with wg_gemv's
wording, the Python operators check element types before any library call, and the facade carries the C++ mirror."""
import os
import subprocess

import numpy as np
import pytest

import wgmath_amd as wg
from wgmath_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_bound_and_exported():
    for name in ("wg_gemv_q4", "wg_debug_gemv_q4_plan"):
        assert name in _lib.declared_symbols() and name in _lib.lib._wg_signatures, name
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " T wg_gemv_q4\n" in exported and " T wg_debug_gemv_q4_plan\n" in exported
    S = _lib.ViewShapeC
    assert _lib.lib.wg_gemv_q4.argtypes == _lib.lib.wg_gemv_q8.argtypes == [_lib.ctypes.c_void_p, _lib.ctypes.c_int, _lib.ctypes.c_uint32] + [_lib.ctypes.c_void_p, S] * 4
    assert _lib.lib.wg_abi_version() == _lib.ABI_VERSION == 5  # (added symbols, no bump)
    hdr = open(_lib.HEADER_PATH).read()
    assert "#define WGEBRA_HIP_ABI_VERSION 5 " in hdr
    assert "WG_F32 = 0" in hdr and "WG_BF16 = 2" in hdr and "WG_U8" not in hdr and "WG_I4" not in hdr and "WG_Q4" not in hdr  # wg_dtype is not extended
    facade = open(os.path.join(ROOT, "include", "wgebra.hpp")).read()
    for name in ("dispatch_q4_generic(", "dispatch_q4_tr(", "wg_gemv_q4(pass.ctx()", "GpuTensorView<uint8_t> m"):
        assert name in facade, name
    for name in ("pack_q4", "unpack_q4", "quantize_q4", "dequantize_q4"):
        assert callable(getattr(wg, name))
    assert _lib.GEMV_Q4_LEAVES == ("nothing", "unsupported", "t", "any_t")
    # wg_dtype has no 4-bit or unsigned 8-bit value: 3 is as unknown as it was
    api = open(os.path.join(ROOT, "wgmath_amd", "csrc", "api.hip")).read()
    assert 'if (dtype != WG_F32 && dtype != WG_F16 && dtype != WG_BF16) return wg_set_error(WG_ERR_INVALID_ARG, "%s: unknown dtype %d", op, (int)dtype);' in api
    for dt in (np.uint8, np.int8):
        with pytest.raises(TypeError):
            wg.wgcore.wg_dtype(dt)


def test_null_context_is_refused_with_gemvs_wording():
    S = _lib.ViewShapeC()
    for g in (0, 32, 64, 7):
        for variant in (0, 2, 7):
            assert _lib.lib.wg_gemv_q4(None, variant, g, None, S, None, S, None, S, None, S) == _lib.WG_ERR_INVALID_ARG
            assert _lib.lib.wg_last_error_string() == b"Gemv: ctx is NULL"


class _NoCtx:
    handle = None


class _NoPass:
    """A pass whose context must never be reached: the element-type checks come first."""

    @property
    def _ctx(self):
        raise AssertionError("the library was called")


def detached(shape, dtype):
    return wg.GpuTensor(_NoCtx(), 0, shape, np.dtype(dtype))


def _args(method, out, m, s, v, g=32):
    return (None, wg.ViewShapeBuffers(), _NoPass(), out, m, s, v, g) + ((wg.GemvVariant.GemvTr,) if method.endswith("generic") else ())


@pytest.mark.parametrize("method", ["dispatch_q4_tr", "dispatch_q4_generic"])
@pytest.mark.parametrize("m_dt,s_dt,v_dt,o_dt", [(np.int8, np.float32, np.float32, np.float32), (np.int16, np.float32, np.float32, np.float32),
                                                 (np.float16, np.float32, np.float32, np.float32), (np.float32, np.float32, np.float32, np.float32),
                                                 (np.uint8, np.float16, np.float32, np.float32), (np.uint8, np.float32, np.float16, np.float32),
                                                 (np.uint8, np.float32, np.float32, np.float16), (np.uint8, np.float32, np.float32, wg.bfloat16),
                                                 (np.uint8, np.float64, np.float32, np.float32), (np.uint8, np.uint8, np.float32, np.float32)])
def test_dispatch_q4_refuses_wrong_element_types(method, m_dt, s_dt, v_dt, o_dt):
    g = wg.Gemv.from_device(None)
    out, m, s, v = detached((32,), o_dt), detached((16, 32), m_dt), detached((1, 32), s_dt), detached((32,), v_dt)
    with pytest.raises(TypeError):
        getattr(g, method)(*_args(method, out, m, s, v))


@pytest.mark.parametrize("method", ["dispatch_q4_tr", "dispatch_q4_generic"])
def test_dispatch_q4_accepts_uint8_and_refuses_row_major(method):
    """The checks pass and the call reaches the library (here: the stand-in pass, which says so)."""
    out, m, s, v = detached((32,), np.float32), detached((16, 32), np.uint8), detached((1, 32), np.float32), detached((32,), np.float32)
    with pytest.raises(AssertionError, match="the library was called"):
        getattr(wg.Gemv.from_device(None), method)(*_args(method, out, m, s, v))
    with pytest.raises(TypeError, match="row-major"):
        getattr(wg.Gemv.from_device(None, wg.row_major_shader_defs()), method)(*_args(method, out, m, s, v))
    # the other Gemv operators keep refusing packed bytes, and a packed tensor is described in bytes
    with pytest.raises(TypeError):
        wg.Gemv.from_device(None).dispatch_mixed(None, wg.ViewShapeBuffers(), _NoPass(), out, m, v)
    with pytest.raises(TypeError):
        wg.Gemv.from_device(None).dispatch_q8_tr(None, wg.ViewShapeBuffers(), _NoPass(), out, m, s, v, 32)
    t = detached((48, 3), np.uint8)
    assert t.dtype == np.dtype(np.uint8) and t.len() == 144
    sh = t.as_embedded_view(3).shape()
    assert (tuple(sh.size), sh.stride, sh.stride_mat, sh.offset) == ((48, 3, 1), 48, 144, 0)
