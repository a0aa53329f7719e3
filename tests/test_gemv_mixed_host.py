"""wg_gemv_mixed without a GPU: the symbol is declared and bound, a NULL context is refused, and the Python operators check element types before any library call."""
import os

import numpy as np
import pytest

import wgmath_amd as wg
from wgmath_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_declared_and_bound():
    assert "wg_gemv_mixed" in _lib.declared_symbols()
    assert _lib.lib._wg_signatures["wg_gemv_mixed"] == _lib.lib._wg_signatures["wg_gemv"]  # (the same argument list: the dtype is the matrix's)
    assert _lib.lib.wg_gemv_mixed.argtypes == _lib.lib.wg_gemv.argtypes
    assert _lib.lib.wg_abi_version() == 5  # (an added symbol, no bump)
    facade = open(os.path.join(ROOT, "include", "wgebra.hpp")).read()
    for name in ("dispatch_mixed_generic", "dispatch_mixed(", "dispatch_mixed_tr(", "wg_gemv_mixed(pass.ctx()"):
        assert name in facade, name


def test_null_context_is_refused():
    S = _lib.ViewShapeC()
    for dt in (_lib.WG_F32, _lib.WG_F16, _lib.WG_BF16, 7):
        assert _lib.lib.wg_gemv_mixed(None, 0, dt, None, S, None, S, None, S) == _lib.WG_ERR_INVALID_ARG
        msg = _lib.lib.wg_last_error_string()
        assert b"NULL" in msg and msg == b"Gemv: ctx is NULL"
    assert _lib.lib.wg_gemv(None, 0, _lib.WG_F16, None, S, None, S, None, S) == _lib.WG_ERR_INVALID_ARG
    assert _lib.lib.wg_last_error_string() == b"Gemv: ctx is NULL"  # (wg_gemv's wording)


class _NoCtx:
    handle = None


class _NoPass:
    """A pass whose context must never be reached: the element-type checks come first."""

    @property
    def _ctx(self):
        raise AssertionError("the library was called")


def detached(shape, dtype):
    return wg.GpuTensor(_NoCtx(), 0, shape, np.dtype(dtype))


@pytest.mark.parametrize("method", ["dispatch_mixed", "dispatch_mixed_tr", "dispatch_mixed_generic"])
@pytest.mark.parametrize("m_dt,v_dt,o_dt", [(np.float16, np.float16, np.float32), (np.float16, np.float32, np.float16), (wg.bfloat16, wg.bfloat16, wg.bfloat16),
                                            (np.float32, np.float16, np.float32), (np.int32, np.float32, np.float32), (np.uint16, np.float32, np.float32),
                                            (np.float64, np.float32, np.float32)])
def test_dispatch_mixed_refuses_wrong_element_types(method, m_dt, v_dt, o_dt):
    g = wg.Gemv.from_device(None)
    out, m, v = detached((8,), o_dt), detached((8, 8), m_dt), detached((8,), v_dt)
    args = (None, wg.ViewShapeBuffers(), _NoPass(), out, m, v) + ((wg.GemvVariant.Gemv,) if method.endswith("generic") else ())
    with pytest.raises(TypeError):
        getattr(g, method)(*args)


@pytest.mark.parametrize("m_dt", [np.float16, wg.bfloat16, np.float32])
def test_dispatch_mixed_accepts_the_three_matrix_types(m_dt):
    """The checks pass and the call reaches the library (here: the stand-in pass, which says so)."""
    g = wg.Gemv.from_device(None)
    out, m, v = detached((8,), np.float32), detached((8, 8), m_dt), detached((8,), np.float32)
    with pytest.raises(AssertionError, match="the library was called"):
        g.dispatch_mixed(None, wg.ViewShapeBuffers(), _NoPass(), out, m, v)
    with pytest.raises(TypeError, match="row-major"):
        wg.Gemv.from_device(None, wg.row_major_shader_defs()).dispatch_mixed(None, wg.ViewShapeBuffers(), _NoPass(), out, m, v)


@pytest.mark.parametrize("method", ["dispatch", "dispatch_tr"])
def test_dispatch_still_refuses_mixed_inputs(method):
    g = wg.Gemv.from_device(None)
    out, m, v = detached((8,), np.float32), detached((8, 8), np.float16), detached((8,), np.float32)
    with pytest.raises(TypeError, match="operands must share one element type"):
        getattr(g, method)(None, wg.ViewShapeBuffers(), _NoPass(), out, m, v)
