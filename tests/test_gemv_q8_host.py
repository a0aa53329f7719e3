"""wg_gemv_q8 without a GPU: the symbols are declared, bound and exported, a NULL context is refused with wg_gemv's wording, the Python operators check element types
before any library call, and quantize_q8 / dequantize_q8 keep their contract."""
import os
import subprocess

import numpy as np
import pytest

import wgmath_amd as wg
from wgmath_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_bound_and_exported():
    for name in ("wg_gemv_q8", "wg_debug_gemv_q8_plan"):
        assert name in _lib.declared_symbols() and name in _lib.lib._wg_signatures, name
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " T wg_gemv_q8\n" in exported and " T wg_debug_gemv_q8_plan\n" in exported
    S = _lib.ViewShapeC
    assert _lib.lib.wg_gemv_q8.argtypes == [_lib.ctypes.c_void_p, _lib.ctypes.c_int, _lib.ctypes.c_uint32] + [_lib.ctypes.c_void_p, S] * 4
    assert _lib.lib.wg_abi_version() == _lib.ABI_VERSION == 5  # (added symbols, no bump)
    hdr = open(_lib.HEADER_PATH).read()
    assert "#define WGEBRA_HIP_ABI_VERSION 5 " in hdr
    assert "WG_F32 = 0" in hdr and "WG_BF16 = 2" in hdr and "WG_I8" not in hdr and "WG_INT8" not in hdr  # wg_dtype is not extended
    facade = open(os.path.join(ROOT, "include", "wgebra.hpp")).read()
    for name in ("dispatch_q8_generic(", "dispatch_q8(", "dispatch_q8_tr(", "wg_gemv_q8(pass.ctx()", "GpuTensorView<int8_t> m"):
        assert name in facade, name
    for name in ("quantize_q8", "dequantize_q8"):
        assert callable(getattr(wg, name))


def test_null_context_is_refused_with_gemvs_wording():
    S = _lib.ViewShapeC()
    for g in (0, 16, 32, 7):
        assert _lib.lib.wg_gemv_q8(None, 0, g, None, S, None, S, None, S, None, S) == _lib.WG_ERR_INVALID_ARG
        assert _lib.lib.wg_last_error_string() == b"Gemv: ctx is NULL"
    assert _lib.lib.wg_gemv(None, 0, _lib.WG_F32, None, S, None, S, None, S) == _lib.WG_ERR_INVALID_ARG
    assert _lib.lib.wg_last_error_string() == b"Gemv: ctx is NULL"  # (wg_gemv's wording)


def test_other_entry_points_still_answer_unknown_dtype():
    """wg_dtype has no 8-bit value: 3 is as unknown as it was. (Reached without a device: a context is needed before the dtype is looked at, so the wording is
    read from the one place that produces it.)"""
    api = open(os.path.join(ROOT, "wgmath_amd", "csrc", "api.hip")).read()
    assert 'if (dtype != WG_F32 && dtype != WG_F16 && dtype != WG_BF16) return wg_set_error(WG_ERR_INVALID_ARG, "%s: unknown dtype %d", op, (int)dtype);' in api
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


def _args(method, out, m, s, v, g=32):
    return (None, wg.ViewShapeBuffers(), _NoPass(), out, m, s, v, g) + ((wg.GemvVariant.GemvTr,) if method.endswith("generic") else ())


@pytest.mark.parametrize("method", ["dispatch_q8", "dispatch_q8_tr", "dispatch_q8_generic"])
@pytest.mark.parametrize("m_dt,s_dt,v_dt,o_dt", [(np.uint8, np.float32, np.float32, np.float32), (np.int16, np.float32, np.float32, np.float32),
                                                 (np.float16, np.float32, np.float32, np.float32), (np.float32, np.float32, np.float32, np.float32),
                                                 (np.int8, np.float16, np.float32, np.float32), (np.int8, np.float32, np.float16, np.float32),
                                                 (np.int8, np.float32, np.float32, np.float16), (np.int8, np.float32, np.float32, wg.bfloat16),
                                                 (np.int8, np.float64, np.float32, np.float32), (np.int8, np.int8, np.float32, np.float32)])
def test_dispatch_q8_refuses_wrong_element_types(method, m_dt, s_dt, v_dt, o_dt):
    g = wg.Gemv.from_device(None)
    out, m, s, v = detached((32,), o_dt), detached((32, 32), m_dt), detached((1, 32), s_dt), detached((32,), v_dt)
    with pytest.raises(TypeError):
        getattr(g, method)(*_args(method, out, m, s, v))


@pytest.mark.parametrize("method", ["dispatch_q8", "dispatch_q8_tr", "dispatch_q8_generic"])
def test_dispatch_q8_accepts_int8_and_refuses_row_major(method):
    """The checks pass and the call reaches the library (here: the stand-in pass, which says so)."""
    out, m, s, v = detached((32,), np.float32), detached((32, 32), np.int8), detached((1, 32), np.float32), detached((32,), np.float32)
    with pytest.raises(AssertionError, match="the library was called"):
        getattr(wg.Gemv.from_device(None), method)(*_args(method, out, m, s, v))
    with pytest.raises(TypeError, match="row-major"):
        getattr(wg.Gemv.from_device(None, wg.row_major_shader_defs()), method)(*_args(method, out, m, s, v))


def test_dispatch_mixed_keeps_refusing_int8():
    out, m, v = detached((32,), np.float32), detached((32, 32), np.int8), detached((32,), np.float32)
    with pytest.raises(TypeError):
        wg.Gemv.from_device(None).dispatch_mixed(None, wg.ViewShapeBuffers(), _NoPass(), out, m, v)


def test_int8_tensors_are_described_in_bytes():
    t = detached((48, 3), np.int8)
    assert t.dtype == np.dtype(np.int8) and t.len() == 144
    s = t.as_embedded_view(3).shape()
    assert (tuple(s.size), s.stride, s.stride_mat, s.offset) == ((48, 3, 1), 48, 144, 0)


# ---- quantize_q8 / dequantize_q8 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,G", [((128, 5), 16), ((128, 5), 32), ((128, 5), 128), ((100, 7), 32), ((100, 7), 48), ((100, 7), 100), ((100, 7), 4096), ((37, 3), 37),
                                     ((64, 4, 3), 16), ((100, 2, 2), 32)])
def test_quantize_round_trip(shape, G):
    rng = np.random.default_rng(shape[0] + G)
    w = (rng.standard_normal(shape) * rng.choice([1e-3, 1.0, 50.0], shape[1:])).astype(np.float32)
    q, s = wg.quantize_q8(w, G)
    rows = shape[0]
    ng = -(-rows // G)
    assert q.dtype == np.int8 and q.shape == w.shape and s.dtype == np.float32 and s.shape == (ng,) + shape[1:]
    assert ng == (1 if G >= rows else ng)  # the per-column mode: one row of scales
    assert q.min() >= -127, "-128 was produced"
    gi = np.arange(rows) // G
    # per group and column s = fl32(max|w| / 127): some weight of every group sits at +-127 (a partial last group included)
    for i in range(ng):
        blk = np.abs(w[i * G:(i + 1) * G])
        assert np.array_equal(s[i], (blk.max(axis=0) / np.float32(127)).astype(np.float32))
        assert (np.abs(q[i * G:(i + 1) * G].astype(np.int32)).max(axis=0) == 127).all()
    d = wg.dequantize_q8(q, s, G)
    assert d.dtype == np.float32 and d.shape == w.shape
    assert np.array_equal(d, (s[gi] * q.astype(np.float32)).astype(np.float32))
    # the round trip is within s / 2 per element. In exact arithmetic |w / s - q| <= 1/2; the f32 quotient (|w / s| <= 127 (1 + 2^-23)) is off by at most
    # 127 * 2^-24 < 2^-17 of a step, the product s q by 2^-24 of at most 127 steps: s (1/2 + 2^-16) bounds both
    err = np.abs(d.astype(np.float64) - w.astype(np.float64))
    assert (err <= s[gi].astype(np.float64) * (0.5 + 2.0 ** -16)).all()


def test_quantize_all_zero_groups_and_errors():
    w = np.ones((64, 3), np.float32)
    w[16:32, 1] = 0  # one all-zero group
    w[:, 2] = 0      # an all-zero column
    q, s = wg.quantize_q8(w, 16)
    assert s[1, 1] == 0 and (q[16:32, 1] == 0).all() and (s[:, 2] == 0).all() and (q[:, 2] == 0).all()
    assert (s[:, 0] == np.float32(1) / np.float32(127)).all() and (q[:, 0] == 127).all()
    assert np.array_equal(wg.dequantize_q8(q, s, 16)[:, 2], np.zeros(64, np.float32)) and np.isfinite(wg.dequantize_q8(q, s, 16)).all()
    q2, s2 = wg.quantize_q8(-w, 1000)  # per column
    assert s2.shape == (1, 3) and (q2[:, 0] == -127).all()
    for bad in (0, -16, 8, 24, 63):
        with pytest.raises(ValueError):
            wg.quantize_q8(w, bad)
    with pytest.raises(TypeError):
        wg.dequantize_q8(q.astype(np.int16), s, 16)
    with pytest.raises(ValueError):
        wg.dequantize_q8(q, s[:2], 16)
