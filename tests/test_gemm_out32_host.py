"""wg_gemm_out32 without a GPU: the symbol is declared, exported and bound at ABI 5; a NULL context is refused; the Python operators check element types (and the
row-major shader defs) before any library call; and the plan of the call -- the 16-bit planner's on the query the launcher fills, after the override that turns the
continuous walk and the panel form off (wg_debug_gemm_out32_query) -- gives the rows of tests/test_gpu_gemm_out32.py the launch logs that file asserts on the GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import wgmath_amd as wg
from wgmath_amd import _lib
from test_gemm16_plan_host import plan, query
from test_gpu_gemm_out32 import AB, ROWS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOT_THIS_LAUNCHER = ("staged",)  # (lengths that are not multiples of 4 are staged in api.hip before the launcher is reached)
PLANNED = [pytest.param(r, tr, id=f"{r.name}-{'tr' if tr else 'nn'}") for r in ROWS if r.name not in NOT_THIS_LAUNCHER for tr in r.variants]


def test_symbol_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "wgebra_hip.h")).read()
    assert re.search(r"#define\s+WGEBRA_HIP_ABI_VERSION\s+5\b", header)
    assert _lib.lib.wg_abi_version() == 5 == _lib.ABI_VERSION  # (added symbols, no bump)
    for name in ("wg_gemm_out32", "wg_debug_gemm_out32_query"):
        assert name in _lib.declared_symbols() and hasattr(_lib.lib, name), name
    assert _lib.lib._wg_signatures["wg_gemm_out32"] == _lib.lib._wg_signatures["wg_gemm_ex"]  # (the same argument list: the dtype is the operands')
    assert _lib.lib.wg_gemm_out32.argtypes == _lib.lib.wg_gemm_ex.argtypes and _lib.lib.wg_gemm_out32.restype == ctypes.c_int
    facade = open(os.path.join(ROOT, "include", "wgebra.hpp")).read()
    for name in ("dispatch_out32_generic", "dispatch_out32(", "dispatch_out32_tr(", "wg_gemm_out32(pass.ctx()"):
        assert name in facade, name


def test_null_arguments_are_refused():
    S = _lib.ViewShapeC()
    for dt in (_lib.WG_F32, _lib.WG_F16, _lib.WG_BF16, 7):
        assert _lib.lib.wg_gemm_out32(None, 0, dt, 1.0, 0.0, None, S, None, S, None, S) == _lib.WG_ERR_INVALID_ARG
        assert _lib.lib.wg_last_error_string() == b"Gemm: ctx is NULL"
    assert _lib.lib.wg_gemm_ex(None, 0, _lib.WG_F16, 1.0, 0.0, None, S, None, S, None, S) == _lib.WG_ERR_INVALID_ARG
    assert _lib.lib.wg_last_error_string() == b"Gemm: ctx is NULL"  # (wg_gemm_ex's wording)
    assert _lib.lib.wg_debug_gemm_out32_query(None) == _lib.WG_ERR_INVALID_ARG


class _NoCtx:
    handle = None


class _NoPass:
    """A pass whose context must never be reached: the checks come first."""

    @property
    def _ctx(self):
        raise AssertionError("the library was called")


def detached(shape, dtype):
    return wg.GpuTensor(_NoCtx(), 0, shape, np.dtype(dtype))


def _args(method, out, m1, m2):
    return (None, wg.ViewShapeBuffers(), _NoPass(), out, m1, m2) + ((wg.GemmVariant.Gemm,) if method.endswith("generic") else ())


METHODS = ["dispatch_out32", "dispatch_out32_tr", "dispatch_out32_generic"]


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("in_dt", [np.float16, wg.bfloat16, np.float32])
def test_row_major_defs_are_a_type_error(method, in_dt):
    out, m1, m2 = detached((8, 8), np.float32), detached((8, 8), in_dt), detached((8, 8), in_dt)
    with pytest.raises(TypeError, match="row-major"):
        getattr(wg.Gemm.from_device(None, wg.row_major_shader_defs()), method)(*_args(method, out, m1, m2))
    with pytest.raises(AssertionError, match="the library was called"):  # (column-major: the checks pass and the call reaches the library)
        getattr(wg.Gemm.from_device(None), method)(*_args(method, out, m1, m2))


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("a_dt,b_dt,o_dt", [(np.float16, np.float16, np.float16), (np.float16, wg.bfloat16, np.float32), (wg.bfloat16, wg.bfloat16, wg.bfloat16),
                                            (np.float16, np.float32, np.float32), (np.int32, np.int32, np.float32), (np.float16, np.float16, np.float64)])
def test_wrong_element_types_are_a_type_error(method, a_dt, b_dt, o_dt):
    out, m1, m2 = detached((8, 8), o_dt), detached((8, 8), a_dt), detached((8, 8), b_dt)
    with pytest.raises(TypeError):
        getattr(wg.Gemm.from_device(None), method)(*_args(method, out, m1, m2))


def test_the_override_turns_the_walk_and_the_panels_off_and_nothing_else():
    q = query(False, 4096, 256, 8192, 1, {"f16_tile": 256, "f16_cont": 1, "f16_sched": 0, "f16_balance": 1}, cus=248, uneven=True, alpha=2.0, beta=0.5, recording=True)
    q.panels, q.panel_cols, q.panel_n_main, q.panel_n_tail, q.bal_valid, q.padded = 1, 1024, 7, 1, 1, 1
    q.panel_tail_cols[0] = 1024
    before = bytes(q)
    _lib.check(_lib.lib.wg_debug_gemm_out32_query(ctypes.byref(q)))
    assert q.cont == 0 and q.panels == 0 and q.panel_cols == 0 and q.panel_n_main == 0 and q.panel_n_tail == 0 and list(q.panel_tail_cols) == [0] * 8
    ref = _lib.Gemm16QueryC.from_buffer_copy(before)
    ref.cont = ref.panels = ref.panel_cols = ref.panel_n_main = ref.panel_n_tail = 0
    ref.panel_tail_cols[0] = 0
    assert bytes(q) == bytes(ref)


@pytest.mark.parametrize("prefix", ["f16", "bf16"])
@pytest.mark.parametrize("row,tr", PLANNED)
def test_table_is_the_16_bit_plan_with_the_prefix_swapped(row, tr, prefix):
    """With cont = 0 the tags are the 16-bit call's with the prefix swapped, and they are what the GPU test asserts -- for (1, 0) and (alpha, beta), on the dense
    output and on the odd one (offset 1, leading dimension M + 3, 7 elements between matrices; rows marked dense only: the dense view)."""
    M, K, N, mats = row.M, row.K, row.N, row.mats
    knobs = dict(row.knobs, f16_cont=0)
    for out in (None,) if row.dense_only else (None, (1, M + 3, (M + 3) * N + 7)):
        for alpha, beta in ((1.0, 0.0), AB):
            q16 = query(tr, M, K, N, mats, knobs, alpha=alpha, beta=beta, out=out)
            q32 = query(tr, M, K, N, mats, knobs, alpha=alpha, beta=beta, out=out)
            if out:
                q32.c_addr = (4 * out[0]) & 15  # (the same element offset is twice as many bytes into an f32 buffer)
            _lib.check(_lib.lib.wg_debug_gemm_out32_query(ctypes.byref(q32)))
            log16, log32 = plan(q16, prefix)[1], plan(q32, prefix + "o32")[1]
            assert log32 == log16.replace(prefix + ".", prefix + "o32."), (log16, log32)
            if row.name == "few_columns" and out is None and (alpha, beta) == (1.0, 0.0):
                assert "gemv" not in log32  # (and nothing in front of the launcher reroutes the out32 call to a Gemv)
            assert row.took(prefix, log32, beta), f"{row.name}: expected {(row.leaf if beta == 0 else row.ab)!r}, planned {log32!r}"


@pytest.mark.parametrize("tr", [False, True], ids=["nn", "tr"])
def test_a_requested_walk_is_planned_as_the_per_tile_kernel(tr):
    """4096 x 256 x 8192 with f16_tile = 256 and f16_cont = 1: the 16-bit call takes the continuous walk; once the launcher's override is applied the same query is
    planned as the per-tile 256 x 256 kernel, whose tiles, k order and accumulation chains the walk shares."""
    q = query(tr, 4096, 256, 8192, 1, {"f16_tile": 256, "f16_cont": 1})
    p16, log16, _ = plan(q, "f16")
    assert p16.cont == 1 and log16 == "f16.cont"
    _lib.check(_lib.lib.wg_debug_gemm_out32_query(ctypes.byref(q)))
    p32, log32, _ = plan(q, "f16o32")
    assert p32.cont == 0 and _lib.GEMM16_LEAVES[p32.leaf] == "m16" and log32.startswith("f16o32.m16") and "cont" not in log32, log32
    assert (p32.tiles_m, p32.tiles_n, p32.nsplit) == (p16.tiles_m, p16.tiles_n, p16.nsplit)
