"""wg_quantize_q8 without a GPU: the symbols are declared, bound and exported, a NULL context is refused with the operator's wording, the Python operator checks
element types before any library call, and the launcher's choice (quantize_q8_plan in wgmath_amd/csrc/quantize_q8.hip, through wg_debug_quantize_q8_plan) is the
rule include/wgebra_hip.h states: the vector kernel for groups of 32 .. 1024 rows (a power of two) on 16-byte-aligned views with rows % 16 == 0, the
element-by-element kernel for everything else; every (group, column) once."""
import ctypes
import itertools
import subprocess

import numpy as np
import pytest

import wgmath_amd as wg
from wgmath_amd import _lib

LEAVES = _lib.QUANTIZE_Q8_LEAVES


def test_symbols_are_declared_bound_and_exported():
    for name in ("wg_quantize_q8", "wg_debug_quantize_q8_plan"):
        assert name in _lib.declared_symbols() and name in _lib.lib._wg_signatures, name
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " T wg_quantize_q8\n" in exported and " T wg_debug_quantize_q8_plan\n" in exported
    S, c = _lib.ViewShapeC, _lib.ctypes
    assert _lib.lib.wg_quantize_q8.argtypes == [c.c_void_p, c.c_int, c.c_uint32] + [c.c_void_p, S] * 3
    assert _lib.lib.wg_abi_version() == _lib.ABI_VERSION == 5  # (added symbols, no bump)
    assert c.sizeof(_lib.QuantizeQ8QueryC) == 56 and c.sizeof(_lib.QuantizeQ8PlanC) == 160
    assert wg.QuantizeQ8.from_device(None) is not None


def test_null_context_and_null_plan_arguments():
    S = _lib.ViewShapeC()
    for dt, g in ((_lib.WG_F32, 32), (_lib.WG_F16, 0), (9, 7)):
        assert _lib.lib.wg_quantize_q8(None, dt, g, None, S, None, S, None, S) == _lib.WG_ERR_INVALID_ARG
        assert _lib.lib.wg_last_error_string() == b"Quantize: ctx is NULL"
    assert _lib.lib.wg_debug_quantize_q8_plan(None, None) == _lib.WG_ERR_INVALID_ARG


def plan(**kw):
    q, p = _lib.QuantizeQ8QueryC(), _lib.QuantizeQ8PlanC()
    for k, v in kw.items():
        assert hasattr(q, k), k
        setattr(q, k, v)
    assert _lib.lib.wg_debug_quantize_q8_plan(ctypes.byref(q), ctypes.byref(p)) == 0
    return q, p


def query(rows, cols, mats, G, es, mis=None):
    kw = dict(rows=rows, cols=cols, mats=mats, group_rows=G, src_elem=es, ldq=rows, ldsrc=rows, q_addr16=0, src_addr16=0)
    if mis == "ldq":
        kw["ldq"] = rows + 8
    if mis == "ldsrc":
        kw["ldsrc"] = rows + 2
    kw["q_batch"] = kw["ldq"] * cols + (8 if mis == "q_batch" else 0)
    kw["src_batch"] = kw["ldsrc"] * cols + (2 if mis == "src_batch" else 0)
    if mis == "q_addr16":
        kw["q_addr16"] = 1
    if mis == "src_addr16":
        kw["src_addr16"] = es
    return kw


def vec_ok(q):
    G, es = q.group_rows, q.src_elem
    g_ok = 32 <= G <= 1024 and G & (G - 1) == 0
    q_ok = q.q_addr16 == 0 and (q.cols <= 1 or q.ldq % 16 == 0) and (q.mats <= 1 or q.q_batch % 16 == 0)
    s_ok = q.src_addr16 == 0 and (q.cols <= 1 or q.ldsrc * es % 16 == 0) and (q.mats <= 1 or q.src_batch * es % 16 == 0)
    return bool(g_ok and q.rows % 16 == 0 and q_ok and s_ok)


def check(q, p):
    what = f"rows {q.rows} cols {q.cols} mats {q.mats} G {q.group_rows} es {q.src_elem}: {LEAVES[p.leaf]}"
    if not q.rows or not q.cols or not q.mats:
        assert LEAVES[p.leaf] == "nothing" and p.status == 0, what
        return None
    if q.mats > 65535:
        assert LEAVES[p.leaf] == "unsupported" and p.status == _lib.WG_ERR_UNSUPPORTED and p.message.decode() == f"Quantize: nmats = {q.mats} exceeds 65535", what
        return None
    vec = vec_ok(q)
    per_col = -(-(q.rows // 16) // 256) if vec else -(-q.rows // min(q.group_rows, q.rows))
    if per_col * q.cols > 2 ** 31 - 1:
        assert LEAVES[p.leaf] == "unsupported" and p.status == _lib.WG_ERR_UNSUPPORTED and "exceed 2^31 - 1" in p.message.decode(), what
        return None
    assert LEAVES[p.leaf] == ("vec" if vec else "any"), what
    assert p.blocks_per_col == per_col and tuple(p.grid) == (per_col * q.cols, 1, q.mats), what
    if vec:
        assert p.block == 256 and p.group_lanes == q.group_rows // 16 and 256 % p.group_lanes == 0, what  # a group never straddles a wave or a workgroup
        assert (p.blocks_per_col - 1) * 256 * 16 < q.rows <= p.blocks_per_col * 256 * 16, what  # every row once, no empty workgroup
    else:
        assert p.block == (64 if min(q.group_rows, q.rows) <= 1024 else 256), what
    return LEAVES[p.leaf]


MIS = [None, "ldq", "ldsrc", "q_batch", "src_batch", "q_addr16", "src_addr16"]


def test_sweep():
    seen, any_because = set(), set()
    for rows, cols, mats, G, es, mis in itertools.product([0, 16, 32, 48, 100, 200, 4096, 4112, 65536], [0, 1, 17, 65, 65536], [1, 2, 70000],
                                                          [16, 32, 48, 64, 96, 128, 1024, 2048, 5000, 1 << 31], [4, 2], MIS):
        leaf = check(*plan(**query(rows, cols, mats, G, es, mis)))
        seen.add(leaf)
        if leaf == "any":
            any_because.add(mis)
    assert seen == {None, "vec", "any"} and any_because == set(MIS)


def test_the_choices_the_header_states():
    for rows, G, leaf in ((64, 32, "vec"), (4096, 1024, "vec"), (160, 64, "vec"), (200, 96, "any"), (192, 96, "any"), (64, 16, "any"), (4096, 2048, "any"), (4096, 1 << 31, "any"),
                          (40, 32, "any"), (32, 32, "vec")):
        for es in (4, 2):
            assert check(*plan(**query(rows, 9, 2, G, es))) == leaf, (rows, G, es)
    for mis in MIS[1:]:
        assert check(*plan(**query(64, 9, 2, 32, 4, mis))) == "any", mis
    kw = query(64, 1, 1, 32, 2)  # one column / one matrix: the stride that is never applied does not count
    kw.update(ldq=67, ldsrc=65, q_batch=3, src_batch=5)
    assert check(*plan(**kw)) == "vec"
    q, p = plan(**query(64, 65536, 1, 32, 4))  # more columns than grid.y holds: they lie on grid.x
    assert check(q, p) == "vec" and tuple(p.grid) == (65536, 1, 1)
    q, p = plan(**query(0xFFFFFFF0, 4096, 1, 16, 4))
    assert check(q, p) is None and "exceed 2^31 - 1" in p.message.decode()


class _NoCtx:
    handle = None


class _NoPass:
    @property
    def _ctx(self):
        raise AssertionError("the library was called")


def detached(shape, dtype):
    return wg.GpuTensor(_NoCtx(), 0, shape, np.dtype(dtype))


@pytest.mark.parametrize("q_dt,s_dt,x_dt", [(np.uint8, np.float32, np.float32), (np.float32, np.float32, np.float32), (np.int8, np.float16, np.float32),
                                            (np.int8, np.int8, np.float16), (np.int8, np.float32, np.float64), (np.int8, np.float32, np.int8)])
def test_dispatch_refuses_wrong_element_types(q_dt, s_dt, x_dt):
    q, s, x = detached((32, 8), q_dt), detached((1, 8), s_dt), detached((32, 8), x_dt)
    with pytest.raises(TypeError):
        wg.QuantizeQ8.from_device(None).dispatch(None, wg.ViewShapeBuffers(), _NoPass(), q, s, x, 32)


@pytest.mark.parametrize("x_dt", [np.float32, np.float16, wg.bfloat16])
def test_dispatch_accepts_the_three_source_types(x_dt):
    q, s, x = detached((32, 8), np.int8), detached((1, 8), np.float32), detached((32, 8), x_dt)
    with pytest.raises(AssertionError, match="the library was called"):
        wg.QuantizeQ8.from_device(None).dispatch(None, wg.ViewShapeBuffers(), _NoPass(), q, s, x, 32)
