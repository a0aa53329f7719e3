"""The Gemv launchers fill their query as the planner's tests assume: after a real call, wg_debug_gemv_plan / wg_debug_gemv_any_plan on a query filled HERE from the
real views -- shapes, strides, wg_buf_device_ptr modulo 16, the context's CU count and tuning -- logs exactly what wg_debug_take_path returns (for a staged call:
behind `stage>`). Every row of tests/test_gpu_operands.py GEMV_LEAVES on the dense and the odd layout, and the mixed cases of tests/test_gpu_gemv_mixed.py; the
operands' values do not matter (zeros). What the kernels compute on these shapes is those two files' business."""
import numpy as np
import pytest

import _gemv_plan as G
from test_gpu_epilogue import F16, knobs  # noqa: F401  (knobs: the fixture)
from test_gpu_gemv_mixed import CASES as MIXED_CASES, KINDS as MIXED_KINDS, build_case, mixed
from test_gpu_operands import GEMV_LEAVES, Stored, _gemv_call, _lib

pytestmark = pytest.mark.gpu


def _cus(gpu):
    info = gpu.adapter()
    return info.get("stream_compute_units", info["compute_units"])


def _assert_planned(gpu, log, elems, tr, R, C, nrhs, mats, m, v, o, bufs, what):
    """m, v, o: (offset, leading dimension, matrix stride) of the views the call was made on; bufs: the buffers of m and v."""
    L = _lib()
    r = G.route(L, elems, tr, R, C, nrhs, mats, m, v, o, base16=tuple(b.device_ptr() % 16 for b in bufs), cus=_cus(gpu), gemvt_lds=gpu.get_tuning("gemvt_lds"))
    assert r is not None, what
    kind, wrapper, q = r
    status, planned = G.planned(L, kind, q)
    assert status == 0 and log.startswith(wrapper), f"{what}: took {log!r}, planned {wrapper + planned!r}"
    rest = log[len(wrapper):]
    if L.GEMV_LEAVES[G.plan(L, q)[0].leaf] == "as_gemm16" and kind == G.K_GEMV:  # the 16-bit Gemm launcher's tags follow (its planner: tests/test_gpu_epilogue.py)
        assert rest.startswith(planned) and rest[len(planned):].startswith("f16.") and ".gemv" not in rest, f"{what}: took {log!r}, planned {planned!r}"
    else:
        assert rest == planned, f"{what}: took {log!r}, planned {wrapper + planned!r}"


@pytest.mark.parametrize("layout", ["dense", "odd"])
@pytest.mark.parametrize("row", GEMV_LEAVES, ids=[r.name for r in GEMV_LEAVES])
def test_launcher_fills_the_query_the_planner_reads(gpu, knobs, row, layout):
    ro, k = (row.C, row.R) if row.tr else (row.R, row.C)
    knobs(row.knobs)
    gpu.take_path()
    A, V = np.zeros((ro, k, row.mats)), np.zeros((k, row.nrhs, row.mats))
    m = Stored(gpu, A, row.dtype, layout, tr=row.tr, ld_mult=row.ld_mult if layout != "odd" else 1)
    vl = "odd" if row.vodd else layout
    v = Stored(gpu, V, row.dtype, vl)
    out = Stored(gpu, np.zeros((ro, row.nrhs, row.mats)), row.dtype, vl)
    _gemv_call(gpu, row, out, m, v)
    log = gpu.take_path()
    _assert_planned(gpu, log, "f16" if row.dtype == F16 else "f32", row.tr, row.R, row.C, row.nrhs, row.mats, *((s.off, s.ld, s.batch) for s in (m, v, out)), (m.buf, v.buf),
                    f"{row.name} {layout}")


@pytest.mark.parametrize("kind", MIXED_KINDS)
@pytest.mark.parametrize("case", MIXED_CASES, ids=[c[0] for c in MIXED_CASES])
def test_mixed_launcher_fills_the_query_the_planner_reads(gpu, case, kind):
    name, _, R, C, nrhs, Z = case[:6]
    tr, _, _, _, m, v, out = build_case(gpu, case, kind, np.random.default_rng(0), integers=True)
    gpu.take_path()
    mixed(gpu, tr, kind, out, m, v)
    log = gpu.take_path()
    _assert_planned(gpu, log, kind + "w", tr, R, C, nrhs, Z, *((s.shape.offset, s.ld, s.batch) for s in (m, v, out)), (m.buf, v.buf), f"{name} {kind}")
