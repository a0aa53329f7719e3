"""The 16-bit Gemm launcher's planner on the host (wgmath_amd/csrc/gemm16_plan.hip through wg_debug_gemm16_plan): no GPU, no context.

The launcher is "fill a query, ask the planner, do what the plan says", and it logs the tags the plan's tag function gives -- so the leaf a call takes can be
checked here, before anything runs on a device.

  test_table_*       the tables of expected launch logs that the GPU tests assert after real launches (test_gpu_epilogue.LEAVES, test_gpu_operands.EXTRA_LEAVES /
                     ODD_LEAF, test_gpu_launch_contexts.CTX_LEAF / RECORD_LEAF, test_gpu_bf16.F16_ROWS / REPLAY), imported, not copied: the planner gives every row
                     of them that this launcher decides the log the table states -- on the whole chip (256 CUs), on the masked contexts' CU counts, while recording,
                     for the operand layouts of those tests and with the bf16 prefix.
  test_invariants_*  the rules the launcher's comments state, over a grid of sizes: K cuts cover [0, K) in whole stages with the minimum per split, grid.y and
                     workspace limits, the continuous walk's preconditions, a padded call's inner call does not pad.
"""
import ctypes
import itertools

import pytest

from wgmath_amd import _lib
from test_gpu_bf16 import F16_ROWS, REPLAY, _bf_dtype_leaf
from test_gpu_epilogue import AB, F16, LEAVES, Row
from test_gpu_launch_contexts import CTX_LEAF, MASKED, RECORD_LEAF
from test_gpu_operands import EXTRA_LEAVES, LAYOUTS, ODD_LEAF

MiB = 1 << 20
KNOBS = {"f16_tile": "tile", "f16_sched": "sched", "f16_cont": "cont", "f16_balance": "balance"}
# decided in api.hip / gemv.hip before the 16-bit launcher is reached (staging of lengths that are not multiples of 4; N right-hand sides as a Gemv)
NOT_THIS_LAUNCHER = ("f16_staged", "f16_as_gemv")
# rows whose expectation depends on device state the query cannot express: none
LEFT_OUT = ()
ROWS = [r for r in LEAVES + EXTRA_LEAVES if r.dtype == F16 and r.name not in NOT_THIS_LAUNCHER + LEFT_OUT]
CASES = [pytest.param(r, tr, id=f"{r.name}-{'tr' if tr else 'nn'}") for r in ROWS for tr in r.variants]


def _geom(rs, cs, layout):
    """(offset, leading dimension, matrix stride) of an rs x cs block stored as tests/test_gpu_operands.py Stored stores it."""
    off, pad, gap, _ = LAYOUTS[layout]
    if pad is None:
        pad = 1 if rs % 2 == 0 else 2
    ld = max(rs + pad, 1)
    return off, ld, ld * cs + gap


def query(tr, M, K, N, mats, knobs=None, cus=256, uneven=False, alpha=1.0, beta=0.0, recording=False, layout="dense", out=None):
    """The query the launcher fills for op(A) (M x K) * B (K x N) on views laid out as `layout` (buffers start 256-byte aligned); out: (offset, ld, batch)."""
    q = _lib.Gemm16QueryC()
    q.trans, q.M, q.N, q.K, q.nmats = int(tr), M, N, K, mats
    (ao, q.lda, q.a_batch), (bo, q.ldb, q.b_batch) = _geom(*((K, M) if tr else (M, K)), layout), _geom(K, N, layout)
    co, q.ldc, q.c_batch = out or _geom(M, N, layout)
    q.a_addr, q.b_addr, q.c_addr = (2 * ao) & 15, (2 * bo) & 15, (2 * co) & 15
    q.alpha, q.beta, q.cus, q.uneven_xcds, q.recording = alpha, beta, cus, int(uneven), int(recording)
    q.tile, q.sched, q.cont, q.balance = 0, -1, -1, 0  # wg_ctx's defaults
    for k, v in (knobs or {}).items():
        if k in KNOBS:
            setattr(q, KNOBS[k], v)
    return q


def plan(q, prefix="f16"):
    p, inner, buf = _lib.Gemm16PlanC(), _lib.Gemm16QueryC(), ctypes.create_string_buffer(256)
    _lib.check(_lib.lib.wg_debug_gemm16_plan(ctypes.byref(q), prefix.encode(), ctypes.byref(p), buf, len(buf), ctypes.byref(inner)))
    return p, buf.value.decode(), inner


def tags(*a, prefix="f16", **kw):
    return plan(query(*a, **kw), prefix)[1]


def _for_prefix(prefix, row):
    """(leaf, ab, not_ab) of a row as the f16 tables state them, or with the bf16 prefix as tests/test_gpu_bf16.py expects them."""
    if prefix == "f16":
        return row.leaf, row.ab, row.not_ab
    return _bf_dtype_leaf(row.leaf), _bf_dtype_leaf(row.ab), None if row.not_ab is None else _bf_dtype_leaf(row.not_ab)[0]


@pytest.mark.parametrize("prefix", ["f16", "bf16"])
@pytest.mark.parametrize("row,tr", CASES)
def test_table_whole_chip(row, tr, prefix):
    """tests/test_gpu_epilogue.py and test_gpu_bf16.py: the (1, 0) log contains `leaf`, every (alpha, beta) log `ab` and not `not_ab` -- on the dense output view and
    (unless the leaf needs an aligned output) on the odd one: offset 1, ld = M + 3, 7 elements between matrices."""
    assert row in F16_ROWS  # (the rows test_gpu_bf16.py runs with the other prefix)
    M, K, N, mats = row.M, row.K, row.N, row.mats
    leaf, ab, not_ab = _for_prefix(prefix, row)
    odd_view = row in LEAVES and not row.dense_only  # (tests/test_gpu_epilogue.py runs the rows of LEAVES only)
    for out in (None, (1, M + 3, (M + 3) * N + 7)) if odd_view else (None,):
        log1 = tags(tr, M, K, N, mats, row.knobs, prefix=prefix, out=out)
        assert Row.took(leaf, log1), f"{row.name}: expected the leaf {leaf!r}, the plan logs {log1!r}"
        log3 = tags(tr, M, K, N, mats, row.knobs, alpha=2.0, beta=0.0, prefix=prefix, out=out)  # (step 3 there: the same kernels as (1, 0), or the (alpha, beta) leaf)
        assert log3 == log1 or Row.took(ab, log3, not_ab), f"{row.name} (2, 0): the plan logs {log3!r}"
        for alpha, beta in AB:
            log = tags(tr, M, K, N, mats, row.knobs, alpha=alpha, beta=beta, prefix=prefix, out=out)
            assert Row.took(ab, log, not_ab), f"{row.name} ({alpha}, {beta}): expected {ab!r} without {not_ab!r}, the plan logs {log!r}"


@pytest.mark.parametrize("layout", ["aligned", "odd"])
@pytest.mark.parametrize("row,tr", CASES)
def test_table_operand_layouts(row, tr, layout):
    """tests/test_gpu_operands.py: operands and output at 16-byte offsets with padded leading dimensions take the dense leaf; at offset 1 with odd leading dimensions
    the leaf ODD_LEAF states, else the dense one (behind the padding wrapper)."""
    leaf = ODD_LEAF.get((row.name, tr), row.leaf) if layout == "odd" else row.leaf
    log = tags(tr, row.M, row.K, row.N, row.mats, row.knobs, layout=layout)
    assert Row.took(leaf, log), f"{row.name} {layout}: expected {leaf!r}, the plan logs {log!r}"


@pytest.mark.parametrize("where", list(MASKED))
@pytest.mark.parametrize("row,tr", CASES)
def test_table_masked_contexts(row, tr, where):
    """tests/test_gpu_launch_contexts.py: on a CU-masked context the whole log CTX_LEAF states, or -- no entry -- the full chip's leaf."""
    cus, uneven = MASKED[where]
    log = tags(tr, row.M, row.K, row.N, row.mats, row.knobs, cus=cus, uneven=uneven)
    moved = CTX_LEAF.get((where, row.name, tr), CTX_LEAF.get((where, row.name)))
    if moved is not None:
        assert log == moved, f"{row.name} on {where}: expected {moved!r} (the CU count moves it), the plan logs {log!r}"
    else:
        assert Row.took(row.leaf, log), f"{row.name} on {where}: expected the full chip's {row.leaf!r}, the plan logs {log!r}"


@pytest.mark.parametrize("row,tr", CASES)
def test_table_recording(row, tr):
    """tests/test_gpu_launch_contexts.py: a recorded call logs the eager leaf, except where RECORD_LEAF says otherwise (no calibrated shares in a recording)."""
    leaf = RECORD_LEAF.get(row.name, row.leaf)
    log = tags(tr, row.M, row.K, row.N, row.mats, row.knobs, recording=True)
    assert Row.took(leaf, log), f"{row.name} recorded: expected {leaf!r}, the plan logs {log!r}"
    if row.name not in RECORD_LEAF:
        assert log == tags(tr, row.M, row.K, row.N, row.mats, row.knobs)


@pytest.mark.parametrize("name,M,K,N,knobs", REPLAY, ids=[r[0] for r in REPLAY])
def test_table_bf16_replay(name, M, K, N, knobs):
    """tests/test_gpu_bf16.py test_recorded_and_masked: a bf16 log, and the recorded call's log is the eager one's -- whole chip and 248 CUs with one short XCD."""
    for cus, uneven in ((256, False), (248, True)):
        log = tags(False, M, K, N, 1, knobs, cus=cus, uneven=uneven, prefix="bf16")
        assert log.startswith("bf16.") and "f16." not in log.replace("bf16.", ""), log
        assert tags(False, M, K, N, 1, knobs, cus=cus, uneven=uneven, recording=True, prefix="bf16") == log
        assert tags(False, M, K, N, 1, knobs, cus=cus, uneven=uneven).replace("f16.", "bf16.") == log


def test_debug_entry_rejects_null_arguments():
    q, p = _lib.Gemm16QueryC(), _lib.Gemm16PlanC()
    L = _lib.lib
    assert L.wg_debug_gemm16_plan(None, b"f16", ctypes.byref(p), None, 0, None) == _lib.WG_ERR_INVALID_ARG
    assert L.wg_debug_gemm16_plan(ctypes.byref(q), b"f16", None, None, 0, None) == _lib.WG_ERR_INVALID_ARG
    assert L.wg_debug_gemm16_plan(ctypes.byref(q), b"f16", ctypes.byref(p), None, 0, None) == _lib.WG_OK
    assert _lib.GEMM16_LEAVES[p.leaf] == "unsupported" and p.status == _lib.WG_OK and p.message == b""  # an empty product: nothing to launch


# ---- the launcher's own rules -----------------------------------------------------------------------------------------------------------------------
SIZES = (8, 64, 72, 192, 200, 256, 512, 1000, 1024, 1028, 4096, 4352, 8192, 16384)


def check_plan(q, p, inner, what):
    """The rules gemm16_plan.hip states in its comments, on one plan (tests/cpp/gemm16_plan_check.cpp asserts the same ones under the host sanitizers)."""
    leaf = _lib.GEMM16_LEAVES[p.leaf]
    if leaf == "unsupported":
        return leaf
    K, krem = q.K, q.K % 64
    if leaf == "pad":
        p2, _, _ = plan(inner)
        assert _lib.GEMM16_LEAVES[p2.leaf] not in ("pad", "unsupported"), f"{what}: the padded call's inner call is {_lib.GEMM16_LEAVES[p2.leaf]} ({p2.message})"
        assert inner.M % 8 == 0 and inner.K % 8 == 0 and inner.K >= 64 and inner.padded == 1, what
        return leaf
    ns, kps = p.nsplit, p.k_per_split
    assert 1 <= ns and q.nmats * ns <= 65535, what
    assert (ns - 1) * kps < K <= ns * kps + krem, f"{what}: {ns} splits of {kps} do not cover K"  # (the last split takes what is left, remainder included)
    if ns > 1:
        assert kps % 64 == 0, f"{what}: {ns} splits of {kps}"
        if leaf != "skinny":  # whole k of every split, the last one included: one stage (128 x 128 tiles), three (256 x 256: its DMA stream runs that far ahead)
            floor = {"t128": 64, "m16": 192}[leaf]
            assert kps >= floor and K - krem - (ns - 1) * kps >= floor and K - krem <= ns * kps, f"{what}: {ns} splits of {kps}"
        assert p.workspace_bytes == 4 * ns * q.M * q.N * q.nmats, what
    assert p.workspace_bytes <= 512 * MiB, f"{what}: {p.workspace_bytes} bytes of workspace"
    if leaf == "m16":
        tiles = p.tiles_m * p.tiles_n
        assert p.tiles_m == -(-q.M // 256) and p.tiles_n == -(-q.N // 256) and K - krem >= 192 and p.tail < tiles
        if p.tail:
            ts, tk = p.tail_split, p.tail_kps
            assert ns == 1 and q.nmats == 1 and 2 * p.tail <= q.cus and (tiles - p.tail) % q.cus == 0, what
            assert ts >= 2 and tk % 64 == 0 and tk >= 192 and K - krem - (ts - 1) * tk >= 192 and K - krem <= ts * tk, f"{what}: tail of {ts} splits of {tk}"
            assert p.workspace_bytes == ts * p.tail * 65536 * 4, what
        if p.cont:
            assert q.beta == 0.0 and krem == 0 and (tiles - p.tail) * q.nmats > q.cus and ns == 1 and p.nwg == q.cus and not p.queues, what
        if p.queues:
            assert ns == 1 and q.nmats == 1 and p.nwg % 8 == 0 and p.nwg >= tiles - p.tail, what
    return leaf


@pytest.mark.parametrize("cus", [8, 256])
@pytest.mark.parametrize("tr", [False, True])
def test_invariants_over_the_size_grid(tr, cus):
    seen = set()
    for M, N, K in itertools.product(SIZES, repeat=3):
        for mats, beta in itertools.product((1, 2, 8), (0.0, 1.0)):
            q = query(tr, M, K, N, mats, cus=cus, beta=beta)
            p, _, inner = plan(q)
            seen.add(check_plan(q, p, inner, f"{'tr' if tr else 'nn'} {M} x {K} x {N} x {mats} beta={beta} cus={cus}"))
    assert seen >= {"t256x128", "t128", "m16", "pad", "generic"} and (not tr or "skinny" in seen), seen  # (the grid reaches every family)


def test_invariants_with_forced_knobs_and_odd_layouts():
    """The same rules where a knob forces a family or the views are off: fewer sizes, every knob value the tables use."""
    sizes = (72, 200, 256, 1000, 1028, 4096, 4352)
    knobs = [{}, {"f16_tile": 128}, {"f16_tile": 256}, {"f16_tile": 256128}, {"f16_tile": 256, "f16_cont": 0}, {"f16_tile": 256, "f16_cont": 1},
             {"f16_tile": 256, "f16_sched": 1}, {"f16_tile": 256, "f16_sched": 0}, {"f16_tile": 256, "f16_balance": 1}]
    for (M, N, K), kn, layout, tr in itertools.product(itertools.product(sizes, repeat=3), knobs, ("dense", "odd"), (False, True)):
        for cus, uneven in ((256, False), (248, True)):
            q = query(tr, M, K, N, 1, kn, cus=cus, uneven=uneven, layout=layout)
            p, _, inner = plan(q)
            check_plan(q, p, inner, f"{'tr' if tr else 'nn'} {M} x {K} x {N} {kn} {layout} cus={cus}")
