"""The f32 Gemm launcher's planner on the host (wgmath_amd/csrc/gemm32_plan.hip through wg_debug_gemm32_plan): no GPU, no context.

The launcher is "fill a query, ask the planner, do what the plan says", and it logs the tags the plan's tag function gives -- so the leaf a call takes can be
checked here, before anything runs on a device.

  test_golden_parent  tests/golden/gemm32_plan_parent.json: the launch logs of f32 wg_gemm_ex calls with the launcher as it was BEFORE it was split into planner and
                      executor -- real calls on an MI355X, and that launcher built for the host for the contexts and leading dimensions no recording reached
                      (tests/golden/make_gemm32_plan_golden.py). The planner gives every row exactly the recorded log.
  test_table_*        the tables of expected launch logs that the GPU tests assert after real launches (test_gpu_epilogue.LEAVES, test_gpu_operands.EXTRA_LEAVES /
                      ODD_LEAF, the f32 and gemv:*_gemm entries of test_gpu_launch_contexts.CTX_LEAF / RECORD_LEAF), imported, not copied.
  test_invariants_*   the rules the launcher's comments state, over a grid of sizes and leading dimensions (past the 32-bit DMA-offset limits too).
"""
import ctypes
import itertools
import json
import os

import pytest

from wgmath_amd import _lib
from test_gpu_epilogue import AB, F32, LEAVES, Row
from test_gpu_launch_contexts import CTX_LEAF, MASKED, RECORD_LEAF
from test_gpu_operands import EXTRA_LEAVES, GEMV_LEAVES, LAYOUTS, ODD_LEAF

MiB = 1 << 20
KNOBS = {"f32_mid": "mid", "f32_mid_split": "mid_split", "f32_skinny": "skinny", "f32_panels": "panels"}
# decided before the f32 launcher is reached: api.hip (staging of lengths that are not multiples of 4; 1 .. 7 right-hand sides as a Gemv) and gemv.hip (on 8 CUs
# 4096 outputs are 128 per CU and more: GemvTr with 8 right-hand sides takes the LDS kernel, not the hand-off to the few-column Gemm kernel)
NOT_THIS_LAUNCHER = ("f32_staged", "f32_as_gemv", ("cu8", "gemv:f32_tr_8rhs_gemm"))
LEFT_OUT = ()
ROWS = [r for r in LEAVES + EXTRA_LEAVES if r.dtype == F32 and r.name not in NOT_THIS_LAUNCHER + LEFT_OUT]
CASES = [pytest.param(r, tr, id=f"{r.name}-{'tr' if tr else 'nn'}") for r in ROWS for tr in r.variants]
GEMV_HANDOFFS = [r for r in GEMV_LEAVES if r.dtype == F32 and r.name.endswith("_gemm")]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm32_plan_parent.json")
LEAF = _lib.GEMM32_LEAVES


def _geom(rs, cs, layout):
    """(leading dimension, matrix stride) of an rs x cs block stored as tests/test_gpu_operands.py Stored stores it."""
    _, pad, gap, _ = LAYOUTS[layout]
    if pad is None:
        pad = 1 if rs % 2 == 0 else 2
    ld = max(rs + pad, 1)
    return ld, ld * cs + gap


def query(tr, M, K, N, mats=1, knobs=None, cus=256, alpha=1.0, beta=0.0, layout="dense", out=None, lda=None, ldb=None):
    """The query the launcher fills for op(A) (M x K) * B (K x N) on views laid out as `layout`; out: (ld, batch); lda / ldb: leading dimensions instead."""
    q = _lib.Gemm32QueryC()
    q.trans, q.M, q.N, q.K, q.nmats = int(tr), M, N, K, mats
    (q.lda, q.a_batch), (q.ldb, q.b_batch) = _geom(*((K, M) if tr else (M, K)), layout), _geom(K, N, layout)
    if lda:
        q.lda, q.a_batch = lda, lda * (M if tr else K)
    if ldb:
        q.ldb, q.b_batch = ldb, ldb * N
    q.ldc, q.c_batch = out or _geom(M, N, layout)
    q.alpha, q.beta, q.cus = alpha, beta, cus
    q.mid, q.mid_split, q.skinny, q.panels = -1, 0, -1, -1  # wg_ctx's defaults
    for k, v in (knobs or {}).items():
        if k in KNOBS:
            setattr(q, KNOBS[k], v)
    return q


def plan(q):
    p, inner, buf = _lib.Gemm32PlanC(), _lib.Gemm32QueryC(), ctypes.create_string_buffer(256)
    _lib.check(_lib.lib.wg_debug_gemm32_plan(ctypes.byref(q), ctypes.byref(p), buf, len(buf), ctypes.byref(inner)))
    return p, buf.value.decode(), inner


def tags(*a, **kw):
    return plan(query(*a, **kw))[1]


# ---- the parent's launcher, row by row ----------------------------------------------------------------------------------------------------------------
def test_golden_parent():
    """Every recorded call: the planner's tags are exactly the log the launcher left before the split, and a call it refused is refused with the same status."""
    assert LEFT_OUT == ()
    doc = json.load(open(GOLDEN))
    fields, rows = doc["fields"], doc["rows"]
    assert len(doc["parent_commit"]) >= 7 and len(rows) > 500
    assert {r[fields.index("ret")] for r in rows} == set(range(len(doc["returns"])))  # (every return the table lists is taken by a row)
    cus, src = fields.index("cus"), fields.index("src")
    assert {r[cus] for r in rows} == {256} | {n for n, _ in MASKED.values()}
    # src 0: recorded on an MI355X; src 1: the same launcher built for the host (tests/golden/make_gemm32_plan_golden.py: it reproduces every src-0 row) -- the
    # 100- and 8-CU contexts and the leading dimensions past the 32-bit offset limits
    assert {(r[cus], r[src]) for r in rows} == {(256, 0), (248, 0), (224, 0), (100, 1), (8, 1), (256, 1)}
    wrong = []
    for r in rows:
        d = dict(zip(fields, r))
        q = _lib.Gemm32QueryC()
        for f in ("trans", "M", "N", "K", "nmats", "lda", "ldb", "ldc", "a_batch", "b_batch", "c_batch", "alpha", "beta", "cus", "mid", "mid_split", "skinny", "panels"):
            setattr(q, f, d[f])
        p, log, _ = plan(q)
        status = p.status if LEAF[p.leaf] in ("nothing", "unsupported") else 0
        if log != d["log"] or status != d["status"]:
            wrong.append((r, log, status))
    assert not wrong, f"{len(wrong)} of {len(rows)} rows differ from the parent's launcher; the first: {wrong[:5]}"


# ---- the tables the GPU tests assert ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row,tr", CASES)
def test_table_whole_chip(row, tr):
    """tests/test_gpu_epilogue.py: the (1, 0) log contains `leaf`, every (alpha, beta) log `ab` and not `not_ab` -- on the dense output view and on the odd one:
    ld = M + 5, 7 elements between matrices."""
    M, K, N, mats = row.M, row.K, row.N, row.mats
    odd_view = row in LEAVES and not row.dense_only  # (tests/test_gpu_epilogue.py runs the rows of LEAVES only)
    for out in (None, (M + 5, (M + 5) * N + 7)) if odd_view else (None,):
        log1 = tags(tr, M, K, N, mats, row.knobs, out=out)
        assert Row.took(row.leaf, log1), f"{row.name}: expected the leaf {row.leaf!r}, the plan logs {log1!r}"
        log3 = tags(tr, M, K, N, mats, row.knobs, alpha=-1.5, beta=0.0, out=out)  # (step 3 there: the same kernels as (1, 0), or the (alpha, beta) leaf)
        assert log3 == log1 or Row.took(row.ab, log3, row.not_ab), f"{row.name} (-1.5, 0): the plan logs {log3!r}"
        for alpha, beta in AB:
            log = tags(tr, M, K, N, mats, row.knobs, alpha=alpha, beta=beta, out=out)
            assert Row.took(row.ab, log, row.not_ab), f"{row.name} ({alpha}, {beta}): expected {row.ab!r} without {row.not_ab!r}, the plan logs {log!r}"


@pytest.mark.parametrize("layout", ["aligned", "odd"])
@pytest.mark.parametrize("row,tr", CASES)
def test_table_operand_layouts(row, tr, layout):
    """tests/test_gpu_operands.py: operands and output at offsets with padded or odd leading dimensions take the dense leaf (ODD_LEAF names no f32 row of this launcher)."""
    leaf = ODD_LEAF.get((row.name, tr), row.leaf) if layout == "odd" else row.leaf
    log = tags(tr, row.M, row.K, row.N, row.mats, row.knobs, layout=layout)
    assert Row.took(leaf, log), f"{row.name} {layout}: expected {leaf!r}, the plan logs {log!r}"


@pytest.mark.parametrize("tr", [False, True])
def test_table_odd_leaf_of_the_gemv_row(tr):
    """ODD_LEAF's f32 entries: 512 x 256 x 3 at odd offsets is no Gemv (api.hip) and reaches this launcher with N = 3."""
    row = next(r for r in LEAVES if r.name == "f32_as_gemv")
    assert tags(tr, row.M, row.K, row.N, row.mats, layout="odd") == ODD_LEAF[(row.name, tr)]


@pytest.mark.parametrize("where", ["full"] + list(MASKED))
@pytest.mark.parametrize("row,tr", CASES)
def test_table_masked_contexts(row, tr, where):
    """tests/test_gpu_launch_contexts.py: on a CU-masked context the whole log CTX_LEAF states, or -- no entry -- the full chip's leaf."""
    cus = 256 if where == "full" else MASKED[where][0]
    log = tags(tr, row.M, row.K, row.N, row.mats, row.knobs, cus=cus)
    moved = CTX_LEAF.get((where, row.name, tr), CTX_LEAF.get((where, row.name)))
    if moved is not None:
        assert log == moved, f"{row.name} on {where}: expected {moved!r} (the CU count moves it), the plan logs {log!r}"
    else:
        assert Row.took(row.leaf, log), f"{row.name} on {where}: expected the full chip's {row.leaf!r}, the plan logs {log!r}"


@pytest.mark.parametrize("where", ["full"] + list(MASKED))
@pytest.mark.parametrize("row", GEMV_HANDOFFS, ids=[r.name for r in GEMV_HANDOFFS])
def test_table_gemv_handoffs(row, where):
    """The Gemv launcher's hand-off to the few-column kernel (gemv.hip: gemm32_skinny_plan) is the plan of the same product as a Gemm with nrhs columns."""
    key = (where, "gemv:" + row.name)
    if key in NOT_THIS_LAUNCHER:
        assert "f32." not in CTX_LEAF[key]
        return
    want = CTX_LEAF.get(key, row.leaf)
    assert want.startswith("gemv>f32.skinny/"), want
    rows_out, k = (row.C, row.R) if row.tr else (row.R, row.C)
    cus = 256 if where == "full" else MASKED[where][0]
    assert "gemv>" + tags(row.tr, rows_out, k, row.nrhs, row.mats, cus=cus) == want


def test_table_recording():
    """tests/test_gpu_launch_contexts.py RECORD_LEAF: recording moves no f32 row (the f32 query has no such field)."""
    assert not [k for k in RECORD_LEAF if k.startswith(("f32", "gemv:f32"))]
    assert not hasattr(_lib.Gemm32QueryC(), "recording")


def test_debug_entry_rejects_null_arguments():
    q, p = _lib.Gemm32QueryC(), _lib.Gemm32PlanC()
    L = _lib.lib
    assert L.wg_debug_gemm32_plan(None, ctypes.byref(p), None, 0, None) == _lib.WG_ERR_INVALID_ARG
    assert L.wg_debug_gemm32_plan(ctypes.byref(q), None, None, 0, None) == _lib.WG_ERR_INVALID_ARG
    assert L.wg_debug_gemm32_plan(ctypes.byref(q), ctypes.byref(p), None, 0, None) == _lib.WG_OK
    assert LEAF[p.leaf] == "nothing" and p.status == _lib.WG_OK and p.message == b""  # an empty product: nothing to launch


# ---- the launcher's own rules -----------------------------------------------------------------------------------------------------------------------
SIZES = (4, 16, 48, 64, 96, 128, 132, 512, 1000, 1024, 4096, 4352, 16384)
KS = (4, 32, 100, 128, 160, 256, 1024, 4100, 32768)
# leading dimensions past the 32-bit DMA-offset limits: ld x rows x 4 bytes >= 2^31 for the 256- / 128-row tiles, the 64-column and the 32-row blocks
BIG_LDS = (1 << 21, 1 << 22, 1 << 23, 1 << 24, (1 << 24) + 4)


def _mid_ok(q):
    return q.K >= 32 and q.K % 4 == 0 and q.M >= 4 and q.N >= 4 and q.nmats <= 65535 and q.lda * 512 < 1 << 31 and q.ldb * 512 < 1 << 31


def check_plan(q, p, inner, what):
    """The rules gemm32_plan.hip states in its comments, on one plan (tests/cpp/gemm32_plan_check.cpp asserts the same ones under the host sanitizers)."""
    leaf = LEAF[p.leaf]
    M, N, K, Z = q.M, q.N, q.K, q.nmats
    if q.mid > 1 and _mid_ok(q) and Z <= 65535:  # a forced tile goes past everything else
        assert leaf in ("mid", "unsupported") and (leaf != "mid" or p.bm * 1000 + p.bn == q.mid), f"{what}: tile {q.mid} forced, took {leaf} {p.bm} x {p.bn}"
    if leaf in ("nothing", "unsupported"):
        assert leaf == "unsupported" or (p.status == 0 and 0 in (M, N, Z)), what
        assert leaf == "nothing" or (p.status != 0 and p.message), what
        return leaf
    assert q.beta == 0.0 or leaf not in ("fewrow", "skinny_t"), f"{what}: beta != 0 needs the old output inside the transposed product"
    assert q.mid != 0 or leaf != "mid", f"{what}: the mid family is off"
    assert q.panels != 0 or leaf != "skinny_panels", f"{what}: the panels are off"
    if q.skinny == 1 and q.mid <= 1 and N <= 64 and M >= 512 and K >= 128 and q.lda * 128 < 1 << 31 and q.ldb * 256 < 1 << 31:
        assert leaf == "skinny", f"{what}: the few-column kernel forced, took {leaf}"
    if leaf == "fewrow":
        p2, _, _ = plan(inner)
        assert LEAF[p2.leaf] not in ("fewrow", "nothing", "unsupported"), f"{what}: the few-row form's inner call is {LEAF[p2.leaf]} ({p2.message})"
        assert (inner.trans, inner.M, inner.N, inner.K, inner.beta) == (1, N, M, K, 0.0) and inner.ldc == N and inner.lda == q.ldb, what
        assert inner.ldb == (q.lda if q.trans else K) and p.copy_a == (not q.trans) and M <= 128, what
        assert p.pad_workspace_bytes == 4 * Z * (N * M + (0 if q.trans else K * M)) and p.workspace_bytes == 0, what
        return leaf
    ns, kps = p.nsplit, p.k_per_split
    assert 1 <= ns and Z * ns <= 65535 and Z * p.tail_sp <= 65535 * max(1, Z), what
    assert (ns - 1) * kps < K <= ns * kps, f"{what}: {ns} splits of {kps} do not cover K without an empty one"
    rows, cols = (N, M) if leaf == "skinny_t" else (M, N)
    if ns > 1:
        assert p.workspace_bytes == 4 * ns * M * N * Z, what
        if leaf == "big":  # >= 8 k-tiles of 16 per split
            assert kps % 16 == 0 and kps >= 128 and not p.tail_r, f"{what}: {ns} splits of {kps}"
        elif leaf == "mid":  # whole 32-k tiles, a whole one in the last split; by estimate >= 256 k per split (a forced count: whatever it gives)
            assert kps % 32 == 0 and K - (ns - 1) * kps >= 32 and (q.mid_split > 1 or kps >= 256) and p.bm != 128 and p.bn != 128, f"{what}: {ns} splits of {kps}"
        else:  # the few-column kernels: 32 k per stage, at most one split per started 128 k -- so >= 128 k per split where 128 divides K
            assert kps % 32 == 0 and ns <= -(-K // 128) and (K % 128 or kps >= 128), f"{what}: {ns} splits of {kps}"
    elif not p.tail_r:
        assert p.workspace_bytes == 0 and kps == K or leaf.startswith("skinny"), what
    if leaf.startswith("skinny"):
        assert p.npanels == (-(-cols // 64) if cols > 64 else 1) and Z * p.npanels <= 65535 and (leaf == "skinny_panels") == (p.npanels > 1), what
    if leaf != "mid":  # (the parent caps the slabs of the 256 x 128 tiles, of their cut-up tail and of the few-column kernels)
        assert p.workspace_bytes <= 512 * MiB, f"{what}: {p.workspace_bytes} bytes of workspace"
    if leaf == "big" and p.tail_r:
        tiles = -(-M // 256) * -(-N // 128) * Z
        ts, tk = p.tail_sp, p.tail_kps
        assert ns == 1 and 0 < p.tail_r < tiles and (tiles - p.tail_r) % q.cus == 0 and p.flat_tiles == (tiles // Z if Z > 1 else 0), f"{what}: tail of {p.tail_r}"
        assert ts >= 2 and tk % 16 == 0 and tk >= 128 and (ts - 1) * tk < K <= ts * tk and ts <= 65535, f"{what}: tail of {ts} splits of {tk}"
        assert p.workspace_bytes == ts * p.tail_r * 256 * 128 * 4, what
    return leaf


@pytest.mark.parametrize("cus", [8, 100, 256])
@pytest.mark.parametrize("tr", [False, True])
def test_invariants_over_the_size_grid(tr, cus):
    seen = set()
    for M, N, K in itertools.product(SIZES, SIZES, KS):
        for mats, beta in ((1, 0.0), (1, 1.0), (3, 0.0), (64, 0.0)):
            q = query(tr, M, K, N, mats, cus=cus, beta=beta)
            p, _, inner = plan(q)
            seen.add(check_plan(q, p, inner, f"{'tr' if tr else 'nn'} {M} x {K} x {N} x {mats} beta={beta} cus={cus}"))
    assert seen >= {"mid", "skinny", "skinny_panels", "skinny_t", "fewrow", "big"}, seen  # (the grid reaches every family)


def test_invariants_with_forced_knobs_and_odd_layouts():
    """The same rules where a knob forces a family or the views are off: fewer sizes, every knob value the tables and tests/test_gpu_parity.py use."""
    sizes = (16, 64, 96, 192, 512, 1000, 4352)
    knobs = [{"f32_mid": t} for t in (0, 1, 128128, 128064, 64128, 64064, 64032, 32064, 96096, 96064, 64096)]
    knobs += [{"f32_mid": t, "f32_mid_split": s} for t in (64064, 64032, 128064, 1, -1) for s in (2, 3, 4, 8, 64)]
    knobs += [{"f32_panels": 0}, {"f32_panels": 1}, {"f32_skinny": 0}, {"f32_skinny": 1}, {"f32_mid": 0, "f32_panels": 0}, {"f32_mid": 0, "f32_panels": 1}]
    for (M, N), K, kn, tr in itertools.product(itertools.product(sizes, repeat=2), (32, 96, 256, 4096), knobs, (False, True)):
        for cus, layout, mats in ((256, "dense", 1), (248, "odd", 2)):
            q = query(tr, M, K, N, mats, kn, cus=cus, layout=layout)
            p, _, inner = plan(q)
            check_plan(q, p, inner, f"{'tr' if tr else 'nn'} {M} x {K} x {N} x {mats} {kn} {layout} cus={cus}")


def test_invariants_past_the_dma_offset_limits():
    """Leading dimensions whose tiles no longer fit 32-bit byte offsets: the families that build such offsets are not taken, the few-row form falls back to
    transposed copies (the branches behind dma_ok == false; the kernels those plans name run on real operands with such leading dimensions in
    tests/test_gpu_far_views.py, whose thresholds tests/test_far_views_host.py finds), and every rule above still holds."""
    seen = set()
    for (M, N, K), lda, ldb, tr, beta in itertools.product(((16, 4096, 256), (64, 16384, 1024), (96, 8192, 256), (4096, 16, 1024), (512, 512, 512), (4096, 4096, 256)),
                                                          (None,) + BIG_LDS, (None,) + BIG_LDS, (False, True), (0.0, 1.0)):
        q = query(tr, M, K, N, lda=lda, ldb=ldb, beta=beta)
        p, _, inner = plan(q)
        leaf = check_plan(q, p, inner, f"{'tr' if tr else 'nn'} {M} x {K} x {N} lda={lda} ldb={ldb} beta={beta}")
        seen.add(leaf)
        if leaf.startswith("skinny"):  # 32 rows (or k) of the streamed operand and 64 columns of the other within 2^31 bytes
            a, b = (q.ldb, q.lda) if leaf == "skinny_t" else (q.lda, q.ldb)
            assert a * 128 < 1 << 31 and b * 256 < 1 << 31, (leaf, lda, ldb)
        if leaf == "mid":
            assert _mid_ok(q)
        if M <= 64 and N >= 512 and beta == 0.0 and (q.ldb * 128 >= 1 << 31 or q.lda * 256 >= 1 << 31) and not (_mid_ok(q) and M >= 48):
            assert leaf == "fewrow", f"{M} x {K} x {N} lda={lda} ldb={ldb}: {leaf}"
    assert seen >= {"fewrow", "big", "skinny", "skinny_t"}, seen


def test_limits_no_launch_reaches():
    """The refusals no real operands reach: more tiles than a grid holds, and matrices x splits past grid.y."""
    p, log, _ = plan(query(False, 1 << 31, 4, 1 << 24, knobs={"f32_mid": 0, "f32_panels": 0}))
    assert LEAF[p.leaf] == "unsupported" and p.status == _lib.WG_ERR_UNSUPPORTED and b"too many tiles" in p.message and log == ""
    p, log, _ = plan(query(False, 4, 4, 4, 65536))
    assert LEAF[p.leaf] == "unsupported" and b"65535 matrices" in p.message and log == ""
