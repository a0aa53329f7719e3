"""The Gemv launchers' planner on the host (wgmath_amd/csrc/gemv_plan.hip through wg_debug_gemv_plan / wg_debug_gemv_any_plan): no GPU, no context.

The launchers (gemv.hip, gemv_any.hip, the fused Gemv + Reduce) are "fill a query, ask the planner, do what the plan says", and they log the tags the plan gives -- so
the leaf a call takes can be checked here, before anything runs on a device. tests/_gemv_plan.py restates which launcher api.hip reaches with which query.

  test_golden_parent  tests/golden/gemv_plan_parent.json: the launch logs of wg_gemv, wg_gemv_mixed and wg_gemv_reduce calls with the launchers as they were BEFORE
                      they were split into planner and executors -- real calls on an MI355X on the whole chip and on every masked context, and those launchers built
                      for the host for what no device holds (tests/golden/make_gemv_plan_golden.py). The planner gives every row exactly the recorded log.
  test_table_*        the tables of expected launch logs that the GPU tests assert after real launches (test_gpu_operands.GEMV_LEAVES, the gemv:* and gemv_reduce:*
                      entries of test_gpu_launch_contexts.CTX_LEAF / RECORD_LEAF, test_gpu_gemv_mixed.CASES), imported, not copied.
  test_invariants_*   the rules the planner's comments state, over a grid of sizes, element types and leading dimensions (tests/cpp/gemv_plan_check.cpp asserts the
                      same ones on a larger grid under the host sanitizers).
"""
import itertools
import json
import os

import pytest

import _gemv_plan as G
from wgmath_amd import _lib
from test_gpu_epilogue import F16, Row
from test_gpu_gemv_mixed import CASES as MIXED_CASES, KINDS as MIXED_KINDS, REPLAY as MIXED_REPLAY
from test_gpu_launch_contexts import CTX_LEAF, GEMV_REDUCE_SHAPES, MASKED, RECORD_LEAF
from test_gpu_operands import GEMV_LEAVES, LAYOUTS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemv_plan_parent.json")
LEAF = _lib.GEMV_LEAVES
LEFT_OUT = ()
WHERE = ["full"] + list(MASKED)


def _cus(where):
    return 256 if where == "full" else MASKED[where][0]


def _stored(rs, cs, layout, ld_mult=1):
    """(offset, leading dimension, matrix stride) of an rs x cs block stored as tests/test_gpu_operands.py Stored stores it."""
    off, pad, gap, _ = LAYOUTS[layout]
    if pad is None:
        pad = 1 if rs % 2 == 0 else 2
    ld = -(-max(rs + pad, 1) // ld_mult) * ld_mult
    return off, ld, ld * cs + gap


def log_of(elems, tr, R, C, nrhs, mats, m, v, o, cus=256, gemvt_lds=0):
    """The log a call leaves, by api.hip's routing and the planner: the wrapper, then the planner's tags."""
    r = G.route(_lib, elems, tr, R, C, nrhs, mats, m, v, o, cus=cus, gemvt_lds=gemvt_lds)
    if r is None:
        return ""
    kind, wrapper, q = r
    status, log = G.planned(_lib, kind, q)
    assert status == 0, (status, log)
    return wrapper + log


def row_log(row, layout, cus=256):
    ro, k = (row.C, row.R) if row.tr else (row.R, row.C)
    vl = "odd" if row.vodd else layout
    return log_of("f16" if row.dtype == F16 else "f32", row.tr, row.R, row.C, row.nrhs, row.mats, _stored(row.R, row.C, layout, row.ld_mult if layout != "odd" else 1),
                  _stored(k, row.nrhs, vl), _stored(ro, row.nrhs, vl), cus, row.knobs.get("gemvt_lds", 0))


def _to_gemm16(leaf):
    return isinstance(leaf, str) and leaf.startswith("gemv>f16.") and not leaf.startswith("gemv>f16.gemv")


def took(leaf, log, not_=None):
    """Row.took for logs that end at the hand-off to the 16-bit Gemm launcher: a leaf "gemv>f16.t128/..." is held to its "gemv>" here (that launcher's planner has its own
    test, tests/test_gemm16_plan_host.py)."""
    if _to_gemm16(leaf):
        return log == "gemv>"
    return Row.took(leaf, log, not_)


# ---- the parent's launchers, row by row ---------------------------------------------------------------------------------------------------------------
def test_golden_parent():
    """Every recorded call: the planner's tags are exactly the log the launchers left before the split, and a call they refused is refused with the same status."""
    assert LEFT_OUT == ()
    doc = json.load(open(GOLDEN))
    fields, rows = doc["fields"], doc["rows"]
    assert tuple(fields) == G.FIELDS and len(doc["parent_commit"]) >= 7 and len(rows) > 1000
    assert {r[fields.index("ret")] for r in rows} == set(range(len(doc["returns"])))  # (every return the table lists is taken by a row)
    cus, src = fields.index("cus"), fields.index("src")
    # src 0: recorded on an MI355X, the whole chip and every masked context; src 1: the same launchers built for the host (it reproduces every src-0 row) for
    # operands no device holds. (A row without a launch carries an empty query: cus 0.)
    assert {(r[cus], r[src]) for r in rows if r[cus]} == {(256, 0), (256, 1)} | {(n, 0) for n, _ in MASKED.values()}
    wrong = []
    for r in rows:
        d = dict(zip(fields, r))
        status, log = G.planned(_lib, d["kind"], G.query(_lib, **{f: d[f] for f in G.QUERY}))
        rec = d["log"][len("stage>"):] if d["log"].startswith("stage>") else d["log"]
        if log.endswith("gemv>") and status == 0 and rec != log:  # handed to the 16-bit Gemm launcher: its tags follow, never a Gemv tag
            ok = rec.startswith(log) and rec[len(log):].startswith("bf16." if d["bf16"] else "f16.") and ".gemv" not in rec
        elif d["kind"] == G.K_REDUCE and log.startswith("gemv_reduce.two>"):  # ... then the Reduce launch's own tag
            ok = rec.startswith(log + " reduce.")
        else:
            ok = rec == log
        if not ok or status != d["status"]:
            wrong.append((r, log, status))
    assert not wrong, f"{len(wrong)} of {len(rows)} rows differ from the parent's launchers; the first: {wrong[:5]}"


# ---- the tables the GPU tests assert ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("row", GEMV_LEAVES, ids=[r.name for r in GEMV_LEAVES])
def test_table_operand_layouts(row, layout):
    """tests/test_gpu_operands.py test_gemv_leaf_operands: the dense and the aligned layout take the row's leaf, the odd one `row.odd`."""
    leaf, not_ = (row.odd, None) if layout == "odd" else (row.leaf, row.not_)
    log = row_log(row, layout)
    assert took(leaf, log, not_), f"{row.name} {layout}: expected {leaf!r}, the plan logs {log!r}"


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("row", GEMV_LEAVES, ids=[r.name for r in GEMV_LEAVES])
def test_table_masked_contexts(row, where):
    """tests/test_gpu_launch_contexts.py test_gemv_leaf_in_context: on a CU-masked context the whole log CTX_LEAF states, or -- no entry -- the full chip's leaf."""
    log = row_log(row, "dense", _cus(where))
    moved = CTX_LEAF.get((where, "gemv:" + row.name))
    if moved is None:
        assert took(row.leaf, log, row.not_), f"{row.name} on {where}: expected the full chip's {row.leaf!r}, the plan logs {log!r}"
    elif _to_gemm16(moved):
        assert log == "gemv>", f"{row.name} on {where}: {log!r}"
    else:
        assert log == moved, f"{row.name} on {where}: expected {moved!r} (the CU count moves it), the plan logs {log!r}"


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("R,C,leaf", GEMV_REDUCE_SHAPES, ids=[f"{R}x{C}" for R, C, _ in GEMV_REDUCE_SHAPES])
def test_table_gemv_reduce(R, C, leaf, where):
    """tests/test_gpu_launch_contexts.py test_gemv_reduce_in_context: fused exactly where wg_gemv would take gemv.small; the Reduce launch's tag ends the other logs."""
    _, _, q = G.route(_lib, "f32", False, R, C, 1, 1, _stored(R, C, "aligned"), (0, C, C), (0, R, R), cus=_cus(where))
    status, log = G.planned(_lib, G.K_REDUCE, q)
    moved = CTX_LEAF.get((where, f"gemv_reduce:{R}x{C}"))
    assert status == 0 and (moved.startswith(log + " reduce.") if moved else leaf in log), f"{R} x {C} on {where}: expected {moved or leaf!r}, the plan logs {log!r}"
    assert G.fused_reduce(_lib, q) == log.startswith("gemv.small_reduce/")


def test_table_recording():
    """RECORD_LEAF: recording moves no Gemv row (the query has no such field)."""
    assert not [k for k in RECORD_LEAF if k.startswith("gemv")]
    assert not hasattr(_lib.GemvQueryC(), "recording")


@pytest.mark.parametrize("kind", MIXED_KINDS)
@pytest.mark.parametrize("case", MIXED_CASES, ids=[c[0] for c in MIXED_CASES])
def test_table_mixed(case, kind):
    """tests/test_gpu_gemv_mixed.py CASES: the tags behind the element prefix, on the views build_case builds; on the masked contexts (REPLAY rows there) the tags of
    the 16-bit wg_gemv call of the same shape, as that test asserts."""
    name, tr, R, C, nrhs, Z, (moff, mpad), voff, want = case
    ro, k = (C, R) if tr else (R, C)
    views = ((moff, R + mpad, (R + mpad) * C + mpad), (voff, k + voff, (k + voff) * nrhs), (voff, ro + voff, (ro + voff) * nrhs))
    log = log_of(kind + "w", tr, R, C, nrhs, Z, *views)
    assert all(t in log for t in want) and ("gemv_any/" in log or f"{kind}w.gemv" in log), f"{name} {kind}: expected {want}, the plan logs {log!r}"
    if case in MIXED_REPLAY:
        for where in MASKED:
            mixed, same16 = (log_of(e, tr, R, C, nrhs, Z, *views, cus=_cus(where)) for e in (kind + "w", kind))
            assert mixed.replace(f"{kind}w.gemv", f"{kind}.gemv") == same16, (name, where, mixed, same16)


def test_debug_entries_reject_null_arguments():
    import ctypes
    q, p, a = _lib.GemvQueryC(), _lib.GemvPlanC(), _lib.GemvAnyPlanC()
    L = _lib.lib
    assert L.wg_debug_gemv_plan(None, ctypes.byref(p), None, 0) == _lib.WG_ERR_INVALID_ARG
    assert L.wg_debug_gemv_plan(ctypes.byref(q), None, None, 0) == _lib.WG_ERR_INVALID_ARG
    assert L.wg_debug_gemv_any_plan(ctypes.byref(q), None, None, 0) == _lib.WG_ERR_INVALID_ARG
    assert L.wg_debug_gemv_plan(ctypes.byref(q), ctypes.byref(p), None, 0) == _lib.WG_OK and LEAF[p.leaf] == "nothing" and p.status == _lib.WG_OK
    assert L.wg_debug_gemv_any_plan(ctypes.byref(q), ctypes.byref(a), None, 0) == _lib.WG_OK and not a.launch and a.status == _lib.WG_OK


# ---- the planner's own rules --------------------------------------------------------------------------------------------------------------------------
OUTS = (4, 64, 124, 128, 1024, 2048, 4096, 16384, 65536)
KS = (0, 4, 64, 68, 1024, 2052, 4096, 8192, 16384, 65536)
MiB = 1 << 20


def check_plan(q, what):
    """The rules gemv_plan.hip states, on one plan; returns the leaf's name."""
    p, log = G.plan(_lib, q)
    leaf = LEAF[p.leaf]
    outs, k, nrhs, Z, ns, kps = q.rows_out, q.k, q.nrhs, q.nmats, p.nsplit, p.k_per_split
    groups = -(-nrhs // 8)
    if leaf == "unsupported":
        assert p.status == _lib.WG_ERR_UNSUPPORTED and p.message and (Z * groups > 65535 or LEAF[p.leaf] == "unsupported"), what
        return leaf
    assert log.startswith("gemv>"), (what, log)
    if leaf == "as_gemm16":
        assert q.gemm16 and q.m_elem == 2 and nrhs >= 3 and log == "gemv>", what
        return leaf
    if leaf == "as_gemm32":
        assert q.m_elem == 4 and 3 <= nrhs <= 64 and outs >= 512 and k >= 128 and q.ldm * 128 < 1 << 31 and q.ldv * 256 < 1 << 31 and log.startswith("gemv>f32.skinny/ns="), what
        assert (p.gemm32.nsplit, p.gemm32.k_per_split, p.gemm32.workspace_bytes) == (ns, kps, p.workspace_bytes), what
        return leaf
    if leaf == "tlds":
        assert q.trans and q.m_elem == 4 and 2 <= nrhs <= 8 and outs % 4 == 0 and k % 4 == 0 and k >= 128 and Z <= 65535, what
        assert p.lds_bytes <= 128 << 10 and p.lds_bytes == p.lds_kc * p.rhs_tile * 4 and p.lds_kc <= k, f"{what}: {p.lds_bytes} bytes of LDS"
        per_wg = p.lds_cols * p.lds_threads // 32
        assert 1 <= p.grid[0] <= -(-outs // per_wg) and (p.grid[1], p.grid[2], p.block) == (1, Z, p.lds_threads) and ns == 1 and p.workspace_bytes == 0, what
        return leaf
    assert Z * groups <= 65535 and p.grid[1] <= 65535 and p.grid[2] <= 65535 and p.block == 256, what
    small_limits = not q.trans and outs >= 128 and outs * k <= 4 * MiB and nrhs <= 65535
    if leaf == "small":
        rl = 8 if outs >= 4096 else 4 if outs >= 2048 else 2
        assert small_limits and (ns, kps, p.workspace_bytes, p.rl) == (1, k, 0, rl) and tuple(p.grid) == (-(-outs // (4 * rl)), nrhs, Z) and "combine" not in log, what
        return leaf
    per_block = {"n": 256, "t": 16, "tcols": 8}[leaf]
    assert (leaf == "n") == (not q.trans), what
    assert tuple(p.grid) == (-(-outs // per_block), ns, Z * groups), f"{what}: grid {tuple(p.grid)}"  # every output block once
    assert ns >= 1 and kps % 4 == 0 and ((ns - 1) * kps < k <= ns * kps if k else ns == 1), f"{what}: {ns} splits of {kps}"  # every contracted element once
    assert p.workspace_bytes == (Z * ns * nrhs * outs * 4 if ns > 1 else 0), f"{what}: workspace {p.workspace_bytes}"
    assert (" gemv.combine/ns=" in log) == (ns > 1), (what, log)
    if ns > 1:
        assert tuple(p.combine_grid) == (-(-(outs // 4) // 4), nrhs, Z) and nrhs <= 65535 and not (leaf == "n" and small_limits), what
    if leaf == "tcols":
        v16 = 16 // q.v_elem
        aligned = (q.m_elem == 2 and q.m_addr16 == 0 and q.v_addr16 == 0 and q.ldm % 8 == 0 and kps % 8 == 0 and (Z == 1 or (q.m_batch % 8 == 0 and q.v_batch % v16 == 0))
                   and (nrhs == 1 or q.ldv % v16 == 0))
        assert (p.e == 8) == aligned and p.v == nrhs <= 2 and p.u in (4, 8), f"{what}: e={p.e} u={p.u} v={p.v}"
        chunks = kps // (32 * p.e)
        assert (p.u == 4) == (nrhs == 2 or chunks <= 8 or (chunks < 32 and chunks % 8 != 0)), f"{what}: u={p.u} for {chunks} chunks"
    return leaf


@pytest.mark.parametrize("cus", [8, 100, 256])
@pytest.mark.parametrize("elems", list(G.ELEMS))
def test_invariants_over_the_size_grid(elems, cus):
    m_elem, v_elem, bf16, gemm16 = G.ELEMS[elems]
    seen = set()
    for tr, ro, k, nrhs, (Z, lds) in itertools.product((0, 1), OUTS, KS, (1, 2, 3, 8, 9, 65), ((1, 0), (3, 0), (1, 1), (9000, 0))):
        R, C = (k, ro) if tr else (ro, k)
        for mis in range(5):  # 0: dense and aligned; else one thing off at a time
            ldm = max(R, 4) + (4 if mis == 1 else 16384 - R % 16384 if mis == 2 else 0)
            q = G.query(_lib, trans=tr, rows_out=ro, k=k, nrhs=nrhs, nmats=Z, m_elem=m_elem, v_elem=v_elem, bf16=bf16, gemm16=gemm16, ldm=ldm, ldv=max(k, 4), ldo=ro,
                        m_batch=ldm * C + (4 if mis == 3 else 0), v_batch=max(k, 4) * nrhs, o_batch=ro * nrhs, m_addr16=8 if mis == 4 else 0, cus=cus, gemvt_lds=lds)
            seen.add(check_plan(q, f"{elems} {'T' if tr else 'N'} {ro} x {k} x {nrhs} x {Z} mis={mis} lds={lds} cus={cus}"))
            # the fused Gemv + Reduce takes a call if and only if the plan of its Gemv -- one right-hand side, one matrix -- is the single-kernel leaf
            if elems == "f32" and mis == 0:
                q1 = G.query(_lib, **{**{f: getattr(q, f) for f in G.QUERY}, "nrhs": 1, "nmats": 1})
                fused = G.planned(_lib, G.K_REDUCE, q)[1].startswith("gemv.small_reduce/")
                assert fused == G.fused_reduce(_lib, q) == (LEAF[G.plan(_lib, q1)[0].leaf] == "small")
    # (16-bit wg_gemv hands more than 8 right-hand sides to the Gemm launcher before the groups of 8 are counted: never refused here)
    want = {"small", "n", "t", "tcols"} | ({"tlds", "as_gemm32", "unsupported"} if elems == "f32" else {"as_gemm16"} if gemm16 else {"unsupported"})
    assert seen == want, (seen, want)  # (the grid reaches every leaf an element type has, and no other)


def test_invariants_of_gemv_any():
    for elems, tr, ro, k, nrhs, Z, cus in itertools.product(("f32", "f16", "bf16w"), (0, 1), (1, 5, 67, 1030, 16385), (1, 3, 70, 4099, 65537), (1, 3, 70000), (1, 2, 65536),
                                                            (8, 100, 256)):
        m_elem, v_elem, bf16, gemm16 = G.ELEMS[elems]
        q = G.query(_lib, trans=tr, rows_out=ro, k=k, nrhs=nrhs, nmats=Z, m_elem=m_elem, v_elem=v_elem, bf16=bf16, gemm16=gemm16, cus=cus)
        p, tag = G.any_plan(_lib, q)
        what, pairs = f"{elems} {'T' if tr else 'N'} {ro} x {k} x {nrhs} x {Z} cus={cus}", nrhs * Z
        if pairs > 0xffffffff:
            assert not p.launch and p.status == _lib.WG_ERR_UNSUPPORTED and p.message and tag == "", what
            continue
        E = 16 // m_elem
        per_block, unit = (16, 64 * E) if tr else (64 * E, 256)
        assert p.launch and p.status == 0 and tag == f"gemv_any/{'t' if tr else 'n'},ns={p.nsplit}" + (f",chunks={p.nchunks}" if p.nchunks > 1 else ""), (what, tag)
        assert p.grid_x == -(-ro // per_block) and 1 <= p.nsplit <= 65535 and p.per_split % unit == 0 and (p.nsplit - 1) * p.per_split < k <= p.nsplit * p.per_split, what
        assert 1 <= p.zchunk <= 65535 and (p.nchunks - 1) * p.zchunk < pairs <= p.nchunks * p.zchunk, what
        assert p.workspace_bytes == (p.zchunk * p.nsplit * ro * 4 if p.nsplit > 1 else 0) and p.nt == (ro * k * m_elem >= 512 * MiB), what


def test_limits_no_launch_reaches():
    """The refusals real operands do not reach: a hand-off the few-column plan refuses, and the leading dimensions past its 32-bit offsets (kept on the Gemv kernels)."""
    base = dict(trans=0, rows_out=1024, k=8192, nrhs=9, nmats=1, m_elem=4, v_elem=4, ldm=1024, ldv=8192, ldo=1024, m_batch=1024 * 8192, v_batch=8192 * 9, o_batch=1024 * 9, cus=256)
    p, log = G.plan(_lib, G.query(_lib, **{**base, "nmats": 65536}))
    assert LEAF[p.leaf] == "unsupported" and p.status == _lib.WG_ERR_UNSUPPORTED and p.message and log == "gemv>"
    for ldm, ldv, leaf in ((1 << 24, 8192, "n"), ((1 << 24) - 4, 8192, "as_gemm32"), (1024, 1 << 23, "n"), (1024, (1 << 23) - 4, "as_gemm32")):
        assert check_plan(G.query(_lib, **{**base, "ldm": ldm, "ldv": ldv}), f"ldm={ldm} ldv={ldv}") == leaf
