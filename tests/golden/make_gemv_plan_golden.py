"""Generates tests/golden/gemv_plan_parent.json: the launch log of the Gemv launchers, call by call, as DATA.

    python tests/golden/make_gemv_plan_golden.py --commit <hash> --tree <checkout of that commit, its library built> --record rows.json      (on an MI355X)
    python tests/golden/make_gemv_plan_golden.py --commit <hash> --gpu-rows rows.json --harness <program> [--out PATH]

Everything in the table is the launchers as they were BEFORE they were split into gemv_plan() / gemv_any_plan() and executors (gemv.hip, gemv_any.hip, and the
size conditions of wg_gemv_reduce in api.hip). A row is one wg_gemv, wg_gemv_mixed or wg_gemv_reduce call -- which launcher the front-end reaches (`kind`,
tests/_gemv_plan.py), the query that launcher's decision reads, the call's status and the log wg_debug_take_path returns after it -- from one of two sources (`src`):
  0  run on an MI355X with that commit's library (`--tree`: its Python package is imported, so that this script runs against that commit unchanged): the whole chip
     and every masked context of tests/test_gpu_launch_contexts.py MASKED. Gemv calls are cheap: every call a device can hold is recorded there (matrices of at
     most 1 GiB).
  1  that commit's launchers compiled for the host (`--harness`: launches and workspace requests are no-ops, wg_path records; a scratch build, not part of the
     repository; it reads "kind query-fields" per line and prints "status<TAB>log"): only what no reasonable device call reaches -- a hand-off the few-column
     kernel refuses, leading dimensions past its 32-bit offset guard, more (matrix, right-hand side) pairs than 2^32 - 1. The script first runs every src-0 row
     through it and stops unless it gives the recorded log for all of them.
tests/test_gemv_plan_host.py holds the planner to every row, on the CPU.

`ret` is an index into RETURNS: which return of the parent's launcher the call left through (derived here from the log and the status; the script stops if a
listed return is taken by no row). Operand values do not matter to the log: the buffers are allocated once, uninitialised, large enough for every view.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

RETURNS = ("empty: no output element (api.hip returns before the launcher; the launcher's first return gives the same: WG_OK, no launch)",
           "refused: matrices x groups of 8 right-hand sides exceed 65535",
           "gemv.tlds: f32 GemvTr, 2 .. 8 vectors in the LDS",
           "gemv.small: one kernel, no partials",
           "gemv.n unsplit",
           "gemv.n with the combine pass",
           "gemv.t unsplit",
           "gemv.t with the combine pass",
           "gemv.tcols, one vector, unsplit",
           "gemv.tcols with the combine pass",
           "gemv.tcols, two vectors",
           "hand-off to the f32 few-column Gemm kernel",
           "hand-off to the 16-bit Gemm launcher",
           "hand-off refused by the few-column kernel's plan",
           "gemv_any, one launch per kernel",
           "gemv_any in chunks of 65535 (matrix, right-hand side) pairs",
           "gemv_any refused: more than 2^32 - 1 pairs",
           "Gemv + Reduce fused into one launch",
           "Gemv + Reduce declined: two launches")
(R_EMPTY, R_GROUPS, R_TLDS, R_SMALL, R_N, R_N_COMBINE, R_T, R_T_COMBINE, R_TCOLS, R_TCOLS_COMBINE, R_TCOLS2, R_GEMM32, R_GEMM16, R_GEMM32_ERR, R_ANY, R_ANY_CHUNKS,
 R_ANY_ERR, R_FUSED, R_TWO) = range(len(RETURNS))
# returns no row can take, and why (tests/test_gemv_plan_host.py covers them through the planner's invariants)
UNREACHED = {"Gemv: too many splits (gemv_any)": "the cut aims at 2 or 4 workgroups per CU: at most 1024 splits on 256 CUs, never 65536",
             "workspace / launch errors": "device state, not a decision"}
WHOLE = 256
MAX_MATRIX_BYTES = 1 << 30


def tables():
    from test_gpu_launch_contexts import GEMV_REDUCE_SHAPES, MASKED
    from test_gpu_operands import F16, GEMV_LEAVES, LAYOUTS
    from test_gpu_gemv_mixed import CASES
    return MASKED, GEMV_REDUCE_SHAPES, F16, GEMV_LEAVES, LAYOUTS, CASES


def stored(rs, cs, layout, LAYOUTS, ld_mult=1):
    """(offset, leading dimension, matrix stride) of an rs x cs block as tests/test_gpu_operands.py Stored stores it."""
    off, pad, gap, _ = LAYOUTS[layout]
    if pad is None:
        pad = 1 if rs % 2 == 0 else 2
    ld = max(rs + pad, 1)
    ld = -(-ld // ld_mult) * ld_mult
    return off, ld, ld * cs + gap


def extent(g, cols, mats):
    """elements from the start of the buffer to the end of a view (offset, leading dimension, matrix stride) of `cols` columns and `mats` matrices"""
    return g[0] + g[1] * cols + g[2] * (mats - 1)


def spec(op, elems, tr, R, C, nrhs=1, mats=1, m=None, v=None, o=None, lds=0):
    """A call: op gemv / mixed / reduce on an R x C matrix as stored; m, v, o: (offset, leading dimension, matrix stride), dense where None."""
    ro, k = (C, R) if tr else (R, C)
    return dict(op=op, elems=elems, tr=tr, R=R, C=C, nrhs=nrhs, mats=mats, m=m or (0, max(R, 1), max(R, 1) * C), v=v or (0, max(k, 1), max(k, 1) * nrhs),
                o=o or (0, max(ro, 1), max(ro, 1) * nrhs), lds=lds)


def specs_for(cus):
    """The calls of one context."""
    MASKED, GEMV_REDUCE_SHAPES, F16, GEMV_LEAVES, LAYOUTS, CASES = tables()
    whole = cus == WHOLE
    out = []

    def add(op, elems, tr, ro, k, nrhs=1, mats=1, **kw):
        """by output length and contraction; skipped above MAX_MATRIX_BYTES"""
        R, C = (k, ro) if tr else (ro, k)
        s = spec(op, elems, tr, R, C, nrhs, mats, **kw)
        if extent(s["m"], C, mats) * (4 if elems == "f32" else 2) <= MAX_MATRIX_BYTES + 64:
            out.append(s)

    # the rows of the tables the GPU tests assert: GEMV_LEAVES on every layout (the masked contexts: dense), the mixed cases, the fused Reduce shapes
    for row in GEMV_LEAVES:
        for layout in LAYOUTS if whole else ("dense",):
            ro, k = (row.C, row.R) if row.tr else (row.R, row.C)
            vl = "odd" if row.vodd else layout
            out.append(spec("gemv", "f16" if row.dtype == F16 else "f32", row.tr, row.R, row.C, row.nrhs, row.mats,
                            m=stored(row.R, row.C, layout, LAYOUTS, row.ld_mult if layout != "odd" else 1), v=stored(k, row.nrhs, vl, LAYOUTS),
                            o=stored(ro, row.nrhs, vl, LAYOUTS), lds=row.knobs.get("gemvt_lds", 0)))
    for _, tr, R, C, nrhs, Z, (moff, mpad), voff, _ in CASES:
        for elems in ("f16w", "bf16w") if whole else ("f16w",):
            ro, k = (C, R) if tr else (R, C)
            out.append(spec("mixed", elems, tr, R, C, nrhs, Z, m=(moff, R + mpad, (R + mpad) * C + mpad), v=(voff, k + voff, (k + voff) * nrhs),
                            o=(voff, ro + voff, (ro + voff) * nrhs)))
    for R, C, _ in GEMV_REDUCE_SHAPES:
        out.append(spec("reduce", "f32", False, R, C, m=stored(R, C, "aligned", LAYOUTS)))
    # every element type over a grid of sizes
    sizes, ks = ((64, 1024, 4096, 16384), (64, 1024, 4096, 32768)) if whole else ((1024, 4096), (1024, 4096))
    for tr in (False, True):
        for elems in ("f32", "f16"):
            for ro in sizes:
                for k in ks:
                    for nrhs in (1, 2, 4, 8) if whole else (1, 2, 8):
                        add("gemv", elems, tr, ro, k, nrhs)
        for elems, op in (("bf16", "gemv"), ("f16w", "mixed"), ("bf16w", "mixed")) if whole else ():
            for ro in (1024, 4096):
                for k in (1024, 4096):
                    for nrhs in (1, 2, 11):
                        add(op, elems, tr, ro, k, nrhs)
        add("gemv", "f32", tr, 1024, 1024, 3, 5)  # a batch
        add("gemv", "f16", tr, 4096, 2048, 1, 3)
    if not whole:
        return out
    # ---- both sides of every threshold the launcher's comments name (the whole chip) ----
    # f32 GemvTr, one vector: columns 64 KiB apart with k <= 16384 stay on the 4-columns-per-wave kernel
    for k in (16384, 16388):
        for ld in (16384, 32768, 16388):
            if ld >= k:
                add("gemv", "f32", True, 2048, k, m=(0, ld, ld * 2048))
    for ld in (16384, 32768):
        add("gemv", "f16", True, 2048, 4096, m=(0, ld, ld * 2048))
    # two vectors on the column kernel: f16 from 2048 outputs on, f32 for 2049 .. 8192 rows onto 4096 .. 16384 outputs
    for ro in (2044, 2048):
        add("gemv", "f16", True, ro, 4096, 2)
        add("mixed", "f16w", True, ro, 4096, 2)
    for k in (2048, 2052, 8192, 8196):
        for ro in (4092, 4096, 16384, 16388):
            add("gemv", "f32", True, ro, k, 2)
    # big_n: 2 workgroups per CU from 256 MiB on, f32 with >= 16384 outputs from 128 MiB on
    for elems, shapes in (("f32", ((4096, 16384), (4096, 16380), (16384, 2048), (16384, 2044), (16380, 2052), (8192, 8192), (4096, 65536))),
                          ("f16", ((8192, 16384), (8192, 16380), (16384, 4096), (16384, 8192)))):
        for ro, k in shapes:
            add("gemv", elems, False, ro, k)
    add("mixed", "bf16w", False, 8192, 16384)
    # the hand-offs to the Gemm kernels: 7-8 right-hand sides from 16 MiB on, 3-6 from 48 MiB on; f32 only with k < 8 outputs (N) / outputs < 8 k (T)
    for tr in (False, True):
        for ro, k, nrhs in ((2048, 2048, 8), (2048, 2044, 8), (2048, 2048, 7), (2048, 2048, 6), (4096, 3072, 4), (4096, 3068, 4), (4096, 3072, 3), (4096, 3072, 2),
                            (4096, 65536, 8), (65536, 4096, 8), (512, 4096, 9), (508, 4096, 9), (4096, 128, 9), (4096, 124, 9), (4096, 1024, 64), (4096, 1024, 65)):
            add("gemv", "f32", tr, ro, k, nrhs)
        for ro, k, nrhs in ((4096, 2048, 8), (4096, 2044, 8), (8192, 3072, 3), (8192, 3068, 3), (1024, 1024, 9), (4096, 2048, 7), (4096, 2048, 6)):
            add("gemv", "f16", tr, ro, k, nrhs)
            add("mixed", "f16w", tr, ro, k, nrhs)
        add("gemv", "bf16", tr, 4096, 2048, 8)
    # the column kernel with 4 loads in flight: columns of at most 8 chunks, and up to 31 when the 8-deep form would end in a partial trip
    for k in (1024, 1152, 2048, 3968, 4096):
        add("gemv", "f32", True, 4096, k)
    for k in (2048, 2304, 4096, 7936, 8192):
        add("gemv", "f16", True, 4096, k)
    # 16-byte loads (e=8) need every base, leading dimension, matrix stride and split to keep them aligned
    for elems, op in (("f16", "gemv"), ("f16w", "mixed")):
        for m in ((4, 1024, 1024 * 1024), (0, 1028, 1028 * 1024), (0, 1032, 1032 * 1024), (8, 1032, 1032 * 1024)):
            add(op, elems, True, 1024, 1024, m=m)
        add(op, elems, True, 1024, 1024, v=(4, 1024, 1024))
        add(op, elems, True, 1024, 1024, 1, 2, m=(0, 1024, 1024 * 1024 + 4))
        add(op, elems, True, 1024, 1024, 1, 2, m=(0, 1024, 1024 * 1024 + 8))
        add(op, elems, True, 1024, 1024, 1, 2, v=(0, 1024, 1028))
        add(op, elems, True, 2048, 1024, 2, v=(0, 1028, 2056))
        add(op, elems, True, 2048, 1024, 2, v=(0, 1032, 2064))
        add(op, elems, True, 4096, 1028)  # (a split of 1028 / 8 is no multiple of 8)
    # WG_TUNE_GEMVT_LDS forced: the outputs per CU from which the LDS kernel runs
    for lds in (1, 64):
        for nrhs in (2, 3, 8):
            for ro in (128, 1024, 16384):
                for k in (124, 128, 4096, 8192, 16384):
                    add("gemv", "f32", True, ro, k, nrhs, lds=lds)
    # ... and unforced: 128 outputs per CU with the vectors whole in the LDS; two vectors from 8 outputs per CU on
    for ro, k, nrhs in ((32764, 4096, 8), (32768, 4096, 8), (32768, 4100, 8), (2044, 1024, 2), (2048, 1024, 2), (2048, 124, 2)):
        add("gemv", "f32", True, ro, k, nrhs)
    add("gemv", "f32", True, 1024, 1024, 4, 3, lds=1)
    # limits of the grids: groups of right-hand sides x matrices, 65535 and more right-hand sides, pairs in chunks, nothing to do
    add("gemv", "f32", False, 4, 4, 1, 65536)
    add("gemv", "f32", False, 4, 4, 1, 65535)
    add("gemv", "f32", False, 4, 4, 65, 8192)
    add("mixed", "f16w", True, 4, 4, 9, 32768)
    add("gemv", "f32", False, 128, 256, 65535)
    add("gemv", "f32", False, 128, 256, 65536)
    add("gemv", "f32", False, 5, 3, 1, 65536, m=(1, 5, 15))
    add("gemv", "f16", True, 5, 3, 2, 40000, m=(1, 3, 15))
    add("gemv", "f32", False, 4, 4, 0)
    add("mixed", "f16w", False, 0, 4)
    # the any-alignment kernels: 4 workgroups per CU for N from 1 GiB on (the matrix at an odd offset)
    for ro, k in ((16384, 16384), (16384, 16380), (1024, 1024), (67, 4099)):
        for tr in (False, True):
            add("gemv", "f32", tr, ro, k, m=(1, k if tr else ro, 0))
    add("gemv", "f16", False, 8192, 8192, 2, m=(1, 8193, 0))
    add("mixed", "bf16w", True, 4099, 67, 3, m=(1, 70, 0))
    # the fused Gemv + Reduce: both sides of 128 outputs, of 4 Mi elements, of a contraction that is cut at all; GemvTr is never fused
    for R, C in ((124, 4096), (128, 4096), (4096, 1024), (4096, 1028), (1024, 64), (1024, 68), (16384, 256), (16384, 260)):
        out.append(spec("reduce", "f32", False, R, C))
    out.append(spec("reduce", "f32", True, 1024, 1024))
    return out


def specs_no_device_reaches():
    """`src` 1, on the whole chip: operands no device holds."""
    out = []
    for tr in (False, True):
        out.append(spec("gemv", "f32", tr, 128 if tr else 512, 512 if tr else 128, 9, 65536))        # the few-column plan refuses more than 65535 matrices
        R, C = (4096, 1024) if tr else (1024, 4096)
        for ldm, ldv in ((1 << 24, None), ((1 << 24) - 4, None), (None, 1 << 23), (None, (1 << 23) - 4)):  # the 32-bit offsets of the few-column kernel
            k = R if tr else C
            out.append(spec("gemv", "f32", tr, R, C, 9, m=(0, ldm or R, (ldm or R) * C), v=(0, ldv or k, (ldv or k) * 9)))
    out.append(spec("gemv", "f32", False, 5, 3, 65536, 65536, m=(1, 5, 15)))                         # 2^32 pairs on the any-alignment kernels
    out.append(spec("gemv", "f32", False, 5, 3, 65535, 65537, m=(1, 5, 15)))                         # 2^32 - 1: in chunks
    return out


def routed(L, s, cus, base16=(0, 0)):
    import _gemv_plan as G
    r = G.route(L, s["elems"], s["tr"], s["R"], s["C"], s["nrhs"], s["mats"], s["m"], s["v"], s["o"], base16, cus, s["lds"])
    if r is None:
        return G.K_GEMV, [0] * len(G.QUERY)
    kind, _, q = r
    return (G.K_REDUCE if s["op"] == "reduce" else kind), [getattr(q, f) for f in G.QUERY]


def label(kind, status, log):
    """Which return of the parent's launchers the call left through."""
    import _gemv_plan as G
    if kind == G.K_REDUCE:
        return R_FUSED if log.startswith("gemv.small_reduce/") else R_TWO
    if kind == G.K_ANY:
        if status:
            return R_ANY_ERR
        assert "gemv_any/" in log, log
        return R_ANY_CHUNKS if "chunks=" in log else R_ANY
    if status:
        return R_GROUPS if ".gemv" in log else R_GEMM32_ERR
    if log == "":
        return R_EMPTY
    combine = "gemv.combine/" in log
    for tag, ret in (("gemv.tlds/", R_TLDS), ("gemv.small/", R_SMALL), ("gemv.n/", R_N_COMBINE if combine else R_N), ("gemv.t/", R_T_COMBINE if combine else R_T),
                     (",v=2,", R_TCOLS2), ("gemv.tcols/", R_TCOLS_COMBINE if combine else R_TCOLS), ("gemv>f32.skinny/", R_GEMM32)):
        if tag in log:
            return ret
    assert log.split("gemv>")[1].startswith(("f16.", "bf16.")) and ".gemv" not in log, log
    return R_GEMM16


def record_on_gpu(tree):
    """The rows of `src` 0: real calls on the whole chip and on every masked context."""
    sys.path.insert(0, tree)
    import wgmath_amd as wg
    from wgmath_amd import _lib as L
    MASKED = tables()[0]
    contexts = ["full"] + list(MASKED)
    plans = {w: specs_for(WHOLE if w == "full" else MASKED[w][0]) for w in contexts}
    need = [16, 16, 16]  # bytes
    for ss in plans.values():
        for s in ss:
            me, ve = (4, 4) if s["elems"] == "f32" else (2, 4) if s["elems"].endswith("w") else (2, 2)
            for i, (g, cols, es) in enumerate(((s["m"], s["C"], me), (s["v"], s["nrhs"], ve), (s["o"], s["nrhs"], ve))):
                need[i] = max(need[i], (extent(g, cols, s["mats"]) + 16) * es)
    main_inst = wg.GpuInstance.new(0)
    bufs = [wg.TensorBuilder.tensor((-(-n // 4),), 128 | 4 | 8).build(main_inst.device(), np.float32) for n in need]
    res = wg.TensorBuilder.tensor((4,), 128 | 4 | 8).build(main_inst.device(), np.float32)
    base16 = tuple(b.device_ptr() % 16 for b in bufs[:2])
    dt = {"f32": L.WG_F32, "f16": L.WG_F16, "bf16": L.WG_BF16, "f16w": L.WG_F16, "bf16w": L.WG_BF16}
    rows = []
    for w in contexts:
        cus = WHOLE if w == "full" else MASKED[w][0]
        inst = main_inst if w == "full" else wg.GpuInstance.new(0, cu_count=cus, one_xcd=MASKED[w][1])
        inst.take_path()
        for i, s in enumerate(plans[w]):
            inst.set_tuning("gemvt_lds", s["lds"])
            tr, R, C, Z, nrhs = s["tr"], s["R"], s["C"], s["mats"], s["nrhs"]
            ro, k = (C, R) if tr else (R, C)
            (mo, ldm, mb), (vo, ldv, vb), (oo, ldo, ob) = s["m"], s["v"], s["o"]
            msh, vsh, osh = wg.ViewShape((R, C, Z), ldm, mb, mo), wg.ViewShape((k, nrhs, Z), ldv, vb, vo), wg.ViewShape((ro, nrhs, Z), ldo, ob, oo)
            variant = int(wg.GemvVariant.GemvTr if tr else wg.GemvVariant.Gemv)
            h = inst._ctx.handle
            if s["op"] == "reduce":
                status = L.lib.wg_gemv_reduce(h, variant, int(wg.ReduceOp.Sum), L.WG_F32, res._h, bufs[0]._h, msh.to_c(), bufs[1]._h, vsh.to_c())
            else:
                fn = L.lib.wg_gemv_mixed if s["op"] == "mixed" else L.lib.wg_gemv
                status = fn(h, variant, dt[s["elems"]], bufs[2]._h, osh.to_c(), bufs[0]._h, msh.to_c(), bufs[1]._h, vsh.to_c())
            log = inst.take_path()
            rows.append((w, s, int(status), log))
            if i % 32 == 31:
                inst.sync()
        inst.set_tuning("gemvt_lds", 0)
        inst.sync()
        print(f"{w}: {len(plans[w])} calls", flush=True)
        if inst is not main_inst:
            inst.close()
    return {"base16": base16, "calls": [[w, s, st, log] for w, s, st, log in rows]}


def on_host(exe, rows):
    """[(status, log)] of (kind, query) rows by the host build of the launchers."""
    r = subprocess.run([exe], input="".join(" ".join(str(v) for v in q) + "\n" for q in rows), capture_output=True, text=True, check=True)
    got = [line.split("\t") for line in r.stdout.split("\n")[:-1]]
    assert len(got) == len(rows), (len(got), len(rows), r.stderr[-500:])
    return [(int(st), log) for st, log in got]


def dump(args, rows):
    import _gemv_plan as G
    doc = {"parent_commit": args.commit, "fields": G.FIELDS, "returns": RETURNS, "unreached": UNREACHED,
           "rows_per_return": {RETURNS[i].split(":")[0][:48]: sum(r[-1] == i for r in rows) for i in range(len(RETURNS))}, "rows": rows}
    text = json.dumps(doc, separators=(",", ":"))
    text = "],\n[".join("],[".join(c) for c in (lambda r: [r[i:i + 4] for i in range(0, len(r), 4)])(text.split("],[")))  # four rows to a line
    with open(args.out, "w") as f:
        f.write(text + "\n")
    return text


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the loaded library and the host program were built from")
    ap.add_argument("--tree", default=ROOT, help="a checkout of that commit with its library built: its wgmath_amd package makes the recorded calls")
    ap.add_argument("--record", help="run the src-0 calls on the device and write them here (then run again with --gpu-rows)")
    ap.add_argument("--gpu-rows", help="the file --record wrote")
    ap.add_argument("--harness", help="the host build of that commit's launchers (see above)")
    ap.add_argument("--out", default=os.path.join(HERE, "gemv_plan_parent.json"))
    args = ap.parse_args()
    if args.record:
        with open(args.record, "w") as f:
            json.dump(record_on_gpu(args.tree), f)
        return
    sys.path.insert(0, ROOT)
    from wgmath_amd import _lib as L
    import _gemv_plan as G
    MASKED = tables()[0]
    rec = json.load(open(args.gpu_rows))
    want = [(w, s) for w in ["full"] + list(MASKED) for s in specs_for(WHOLE if w == "full" else MASKED[w][0])]
    assert [[w, s] for w, s, _, _ in rec["calls"]] == json.loads(json.dumps(want)), "the recording is not of this grid"
    rows = []
    for w, s, status, log in rec["calls"]:
        cus = WHOLE if w == "full" else MASKED[w][0]
        kind, q = routed(L, s, cus, tuple(rec["base16"]))
        rows.append([kind] + q + [status, log, 0, label(kind, status, log)])
    # the host build is the same launcher: it must give every recorded call its recorded log (behind the staging wrapper, up to the Reduce launch's own tag)
    again = on_host(args.harness, [r[:1 + len(G.QUERY)] for r in rows])
    def own(r):  # the part of a recorded log that is this launcher's: behind the staging wrapper, up to the Reduce launch's tag or the 16-bit Gemm launcher's tags
        log = r[-3][len("stage>"):] if r[-3].startswith("stage>") else r[-3].split(" reduce.")[0]
        return log[:log.index("gemv>") + 5] if r[-1] == R_GEMM16 else log
    differ = [(r, g) for r, g in zip(rows, again) if (r[-4], own(r)) != g]
    assert not differ, f"{len(differ)} of {len(rows)} recorded calls differ on the host build: {differ[:3]}"
    print(f"{len(rows)} recorded calls: the host build logs the same", flush=True)
    host = specs_no_device_reaches()
    hq = [routed(L, s, WHOLE) for s in host]
    for (kind, q), (status, log) in zip(hq, on_host(args.harness, [[kind] + q for kind, q in hq])):
        rows.append([kind] + q + [status, log, 1, label(kind, status, log)])
    text = dump(args, rows)
    seen = {r[-1] for r in rows}
    assert seen == set(range(len(RETURNS))), f"returns no row took: {[RETURNS[i] for i in set(range(len(RETURNS))) - seen]}"
    assert len(text) <= 256 << 10, f"{len(text)} bytes"
    print(f"{args.out}: {len(rows)} rows ({sum(r[-2] for r in rows)} from the host build), {len(text)} bytes")


if __name__ == "__main__":
    main()
