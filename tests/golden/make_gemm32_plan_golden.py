"""Generates tests/golden/gemm32_plan_parent.json: the launch log of the f32 Gemm launcher, call by call, as DATA.

    python tests/golden/make_gemm32_plan_golden.py --commit <hash of the commit the library was built from> --harness <program> [--out PATH]

Everything in the table is the launcher as it was BEFORE it was split into gemm32_plan() and an executor. A row is one f32 wg_gemm_ex call -- the query (everything
the launcher's decision reads) and the log wg_debug_take_path returns after it -- from one of two sources (`src`):
  0  run on an MI355X with that commit's library: the whole chip and the masked contexts GPU_CONTEXTS;
  1  that commit's wgk_gemm_f32 (with its two launchers) compiled for the host and called with the query: the masked contexts HOST_CONTEXTS, and leading dimensions
     no operand of the tests of that commit reached (the branches behind dma_ok == false; tests/test_gpu_far_views.py runs them on a device since). The CU count and the leading dimensions are only numbers in the launcher's host arithmetic, so
     no device is needed; the program (`--harness`: launches and workspace requests are no-ops, wg_path records, the slab reduces and transposes log their tags) is
     a scratch build and not part of the repository. It reads one query per line (the first 18 FIELDS) and prints "status<TAB>log". The script first runs every src-0
     row through it as well and stops unless it gives the recorded log for all of them.
tests/test_gemm32_plan_host.py holds the planner to every row, on the CPU.

A row is a list, in the order of FIELDS:
    trans, M, N, K, nmats, lda, ldb, ldc, a_batch, b_batch, c_batch, alpha, beta, cus, mid, mid_split, skinny, panels, status, log, src, ret
`cus` is the CU count of the context (256: the whole chip; the masked ones of tests/test_gpu_launch_contexts.py MASKED), mid .. panels the values of
WG_TUNE_F32_MID, _MID_SPLIT, _SKINNY, _PANELS, `status` the call's return value, `ret` an index into RETURNS: which `return` of the launcher the call left
through (derived here from the log and the conditions in front of that return; the script stops if a log contradicts its own label).

Operand values do not matter to the log: the buffers are allocated once, uninitialised, large enough for every view. Every call on a device stays below 2^35 flop.
Only views whose lengths are multiples of 4 (or N free, from 129 rows on) are used: those reach the launcher as they are (api.hip), so
the leading dimensions and matrix strides of the views are the ones the launcher reads.
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
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FIELDS = ("trans", "M", "N", "K", "nmats", "lda", "ldb", "ldc", "a_batch", "b_batch", "c_batch", "alpha", "beta", "cus", "mid", "mid_split", "skinny", "panels",
          "status", "log", "src", "ret")
# the returns of wgk_gemm_f32 (and the refusals of the two launchers it calls, which are part of the same decision)
RETURNS = ("empty product: nothing to do (api.hip returns before the launcher; the launcher's first return gives the same: WG_OK, no launch)",
           "more than 65535 matrices",
           "early mid: one row or column of 64 x 64 tiles, K cut or unsplit (wgk_gemm_f32_mid, 64, 64)",
           "few-row form on transposed copies, 65 .. 128 rows (f32.fewrow>, then the inner call)",
           "transposed few-row form of the few-column kernel (f32.skinnyT)",
           "few-column kernel, N <= 64",
           "short K on a large output: 128 x 64 / 64 x 128 of the mid family",
           "64-column panels of the few-column kernel (or its single panel for batches of small matrices)",
           "mid family by estimate or knob",
           "256 x 128 tiles with the cut-up tail (f32.big f32.bigtail f32.tail_reduce)",
           "256 x 128 tiles, split-K slabs and reduce",
           "256 x 128 tiles, one launch",
           "refused by wgk_gemm_f32_skinny (matrices x panels > 65535)",
           "refused by wgk_gemm_f32_mid (matrices x splits > 65535)",
           "few-row form on transposed copies, M <= 64: leading dimensions past the few-column kernel's 32-bit offsets (dma_ok == false)")
# (the last one: on a device in tests/test_gpu_far_views.py; the text above is part of the recorded table and stays as it was recorded)
(R_EMPTY, R_MATS, R_EARLY_MID, R_FEWROW, R_SKINNYT, R_SKINNY, R_SHORTK, R_PANELS, R_MID, R_TAIL, R_SPLITK, R_BIG, R_SKINNY_ERR, R_MID_ERR, R_FEWROW_DMA) = range(len(RETURNS))
# returns no row can take, and why (tests/test_gemm32_plan_host.py covers them through the planner's invariants)
UNREACHED = {"Gemm: too many tiles": "more than 2^31 tiles of 256 x 128: an output of 2^46 floats",
             "Gemm: nmats * splits exceeds 65535 (256 x 128 tiles)": "a K cut is only planned while the tiles leave CUs idle: never with thousands of matrices",
             "workspace / transpose / launch errors": "device state, not a decision"}
GPU_CONTEXTS, HOST_CONTEXTS = ("full", "cu248", "cu224"), ("cu100", "cu8")  # `src` 0 and 1
DEFAULT = {"f32_mid": -1, "f32_mid_split": 0, "f32_skinny": -1, "f32_panels": -1}
from test_gpu_launch_contexts import MASKED  # noqa: E402
from test_gpu_operands import LAYOUTS  # noqa: E402  (offset, extra leading dimension, gap between matrices, elements after the end)


def geom(rs, cs, layout, ld=None):
    off, pad, gap, _ = LAYOUTS[layout]
    if pad is None:
        pad = 1 if rs % 2 == 0 else 2
    ld = ld or max(rs + pad, 1)
    return off, ld, ld * cs + gap


def spec(tr, M, N, K, mats=1, layout="dense", lda=None, ldb=None, alpha=1.0, beta=0.0, **knobs):
    a = geom(*((K, M) if tr else (M, K)), layout, lda)
    b = geom(K, N, layout, ldb)
    c = geom(M, N, layout)
    return dict(tr=tr, M=M, N=N, K=K, mats=mats, a=a, b=b, c=c, alpha=alpha, beta=beta, knobs={**DEFAULT, **knobs})


def reaches_launcher(s):
    """Lengths the API hands to the launcher as they are, and not the Gemv route of 1 .. 7 columns."""
    M, N, K = s["M"], s["N"], s["K"]
    if M % 4 or K % 4 or (N % 4 and M <= 128):
        return False
    return not (N % 4 and N < 8)


def specs_for(cus):
    """The calls of one context. flop cap: 2^35 per call, 2^34 on 100 CUs, 2^31 on 8."""
    cap = {256: 1 << 35, 248: 1 << 35, 224: 1 << 35, 100: 1 << 34, 8: 1 << 31}[cus]
    out = []

    def add(*a, **kw):
        s = spec(*a, **kw)
        if 2 * s["M"] * s["N"] * s["K"] * s["mats"] <= cap and reaches_launcher(s):
            out.append(s)

    whole = cus == 256  # (the masked contexts: a thinner grid of the same kinds)
    sizes = (16, 64, 128, 512, 4096, 16384) if whole else (64, 512, 4096)
    named = ((64, 16384, 512), (64, 4096, 4096), (1024, 1024, 256), (256, 256, 4096), (96, 8192, 256), (32, 4096, 512), (16384, 16, 128), (4096, 16, 1024),
             (512, 512, 512), (4096, 4096, 256), (512, 512, 4096), (4352, 2048, 1024), (1000, 1000, 300), (64, 11008, 4096), (128, 11008, 4096), (128, 14336, 4096),
             (1536, 1536, 1536), (1536, 5120, 384), (3072, 3072, 1024), (768, 5120, 3072), (11008, 32, 4096), (260, 384, 132), (4100, 4096, 260), (516, 9, 260),
             (4096, 4097, 64), (132, 4101, 128), (8192, 8192, 128), (6144, 6144, 256), (5120, 5120, 512), (4352, 4352, 512), (2304, 2304, 2304))
    for tr in (False, True):
        for M in sizes:
            for N in sizes:
                for K in (128, 512, 4096) if whole else (128, 4096):
                    add(tr, M, N, K)
        # the rows of the tables the GPU tests assert, and shapes the launcher's comments name: dense and odd layouts, beta 0 and non-zero
        for i, (M, N, K) in enumerate(named if whole else named[:13]):
            add(tr, M, N, K, layout="odd")
            if whole:
                add(tr, M, N, K)
                if i < 13:
                    add(tr, M, N, K, alpha=0.5, beta=0.25)
        # beta != 0: the few-row forms are not taken, everything else applies it in its own epilogue
        for M in (64, 128, 4096):
            for N in (64, 4096, 8192):
                add(tr, M, N, 1024, alpha=-1.5, beta=0.25)
        # batches
        for M, N, K in ((32, 32, 32), (128, 128, 4096), (1024, 1024, 128), (64, 4096, 1024), (96, 8192, 256), (4096, 16, 1024), (512, 512, 512)) if not whole else ():
            add(tr, M, N, K, 8)
        if whole:
            for M, N, K in named[:13]:
                add(tr, M, N, K, layout="aligned")
            add(tr, 64, 64, 96, f32_mid=64064, f32_mid_split=2)   # (a forced split the launcher lowers: no whole k-tile would be left for the last part)
            add(tr, 128, 192, 1000, f32_mid=64064, f32_mid_split=3)
            for M, N, K in ((32, 32, 32), (64, 64, 64), (128, 128, 128), (128, 128, 4096), (256, 256, 4096), (1024, 1024, 128), (1024, 1024, 1024), (2048, 2048, 128),
                            (4096, 7168, 2048), (64, 4096, 1024), (96, 8192, 256), (4096, 16, 1024), (32, 16, 32), (512, 512, 512), (1000, 1000, 300)):
                add(tr, M, N, K, 8)
            # leading dimensions that are large powers of two, multiples of 1024, and not multiples of 16 (the pow2_ld / pow2_ldb / % 16 terms of the mid model)
            for M, N, K in ((2048, 2048, 2048), (2048, 2048, 4096), (1024, 4096, 1024)):
                rows_a = K if tr else M
                for lda in (None, 1024, 2048, 3072, 4096, 8192, 16384, rows_a + 4, rows_a + 8, rows_a + 16):
                    if lda is None or lda >= rows_a:
                        add(tr, M, N, K, lda=lda)
                for ldb in (8192, 16384, K + 4, K + 1024):
                    if ldb >= K:
                        add(tr, M, N, K, ldb=ldb)
                        add(tr, M, N, K, lda=max(rows_a, 8192), ldb=ldb)
        # forced knobs: every value the tests use, on rows of tests/test_gpu_epilogue.py LEAVES that set a knob
        for M, N, K in ((1024, 1024, 256), (256, 256, 4096), (512, 512, 512), (4352, 2048, 1024)) if whole else ((1024, 1024, 256), (512, 512, 4096)):
            for mid in (128128, 128064, 64128, 64064, 64032, 32064, 96096, 96064, 64096, 0, 1):
                add(tr, M, N, K, f32_mid=mid)
            for mid, sp in ((64064, 2), (64064, 3), (64064, 4), (64064, 8), (64032, 4), (64032, 8))[:3 if cus in (248, 224) else 6]:  # (tests/test_gpu_parity.py test_gemm_f32_mid_split_k)
                add(tr, M, N, K, f32_mid=mid, f32_mid_split=sp)
            for panels in (0, 1):
                add(tr, M, N, K, f32_panels=panels)
                add(tr, M, N, K, f32_panels=panels, f32_mid=0)
            if whole:
                for skinny in (0, 1):
                    add(tr, M, N, K, f32_skinny=skinny)
                    add(tr, M, N, K, f32_skinny=skinny, f32_mid=0, f32_panels=0)
                add(tr, M, N, K, f32_mid=0, f32_panels=0, alpha=2.0, beta=1.0)
    if whole:
        out.append(spec(False, 4, 4, 4, 65536))                                                   # more matrices than grid.y holds
        out.append(spec(True, 32, 4096, 32, 2048, f32_panels=1))                                  # 2048 matrices x 64 panels
        out.append(spec(False, 64, 64, 2048, 2048, f32_mid=64064, f32_mid_split=64))              # 2048 matrices x 64 splits
        out.append(spec(False, 64, 0, 64))                                                        # nothing to do
    return out


def specs_past_dma_limits():
    """Leading dimensions whose blocks no longer fit the kernels' 32-bit byte offsets (ld x 256 / 128 / 64 / 32 rows x 4 bytes >= 2^31), on the whole chip: `src` 1."""
    out = []
    for tr in (False, True):
        for M, N, K in ((16, 4096, 256), (64, 16384, 1024), (96, 8192, 256), (4096, 16, 1024), (512, 512, 512), (4096, 4096, 256)):
            for lda, ldb in [(ld, None) for ld in (1 << 21, 1 << 22, 1 << 23, 1 << 24)] + [(None, ld) for ld in (1 << 21, 1 << 22, 1 << 23, 1 << 24)] + [(1 << 24, 1 << 24)]:
                out.append(spec(tr, M, N, K, lda=lda, ldb=ldb))
            out.append(spec(tr, M, N, K, lda=1 << 24, ldb=1 << 24, alpha=0.5, beta=0.25))
    return out


def query_of(s, cus):
    """The first 18 FIELDS of a call."""
    kn = s["knobs"]
    return [int(s["tr"]), s["M"], s["N"], s["K"], s["mats"], s["a"][1], s["b"][1], s["c"][1], s["a"][2], s["b"][2], s["c"][2], s["alpha"], s["beta"], cus,
            kn["f32_mid"], kn["f32_mid_split"], kn["f32_skinny"], kn["f32_panels"]]


def on_host(exe, queries):
    """[(status, log)] of the queries by the host build of the launcher."""
    r = subprocess.run([exe], input="".join(" ".join(str(v) for v in q) + "\n" for q in queries), capture_output=True, text=True, check=True)
    got = [line.split("\t") for line in r.stdout.split("\n")[:-1]]
    assert len(got) == len(queries), (len(got), len(queries), r.stderr[-500:])
    return [(int(st), log) for st, log in got]


def label(s, cus, status, log):
    """Which return of wgk_gemm_f32 the call left through: from the log, and where two returns log the same family, from the conditions in front of them."""
    tr, M, N, K, mats, kn = s["tr"], s["M"], s["N"], s["K"], s["mats"], s["knobs"]
    mid, panels, skinny = kn["f32_mid"], kn["f32_panels"], kn["f32_skinny"]
    if N == 0:
        return R_EMPTY
    if status != 0:
        assert log == "", log
        return R_MATS if mats > 65535 else (R_SKINNY_ERR if panels == 1 else R_MID_ERR)
    mid_forced, other_forced = mid > 1, skinny == 1 or panels == 1
    mid_ok = K >= 32 and M >= 4 and N >= 4 and s["a"][1] * 512 < 1 << 31 and s["b"][1] * 512 < 1 << 31
    t64 = -(-M // 64) * -(-N // 64) * mats
    if log.startswith("f32.fewrow>"):
        assert M <= 128 and N >= 512 and s["beta"] == 0.0, (s, log)
        if M <= 64:
            assert s["b"][1] * 128 >= 1 << 31 or s["a"][1] * 256 >= 1 << 31, (s, log)
            return R_FEWROW_DMA
        return R_FEWROW
    if log.startswith("f32.skinnyT"):
        assert M <= 64 and N >= 512 and s["beta"] == 0.0, (s, log)
        return R_SKINNYT
    if log.startswith("f32.skinny/p="):
        return R_PANELS
    if log.startswith("f32.skinny/"):
        return R_SKINNY if (not mid_forced and N <= 64 and M >= 512 and K >= 128 and skinny != 0) else R_PANELS
    if log.startswith("f32.mid"):
        early = (mid != 0 and not mid_forced and not other_forced and (M <= 64 or N <= 64) and M >= 48 and N >= 48 and mid_ok and
                 ((K >= 1024 and t64 <= cus) or (4 * t64 >= 3 * cus and t64 <= 2 * cus and K >= 128)))
        if early:
            assert log.startswith("f32.mid64x64/"), (s, log)
            return R_EARLY_MID
        tiles = -(-M // 256) * -(-N // 128)
        short_k = (K <= 256 or (not tr and K <= 512)) and 2 * tiles * mats >= cus
        if short_k and mid_ok and mid < 1 and mid != 0 and not other_forced:
            assert log in ("f32.mid128x64/ns=1", "f32.mid64x128/ns=1"), (s, log)
            return R_SHORTK
        return R_MID
    assert log.startswith("f32.big/"), (s, log)
    if "f32.bigtail" in log:
        return R_TAIL
    return R_SPLITK if "splitk.reduce" in log else R_BIG


def dump(args, rows):
    doc = {"parent_commit": args.commit, "fields": FIELDS, "returns": RETURNS, "unreached": UNREACHED,
           "rows_per_return": {RETURNS[i].split(":")[0][:48]: sum(r[-1] == i for r in rows) for i in range(len(RETURNS))}, "rows": rows}
    text = json.dumps(doc, separators=(",", ":"))
    text = "],\n[".join("],[".join(c) for c in (lambda r: [r[i:i + 4] for i in range(0, len(r), 4)])(text.split("],[")))  # four rows to a line
    with open(args.out, "w") as f:
        f.write(text + "\n")
    return text


def record_on_gpu(contexts):
    """The rows of `src` 0: real calls on the whole chip and on masked contexts."""
    import wgmath_amd as wg
    from wgmath_amd import _lib as L

    plans = {w: specs_for(256 if w == "full" else MASKED[w][0]) for w in contexts}
    need = [1, 1, 1]
    for ss in plans.values():
        for s in ss:
            for i, g in enumerate((s["a"], s["b"], s["c"])):
                need[i] = max(need[i], g[0] + g[2] * s["mats"] + 8)
    main_inst = wg.GpuInstance.new(0)
    bufs = [wg.TensorBuilder.tensor((n,), 128 | 4 | 8).build(main_inst.device(), np.float32) for n in need]
    rows = []
    for w in contexts:
        cus = 256 if w == "full" else MASKED[w][0]
        inst = main_inst if w == "full" else wg.GpuInstance.new(0, cu_count=cus, one_xcd=MASKED[w][1])
        inst.take_path()
        for i, s in enumerate(plans[w]):
            for k, v in s["knobs"].items():
                inst.set_tuning(k, v)
            tr, M, N, K, Z = s["tr"], s["M"], s["N"], s["K"], s["mats"]
            (ao, lda, ab), (bo, ldb, bb), (co, ldc, cb) = s["a"], s["b"], s["c"]
            ash = wg.ViewShape(((K, M) if tr else (M, K)) + (Z,), lda, ab, ao)
            bsh, csh = wg.ViewShape((K, N, Z), ldb, bb, bo), wg.ViewShape((M, N, Z), ldc, cb, co)
            variant = int(wg.GemmVariant.GemmTr if tr else wg.GemmVariant.Gemm)
            status = L.lib.wg_gemm_ex(inst._ctx.handle, variant, 0, ctypes.c_float(s["alpha"]), ctypes.c_float(s["beta"]), bufs[2]._h, csh.to_c(), bufs[0]._h, ash.to_c(),
                                      bufs[1]._h, bsh.to_c())
            log = inst.take_path()
            assert "stage" not in log and "gemv" not in log, (s, log)  # (decided in front of the launcher: not a row of this table)
            rows.append(query_of(s, cus) + [int(status), log, 0, label(s, cus, int(status), log)])
            if i % 64 == 63:
                inst.sync()
        for k, v in DEFAULT.items():
            inst.set_tuning(k, v)
        inst.sync()
        print(f"{w}: {len(plans[w])} calls", flush=True)
        if inst is not main_inst:
            inst.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the loaded library and the host program were built from")
    ap.add_argument("--harness", required=True, help="the host build of that commit's launcher (see above)")
    ap.add_argument("--gpu-rows", help="an earlier table of this script: its src-0 rows are taken over instead of being run again (all of this grid's must be in it)")
    ap.add_argument("--out", default=os.path.join(HERE, "gemm32_plan_parent.json"))
    args = ap.parse_args()

    if args.gpu_rows:
        old = json.load(open(args.gpu_rows))
        src = old["fields"].index("src") if "src" in old["fields"] else None
        have = {tuple(r[:18]): r for r in old["rows"] if src is None or r[src] == 0}
        rows = []
        for w in GPU_CONTEXTS:
            cus = 256 if w == "full" else MASKED[w][0]
            for s in specs_for(cus):
                r = have[tuple(query_of(s, cus))]
                rows.append(r[:18] + [r[18], r[19], 0, label(s, cus, r[18], r[19])])
    else:
        rows = record_on_gpu(GPU_CONTEXTS)
    # the host build is the same launcher: it must give every recorded call its recorded log
    again = on_host(args.harness, [r[:18] for r in rows])
    differ = [(r, g) for r, g in zip(rows, again) if (r[18], r[19]) != g]
    assert not differ, f"{len(differ)} of {len(rows)} recorded calls differ on the host build: {differ[:3]}"
    print(f"{len(rows)} recorded calls: the host build logs the same", flush=True)
    host = [(s, MASKED[w][0]) for w in HOST_CONTEXTS for s in specs_for(MASKED[w][0])] + [(s, 256) for s in specs_past_dma_limits()]
    for (s, cus), (status, log) in zip(host, on_host(args.harness, [query_of(s, cus) for s, cus in host])):
        rows.append(query_of(s, cus) + [status, log, 1, label(s, cus, status, log)])
    text = dump(args, rows)
    seen = {r[-1] for r in rows}
    assert seen == set(range(len(RETURNS))), f"returns no row took: {[RETURNS[i] for i in set(range(len(RETURNS))) - seen]}"
    largest = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f.endswith(".npz"))
    assert len(text) <= largest, f"{len(text)} bytes: larger than the largest fixture in tests/golden ({largest})"
    print(f"{args.out}: {len(rows)} rows ({sum(r[-2] for r in rows)} from the host build), {len(text)} bytes")


if __name__ == "__main__":
    main()
