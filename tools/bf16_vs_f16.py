"""bf16 against f16 in the same run: the yardstick of the bfloat16 kernels is the f16 path they were compiled from (same instruction rate, same bytes, same schedule).

One process. Per shape: seeded U[-1, 1) operands rounded to each format (operands of more than 2^26 elements repeat a seeded block of 2^26), 10 warm-up launches
per format, then REPS (>= 7) repetitions ALTERNATING f16 and bf16, each at least MIN_SECONDS (0.3) of launches between two device events and bracketed by
wg_debug_clock_begin / _end. The OpAssign row runs both formats in the same device memory (why: at the row). Per row: median time per launch, TFLOP/s or GB/s, mean shader clock, and the f16 repetitions' own spread s = (max - min) / median.

A row passes when median(bf16) / median(f16) <= 1 + 2 s. A row that misses is attributed to the clocks only if the cycle counts (time x mean clock) agree within 2 s
-- a power effect of the bit patterns; anything else is a defect of the port. The verdict per row is printed; the exit status is 1 if any row is a defect.

    python tools/bf16_vs_f16.py [--reps 7] [--min-seconds 0.3] [--only gemm|gemv|reduce|op] > profiles/bf16_vs_f16.txt
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import wgmath_amd as wg  # noqa: E402
from wgmath_amd import _lib as L  # noqa: E402

S = wg.BufferUsages.STORAGE | wg.BufferUsages.COPY_SRC | wg.BufferUsages.COPY_DST
BLOCK = 1 << 26


def operands(seed, n):
    """n seeded U[-1, 1) values as (f16 array, bf16 array)."""
    x = np.random.default_rng(seed).random(min(n, BLOCK), dtype=np.float32) * 2 - 1
    h, b = x.astype(np.float16), wg.to_bfloat16(x)
    if n > BLOCK:
        reps = -(-n // BLOCK)
        h, b = np.tile(h, reps)[:n], np.tile(b, reps)[:n]
    return h, b


def upload(gpu, arr):
    return wg.TensorBuilder.tensor((arr.size,), S).build_init(gpu.device(), arr, arr.dtype)


def empty(gpu, n, dtype):
    return wg.TensorBuilder.tensor((n,), S).build(gpu.device(), dtype)


def measure(gpu, launch, min_seconds):
    """One repetition: (seconds per launch, mean shader clock in GHz or None)."""
    dev = gpu.device()
    ts = wg.GpuTimestamps(dev, 2)
    ts.write(dev); launch(); ts.write(dev)
    t = ts.wait_for_results_ms()
    one = max((t[1] - t[0]) * 1e-3, 1e-6)
    n = max(1, int(min_seconds / one) + 1)
    ts = wg.GpuTimestamps(dev, 2)
    probe = gpu.clock_probe()
    ts.write(dev)
    for _ in range(n):
        launch()
    ts.write(dev)
    clock = probe.end()
    t = ts.wait_for_results_ms()
    return (t[1] - t[0]) * 1e-3 / n, (clock or {}).get("mean")


def row(gpu, name, launches, work, unit, reps, min_seconds, prepare=None):
    """launches: {"f16": fn, "bf16": fn}; work: FLOP or bytes per launch; prepare: {"f16": fn, "bf16": fn} run before a format's launches, outside the timed
    interval (the formats share their device memory: see main)."""
    for dt, fn in launches.items():
        if prepare:
            prepare[dt]()
        for _ in range(10):
            fn()
    gpu.sync()
    times, clocks = {"f16": [], "bf16": []}, {"f16": [], "bf16": []}
    for _ in range(reps):
        for dt in ("f16", "bf16"):
            if prepare:
                prepare[dt]()
            s, c = measure(gpu, launches[dt], min_seconds)
            times[dt].append(s)
            if c:
                clocks[dt].append(c)
    med = {dt: statistics.median(times[dt]) for dt in times}
    clk = {dt: (statistics.mean(clocks[dt]) if clocks[dt] else float("nan")) for dt in times}
    spread = (max(times["f16"]) - min(times["f16"])) / med["f16"]
    ratio = med["bf16"] / med["f16"]
    cyc = (med["bf16"] * clk["bf16"]) / (med["f16"] * clk["f16"])
    if ratio <= 1 + 2 * spread:
        verdict = "pass"
    elif cyc == cyc and cyc <= 1 + 2 * spread:
        verdict = "clock (the cycle counts agree within 2 s: a power effect of the bit patterns)"
    else:
        verdict = "DEFECT (more cycles than f16)"
    scale = 1e-12 if unit == "TFLOP/s" else 1e-9
    print(f"{name:44s} f16 {med['f16'] * 1e6:9.1f} us {work / med['f16'] * scale:8.1f} {unit} {clk['f16']:.3f} GHz | "
          f"bf16 {med['bf16'] * 1e6:9.1f} us {work / med['bf16'] * scale:8.1f} {unit} {clk['bf16']:.3f} GHz | s {spread:.4f} ratio {ratio:.4f} cycles {cyc:.4f} | {verdict}",
          flush=True)
    return verdict


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    assert args.reps >= 7 and args.min_seconds >= 0.3, "the protocol: >= 7 repetitions of >= 0.3 s"
    gpu = wg.GpuInstance.new()
    h = gpu._ctx.handle
    info = gpu.adapter()
    print(f"# bf16 vs f16, {info['name']}, {info['compute_units']} CUs; {args.reps} repetitions alternating f16 / bf16, >= {args.min_seconds} s of launches each, "
          f"10 warm-up launches per format; s = (max - min) / median of the f16 repetitions; pass: ratio <= 1 + 2 s")
    DT = {"f16": (L.WG_F16, np.float16), "bf16": (L.WG_BF16, wg.bfloat16)}
    verdicts = []
    want = lambda k: not args.only or args.only == k

    if want("gemm"):
        for M, K, N in ((8192, 8192, 8192), (8192, 1024, 8192), (4096, 4096, 4096), (2048, 2048, 2048), (131072, 8192, 1024)):
            a, b = operands(M + K, M * K), operands(K + N + 1, K * N)
            bufs = {dt: (upload(gpu, a[i]), upload(gpu, b[i]), empty(gpu, M * N, DT[dt][1])) for i, dt in enumerate(("f16", "bf16"))}
            del a, b
            for tr in (False, True):
                ash = wg.ViewShape(((K, M) if tr else (M, K)) + (1,), K if tr else M, M * K, 0).to_c()
                bsh, osh = wg.ViewShape((K, N, 1), K, K * N, 0).to_c(), wg.ViewShape((M, N, 1), M, M * N, 0).to_c()
                variant = int(wg.GemmVariant.GemmTr if tr else wg.GemmVariant.Gemm)
                launches = {dt: (lambda dt=dt: L.check(L.lib.wg_gemm(h, variant, DT[dt][0], bufs[dt][2]._h, osh, bufs[dt][0]._h, ash, bufs[dt][1]._h, bsh))) for dt in DT}
                gpu.take_path()
                for dt in DT:
                    launches[dt]()
                path = gpu.take_path()
                verdicts.append(row(gpu, f"{'GemmTr' if tr else 'Gemm'} {M}x{N}x{K} [{' '.join(t for t in path.split() if 'bf16' in t)}]", launches, 2.0 * M * N * K,
                                    "TFLOP/s", args.reps, args.min_seconds))
            del bufs

    if want("gemv") or want("reduce"):
        R, C = 4096, 65536
        m = operands(7, R * C)
        mats = {dt: upload(gpu, m[i]) for i, dt in enumerate(("f16", "bf16"))}
        del m
        if want("gemv"):
            for tr in (False, True):
                for nrhs in (1, 8):
                    ro, k = (C, R) if tr else (R, C)
                    v = operands(8 + nrhs, k * nrhs)
                    vec = {dt: (upload(gpu, v[i]), empty(gpu, ro * nrhs, DT[dt][1])) for i, dt in enumerate(("f16", "bf16"))}
                    msh, vsh, osh = wg.ViewShape((R, C, 1), R, R * C, 0).to_c(), wg.ViewShape((k, nrhs, 1), k, k * nrhs, 0).to_c(), wg.ViewShape((ro, nrhs, 1), ro, ro * nrhs, 0).to_c()
                    variant = int(wg.GemvVariant.GemvTr if tr else wg.GemvVariant.Gemv)
                    launches = {dt: (lambda dt=dt: L.check(L.lib.wg_gemv(h, variant, DT[dt][0], vec[dt][1]._h, osh, mats[dt]._h, msh, vec[dt][0]._h, vsh))) for dt in DT}
                    verdicts.append(row(gpu, f"{'GemvTr' if tr else 'Gemv'} {R}x{C}, {nrhs} rhs", launches, 2.0 * R * C, "GB/s", args.reps, args.min_seconds))
        if want("reduce"):  # Sum of each of the 4096 vectors of 65536 elements (the same memory seen as 65536 x 4096)
            res = {dt: empty(gpu, R, DT[dt][1]) for dt in DT}
            vsh = wg.ViewShape((C, R, 1), C, R * C, 0).to_c()
            launches = {dt: (lambda dt=dt: L.check(L.lib.wg_reduce_batched(h, int(wg.ReduceOp.Sum), DT[dt][0], mats[dt]._h, vsh, res[dt]._h))) for dt in DT}
            verdicts.append(row(gpu, f"Reduce Sum, {R} vectors of {C}", launches, 2.0 * R * C, "GB/s", args.reps, args.min_seconds))
        del mats

    if want("op"):
        n = 1 << 26
        x = operands(20, n)
        small = np.random.default_rng(21).random(n, dtype=np.float32) * np.float32(2.0 ** -12)  # (a += b thousands of times: b small, so that a stays finite in f16)
        y = (small.astype(np.float16), wg.to_bfloat16(small))
        # ONE pair of buffers for both formats, rewritten with the format's operands before each of its repetitions. This stream runs within a few per cent of what
        # the memory gives, and how fast a 128 MiB allocation streams depends on where it lies: the SAME f16 kernel on the same data takes 53.9 .. 54.3 us in one
        # process and 55.0 .. 55.2 us in the next (s = 0.0003 inside either), and with a pair of buffers per format the row compared two allocations, not two
        # kernels -- bf16 2.4 % ahead in one process and 2.1 % behind in the next (profiles/bf16_vs_f16.txt).
        ta, tb = empty(gpu, n, np.uint16), empty(gpu, n, np.uint16)
        sh = wg.ViewShape((n, 1, 1), n, n, 0).to_c()
        data = {dt: (x[i].view(np.uint16), y[i].view(np.uint16)) for i, dt in enumerate(("f16", "bf16"))}
        prepare = {dt: (lambda dt=dt: (gpu.queue().write_buffer(ta, 0, data[dt][0]), gpu.queue().write_buffer(tb, 0, data[dt][1]))) for dt in DT}
        launches = {dt: (lambda dt=dt: L.check(L.lib.wg_op_assign(h, int(wg.OpAssignVariant.Add), DT[dt][0], ta._h, sh, tb._h, sh))) for dt in DT}
        verdicts.append(row(gpu, "OpAssign Add, 2^26 (one pair of buffers)", launches, 3.0 * 2 * n, "GB/s", args.reps, args.min_seconds, prepare))  # (a: read + write, b: read)

    bad = [v for v in verdicts if v.startswith("DEFECT")]
    print(f"# {len(verdicts)} rows: {sum(v == 'pass' for v in verdicts)} pass, {sum(v.startswith('clock') for v in verdicts)} attributed to the clock, {len(bad)} defects")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
