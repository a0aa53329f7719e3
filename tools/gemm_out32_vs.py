"""Gemm on 16-bit operands with an f32 result (wg_gemm_out32) against the 16-bit wg_gemm_ex of the same shape, in the same run. The 16-bit call is unchanged code: it
is the yardstick. What differs is the epilogue: the same tiles and MFMA chains, then twice the bytes and twice the store instructions for the result.

One process. Per shape, variant and 16-bit type: seeded U[-1, 1) operands rounded to the type (operands of more than 2^26 elements repeat a seeded block of 2^26). Each
call is run eagerly (scratch grows, code objects load), then RECORDED -- LAUNCHES launches in one command buffer -- and the command buffer is replayed: 5 warm-up
submits, then REPS (>= 7) repetitions ALTERNATING out32 / 16-bit, each at least MIN_SECONDS of submits between two device events. Per row: the leaf both calls took,
median time per launch and TFLOP/s for the two calls, the 16-bit call's own spread s = (max - min) / median over its repetitions, out32 / 16-bit, and one line of
reason: the bytes of the result against the bytes and flops of the product. Where the 16-bit call takes the continuous walk (which the out32 call does not have) a
second yardstick is timed as well: the 16-bit call with the walk switched off (WG_TUNE_F16_CONT = 0), i.e. the same kernel as the out32 call.

Nothing here is asserted by a test.

    python tools/gemm_out32_vs.py [--reps 7] [--min-seconds 0.1] > profiles/gemm_out32.txt
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
LAUNCHES = 10

# (M, K, N, variants): out (M x N) = op(m1) (M x K) m2 (K x N)
SHAPES = [(8192, 8192, 8192, ("Gemm", "GemmTr")), (8192, 1024, 8192, ("Gemm", "GemmTr")), (8192, 256, 8192, ("Gemm", "GemmTr")), (4096, 2048, 2048, ("Gemm", "GemmTr")),
          (2048, 2048, 2048, ("Gemm", "GemmTr")), (512, 16384, 8, ("GemmTr",))]


def values(seed, n, kind):
    x = np.random.default_rng(seed).random(min(n, BLOCK), dtype=np.float32) * 2 - 1
    h = x.astype(np.float16) if kind == "f16" else wg.to_bfloat16(x)
    return np.tile(h, -(-n // BLOCK))[:n] if n > BLOCK else h


def upload(gpu, arr):
    return wg.TensorBuilder.tensor((arr.size,), S).build_init(gpu.device(), arr, arr.dtype)


def empty(gpu, n, dtype):
    return wg.TensorBuilder.tensor((n,), S).build(gpu.device(), dtype)


def record(gpu, fn):
    fn()  # eagerly first: scratch cannot grow inside a recording
    gpu.sync()
    enc = gpu.device().create_command_encoder(record=True)
    try:
        for _ in range(LAUNCHES):
            fn()
    finally:
        cb = enc.finish()
    return cb


def measure(gpu, cb, min_seconds):
    """One repetition: seconds per launch over >= min_seconds of replays of the command buffer."""
    dev, q = gpu.device(), gpu.queue()
    ts = wg.GpuTimestamps(dev, 2)
    ts.write(dev); q.submit([cb]); ts.write(dev)
    t = ts.wait_for_results_ms()
    one = max((t[1] - t[0]) * 1e-3, 1e-6)
    n = max(1, int(min_seconds / one) + 1)
    ts = wg.GpuTimestamps(dev, 2)
    ts.write(dev)
    for _ in range(n):
        q.submit([cb])
    ts.write(dev)
    t = ts.wait_for_results_ms()
    return (t[1] - t[0]) * 1e-3 / (n * LAUNCHES)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--min-seconds", type=float, default=0.1)
    ap.add_argument("--only", default="", help="run only the shapes whose 'MxKxN' contains this text")
    args = ap.parse_args()
    assert args.reps >= 7, "the protocol: >= 7 alternating repetitions"
    gpu = wg.GpuInstance.new()
    h = gpu._ctx.handle
    info = gpu.adapter()
    print(f"# Gemm with an f32 result (wg_gemm_out32) vs the 16-bit wg_gemm_ex, {info['name']}, {info['compute_units']} CUs; command buffers of {LAUNCHES} launches replayed, "
          f"{args.reps} repetitions alternating the calls, >= {args.min_seconds} s of replays each; us per launch (median); s = (max - min) / median of the 16-bit call's "
          f"repetitions; M x K x N")
    DT = {"f16": (L.WG_F16, np.float16), "bf16": (L.WG_BF16, wg.bfloat16)}
    ratios = []
    for M, K, N, variants in SHAPES:
        if args.only and args.only not in f"{M}x{K}x{N}":
            continue
        for variant_name in variants:
            tr = variant_name == "GemmTr"
            variant = int(wg.GemmVariant.GemmTr if tr else wg.GemmVariant.Gemm)
            ash = wg.ViewShape(((K, M) if tr else (M, K)) + (1,), K if tr else M, M * K, 0).to_c()
            bsh, osh = wg.ViewShape((K, N, 1), K, K * N, 0).to_c(), wg.ViewShape((M, N, 1), M, M * N, 0).to_c()
            for kind, (dt, npdt) in DT.items():
                bufs = dict(a=upload(gpu, values(M * 7 + K, M * K, kind)), b=upload(gpu, values(K + N * 3 + 1, K * N, kind)), o16=empty(gpu, M * N, npdt),
                            o32=empty(gpu, M * N, np.float32))
                calls = {
                    "out32": lambda: L.check(L.lib.wg_gemm_out32(h, variant, dt, 1.0, 0.0, bufs["o32"]._h, osh, bufs["a"]._h, ash, bufs["b"]._h, bsh)),
                    "16": lambda: L.check(L.lib.wg_gemm_ex(h, variant, dt, 1.0, 0.0, bufs["o16"]._h, osh, bufs["a"]._h, ash, bufs["b"]._h, bsh)),
                }
                gpu.take_path()
                calls["out32"]()
                p32 = gpu.take_path()
                calls["16"]()
                p16 = gpu.take_path()
                cbs = {name: record(gpu, fn) for name, fn in calls.items()}
                if "cont" in p16:  # the 16-bit call on the out32 call's kernel: the walk switched off while this command buffer is recorded
                    old = gpu.set_tuning("f16_cont", 0)
                    cbs["16/no walk"] = record(gpu, calls["16"])
                    gpu.set_tuning("f16_cont", old)
                for cb in cbs.values():
                    for _ in range(5):
                        gpu.queue().submit([cb])
                gpu.sync()
                gpu.take_path()
                times = {name: [] for name in cbs}
                for _ in range(args.reps):
                    for name, cb in cbs.items():
                        times[name].append(measure(gpu, cb, args.min_seconds))
                med = {name: statistics.median(t) for name, t in times.items()}
                spread = (max(times["16"]) - min(times["16"])) / med["16"]
                ratio = med["out32"] / med["16"]
                tf = {name: 2.0 * M * N * K / med[name] * 1e-12 for name in med}
                extra = ""
                if "16/no walk" in med:
                    extra = f" | {kind} without the walk {med['16/no walk'] * 1e6:8.2f} us, out32 / that {med['out32'] / med['16/no walk']:.4f}"
                    ratios.append(med["out32"] / med["16/no walk"])
                ratios.append(ratio)
                in_mb, o16_mb, o32_mb = (M * K + K * N) * 2 / 2 ** 20, M * N * 2 / 2 ** 20, M * N * 4 / 2 ** 20
                reason = (f"result {o16_mb:.0f} -> {o32_mb:.0f} MiB beside {in_mb:.0f} MiB of operands and {2.0 * M * N * K * 1e-9:.0f} GFLOP: "
                          f"{(o32_mb - o16_mb) * 2 ** 20 / med['16'] * 1e-12:.2f} TB/s more to store in the 16-bit call's time")
                print(f"{variant_name:6s} {M:5d} x {K:5d} x {N:5d} {kind:4s} [{p32} | {p16}] out32 {med['out32'] * 1e6:8.2f} us {tf['out32']:7.1f} TFLOP/s | {kind} "
                      f"{med['16'] * 1e6:8.2f} us {tf['16']:7.1f} TFLOP/s | s {spread:.4f} out32/{kind} {ratio:.4f}{extra} | {reason}", flush=True)
                del cbs, bufs
    if ratios:
        print(f"# out32 / 16-bit over {len(ratios)} ratios: {min(ratios):.3f} .. {max(ratios):.3f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
