"""The mixed-precision Gemv (16-bit matrix, f32 vectors and result: wg_gemv_mixed) against the two calls a caller had before it, in the same run: the 16-bit wg_gemv
(the same kernels on the same matrix bytes -- the yardstick) and the f32 wg_gemv (twice the bytes).

One process. Per shape and 16-bit type: a seeded U[-1, 1) matrix rounded to the type (operands of more than 2^26 elements repeat a seeded block of 2^26), the f32 matrix
holds the same values widened; v is drawn in the 16-bit type so that all three calls multiply the same numbers. Each call is run eagerly (scratch grows, code objects load),
then RECORDED -- LAUNCHES launches in one command buffer -- and the command buffer is replayed: 5 warm-up submits, then REPS (>= 7) repetitions ALTERNATING mixed / 16-bit /
f32, each at least MIN_SECONDS of submits between two device events. Per row: median time per launch and GB/s of matrix bytes for the three calls, the 16-bit call's own
spread s = (max - min) / median over its repetitions, and mixed / 16-bit.

The expectation rests on bytes: the mixed call streams the 16-bit call's matrix plus < 0.1 % for the wider vectors, so it should take the 16-bit call's time. A row is
"within" when |mixed / 16-bit - 1| <= s; rows outside are listed again at the end. Nothing here is asserted by a test.

    python tools/mixed_gemv_vs.py [--reps 7] [--min-seconds 0.1] > profiles/mixed_gemv.txt
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
LAUNCHES = 20

# (variant, stored rows, stored columns): the decode shapes of a 4096-wide model (both variants), the two flagship streams, one launch-bound size
SHAPES = [("Gemv", 4096, 65536), ("GemvTr", 65536, 4096), ("Gemv", 4096, 11008), ("GemvTr", 4096, 11008), ("Gemv", 11008, 4096), ("GemvTr", 11008, 4096),
          ("Gemv", 4096, 4096), ("GemvTr", 4096, 4096), ("Gemv", 1024, 1024), ("GemvTr", 1024, 1024)]


def to16(kind, x32):
    return x32.astype(np.float16) if kind == "f16" else wg.to_bfloat16(x32)


def widen(kind, x16):
    return x16.astype(np.float32) if kind == "f16" else wg.from_bfloat16(x16)


def values(seed, n, kind):
    """n seeded U[-1, 1) values as (16-bit array, the same values as f32)."""
    x = np.random.default_rng(seed).random(min(n, BLOCK), dtype=np.float32) * 2 - 1
    h = to16(kind, x)
    w = widen(kind, h)
    if n > BLOCK:
        reps = -(-n // BLOCK)
        h, w = np.tile(h, reps)[:n], np.tile(w, reps)[:n]
    return h, w


def upload(gpu, arr):
    return wg.TensorBuilder.tensor((arr.size,), S).build_init(gpu.device(), arr, arr.dtype)


def empty(gpu, n, dtype):
    return wg.TensorBuilder.tensor((n,), S).build(gpu.device(), dtype)


def record(gpu, fn):
    fn()  # eagerly first: the scratch of a split cannot grow inside a recording
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
    ap.add_argument("--only", default="", help="run only the shapes whose 'RxC' contains this text")
    args = ap.parse_args()
    assert args.reps >= 7, "the protocol: >= 7 alternating repetitions"
    gpu = wg.GpuInstance.new()
    h = gpu._ctx.handle
    info = gpu.adapter()
    print(f"# mixed Gemv (16-bit matrix, f32 vectors) vs the 16-bit wg_gemv vs the f32 wg_gemv, {info['name']}, {info['compute_units']} CUs; command buffers of {LAUNCHES} "
          f"launches replayed, {args.reps} repetitions alternating the three calls, >= {args.min_seconds} s of replays each; us per launch (median), GB/s of matrix bytes; "
          f"s = (max - min) / median of the 16-bit call's repetitions; within: |mixed / 16-bit - 1| <= s")
    DT = {"f16": (L.WG_F16, np.float16), "bf16": (L.WG_BF16, wg.bfloat16)}
    outside = []
    for variant_name, R, C in SHAPES:
        if args.only and args.only not in f"{R}x{C}":
            continue
        tr = variant_name == "GemvTr"
        k, ro = (R, C) if tr else (C, R)
        variant = int(wg.GemvVariant.GemvTr if tr else wg.GemvVariant.Gemv)
        msh, vsh, osh = wg.ViewShape((R, C, 1), R, R * C, 0).to_c(), wg.ViewShape((k, 1, 1), k, k, 0).to_c(), wg.ViewShape((ro, 1, 1), ro, ro, 0).to_c()
        for kind, (dt, npdt) in DT.items():
            m16, m32 = values(R * 7 + C, R * C, kind)
            v16, v32 = values(R + C * 3 + 1, k, kind)
            bufs = dict(m16=upload(gpu, m16), m32=upload(gpu, m32), v16=upload(gpu, v16), v32=upload(gpu, v32), o16=empty(gpu, ro, npdt), o32=empty(gpu, ro, np.float32),
                        o32b=empty(gpu, ro, np.float32))
            del m16, m32
            calls = {
                "mixed": lambda: L.check(L.lib.wg_gemv_mixed(h, variant, dt, bufs["o32"]._h, osh, bufs["m16"]._h, msh, bufs["v32"]._h, vsh)),
                "16": lambda: L.check(L.lib.wg_gemv(h, variant, dt, bufs["o16"]._h, osh, bufs["m16"]._h, msh, bufs["v16"]._h, vsh)),
                "f32": lambda: L.check(L.lib.wg_gemv(h, variant, L.WG_F32, bufs["o32b"]._h, osh, bufs["m32"]._h, msh, bufs["v32"]._h, vsh)),
            }
            gpu.take_path()
            calls["mixed"]()
            path = " ".join(t for t in gpu.take_path().split() if "gemv." in t or "gemv_any" in t)
            cbs = {name: record(gpu, fn) for name, fn in calls.items()}
            for cb in cbs.values():
                for _ in range(5):
                    gpu.queue().submit([cb])
            gpu.sync()
            times = {name: [] for name in cbs}
            for _ in range(args.reps):
                for name, cb in cbs.items():
                    times[name].append(measure(gpu, cb, args.min_seconds))
            med = {name: statistics.median(t) for name, t in times.items()}
            spread = (max(times["16"]) - min(times["16"])) / med["16"]
            ratio = med["mixed"] / med["16"]
            verdict = "within" if abs(ratio - 1) <= spread else ("OUTSIDE (slower)" if ratio > 1 else "OUTSIDE (faster)")
            gbs = {name: R * C * (4 if name == "f32" else 2) / med[name] * 1e-9 for name in med}
            line = (f"{variant_name:6s} {R:5d} x {C:5d} {kind:4s} [{path}] mixed {med['mixed'] * 1e6:8.2f} us {gbs['mixed']:7.1f} GB/s | {kind} {med['16'] * 1e6:8.2f} us "
                    f"{gbs['16']:7.1f} GB/s | f32 {med['f32'] * 1e6:8.2f} us {gbs['f32']:7.1f} GB/s | s {spread:.4f} mixed/{kind} {ratio:.4f} f32/mixed {med['f32'] / med['mixed']:.3f} | {verdict}")
            print(line, flush=True)
            if verdict != "within":
                outside.append(line)
            del cbs, bufs
    print(f"# rows outside the 16-bit call's own spread: {len(outside)}")
    for line in outside:
        print("#   " + line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
