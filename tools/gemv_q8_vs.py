"""The q8 Gemv (int8 matrix with f32 group scales, f32 vectors and result: wg_gemv_q8) against the two calls a caller had before it, in the same run: wg_gemv_mixed on
an f16 matrix of the same values (twice the matrix bytes -- the yardstick) and the f32 wg_gemv (four times).

One process. Per shape (tools/mixed_gemv_vs.py's), variant, number of right-hand sides (1, 2, 8) and group_rows (32, 128, per column): seeded int8 weights in [-127, 127]
and power-of-two group scales in [2^-2, 2^2], so that the dequantised matrix is exact in f16 and all three calls multiply the same numbers (operands of more than 2^26
elements repeat a seeded block of 2^26); v is seeded U[-1, 1) f32. Each call is run eagerly (scratch grows, code objects load), then RECORDED -- LAUNCHES launches in one
command buffer -- and the command buffer is replayed: 5 warm-up submits, then REPS (>= 7) repetitions ALTERNATING q8 / f16 / f32, each at least MIN_SECONDS of
submits between two device events. Per row: median time per launch and GB/s of matrix bytes (the scales included for q8) for the three calls, the f16 call's own
spread s = (max - min) / median over its repetitions, and q8 / f16.

The expectation rests on bytes: (1 + 4 / G) bytes per weight against 2, i.e. q8 / f16 = 0.53 .. 0.56 on shapes that stream from HBM. Rows above 0.60 are listed again at
the end. Nothing here is asserted by a test.

    python tools/gemv_q8_vs.py [--reps 7] [--min-seconds 0.1] > profiles/gemv_q8.txt
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
from tools.mixed_gemv_vs import BLOCK, LAUNCHES, SHAPES, empty, measure, record, upload  # noqa: E402

NRHS = [1, 2, 8]
GROUPS = [32, 128, 0]  # 0: per column (group_rows = rows)


def tiled(block, n):
    return block if n <= block.size else np.tile(block, -(-n // block.size))[:n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--min-seconds", type=float, default=0.1)
    ap.add_argument("--only", default="", help="run only the shapes whose 'RxC' contains this text")
    ap.add_argument("--nrhs", default="", help="run only this number of right-hand sides")
    args = ap.parse_args()
    assert args.reps >= 7, "the protocol: >= 7 alternating repetitions"
    gpu = wg.GpuInstance.new()
    h = gpu._ctx.handle
    info = gpu.adapter()
    print(f"# q8 Gemv (int8 matrix, f32 group scales, f32 vectors) vs wg_gemv_mixed on the same values in f16 vs the f32 wg_gemv, {info['name']}, {info['compute_units']} CUs; "
          f"command buffers of {LAUNCHES} launches replayed, {args.reps} repetitions alternating the three calls, >= {args.min_seconds} s of replays each; us per launch "
          f"(median), GB/s of matrix bytes (q8: weights + scales); s = (max - min) / median of the f16 call's repetitions; expected q8 / f16 = (1 + 4 / G) / 2", flush=True)
    above = []
    for variant_name, R, C in SHAPES:
        if args.only and args.only not in f"{R}x{C}":
            continue
        tr = variant_name == "GemvTr"
        k, ro = (R, C) if tr else (C, R)
        variant = int(wg.GemvVariant.GemvTr if tr else wg.GemvVariant.Gemv)
        rng = np.random.default_rng(R * 7 + C)
        qblock = rng.integers(-127, 128, min(R * C, BLOCK)).astype(np.int8)
        q = tiled(qblock, R * C)
        mq = upload(gpu, q)
        msh = wg.ViewShape((R, C, 1), R, R * C, 0).to_c()
        for G in GROUPS:
            g = G or R
            ng = -(-R // g)
            s = np.ldexp(np.float32(1), rng.integers(-2, 3, ng * C)).astype(np.float32)
            w = (np.repeat(s.reshape(C, ng), g, axis=1)[:, :R].reshape(-1) * q.astype(np.float32)).astype(np.float32)  # column-major: column c, rows 0 .. R
            bufs = dict(s=upload(gpu, s), m16=upload(gpu, w.astype(np.float16)), m32=upload(gpu, w))
            del w
            ssh = wg.ViewShape((ng, C, 1), ng, ng * C, 0).to_c()
            for nrhs in NRHS:
                if args.nrhs and int(args.nrhs) != nrhs:
                    continue
                v = (np.random.default_rng(R + C * 3 + nrhs).random(k * nrhs, dtype=np.float32) * 2 - 1).astype(np.float32)
                bv = upload(gpu, v)
                outs = [empty(gpu, ro * nrhs, np.float32) for _ in range(3)]
                vsh, osh = wg.ViewShape((k, nrhs, 1), k, k * nrhs, 0).to_c(), wg.ViewShape((ro, nrhs, 1), ro, ro * nrhs, 0).to_c()
                calls = {
                    "q8": lambda: L.check(L.lib.wg_gemv_q8(h, variant, g, outs[0]._h, osh, mq._h, msh, bufs["s"]._h, ssh, bv._h, vsh)),
                    "f16": lambda: L.check(L.lib.wg_gemv_mixed(h, variant, L.WG_F16, outs[1]._h, osh, bufs["m16"]._h, msh, bv._h, vsh)),
                    "f32": lambda: L.check(L.lib.wg_gemv(h, variant, L.WG_F32, outs[2]._h, osh, bufs["m32"]._h, msh, bv._h, vsh)),
                }
                gpu.take_path()
                calls["q8"]()
                path = gpu.take_path()
                cbs = {name: record(gpu, fn) for name, fn in calls.items()}
                for cb in cbs.values():
                    for _ in range(5):
                        gpu.queue().submit([cb])
                gpu.sync()
                # the three calls agree (the same numbers: a wrong kernel is not worth timing)
                res = [o.read(gpu.device()).astype(np.float64) for o in outs]
                scale = np.abs(res[2]).max() + 1e-30
                assert np.abs(res[0] - res[2]).max() <= 1e-3 * scale and np.abs(res[1] - res[2]).max() <= 1e-3 * scale, (variant_name, R, C, g, nrhs)
                times = {name: [] for name in cbs}
                for _ in range(args.reps):
                    for name, cb in cbs.items():
                        times[name].append(measure(gpu, cb, args.min_seconds))
                med = {name: statistics.median(t) for name, t in times.items()}
                spread = (max(times["f16"]) - min(times["f16"])) / med["f16"]
                ratio, expect = med["q8"] / med["f16"], (1 + 4 / g) / 2
                bytes_ = {"q8": R * C + 4 * ng * C, "f16": 2 * R * C, "f32": 4 * R * C}
                gbs = {name: bytes_[name] / med[name] * 1e-9 for name in med}
                line = (f"{variant_name:6s} {R:5d} x {C:5d} rhs {nrhs} G {G or 'col':>3} [{path}] q8 {med['q8'] * 1e6:8.2f} us {gbs['q8']:7.1f} GB/s | f16 {med['f16'] * 1e6:8.2f} us "
                        f"{gbs['f16']:7.1f} GB/s | f32 {med['f32'] * 1e6:8.2f} us {gbs['f32']:7.1f} GB/s | s {spread:.4f} q8/f16 {ratio:.3f} (bytes: {expect:.3f}) f32/q8 "
                        f"{med['f32'] / med['q8']:.2f}")
                print(line, flush=True)
                if ratio > 0.60:
                    above.append(line)
                del cbs, outs, bv
            del bufs
        del mq
    print(f"# rows with q8 / f16 above 0.60: {len(above)}")
    for line in above:
        print("#   " + line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
