"""The q4 GemvTr (packed 4-bit weights with f32 group scales, f32 vectors and result: wg_gemv_q4) against the two calls a caller had before it, in the same run:
wg_gemv_q8 on the same values unpacked to int8 (twice the weight bytes) and wg_gemv_mixed on them dequantised to f16 (four times).

One process. Per shape (k x outputs: 65536 x 4096, 11008 x 4096, 4096 x 11008, 4096 x 4096), number of right-hand sides (1, 2, 8) and group_rows (32, 128, per
column): seeded weights over all 16 values and power-of-two group scales in [2^-2, 2^2], so that the dequantised matrix is exact in f16 and all three calls multiply the
same numbers (operands of more than 2^26 weights repeat a seeded block of 2^26); v is seeded U[-1, 1) f32. Each call is run eagerly (scratch grows, code objects
load), then RECORDED -- LAUNCHES launches in one command buffer -- and the command buffer is replayed: 5 warm-up submits, then REPS (>= 7) repetitions ALTERNATING
q4 / q8 / f16, each at least MIN_SECONDS of submits between two device events. Per row: median time per launch and GB/s of matrix bytes (the scales included for q4
and q8) for the three calls, the q8 call's own spread s = (max - min) / median over its repetitions, q4 / q8 and q4 / f16.

The expectation rests on bytes and nothing else: q4 / q8 = (0.5 + 4 / G) / (1 + 4 / G) -- 0.556 at G = 32, 0.515 at 128, 0.50 per column. Rows more than 0.05 above it
are listed again at the end. Nothing here is asserted by a test.

    python tools/gemv_q4_vs.py [--reps 7] [--min-seconds 0.1] > profiles/gemv_q4.txt
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
from tools.mixed_gemv_vs import BLOCK, LAUNCHES, empty, measure, record, upload  # noqa: E402

SHAPES = [(65536, 4096), (11008, 4096), (4096, 11008), (4096, 4096)]  # k x outputs
NRHS = [1, 2, 8]
GROUPS = [32, 128, 0]  # 0: per column (group_rows = k)


def tiled(block, n):
    return block if n <= block.size else np.tile(block, -(-n // block.size))[:n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--min-seconds", type=float, default=0.1)
    ap.add_argument("--only", default="", help="run only the shapes whose 'KxC' contains this text")
    ap.add_argument("--nrhs", default="", help="run only this number of right-hand sides")
    args = ap.parse_args()
    assert args.reps >= 7, "the protocol: >= 7 alternating repetitions"
    gpu = wg.GpuInstance.new()
    h = gpu._ctx.handle
    info = gpu.adapter()
    variant = int(wg.GemvVariant.GemvTr)
    print(f"# q4 GemvTr (packed 4-bit weights, f32 group scales, f32 vectors) vs wg_gemv_q8 on the same values in int8 vs wg_gemv_mixed on them in f16, {info['name']}, "
          f"{info['compute_units']} CUs; command buffers of {LAUNCHES} launches replayed, {args.reps} repetitions alternating the three calls, >= {args.min_seconds} s of "
          f"replays each; us per launch (median), GB/s of matrix bytes (q4, q8: weights + scales); s = (max - min) / median of the q8 call's repetitions; expected "
          f"q4 / q8 = (0.5 + 4 / G) / (1 + 4 / G)", flush=True)
    above = []
    for K, C in SHAPES:
        if args.only and args.only not in f"{K}x{C}":
            continue
        rng = np.random.default_rng(K * 7 + C)
        qblock = rng.integers(-8, 8, min(K * C, BLOCK), dtype=np.int8)
        q = tiled(qblock, K * C)  # column-major: column c, logical rows 0 .. K
        n = (q.astype(np.int16) + 8).astype(np.uint8)
        packed = (n[0::2] | (n[1::2] << 4)).astype(np.uint8)  # K is even: a byte never spans two columns
        del n
        m4, m8 = upload(gpu, packed), upload(gpu, q)
        del packed
        sh4, sh8 = wg.ViewShape((K // 2, C, 1), K // 2, K // 2 * C, 0).to_c(), wg.ViewShape((K, C, 1), K, K * C, 0).to_c()
        for G in GROUPS:
            g = G or K
            ng = -(-K // g)
            s = np.ldexp(np.float32(1), rng.integers(-2, 3, ng * C)).astype(np.float32)
            w16 = (np.repeat(s.reshape(C, ng), g, axis=1)[:, :K].reshape(-1) * q.astype(np.float32)).astype(np.float16)  # exact: 4 bits times a power of two
            bufs = dict(s=upload(gpu, s), m16=upload(gpu, w16))
            del w16
            ssh = wg.ViewShape((ng, C, 1), ng, ng * C, 0).to_c()
            for nrhs in NRHS:
                if args.nrhs and int(args.nrhs) != nrhs:
                    continue
                v = (np.random.default_rng(K + C * 3 + nrhs).random(K * nrhs, dtype=np.float32) * 2 - 1).astype(np.float32)
                bv = upload(gpu, v)
                outs = [empty(gpu, C * nrhs, np.float32) for _ in range(3)]
                vsh, osh = wg.ViewShape((K, nrhs, 1), K, K * nrhs, 0).to_c(), wg.ViewShape((C, nrhs, 1), C, C * nrhs, 0).to_c()
                calls = {
                    "q4": lambda: L.check(L.lib.wg_gemv_q4(h, variant, g, outs[0]._h, osh, m4._h, sh4, bufs["s"]._h, ssh, bv._h, vsh)),
                    "q8": lambda: L.check(L.lib.wg_gemv_q8(h, variant, g, outs[1]._h, osh, m8._h, sh8, bufs["s"]._h, ssh, bv._h, vsh)),
                    "f16": lambda: L.check(L.lib.wg_gemv_mixed(h, variant, L.WG_F16, outs[2]._h, osh, bufs["m16"]._h, sh8, bv._h, vsh)),
                }
                gpu.take_path()
                calls["q4"]()
                path = gpu.take_path()
                cbs = {name: record(gpu, fn) for name, fn in calls.items()}
                for cb in cbs.values():
                    for _ in range(5):
                        gpu.queue().submit([cb])
                gpu.sync()
                # the three calls agree (the same numbers: a wrong kernel is not worth timing)
                res = [o.read(gpu.device()).astype(np.float64) for o in outs]
                scale = np.abs(res[2]).max() + 1e-30
                assert np.abs(res[0] - res[2]).max() <= 1e-3 * scale and np.abs(res[1] - res[2]).max() <= 1e-3 * scale, (K, C, g, nrhs)
                times = {name: [] for name in cbs}
                for _ in range(args.reps):
                    for name, cb in cbs.items():
                        times[name].append(measure(gpu, cb, args.min_seconds))
                med = {name: statistics.median(t) for name, t in times.items()}
                spread = (max(times["q8"]) - min(times["q8"])) / med["q8"]
                ratio, expect = med["q4"] / med["q8"], (0.5 + 4 / g) / (1 + 4 / g)
                bytes_ = {"q4": K * C // 2 + 4 * ng * C, "q8": K * C + 4 * ng * C, "f16": 2 * K * C}
                gbs = {name: bytes_[name] / med[name] * 1e-9 for name in med}
                line = (f"GemvTr {K:5d} x {C:5d} rhs {nrhs} G {G or 'col':>3} [{path}] q4 {med['q4'] * 1e6:8.2f} us {gbs['q4']:7.1f} GB/s | q8 {med['q8'] * 1e6:8.2f} us "
                        f"{gbs['q8']:7.1f} GB/s | f16 {med['f16'] * 1e6:8.2f} us {gbs['f16']:7.1f} GB/s | s {spread:.4f} q4/q8 {ratio:.3f} (bytes: {expect:.3f}) q4/f16 "
                        f"{med['q4'] / med['f16']:.3f}")
                print(line, flush=True)
                if ratio > expect + 0.05:
                    above.append(line)
                del cbs, outs, bv
            del bufs
        del m4, m8
    print(f"# rows with q4 / q8 more than 0.05 above the byte ratio: {len(above)}")
    for line in above:
        print("#   " + line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
