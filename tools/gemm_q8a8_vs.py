"""The W8A8 Gemm (int8 weights x int8 activations, f32 group scales on both sides, on the i8 matrix cores: wg_gemm_q8a8) against the calls a caller had before it, in
the same run: wg_gemm_q8 on the same weights with f16 columns of the same values, and wg_gemm_out32 WG_GEMM_TR on the weights dequantised to f16 (twice the weight
bytes) -- and, alone, wg_quantize_q8 of the N f16 columns, the pass that has to run in front of the new call when the activations arrive as f16.

One process. Per shape (k x outputs), pair of group sizes (G, Gx) in (32, 32), (128, per column), (per output, per column) and number of columns (1, 8, 16, 32,
64, 128): seeded int8 weights and activations in [-127, 127] with power-of-two group scales in [2^-2, 2^2], so that the dequantised weights and the f16 columns
x_scale * x are exact and all three products multiply the same numbers. Each call is run eagerly (scratch grows, code objects load), then RECORDED -- LAUNCHES
launches in one command buffer -- and the command buffer is replayed: 5 warm-up submits, then REPS (>= 7) repetitions ALTERNATING the four calls, each at least
MIN_SECONDS of submits between two device events. Per row: the tags the new call logged, median time per launch of the four calls, GB/s of weight bytes for the new
call, the spread s = (max - min) / median of the wg_gemm_q8 repetitions (the baseline), and the ratios. Rows where the new call is slower than wg_gemm_q8 are listed
again at the end.

The yardsticks are the other calls in the same run and the weight bytes. Nothing here is asserted by a test.

    python tools/gemm_q8a8_vs.py [--reps 7] [--min-seconds 0.1] > profiles/gemm_q8a8.txt
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
from tools.mixed_gemv_vs import LAUNCHES, empty, measure, record, upload  # noqa: E402

SHAPES = [(65536, 4096), (11008, 4096), (4096, 11008), (4096, 4096)]  # k x outputs
COLS = [1, 8, 16, 32, 64, 128]
GROUPS = [(32, 32), (128, 0), (0, 0)]  # 0: one scale per output / per column (group size = k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--min-seconds", type=float, default=0.1)
    ap.add_argument("--only", default="", help="run only the shapes whose 'KxO' contains this text")
    ap.add_argument("--cols", default="", help="run only this number of columns")
    args = ap.parse_args()
    assert args.reps >= 7, "the protocol: >= 7 alternating repetitions"
    gpu = wg.GpuInstance.new()
    h = gpu._ctx.handle
    info = gpu.adapter()
    print(f"# W8A8 Gemm (int8 weights x int8 activations, f32 group scales, i8 MFMA) vs wg_gemm_q8 on the same weights with f16 columns of the same values vs wg_gemm_out32 "
          f"GemmTr on the weights dequantised to f16, and wg_quantize_q8 of the N f16 columns alone; {info['name']}, {info['compute_units']} CUs; command buffers of "
          f"{LAUNCHES} launches replayed, {args.reps} repetitions alternating the four calls, >= {args.min_seconds} s of replays each; us per launch (median), GB/s of "
          f"weight bytes (weights + scales); s = (max - min) / median of the wg_gemm_q8 repetitions", flush=True)
    TR = int(wg.GemmVariant.GemmTr)
    slower = []
    for K, O in SHAPES:
        if args.only and args.only not in f"{K}x{O}":
            continue
        rng = np.random.default_rng(K * 7 + O)
        q = rng.integers(-127, 128, K * O).astype(np.int8)
        mq = upload(gpu, q)
        msh = wg.ViewShape((K, O, 1), K, K * O, 0).to_c()
        for G, Gx in GROUPS:
            g, gx = G or K, Gx or K
            ng, ngx = -(-K // g), -(-K // gx)
            s = np.ldexp(np.float32(1), rng.integers(-2, 3, ng * O)).astype(np.float32)
            w16 = (np.repeat(s.reshape(O, ng), g, axis=1)[:, :K].reshape(-1) * q.astype(np.float32)).astype(np.float16)  # column-major: output o, rows 0 .. K
            bs, m16 = upload(gpu, s), upload(gpu, w16)
            del w16
            ssh = wg.ViewShape((ng, O, 1), ng, ng * O, 0).to_c()
            for N in COLS:
                if args.cols and int(args.cols) != N:
                    continue
                r2 = np.random.default_rng(K + O * 3 + N)
                x = r2.integers(-127, 128, K * N).astype(np.int8)
                xs = np.ldexp(np.float32(1), r2.integers(-2, 3, ngx * N)).astype(np.float32)
                x16 = (np.repeat(xs.reshape(N, ngx), gx, axis=1)[:, :K].reshape(-1) * x.astype(np.float32)).astype(np.float16)
                bx, bxs, bx16 = upload(gpu, x), upload(gpu, xs), upload(gpu, x16)
                qx, qxs = empty(gpu, K * N, np.int8), empty(gpu, ngx * N, np.float32)  # the quantiser's own outputs
                outs = [empty(gpu, O * N, np.float32) for _ in range(3)]
                xsh, osh = wg.ViewShape((K, N, 1), K, K * N, 0).to_c(), wg.ViewShape((O, N, 1), O, O * N, 0).to_c()
                xssh = wg.ViewShape((ngx, N, 1), ngx, ngx * N, 0).to_c()
                calls = {
                    "q8a8": lambda: L.check(L.lib.wg_gemm_q8a8(h, TR, g, gx, outs[0]._h, osh, mq._h, msh, bs._h, ssh, bx._h, xsh, bxs._h, xssh)),
                    "gemm_q8": lambda: L.check(L.lib.wg_gemm_q8(h, TR, g, L.WG_F16, outs[1]._h, osh, mq._h, msh, bs._h, ssh, bx16._h, xsh)),
                    "out32": lambda: L.check(L.lib.wg_gemm_out32(h, TR, L.WG_F16, 1.0, 0.0, outs[2]._h, osh, m16._h, msh, bx16._h, xsh)),
                    "quant": lambda: L.check(L.lib.wg_quantize_q8(h, L.WG_F16, gx, qx._h, xsh, qxs._h, xssh, bx16._h, xsh)),
                }
                gpu.take_path()
                calls["q8a8"]()
                path = gpu.take_path()
                calls["quant"]()
                qpath = gpu.take_path()
                cbs = {name: record(gpu, fn) for name, fn in calls.items()}
                for cb in cbs.values():
                    for _ in range(5):
                        gpu.queue().submit([cb])
                gpu.sync()
                # the three products agree (the same numbers: a wrong kernel is not worth timing), and the quantiser gives back x and its scales
                res = [o.read(gpu.device()).astype(np.float64) for o in outs]
                scale = np.abs(res[1]).max() + 1e-30
                assert np.abs(res[0] - res[1]).max() <= 1e-3 * scale and np.abs(res[2] - res[1]).max() <= 1e-3 * scale, (K, O, g, gx, N)
                times = {name: [] for name in cbs}
                for _ in range(args.reps):
                    for name, cb in cbs.items():
                        times[name].append(measure(gpu, cb, args.min_seconds))
                med = {name: statistics.median(t) for name, t in times.items()}
                spread = (max(times["gemm_q8"]) - min(times["gemm_q8"])) / med["gemm_q8"]
                wbytes = K * O + 4 * ng * O
                line = (f"{K:5d} x {O:5d} N {N:3d} G {G or 'out':>3} Gx {Gx or 'col':>3} [{path}] q8a8 {med['q8a8'] * 1e6:8.2f} us {wbytes / med['q8a8'] * 1e-9:7.1f} GB/s | gemm_q8 "
                        f"{med['gemm_q8'] * 1e6:8.2f} us | out32(f16) {med['out32'] * 1e6:8.2f} us | [{qpath}] {med['quant'] * 1e6:7.2f} us | s {spread:.4f} "
                        f"q8a8/gemm_q8 {med['q8a8'] / med['gemm_q8']:.3f} q8a8/out32 {med['q8a8'] / med['out32']:.3f} quant/q8a8 {med['quant'] / med['q8a8']:.3f}")
                print(line, flush=True)
                if med["q8a8"] > med["gemm_q8"]:
                    slower.append(line)
                del cbs, outs, bx, bxs, bx16, qx, qxs
            del bs, m16
        del mq
    print(f"# rows where wg_gemm_q8a8 is slower than wg_gemm_q8: {len(slower)}")
    for line in slower:
        print("#   " + line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
