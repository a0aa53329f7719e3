"""The q8 Gemm (int8 weights with f32 group scales against N columns of f16 activations on the matrix cores: wg_gemm_q8) against the two calls a caller had before it,
in the same run: wg_gemv_q8 on the same weights with the columns as f32 right-hand sides (a vector-ALU kernel: groups of 8 on grid.z, the matrix streamed once per
group) and wg_gemm_out32 WG_GEMM_TR on the weights dequantised to f16 (twice the weight bytes).

One process. Per shape (k x outputs), group_rows (32, 128, per column) and number of columns (1, 8, 16, 32, 64, 128): seeded int8 weights in [-127, 127] and
power-of-two group scales in [2^-2, 2^2], so that the dequantised matrix is exact in f16 and all three calls multiply the same numbers; x is seeded U[-1, 1) rounded
to f16. Each call is run eagerly (scratch grows, code objects load), then RECORDED -- LAUNCHES launches in one command buffer -- and the command buffer is replayed: 5
warm-up submits, then REPS (>= 7) repetitions ALTERNATING the three calls, each at least MIN_SECONDS of submits between two device events. Per row: the tags the new
call logged, median time per launch of the three calls, GB/s of weight bytes (1 + 4 / G per weight) for the new call, the spread s = (max - min) / median of the
wg_gemv_q8 repetitions (the baseline), and the two ratios. Rows where the new call is not the fastest of the three are listed again at the end.

The yardsticks are the other calls in the same run and the weight bytes. Nothing here is asserted by a test.

    python tools/gemm_q8_vs.py [--reps 7] [--min-seconds 0.1] > profiles/gemm_q8.txt
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

SHAPES = [(65536, 4096), (11008, 4096), (4096, 4096)]  # k x outputs
COLS = [1, 8, 16, 32, 64, 128]
GROUPS = [32, 128, 0]  # 0: per column (group_rows = k)


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
    print(f"# q8 Gemm (int8 weights, f32 group scales, f16 columns, MFMA) vs wg_gemv_q8 on the same weights with f32 right-hand sides vs wg_gemm_out32 GemmTr on the "
          f"weights dequantised to f16, {info['name']}, {info['compute_units']} CUs; command buffers of {LAUNCHES} launches replayed, {args.reps} repetitions alternating the "
          f"three calls, >= {args.min_seconds} s of replays each; us per launch (median), GB/s of weight bytes (weights + scales); s = (max - min) / median of the "
          f"wg_gemv_q8 repetitions", flush=True)
    TR_V, TR_M = int(wg.GemvVariant.GemvTr), int(wg.GemmVariant.GemmTr)
    losing = []
    for K, O in SHAPES:
        if args.only and args.only not in f"{K}x{O}":
            continue
        rng = np.random.default_rng(K * 7 + O)
        q = rng.integers(-127, 128, K * O).astype(np.int8)
        mq = upload(gpu, q)
        msh = wg.ViewShape((K, O, 1), K, K * O, 0).to_c()
        for G in GROUPS:
            g = G or K
            ng = -(-K // g)
            s = np.ldexp(np.float32(1), rng.integers(-2, 3, ng * O)).astype(np.float32)
            w16 = (np.repeat(s.reshape(O, ng), g, axis=1)[:, :K].reshape(-1) * q.astype(np.float32)).astype(np.float16)  # column-major: output o, rows 0 .. K
            bs, m16 = upload(gpu, s), upload(gpu, w16)
            del w16
            ssh = wg.ViewShape((ng, O, 1), ng, ng * O, 0).to_c()
            for N in COLS:
                if args.cols and int(args.cols) != N:
                    continue
                x16 = (np.random.default_rng(K + O * 3 + N).random(K * N, dtype=np.float32) * 2 - 1).astype(np.float16)
                bx16, bx32 = upload(gpu, x16), upload(gpu, x16.astype(np.float32))
                outs = [empty(gpu, O * N, np.float32) for _ in range(3)]
                xsh, osh = wg.ViewShape((K, N, 1), K, K * N, 0).to_c(), wg.ViewShape((O, N, 1), O, O * N, 0).to_c()
                calls = {
                    "gemm_q8": lambda: L.check(L.lib.wg_gemm_q8(h, TR_M, g, L.WG_F16, outs[0]._h, osh, mq._h, msh, bs._h, ssh, bx16._h, xsh)),
                    "gemv_q8": lambda: L.check(L.lib.wg_gemv_q8(h, TR_V, g, outs[1]._h, osh, mq._h, msh, bs._h, ssh, bx32._h, xsh)),
                    "out32": lambda: L.check(L.lib.wg_gemm_out32(h, TR_M, L.WG_F16, 1.0, 0.0, outs[2]._h, osh, m16._h, msh, bx16._h, xsh)),
                }
                gpu.take_path()
                calls["gemm_q8"]()
                path = gpu.take_path()
                cbs = {name: record(gpu, fn) for name, fn in calls.items()}
                for cb in cbs.values():
                    for _ in range(5):
                        gpu.queue().submit([cb])
                gpu.sync()
                # the three calls agree (the same numbers: a wrong kernel is not worth timing)
                res = [o.read(gpu.device()).astype(np.float64) for o in outs]
                scale = np.abs(res[1]).max() + 1e-30
                assert np.abs(res[0] - res[1]).max() <= 1e-3 * scale and np.abs(res[2] - res[1]).max() <= 1e-3 * scale, (K, O, g, N)
                times = {name: [] for name in cbs}
                for _ in range(args.reps):
                    for name, cb in cbs.items():
                        times[name].append(measure(gpu, cb, args.min_seconds))
                med = {name: statistics.median(t) for name, t in times.items()}
                spread = (max(times["gemv_q8"]) - min(times["gemv_q8"])) / med["gemv_q8"]
                wbytes = K * O + 4 * ng * O
                line = (f"{K:5d} x {O:4d} N {N:3d} G {G or 'col':>3} [{path}] gemm_q8 {med['gemm_q8'] * 1e6:8.2f} us {wbytes / med['gemm_q8'] * 1e-9:7.1f} GB/s | gemv_q8 "
                        f"{med['gemv_q8'] * 1e6:8.2f} us | out32(f16) {med['out32'] * 1e6:8.2f} us | s {spread:.4f} gemm_q8/gemv_q8 {med['gemm_q8'] / med['gemv_q8']:.3f} "
                        f"gemm_q8/out32 {med['gemm_q8'] / med['out32']:.3f}")
                print(line, flush=True)
                if med["gemm_q8"] > min(med["gemv_q8"], med["out32"]):
                    losing.append(line)
                del cbs, outs, bx16, bx32
            del bs, m16
        del mq
    print(f"# rows where wg_gemm_q8 is not the fastest of the three: {len(losing)}")
    for line in losing:
        print("#   " + line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
