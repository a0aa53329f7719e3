"""The q4 Gemm (packed 4-bit weights with f32 group scales against N columns of f16 / bf16 activations on the matrix cores: wg_gemm_q4) against the three calls a
caller had before it, in the same run and on the same values: wg_gemm_q8 on the unpacked int8 (twice the weight bytes), wg_gemv_q4 on the same packed bytes with the
columns as f32 right-hand sides (a vector-ALU kernel: groups of 8 on grid.z, the matrix streamed once per group) and wg_gemm_out32 WG_GEMM_TR on the weights
dequantised to the 16-bit type (four times the weight bytes).

One process. Per shape (k x outputs), element type, group_rows (32, 128, per column) and number of columns (1, 8, 16, 32, 64, 128): seeded nibbles over all 16 values
and power-of-two group scales in [2^-2, 2^2], so that the dequantised matrix is exact in f16 and in bf16 and all four calls multiply the same numbers; x is seeded
U[-1, 1) rounded to the 16-bit type. Each call is run eagerly (scratch grows, code objects load), then RECORDED -- LAUNCHES launches in one command buffer -- and the
command buffer is replayed: 5 warm-up submits, then REPS (>= 7) repetitions ALTERNATING the four calls, each at least MIN_SECONDS of submits between two device
events. Per row: the tags the new call logged, median [min .. max] time per launch of the new call, GB/s of its weight bytes (1/2 + 4 / G per weight), the medians of
the three others, the spread s = (max - min) / median of the wg_gemm_q8 repetitions (the baseline), and the three ratios. The rows that miss an expectation -- no
slower than wg_gemm_q8 in any row, faster than wg_gemv_q4 from 8 columns on -- are listed again at the end.

The yardsticks are the other calls in the same run and the weight bytes. Nothing here is asserted by a test.

    python tools/gemm_q4_vs.py [--reps 7] [--min-seconds 0.05] [--only KxO] [--dtype f16] > profiles/gemm_q4.txt
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
GROUPS = [32, 128, 0]  # 0: per column (group_rows = k)
DTYPES = ["f16", "bf16"]


def to16(dt, a32):
    return a32.astype(np.float16) if dt == "f16" else wg.to_bfloat16(a32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--min-seconds", type=float, default=0.05)
    ap.add_argument("--only", default="", help="run only the shapes whose 'KxO' contains this text")
    ap.add_argument("--dtype", default="", help="run only this element type of x (f16 or bf16)")
    ap.add_argument("--cols", default="", help="run only this number of columns")
    args = ap.parse_args()
    assert args.reps >= 7, "the protocol: >= 7 alternating repetitions"
    gpu = wg.GpuInstance.new()
    h = gpu._ctx.handle
    info = gpu.adapter()
    print(f"# q4 Gemm (packed 4-bit weights, f32 group scales, 16-bit columns, MFMA) vs wg_gemm_q8 on the unpacked int8 vs wg_gemv_q4 on the same bytes with f32 "
          f"right-hand sides vs wg_gemm_out32 GemmTr on the weights dequantised to the 16-bit type, {info['name']}, {info['compute_units']} CUs; command buffers of "
          f"{LAUNCHES} launches replayed, {args.reps} repetitions alternating the four calls, >= {args.min_seconds} s of replays each; us per launch: median "
          f"[min .. max] for the new call, medians for the others; GB/s of weight bytes (packed weights + scales); s = (max - min) / median of the wg_gemm_q8 "
          f"repetitions", flush=True)
    TR_V, TR_M = int(wg.GemvVariant.GemvTr), int(wg.GemmVariant.GemmTr)
    slower_than_q8, slower_than_gemv = [], []
    for K, O in SHAPES:
        if args.only and args.only not in f"{K}x{O}":
            continue
        rng = np.random.default_rng(K * 7 + O)
        q = rng.integers(-8, 8, K * O).astype(np.int8)  # column-major: output o, rows 0 .. K
        n = (q + 8).astype(np.uint8)
        m4, m8 = upload(gpu, (n[0::2] | (n[1::2] << 4)).astype(np.uint8)), upload(gpu, q)  # (k is even: a byte's two rows lie in one column)
        del n
        m4sh, m8sh = wg.ViewShape((K // 2, O, 1), K // 2, K // 2 * O, 0).to_c(), wg.ViewShape((K, O, 1), K, K * O, 0).to_c()
        for G in GROUPS:
            g = G or K
            ng = -(-K // g)
            s = np.ldexp(np.float32(1), rng.integers(-2, 3, ng * O)).astype(np.float32)
            w32 = np.repeat(s.reshape(O, ng), g, axis=1)[:, :K].reshape(-1) * q.astype(np.float32)
            bs = upload(gpu, s)
            ssh = wg.ViewShape((ng, O, 1), ng, ng * O, 0).to_c()
            for dt in DTYPES:
                if args.dtype and args.dtype != dt:
                    continue
                xd = L.WG_F16 if dt == "f16" else L.WG_BF16
                m16 = upload(gpu, to16(dt, w32))
                for N in COLS:
                    if args.cols and int(args.cols) != N:
                        continue
                    x32 = np.random.default_rng(K + O * 3 + N).random(K * N, dtype=np.float32) * 2 - 1
                    x16 = to16(dt, x32)
                    bx16, bx32 = upload(gpu, x16), upload(gpu, x16.astype(np.float32) if dt == "f16" else wg.from_bfloat16(x16))
                    outs = [empty(gpu, O * N, np.float32) for _ in range(4)]
                    xsh, osh = wg.ViewShape((K, N, 1), K, K * N, 0).to_c(), wg.ViewShape((O, N, 1), O, O * N, 0).to_c()
                    calls = {
                        "gemm_q4": lambda: L.check(L.lib.wg_gemm_q4(h, TR_M, g, xd, outs[0]._h, osh, m4._h, m4sh, bs._h, ssh, bx16._h, xsh)),
                        "gemm_q8": lambda: L.check(L.lib.wg_gemm_q8(h, TR_M, g, xd, outs[1]._h, osh, m8._h, m8sh, bs._h, ssh, bx16._h, xsh)),
                        "gemv_q4": lambda: L.check(L.lib.wg_gemv_q4(h, TR_V, g, outs[2]._h, osh, m4._h, m4sh, bs._h, ssh, bx32._h, xsh)),
                        "out32": lambda: L.check(L.lib.wg_gemm_out32(h, TR_M, xd, 1.0, 0.0, outs[3]._h, osh, m16._h, m8sh, bx16._h, xsh)),
                    }
                    gpu.take_path()
                    calls["gemm_q4"]()
                    path = gpu.take_path()
                    cbs = {name: record(gpu, fn) for name, fn in calls.items()}
                    for cb in cbs.values():
                        for _ in range(5):
                            gpu.queue().submit([cb])
                    gpu.sync()
                    # the four calls agree (the same numbers: a wrong kernel is not worth timing)
                    res = [o.read(gpu.device()).astype(np.float64) for o in outs]
                    scale = np.abs(res[1]).max() + 1e-30
                    assert all(np.abs(r - res[1]).max() <= 1e-3 * scale for r in res), (K, O, g, N, dt)
                    times = {name: [] for name in cbs}
                    for _ in range(args.reps):
                        for name, cb in cbs.items():
                            times[name].append(measure(gpu, cb, args.min_seconds))
                    med = {name: statistics.median(t) for name, t in times.items()}
                    spread = (max(times["gemm_q8"]) - min(times["gemm_q8"])) / med["gemm_q8"]
                    wbytes = K * O // 2 + 4 * ng * O
                    t4 = times["gemm_q4"]
                    line = (f"{K:5d} x {O:5d} {dt:>4} N {N:3d} G {G or 'col':>3} [{path}] gemm_q4 {med['gemm_q4'] * 1e6:8.2f} [{min(t4) * 1e6:8.2f} .. {max(t4) * 1e6:8.2f}] us "
                            f"{wbytes / med['gemm_q4'] * 1e-9:7.1f} GB/s | gemm_q8 {med['gemm_q8'] * 1e6:8.2f} us | gemv_q4 {med['gemv_q4'] * 1e6:8.2f} us | out32 "
                            f"{med['out32'] * 1e6:8.2f} us | s {spread:.4f} q4/gemm_q8 {med['gemm_q4'] / med['gemm_q8']:.3f} q4/gemv_q4 {med['gemm_q4'] / med['gemv_q4']:.3f} "
                            f"q4/out32 {med['gemm_q4'] / med['out32']:.3f}")
                    print(line, flush=True)
                    if med["gemm_q4"] > med["gemm_q8"]:
                        slower_than_q8.append(line)
                    if N >= 8 and med["gemm_q4"] >= med["gemv_q4"]:
                        slower_than_gemv.append(line)
                    del cbs, outs, bx16, bx32
                del m16
            del bs, w32
        del m4, m8
    print(f"# rows where wg_gemm_q4 is slower than wg_gemm_q8 on the same values: {len(slower_than_q8)}")
    for line in slower_than_q8:
        print("#   " + line)
    print(f"# rows with 8 or more columns where wg_gemm_q4 is not faster than wg_gemv_q4: {len(slower_than_gemv)}")
    for line in slower_than_gemv:
        print("#   " + line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
