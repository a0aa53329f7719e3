"""Records tests/golden/f16_bits_before_bf16.npz: the bits of four f16 Gemm leaves on seeded operands, taken on the commit BEFORE the element type of the
16-bit Gemm sources became a compile-time switch. tests/test_gpu_bf16.py recomputes them and compares: the refactor must not change one bit of f16.

Per case and variant: sha256 of the whole output, 4096 sampled elements (their flat indices are seeded), and the launch log, so that a heuristic change that
moves a case to another leaf shows as such and not as a bit difference.

Run on the GPU from the repository root, on the commit to record:  python tools/record_f16_bits.py [output.npz]
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "f16_bits_before_bf16.npz")

# name, (M, K, N, mats), knobs, the tags the log must hold
CASES = [
    ("cont", (4096, 256, 8192, 1), {"f16_tile": 256, "f16_cont": 1}, "f16.cont"),
    ("m16_tail", (4352, 1024, 4096, 1), {"f16_tile": 256, "f16_cont": 0}, "f16.m16/ns=1 f16.m16tail/ns=4 f16.tail_reduce"),
    ("t128_splitk", (512, 4096, 512, 1), {"f16_tile": 128}, "f16.t128/ns=4 splitk.reduce/ns=4"),
    ("generic", (72, 36, 40, 3), {}, "f16.generic"),
]
NSAMPLE = 4096
S_STORAGE = 128 | 4 | 8


def compute(gpu, name, tr):
    """-> (uint16 bits of the output, flat; launch log) of case `name` as Gemm (tr False) or GemmTr."""
    import wgmath_amd as wg
    from wgmath_amd import _lib as L

    _, (M, K, N, mats), knobs, _ = next(c for c in CASES if c[0] == name)
    saved = {k: gpu.set_tuning(k, v) for k, v in knobs.items()}
    try:
        rng = np.random.default_rng(M * 7 + K * 5 + N * 3 + mats + int(tr))
        a = (rng.random(mats * M * K, dtype=np.float32) * 2 - 1).astype(np.float16)
        b = (rng.random(mats * K * N, dtype=np.float32) * 2 - 1).astype(np.float16)
        up = lambda flat: wg.TensorBuilder.tensor((flat.size,), S_STORAGE).build_init(gpu.device(), flat, flat.dtype.type)
        ta, tb, tc = up(a), up(b), up(np.full(mats * M * N, np.nan, np.float16))
        ash = wg.ViewShape(((K, M) if tr else (M, K)) + (mats,), K if tr else M, M * K, 0)
        bsh = wg.ViewShape((K, N, mats), K, K * N, 0)
        osh = wg.ViewShape((M, N, mats), M, M * N, 0)
        gpu.take_path()
        variant = int(wg.GemmVariant.GemmTr if tr else wg.GemmVariant.Gemm)
        L.check(L.lib.wg_gemm(gpu._ctx.handle, variant, L.WG_F16, tc._h, osh.to_c(), ta._h, ash.to_c(), tb._h, bsh.to_c()))
        bits = tc.read(gpu.device()).view(np.uint16)
        return bits, gpu.take_path()
    finally:
        for k, v in saved.items():
            gpu.set_tuning(k, v)


def sample_index(name, tr, size):
    return np.sort(np.random.default_rng(len(name) * 1000003 + size * 7 + int(tr)).choice(size, min(NSAMPLE, size), replace=False))


def digest(bits):
    return hashlib.sha256(np.ascontiguousarray(bits).tobytes()).hexdigest()


def main():
    sys.path.insert(0, ROOT)
    import wgmath_amd as wg

    gpu = wg.GpuInstance.new()
    out = {}
    for name, _, _, tags in CASES:
        for tr in (False, True):
            bits, log = compute(gpu, name, tr)
            assert all(t in log for t in tags.split()), (name, tr, log)
            key = f"{name}_{'tr' if tr else 'nn'}"
            out[key + "_sha256"] = np.array(digest(bits))
            out[key + "_sample"] = bits[sample_index(name, tr, bits.size)]
            out[key + "_log"] = np.array(log)
            print(key, digest(bits), log)
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    np.savez_compressed(path, **out)
    print("wrote", path)


if __name__ == "__main__":
    main()
