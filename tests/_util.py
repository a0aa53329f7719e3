"""Shared helpers for the parity tests: tolerances (stated once, here) and fixture loading."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# ---- tolerances ---------------------------------------------------------------------------------------------
# OpAssign (+ - * / copy)                      : 0 ulp vs the oracle (correctly rounded everywhere).
# Reduce Min/Max/Sum/Prod/SqNorm               : 0 ulp vs the oracle: the HIP kernel keeps the reference's order
#                                                (reduce.wgsl:68-87) and rounds x*x separately like the oracle does.
# Gemm / Gemv f32 (summation order differs from the WGSL orders: MFMA-blocked / per-lane + butterfly):
#     |gpu - f64 truth|  <= GATE_C * sqrt(K) * 2^-24 * sum_k |a||b|           (GATE_C = 2; hard bound is K * 2^-24 * ...)
#     |gpu - oracle|     <= 2 * that                                           (both sit within the gate of the truth)
#   and, at the reference's own test shapes, the reference's literal bar: abs <= 1e-3 (gemm.rs:199, gemv.rs:194).
# f16 Gemm (extension, no reference kernel)    : f16 inputs, f32 accumulate, one RNE rounding to f16:
#     |gpu - f64 truth|  <= f32 gate + 2^-11 * |truth|   (half an f16 ulp of the result; 2^-24 floor for subnormals)
GATE_C = 2.0
REF_ABS_EPS = 1.0e-3


def f32_gate(k: int, sabs) -> np.ndarray:
    return GATE_C * np.sqrt(max(int(k), 1)) * 2.0 ** -24 * np.asarray(sabs, np.float64) + 1e-37


def assert_close_f64(got, truth, k, sabs, what=""):
    got = np.asarray(got, np.float64).ravel()
    truth = np.asarray(truth, np.float64).ravel()
    tol = f32_gate(k, np.asarray(sabs).ravel())
    err = np.abs(got - truth)
    bad = err > tol
    assert not bad.any(), (f"{what}: {bad.sum()} of {bad.size} elements exceed {GATE_C}*sqrt({k})*2^-24*sum|a||b|; "
                           f"worst err/tol = {(err / tol).max():.3g}, max abs err = {err.max():.3g}")
    return float((err / tol).max())


def assert_close_oracle(got, oracle, k, sabs, what=""):
    got = np.asarray(got, np.float64).ravel()
    oracle = np.asarray(oracle, np.float64).ravel()
    tol = 2.0 * f32_gate(k, np.asarray(sabs).ravel())
    err = np.abs(got - oracle)
    bad = err > tol
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} elements differ from the oracle by more than 2x the gate; worst {(err / tol).max():.3g}"


def max_ulp(a, b) -> int:
    a = np.asarray(a, np.float32).ravel()
    b = np.asarray(b, np.float32).ravel()
    ia = a.view(np.int32).astype(np.int64)
    ib = b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return int(np.abs(ia - ib).max()) if a.size else 0


def assert_bits_equal(got, expected, what=""):
    got = np.ascontiguousarray(got)
    expected = np.ascontiguousarray(expected)
    assert got.dtype == expected.dtype and got.shape == expected.shape, (what, got.dtype, expected.dtype, got.shape, expected.shape)
    if got.tobytes() != expected.tobytes():
        g32, e32 = got.view(np.uint32 if got.dtype.itemsize == 4 else np.uint16), expected.view(np.uint32 if got.dtype.itemsize == 4 else np.uint16)
        idx = np.flatnonzero(g32.ravel() != e32.ravel())
        raise AssertionError(f"{what}: {idx.size} of {got.size} elements differ bitwise; first at {idx[0]}: "
                             f"got {got.ravel()[idx[0]]!r}, expected {expected.ravel()[idx[0]]!r}")


def golden(name: str):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def relative_eq(a, b, epsilon, max_relative=np.finfo(np.float32).eps):
    """approx::assert_relative_eq! semantics: |a-b| <= epsilon or |a-b| <= max_relative * max(|a|,|b|)."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    d = np.abs(a - b)
    return bool(np.all((d <= epsilon) | (d <= max_relative * np.maximum(np.abs(a), np.abs(b)))))


def fmaf_f32(b, c, v) -> np.ndarray:
    """fmaf(b, c, v) on float32 arrays, correctly rounded once (what the kernels' f32 epilogue fmaf(beta, c, fl32(alpha * acc)) computes): b * c is
    exact in f64 (24 + 24 bits), the sum with v is made exact by TwoSum, a nonzero error term nudges an even sum one f64 ulp toward it ("round to
    odd": 53 >= 2 * 24 + 2 bits, so the final rounding to f32 is then the single correct one)."""
    b, c, v = np.broadcast_arrays(np.asarray(b, np.float32), np.asarray(c, np.float32), np.asarray(v, np.float32))
    p, q = b.astype(np.float64) * c.astype(np.float64), v.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + q
        bv = s - p
        err = (p - (s - bv)) + (q - bv)
        fix = np.isfinite(s) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def special_product(A, B, dtype):
    """op(A) B per matrix, rounded once to `dtype`, for operands whose finite part multiplies exactly (integers with every partial sum below 2^24 in
    magnitude: any summation order and any split of K give the same f32 sum). A is M x K x mats, B is K x N x mats, in float64; they may hold +-Inf and
    NaN. The result is the exact product over the k whose column of A and row of B are finite, plus in f64 the outer product A[:, k] x B[k, :] of every
    other k (Inf * 0 = NaN, Inf + -Inf = NaN: IEEE, and order-free once the finite part is exact), then one rounding. A negative zero becomes +0: the
    sign of an exact zero sum depends on where an accumulator starts, which the contract leaves open (tests compare zeros as one class)."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    fin = np.isfinite(A).all(axis=0) & np.isfinite(B).all(axis=1)  # K x mats
    out = np.zeros((A.shape[0], B.shape[1], A.shape[2]), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for z in range(A.shape[2]):
            ks = np.flatnonzero(fin[:, z])
            out[:, :, z] = A[:, ks, z] @ B[ks, :, z]
            for k in np.flatnonzero(~fin[:, z]):
                out[:, :, z] += np.outer(A[:, k, z], B[k, :, z])
        return (out + 0.0).astype(dtype)


def assert_same_class_bits(got, want, what=""):
    """Bit equality with NaN compared as a class (any payload) and zeros as one class; Inf with its sign."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    ut = np.uint32 if got.dtype.itemsize == 4 else np.uint16
    g = np.where(got == 0, 0, got).astype(got.dtype).view(ut)
    w = np.where(want == 0, 0, want).astype(want.dtype).view(ut)
    bad = (gn != wn) | (~gn & ~wn & (g != w))
    if bad.any():
        i = np.flatnonzero(bad.ravel())
        raise AssertionError(f"{what}: {i.size} of {got.size} elements differ; first at {np.unravel_index(i[0], got.shape)}: got {got.ravel()[i[0]]!r}, "
                             f"expected {want.ravel()[i[0]]!r}")
