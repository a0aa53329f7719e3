"""Shared helpers for the parity tests: tolerances (stated once, here) and fixture loading."""
import functools
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


# ---- the exponent range: subnormal operands and results, the second rounding (tests/test_gpu_exponent_range.py) ---------------------------------
# per element type: significant bits, the exponent of the smallest normal, log2 of the subnormal quantum (= EMIN - (PREC - 1))
PREC = {"f32": 24, "f16": 11, "bf16": 8}
EMIN = {"f32": -126, "f16": -14, "bf16": -126}
EMAX = {"f32": 127, "f16": 15, "bf16": 127}
QUANTUM = {k: EMIN[k] - (PREC[k] - 1) for k in PREC}  # f32: -149, f16: -24, bf16: -133
BITS_T = {"f32": np.uint32, "f16": np.uint16, "bf16": np.uint16}


def rne_grid(kind, x) -> np.ndarray:
    """The integer model of ONE round-to-nearest-even of float64 values to `kind`, as float64: x is scaled onto its binade's grid (2^(e - PREC + 1), and
    2^QUANTUM below the smallest normal) by a power of two (exact), rounded to an integer by np.rint (ties to even), and scaled back; past the largest
    finite value: Inf. No conversion of NumPy's takes part."""
    x = np.asarray(x, np.float64)
    _, e = np.frexp(x)  # |x| = m 2^e with 0.5 <= m < 1
    q = np.maximum(e - PREC[kind], QUANTUM[kind])
    with np.errstate(over="ignore", invalid="ignore"):
        r = np.ldexp(np.rint(np.ldexp(x, -q)), q)
    r = np.where(np.abs(r) >= 2.0 ** (EMAX[kind] + 1), np.copysign(np.inf, x), r)
    return np.where(np.isfinite(x), r, x)


def narrow_bits(kind, x) -> np.ndarray:
    """Values -> the bit patterns of `kind` after one RNE: astype for f32 and f16, tests/_bf16.py for bf16 (which passes through float32: x must be a
    float32 value already, or lie on the f32 grid, for that to be ONE rounding -- rne_grid(kind, x) is)."""
    import _bf16
    with np.errstate(over="ignore"):
        if kind == "bf16":
            return _bf16.to_bits(x)
        return np.ascontiguousarray(np.asarray(x).astype(np.float32 if kind == "f32" else np.float16)).view(BITS_T[kind])


def widen_bits(kind, bits) -> np.ndarray:
    """Bit patterns of `kind` -> float64, exactly."""
    import _bf16
    bits = np.ascontiguousarray(bits, BITS_T[kind])
    return (_bf16.from_bits(bits) if kind == "bf16" else bits.view(np.float32 if kind == "f32" else np.float16)).astype(np.float64)


def int_product(IA, IB) -> np.ndarray:
    """IA (M x K x mats) times IB (K x N x mats) per matrix for integer operands, in float64, exact; asserts that every partial sum in any order stays
    below 2^24 (sum_k |a||b| < 2^24): the f32 accumulation of IA 2^ea times IB 2^eb is then exact in any order and any split of K wherever
    2^(ea + eb) times an integer below 2^24 is an f32 value (ea + eb >= -149)."""
    IA, IB = np.asarray(IA, np.float64), np.asarray(IB, np.float64)
    assert np.array_equal(IA, np.rint(IA)) and np.array_equal(IB, np.rint(IB))
    sabs = float((np.abs(IA) * np.abs(IB).max(axis=1)[None, :, :]).sum(axis=1).max())  # (a bound of sum_k |a||b| over every output)
    assert sabs < 2.0 ** 24, "the operands must multiply exactly in f32"
    # (integers below 2^24: the float32 product is exact too, whatever the library's order, and twice as fast)
    return np.stack([(IA[:, :, z].astype(np.float32) @ IB[:, :, z].astype(np.float32)).astype(np.float64) for z in range(IA.shape[2])], -1)


def scaled_product(IA, IB, ea, eb, kind, P=None):
    """(exact value, bits): op(A) B for A = IA 2^ea and B = IB 2^eb (integer IA, IB: int_product's condition), rounded ONCE to `kind`. The exact value
    P 2^(ea + eb) is a float64 and an f32 value (|P| < 2^24, ea + eb >= -149), so the conversion below is the contract's single rounding. An exact zero
    is +0 (tests compare the sign of an exact zero sum as one class: special_product's note)."""
    assert ea + eb >= QUANTUM["f32"], (ea, eb)
    P = int_product(IA, IB) if P is None else P
    x = np.ldexp(P, ea + eb)  # (P = +0 where it is zero: a matrix product of float64 starts from +0)
    return x, narrow_bits(kind, x)


def fma_round_odd(b, c, v) -> np.ndarray:
    """b * c + v in float64 with round-to-odd, for f32 values b and c (their product is exact in float64) and a float64 v: TwoSum makes the sum exact, a
    nonzero error term nudges an even sum one ulp toward it. A later rounding to 51 bits or fewer is then the single correct one (fmaf_f32's device)."""
    p, q = np.asarray(b, np.float32).astype(np.float64) * np.asarray(c, np.float32).astype(np.float64), np.asarray(v, np.float64)
    s = p + q
    bv = s - p
    err = (p - (s - bv)) + (q - bv)
    fix = np.isfinite(s) & (err != 0) & ((s.view(np.int64) & 1) == 0)
    return np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)


def epilogue_model(kind, alpha, acc, beta=0.0, c=None):
    """The contract's epilogue on an exact f32 accumulator: w = fmaf_f32(beta, c, fl32(alpha * acc)) (fl32(alpha * acc) when beta == 0), THEN one rounding
    to `kind`. Returns (bits, zero, fused_bits): `zero` marks the outputs whose f32 value w is an exact zero (its sign is open); `fused_bits` is the
    neighbouring behaviour the tests must tell apart -- the exact alpha * acc + beta * c rounded straight to `kind` (what a fused v_fma_mix* gives):
    alpha * acc and beta * c are exact in float64 (24 + 24 bits), their sum is formed with round-to-odd (fmaf_f32's device), which makes the final
    rounding by rne_grid the single correct one (53 >= PREC + 2)."""
    acc = np.asarray(acc, np.float64)
    a32 = acc.astype(np.float32)
    assert np.array_equal(a32.astype(np.float64), acc), "the accumulator must be an f32 value"
    with np.errstate(over="ignore", under="ignore"):
        v = (np.float32(alpha) * a32).astype(np.float32)
    p = np.float64(np.float32(alpha)) * acc
    if beta == 0.0:
        w, s = v, p
    else:
        c32 = np.asarray(c, np.float64).astype(np.float32)
        assert np.array_equal(c32.astype(np.float64), np.asarray(c, np.float64))
        w = fmaf_f32(np.float32(beta), c32, v)
        s = fma_round_odd(beta, c32, p)
    return narrow_bits(kind, w), w == 0, narrow_bits(kind, rne_grid(kind, s))


def epilogue_bits(kind, alpha, P, s, beta=0.0, IC=None, ce=0, IC8=None):
    """(bits, zero) of epilogue_model for acc = P 2^s and c = IC 2^ce (integers; IC in [-8, 8]): through a table over the distinct pairs (P, c) where the
    range of P is small against the number of outputs; the same bits either way."""
    P = np.asarray(P, np.float64)
    lo, hi = int(P.min()), int(P.max())
    if (hi - lo + 1) * 17 > max(P.size // 4, 1 << 16):
        return epilogue_model(kind, alpha, np.ldexp(P, s), beta, None if beta == 0.0 else np.ldexp(IC, ce))[:2]
    pv, cv = np.repeat(np.arange(lo, hi + 1, dtype=np.float64), 17), np.tile(np.arange(-8.0, 9.0), hi - lo + 1)
    bits, zero, _ = epilogue_model(kind, alpha, np.ldexp(pv, s), beta, np.ldexp(cv, ce))
    key = (P.astype(np.int32) - np.int32(lo)) * np.int32(17)
    key += ((np.asarray(IC) + 8).astype(np.int32) if IC8 is None else IC8) if beta != 0.0 else np.int32(8)  # (IC8: IC + 8 as int32, where the caller keeps it)
    return bits[key], zero[key]


def range_shares(kind, x, n=None):
    """Of the exact values x (each counted n times): the shares whose rounding to `kind` is a nonzero subnormal, whose rounding is normal, and that lie
    exactly halfway between two values of the subnormal grid (below the smallest normal)."""
    x = np.asarray(x, np.float64)
    n = np.ones(x.shape) if n is None else np.asarray(n, np.float64)
    r = np.abs(rne_grid(kind, x))
    lo = 2.0 ** EMIN[kind]
    k = np.ldexp(np.abs(x), -QUANTUM[kind])
    tie = (np.abs(x) < lo) & (k - np.floor(k) == 0.5)
    return tuple(float(n[m].sum() / n.sum()) for m in ((r > 0) & (r < lo), r >= lo, tie))


def plan_straddle(kind, P0, anchored):
    """(j, t, s, shares) for the `sub_out` case: results (P0 + anchored 2^t) 2^s with s = QUANTUM - 1 - j (16 bits; f32: s = QUANTUM, the finest scale at
    which the f32 accumulation is exact, so no f32 output is a tie) straddle the smallest normal 2^EMIN = 2^t 2^s; `anchored` is +-1 on the rows that
    carry the anchor and 0 elsewhere. The first j of 0 .. 4 whose model has at least 1/4 nonzero subnormal outputs, 1/10 normal ones and (16 bits) 1/20
    ties on the subnormal grid: asserted here, on the model (on the distinct values of P0 per kind of row, with their counts)."""
    groups = [(g,) + count_pairs(P0[anchored[:, 0, 0] == g])[::2] for g in (-1.0, 0.0, 1.0) if (anchored == g).any()]
    for j in range(5 if kind != "f32" else 1):
        s = QUANTUM[kind] - (1 + j if kind != "f32" else 0)
        t = EMIN[kind] - s
        x, n = np.concatenate([np.ldexp(v + g * 2.0 ** t, s) for g, v, _ in groups]), np.concatenate([c for _, _, c in groups])
        sub, nrm, tie = range_shares(kind, x, n)
        if sub >= 0.25 and nrm >= 0.10 and (tie >= 0.05 or kind == "f32"):
            return j, t, s, (sub, nrm, tie)
    raise AssertionError(f"{kind}: no scale straddles the smallest normal; the last shares were {sub:.3f} subnormal, {nrm:.3f} normal, {tie:.3f} ties")


def witness_candidates(n=4096):
    """The fixed candidate list of generic f32 scalars for the second-rounding tests: magnitudes in [0.25, 1.75), every second one negative."""
    c = (0.25 + 1.5 * np.random.default_rng(20240229).random(n)).astype(np.float32)
    c[1::2] *= np.float32(-1)
    return c


def count_pairs(acc_int, c_int=None):
    """The distinct values of an integer array (or distinct pairs with a second one in [-8, 8]) and how often each occurs: (acc values, c values, counts)."""
    a = np.asarray(acc_int).astype(np.int64).ravel()
    lo = int(a.min())
    key = (a - lo) * 17 + (0 if c_int is None else np.asarray(c_int).astype(np.int64).ravel() + 8)
    n = np.bincount(key)
    k = np.flatnonzero(n)
    return (k // 17 + lo).astype(np.float64), (k % 17 - 8).astype(np.float64), n[k]


def plan_witnesses(kind, acc_int, s, need, alpha=None, c_int=None, c_exp=0, cands=None):
    """The first candidate scalar (alpha when `alpha` is None, else beta beside that alpha) for which at least `need` outputs are WITNESSES: the
    contract's value narrow(fmaf_f32(beta, c, fl32(alpha acc))) differs from the single rounding of the exact alpha acc + beta c (epilogue_model).
    acc = acc_int 2^s, c = c_int 2^c_exp. Returns (scalar, witnesses); asserts that the list holds one."""
    cands = witness_candidates() if cands is None else cands
    av, cv, n = count_pairs(acc_int, c_int if alpha is not None else None)
    acc, c = np.ldexp(av, s), np.ldexp(cv, c_exp)
    for x in cands:
        bits, _, fused = epilogue_model(kind, x, acc) if alpha is None else epilogue_model(kind, alpha, acc, x, c)
        w = int(n[bits != fused].sum())
        if w >= need:
            return float(x), w
    raise AssertionError(f"{kind}: no candidate of {len(cands)} gives {need} witnesses")


AXPY_ALPHA = 0.7853981852531433  # fl32(pi / 4): a generic f32 value


def axpy_witness_pairs(kind, alpha=AXPY_ALPHA, count=16):
    """(a, b): the first `count` pairs, of a fixed grid of 1024 x 1024 values of `kind` (consecutive bit patterns from 0.25 and from 1 on), on which
    narrow(fmaf_f32(alpha, b, a)) differs from the single rounding of the exact alpha b + a."""
    a = widen_bits(kind, (int(narrow_bits(kind, np.float32([0.25]))[0]) + np.arange(1024)).astype(BITS_T[kind]))[:, None]
    b = widen_bits(kind, (int(narrow_bits(kind, np.float32([1.0]))[0]) + np.arange(1024)).astype(BITS_T[kind]))[None, :]
    a, b = (x.ravel() for x in np.broadcast_arrays(a, b))
    two = narrow_bits(kind, fmaf_f32(np.float32(alpha), b.astype(np.float32), a.astype(np.float32)))
    one = narrow_bits(kind, rne_grid(kind, fma_round_odd(np.float32(alpha), b, a)))
    w = np.flatnonzero(two != one)[:count] if kind != "f32" else np.arange(count)  # (an f32 Axpy is the one fmaf: the first pairs of the grid)
    assert w.size == count, f"{kind}: only {w.size} witness pairs on the grid"
    return a[w], b[w]


@functools.lru_cache(None)
def prod_witness(kind):
    """(four factors, v): values of `kind` in [1, 2) whose product in two exact pairs, v = fl32((f0 f2) (f1 f3)), is narrowed by the contract to another value
    than the exact product rounded straight to `kind` -- the first such of a fixed grid. A pair's product is exact in f32 (2 PREC <= 24 bits), so v is the
    one f32 rounding of the exact product however the four are paired; the last multiplication is the inexact one, which a fused multiply-narrow gets wrong."""
    one = int(narrow_bits(kind, np.float32([1.0]))[0])
    m = widen_bits(kind, (one + np.arange(1, 1 << (PREC[kind] - 1), 2)).astype(BITS_T[kind]))  # the odd significands
    if kind == "f16":
        f0, f1 = m[len(m) // 3], m[len(m) // 5]
        f2, f3 = (x.ravel() for x in np.meshgrid(m, m, indexing="ij"))
    else:  # (64 odd significands: all four factors vary, a witness being one product in 2^16 or so)
        f0, f1, f2, f3 = (x.ravel() for x in np.meshgrid(m[::4], m, m, m, indexing="ij"))
    v = ((f0 * f2).astype(np.float32) * (f1 * f3).astype(np.float32)).astype(np.float64)
    w = np.flatnonzero(narrow_bits(kind, v.astype(np.float32)) != narrow_bits(kind, rne_grid(kind, (f0 * f2) * (f1 * f3))))
    assert w.size, f"{kind}: no witness on the grid"
    return np.array([np.broadcast_to(f, v.shape)[w[0]] for f in (f0, f1, f2, f3)]), float(v[w[0]])


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
