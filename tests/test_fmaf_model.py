"""tests/_util.py fmaf_f32 -- the exact model of the f32 Gemm epilogue that tests/test_gpu_epilogue.py checks kernels against bit for bit -- against
exact rational arithmetic (no GPU)."""
import math
from fractions import Fraction

import numpy as np

import _util as U


def _round_f32(x: Fraction) -> np.float32:
    """x rounded to float32, to nearest with ties to even (subnormals and overflow included)."""
    if x == 0:
        return np.float32(0.0)
    sign, a = (-1.0 if x < 0 else 1.0), abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()  # 2^e <= a < 2^(e+2)
    while Fraction(2) ** (e + 1) <= a:
        e += 1
    while Fraction(2) ** e > a:
        e -= 1
    q = max(e, -126) - 23  # the quantum of the binade (of the subnormals below 2^-126)
    n = round(a / Fraction(2) ** q)  # Fraction.__round__: half to even
    if n * Fraction(2) ** q >= Fraction(2) ** 128:
        return np.float32(sign * np.inf)
    return np.float32(sign * math.ldexp(float(n), q))


def _exact(b, c, v) -> np.ndarray:
    # (an exact zero takes its sign from IEEE's rules for x * y + z, which the f64 expression follows: it is exact then)
    return np.array([_round_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) if float(x) * float(y) + float(z) != 0 else
                     np.float32(float(x) * float(y) + float(z)) for x, y, z in zip(b, c, v)], np.float32)


def _f32(bits) -> np.ndarray:
    return np.asarray(bits, np.uint32).view(np.float32)


def test_fmaf_f32_random_triples():
    rng = np.random.default_rng(2024)
    n = 10000
    # b, c: random mantissas over +-2^20; v: around the product's magnitude (where the rounding of the sum matters), some far from it, some subnormal
    b = (rng.random(n) * 2 - 1).astype(np.float32) * np.exp2(rng.integers(-20, 21, n)).astype(np.float32)
    c = (rng.random(n) * 2 - 1).astype(np.float32) * np.exp2(rng.integers(-20, 21, n)).astype(np.float32)
    p = b.astype(np.float64) * c
    v = ((rng.random(n) * 2 - 1) * np.abs(p) * np.exp2(rng.integers(-30, 31, n))).astype(np.float32)
    v[::7] = -(b[::7].astype(np.float64) * c[::7]).astype(np.float32)  # near-total cancellation
    v[3::11] = _f32(rng.integers(1, 1 << 23, v[3::11].size, dtype=np.uint32))  # subnormal addends
    got, want = U.fmaf_f32(b, c, v), _exact(b, c, v)
    U.assert_bits_equal(got, want, "fmaf_f32 vs exact rationals")


def test_fmaf_f32_constructed():
    one, u = 1.0, 2.0 ** -23
    cases = [
        # exact f32 midpoints: ties to even, both directions
        (2.0 ** -12, 2.0 ** -12, one),                       # 1 + 2^-24 -> 1
        (2.0 ** -12, 2.0 ** -12, one + u),                   # 1 + 3 * 2^-24 -> 1 + 2^-22
        (-(2.0 ** -12), 2.0 ** -12, -one),                   # -(1 + 2^-24) -> -1
        # just below / above a midpoint by far less than an f64 ulp of the sum: rounding the f64 sum first lands ON the midpoint
        (1 + u, 2.0 ** -24 * (1 - u), one + u),              # 1 + 2^-23 + 2^-24 - 2^-70 -> 1 + 2^-23 (double rounding: 1 + 2^-22)
        (1 + u, 2.0 ** -24 * (1 + u), one),                  # 1 + 2^-24 + 2^-46 + 2^-70 -> 1 + 2^-23
        (1 - u / 2, 2.0 ** -24 * (1 - u), -one - u),
        # cancellation: the exact result is far below the operands
        (1 + u, 1 + u, -(one + 2 * u)),                      # 2^-46
        (1 + u, -(1 - u), one),                              # 2^-46
        (3.0, float(np.float32(1.0 / 3.0)), -one),
        # results straddling a binade: just below 2, rounding up into the next binade; and down across 1
        (2.0 ** -12, 2.0 ** -12 * (1 + u), 2.0 - u),         # 2 - 2^-23 + 2^-24 + 2^-47 -> 2
        (2.0 ** -13, -(2.0 ** -13), one),                    # 1 - 2^-26 -> 1
        (2.0 ** -12, -(2.0 ** -12) * (1 + u), one),          # 1 - 2^-24 - 2^-47 -> 1 - 2^-24 (below 1 the ulp halves)
        (2.0 ** -12, -(2.0 ** -12), one),                    # 1 - 2^-24: representable
        # subnormal results, overflow, signed zeros
        (2.0 ** -70, 2.0 ** -70, 2.0 ** -149),
        (2.0 ** -75, 2.0 ** -75, -(2.0 ** -149)),
        (float(np.float32(3.0e38)), 2.0, -float(np.float32(3.0e38))),
        (float(np.float32(3.0e38)), 2.0, 1.0),
        (0.0, -1.0, 0.0),
        (-0.0, 1.0, -0.0),
        (1.0, -1.0, 1.0),
    ]
    b, c, v = (np.array([t[i] for t in cases], np.float32) for i in range(3))
    # the operands above must be what they claim (exact in f32)
    for i in range(3):
        assert all(float(np.float32(t[i])) == t[i] for t in cases), i
    U.assert_bits_equal(U.fmaf_f32(b, c, v), _exact(b, c, v), "fmaf_f32 on constructed cases")
