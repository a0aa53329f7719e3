"""The expected-value model of tests/test_gpu_operands.py (U.special_product), checked on the CPU: on integer operands with +-Inf and NaN inside, the
split into a finite exact product and outer products of the special k, rounded once, equals the naive f64 sum over k in index order rounded once; and
the f16 rounding edges the GPU tests rely on (RNE above 2048, 65504 the largest finite value, 65520 the first value that rounds to Inf)."""
import numpy as np
import pytest

import _util as U


def _naive(A, B, dtype):
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.einsum("mkz,knz->mnz", A, B, optimize=False) + 0.0).astype(dtype)


@pytest.mark.parametrize("seed", range(40))
@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_split_model_matches_naive_sum(seed, dtype):
    rng = np.random.default_rng(seed)
    M, K, N, Z = (int(x) for x in rng.integers(1, 9, 4))
    A = rng.integers(-8, 9, (M, K, Z)).astype(np.float64)
    B = rng.integers(-8, 9, (K, N, Z)).astype(np.float64)
    if dtype == np.float16:  # reach past 2048 and past the largest finite f16 too
        A[:, 0, :] *= 2047
    for X in (A, B):
        n = int(rng.integers(0, 4))
        idx = tuple(rng.integers(0, s, n) for s in X.shape)
        X[idx] = rng.choice([np.inf, -np.inf, np.nan], n)
    U.assert_same_class_bits(U.special_product(A, B, dtype), _naive(A, B, dtype), f"seed {seed}")


def test_inf_times_zero_and_opposite_infs():
    A = np.array([[np.inf, 1.0], [np.inf, 0.0], [2.0, 3.0]])[:, :, None]
    B = np.array([[0.0, 1.0, -1.0], [5.0, np.inf, 4.0]])[:, :, None]
    got = U.special_product(A, B, np.float32)[:, :, 0]
    # row 0: Inf*0 = NaN | Inf + Inf | -Inf + 4; row 1: NaN | Inf + 0*Inf = NaN | -Inf; row 2: 15 | Inf | 10
    want = np.array([[np.nan, np.inf, -np.inf], [np.nan, np.nan, -np.inf], [15.0, np.inf, 10.0]], np.float32)
    U.assert_same_class_bits(got, want)


def test_f16_rounding_edges():
    v = np.array([2049, 2051, 6141, 65504, 65511, 65519, 65520, 65525, -65519, -65520], np.float64)
    with np.errstate(over="ignore"):
        h = v.astype(np.float16)
        h32 = v.astype(np.float32).astype(np.float16)  # the kernels round the exact f32 sum: the same single rounding
    assert h.tobytes() == h32.tobytes()
    assert list(h[:3]) == [2048, 2052, 6140]  # ties to even, then the nearest multiple of 4
    assert list(h[3:6]) == [65504] * 3 and np.isposinf(h[6]) and np.isposinf(h[7]) and h[8] == -65504 and np.isneginf(h[9])


def test_class_compare_catches_one_ulp_and_sign():
    a = np.array([1.0, np.inf, np.nan, 0.0], np.float16)
    U.assert_same_class_bits(a, np.array([1.0, np.inf, np.nan, -0.0], np.float16))
    for bad in ([np.nextafter(np.float16(1), np.float16(2)), np.inf, np.nan, 0.0], [1.0, -np.inf, np.nan, 0.0], [1.0, np.inf, 0.0, 0.0]):
        with pytest.raises(AssertionError):
            U.assert_same_class_bits(a, np.array(bad, np.float16))
