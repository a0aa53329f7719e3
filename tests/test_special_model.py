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


# --------------------------------------------------------------------------------------------------------
# the models of tests/test_gpu_exponent_range.py: the three subnormal grids, and per row the shares and the witness counts the GPU tests rely on
# --------------------------------------------------------------------------------------------------------
import _bf16  # noqa: E402
import test_gpu_exponent_range as X  # noqa: E402  (its tables, operands and plans; nothing in it touches a GPU at import)


def test_process_does_not_flush_to_zero():
    assert np.float32(2.0 ** -140) * np.float32(0.5) != 0 and np.float32(2.0 ** -140) * np.float32(0.5) == 2.0 ** -141
    assert np.float16(2.0 ** -20) * np.float16(0.5) == 2.0 ** -21 and np.float64(np.float32(2.0 ** -149)) == 2.0 ** -149


@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
def test_subnormal_grid_rounds_to_nearest_even(kind):
    """m / 8 quanta for every m up to past the smallest normal (f32: the first 2^16, the last 2^16 and 2^18 random ones): the conversions the GPU tests use
    (astype from float64; tests/_bf16.py from the float32 the value already is) and U.rne_grid give floor(m / 8) quanta, one more above the half and, at
    the half, the even neighbour -- in integer arithmetic."""
    q, top = U.QUANTUM[kind], 8 * (2 ** (U.PREC[kind] - 1) + 4)
    m = np.arange(top + 1, dtype=np.int64)
    if kind == "f32":
        m = np.unique(np.concatenate([m[:1 << 16], m[-(1 << 16):], np.random.default_rng(0).integers(0, top, 1 << 18)]))
    k, r = m // 8, m % 8
    want = k + ((r > 4) | ((r == 4) & (k % 2 == 1)))
    assert ((r == 4) & (k % 2 == 0)).any() and ((r == 4) & (k % 2 == 1)).any()
    for sign in (1.0, -1.0):
        x = sign * np.ldexp(m.astype(np.float64), q - 3)
        w64 = sign * np.ldexp(want.astype(np.float64), q)
        assert np.array_equal(U.rne_grid(kind, x), w64)
        got = x.astype(np.float32) if kind == "f32" else x.astype(np.float16) if kind == "f16" else _bf16.from_bits(_bf16.to_bits(x.astype(np.float32)))
        if kind == "bf16":
            assert np.array_equal(x.astype(np.float32).astype(np.float64), x)  # (m 2^-136 is an f32 value: to_bits rounds once)
        assert np.array_equal(got.astype(np.float64), w64) and np.array_equal(np.signbit(got), np.signbit(w64))
        assert np.array_equal(U.widen_bits(kind, U.narrow_bits(kind, x)), w64)


def test_rne_grid_is_numpy_rounding_in_the_normal_range():
    rng = np.random.default_rng(1)
    x = np.ldexp(rng.random(1 << 16) + 0.5, rng.integers(-30, 17, 1 << 16)) * np.where(rng.random(1 << 16) < 0.5, -1, 1)
    with np.errstate(over="ignore"):
        assert np.array_equal(U.rne_grid("f16", x), x.astype(np.float16).astype(np.float64))
        assert np.array_equal(U.rne_grid("f32", x), x.astype(np.float32).astype(np.float64))
    x32 = x.astype(np.float32)
    assert np.array_equal(U.rne_grid("bf16", x32), _bf16.round_f32(x32).astype(np.float64))


def test_epilogue_model_tells_the_two_roundings_apart():
    """alpha = fl32(pi / 4) on the accumulators 1 .. 2^16 - 1, narrowed to f16: about 2^-13 of the outputs are witnesses, and each is what the name says -- the
    f32 product sits exactly on an f16 tie (which RNE resolves to the even neighbour) while the exact product lies off it, so that its single rounding is
    the other neighbour, one f16 ulp away. With beta c added the same holds of fmaf_f32's value."""
    al = np.float32(U.AXPY_ALPHA)
    acc = np.arange(1.0, 1 << 16)
    bits, _, fused = U.epilogue_model("f16", al, acc)
    w = np.flatnonzero(bits != fused)
    assert 0 < w.size < 64
    for i in w:
        v, exact = float(al * np.float32(acc[i])), float(al) * acc[i]
        ulp = 2.0 ** (np.frexp(v)[1] - 11)
        two, one = U.widen_bits("f16", bits[i:i + 1])[0], U.widen_bits("f16", fused[i:i + 1])[0]
        assert v != exact and (v / ulp) % 1.0 == 0.5 and (two / ulp) % 2.0 == 0.0 and abs(one - two) == ulp and abs(one - exact) < abs(two - exact)
    c = np.resize(np.arange(-8.0, 9.0), acc.size)
    bits, zero, fused = U.epilogue_model("bf16", al, acc, np.float32(-1.37), c)
    w = np.flatnonzero(bits != fused)
    assert w.size and not zero.any()
    for i in w:
        v = float(U.fmaf_f32(np.float32(-1.37), np.float32(c[i]), al * np.float32(acc[i])))
        ulp = 2.0 ** (np.frexp(v)[1] - 8)
        assert (v / ulp) % 1.0 == 0.5 and abs(U.widen_bits("bf16", fused[i:i + 1])[0] - U.widen_bits("bf16", bits[i:i + 1])[0]) == ulp


def test_epilogue_bits_is_the_model():
    rng = np.random.default_rng(0)
    P, IC = rng.integers(-3000, 3000, (300, 500, 1)).astype(np.float64), rng.integers(-8, 9, (300, 500, 1)).astype(np.float64)
    for kind, s, ce in (("f16", 0, 0), ("bf16", -136, -133), ("f16", -26, -24), ("f32", -149, -149)):
        for al, be in ((0.77, 0.0), (0.77, -1.3), (0.5, 0.25)):
            b1, z1 = U.epilogue_bits(kind, al, P, s, be, IC, ce)
            b2, z2, _ = U.epilogue_model(kind, al, np.ldexp(P, s), be, np.ldexp(IC, ce))
            assert np.array_equal(b1, b2) and np.array_equal(z1, z2)


def _shares_and_witnesses(d, kinds, second):
    for kind in kinds:
        IA, IB, P, s = X.sub_out_operands(d, kind)
        assert np.array_equal(P[::61], U.int_product(IA[::61], IB)), "the anchored product is P0 + the anchor"  # (every 61st row: rows of all four kinds)
        pv, _, n = U.count_pairs(P)
        sub, nrm, tie = U.range_shares(kind, np.ldexp(pv, s), n)
        assert sub >= 0.25 and nrm >= 0.10 and (tie >= 0.05 or kind == "f32"), (kind, sub, nrm, tie)
        for name, IA, ea, IB, eb, Pc, ce in X.cases_of(d, kind):
            A, B = np.ldexp(IA, ea), np.ldexp(IB, eb)
            for V in (A, B):
                assert np.array_equal(U.widen_bits(kind, U.narrow_bits(kind, V)), V), f"{name}: an operand is not a {kind} value"
            lo = 2.0 ** U.EMIN[kind]
            if name == "sub_out":
                assert (np.abs(A[A != 0]) >= lo).all() and (np.abs(B[B != 0]) >= lo).all(), "sub_out: the operands must be normal"
            else:
                assert (np.abs(A if name == "sub_in" else B) < lo).all() and (np.abs(np.ldexp(Pc[Pc != 0], ea + eb)) >= lo).all()
        if kind == "f32":  # an f32 output cannot tie; fl32(0.5 acc) of gemm_ex(0.5, .) can
            assert (np.abs(P[::61]) % 2 == 1).mean() >= 0.05
        if second:
            for rng_name in ("normal", "sub_out"):
                P, s, ce, alpha, beta, w0, w1 = X.second_plan(d, kind, rng_name)
                need = 8 if P.size >= 2 ** 16 else 1
                pv, cv, n = U.count_pairs(P, d["IC"])  # (the distinct pairs with their counts: the model is a function of the pair)
                for al, be, w in ((alpha, 0.0, w0), (alpha, beta, w1)):
                    bits, _, fused = U.epilogue_model(kind, al, np.ldexp(pv, s), be, np.ldexp(cv, ce))
                    assert n[bits != fused].sum() == w >= need, (kind, rng_name, al, be, w)
                    assert float(np.float32(al)) * 2.0 ** 12 % 1.0 != 0.0, "alpha must be a generic f32 value"


@pytest.mark.parametrize("row", X.GEMM_ROWS, ids=lambda r: r.name)
def test_exponent_range_plans_gemm(row):
    d = X.base_operands(row.name, row.M, row.K, row.N, row.mats)
    _shares_and_witnesses(d, X.kinds_of(row.dtype), second=row.dtype == np.float16 and getattr(row, "api", "cm") != "rm")


@pytest.mark.parametrize("row", X.GEMV_LEAVES, ids=lambda r: r.name)
def test_exponent_range_plans_gemv(row):
    ro, k = (row.C, row.R) if row.tr else (row.R, row.C)
    _shares_and_witnesses(X.base_operands("gemv" + row.name, ro, k, row.nrhs, row.mats), X.kinds_of(row.dtype), second=False)


@pytest.mark.parametrize("case", X.MIXED_CASES, ids=lambda c: c[0])
def test_exponent_range_plans_mixed_gemv(case):
    name, tr, R, C, nrhs, Z = case[:6]
    k, ro = (R, C) if tr else (C, R)
    d = X.base_operands("mixed" + name, ro, k, nrhs, Z)
    for kind in ("f16", "bf16"):
        for cname, IA, ea, IB, eb, P in X.mixed_cases(d, kind):
            A, B = np.ldexp(IA, ea), np.ldexp(IB, eb)
            assert np.array_equal(U.widen_bits(kind, U.narrow_bits(kind, A)), A) and np.array_equal(B.astype(np.float32).astype(np.float64), B)
            assert ea + eb >= -149 and np.array_equal(P[::61], U.int_product(IA[::61], IB))
            if cname == "sub_out":
                sub, nrm, _ = U.range_shares("f32", np.ldexp(P, ea + eb))
                assert sub >= 0.25 and nrm >= 0.10, (kind, sub, nrm)


@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
def test_exponent_range_reduce_and_op_assign_operands(kind):
    for n in (1000, 4097):
        for opn, case, x, exact in X.reduce_cases(kind, n, np.random.default_rng(n)):
            assert np.array_equal(U.widen_bits(kind, U.narrow_bits(kind, x)), x), (opn, case)
            if case == "second rounding":  # the f32 product of the reference's order (the C oracle) is the model's, and a witness
                from oracle import wgsl_oracle as wo
                ref = wo.CLib().reduce(int(wo.PROD), x.astype(np.float32), wo.Shape(n, 1, 1, n, n, 0))
                assert float(ref) == exact and U.narrow_bits(kind, np.float32([ref]))[0] != U.narrow_bits(kind, U.rne_grid(kind, np.prod(x[:4])))[()]
                continue
            assert exact != 0 and abs(exact) < 2.0 ** U.EMIN[kind] and U.rne_grid(kind, exact) == exact or opn == "SqNorm", (opn, case, exact)
            ref = {"Sum": np.sum, "Min": np.min, "Max": np.max, "Prod": np.prod, "SqNorm": lambda v: ((v * v).astype(np.float32).astype(np.float64)).sum()}[opn](x)
            assert ref == exact, (opn, case, ref, exact)
    lo = 2.0 ** U.EMIN[kind]
    a, b = X.op_assign_operands(kind, 100003, np.random.default_rng(5))
    wants, fused = X.op_assign_model(kind, a, b)
    val = {k: np.abs(U.widen_bits(kind, v)) for k, v in wants.items()}
    sub = {k: ((v > 0) & (v < lo)).mean() for k, v in val.items()}
    assert all(s > 0.05 for s in sub.values()), sub  # every operator: subnormal results
    assert (val["Mul"] == 0).mean() > 0.05 and (val["Mul"][(a != 0) & (b != 0)] == 2.0 ** U.QUANTUM[kind]).any()  # complete underflow, to zero and to one quantum
    exact_q = np.abs(a / b) / 2.0 ** U.QUANTUM[kind]
    assert ((exact_q % 1.0 == 0.5) & (exact_q < 2.0 ** (U.PREC[kind] - 1))).mean() > 0.01, "no quotient ties on the subnormal grid"
    assert kind == "f32" or (fused != wants["Axpy"]).sum() >= 8
