"""The yardsticks of tests/test_gpu_gemm_q8a8.py without a device: the NumPy float32 model of wg_gemm_q8a8's arithmetic (tests/_gemm_q8a8.py) against the float64
truth, on the GPU tests' own inputs.

The gate is derived, not measured: a chain's integer sum is exact, and each chain takes one multiply rounding (u = x_scale * d) and one FMA rounding, so an output
of C chains is a sum of 2 C rounded terms: f32_gate(2 C, sum over chains |w_scale * x_scale * d|)."""
import numpy as np
import pytest

import _gemm_q8a8 as GA
import _util as U


@pytest.mark.parametrize("case", GA.CASES, ids=GA.CASE_IDS)
def test_model_within_the_gate(case):
    q, s, x, xs = GA.random_inputs(case)
    truth, sabs, nch = GA.truth64(q, s, x, xs, case["G"], case["Gx"])
    for kps in (None,) + ((1024, 4096) if case["name"] == "cut" else (1024,) if case["name"] == "chain_cap" else ()):
        got = GA.model32(q, s, x, xs, case["G"], case["Gx"], kps)
        err = np.abs(got.astype(np.float64) - truth)
        tol = GA.gate(nch + (-(-case["k"] // kps) if kps else 0), sabs)  # (a cut adds one rounding per split)
        assert (err <= tol).all(), f"{case['name']} kps {kps}: worst err / gate = {(err / tol).max():.3g}"


def test_chains():
    """The chain boundaries of the contract: every boundary of either side's groups, and every 1024 rows from the start of the finer group."""
    W = GA.WHOLE
    assert GA.chains(512, 64, 128) == [(r, r + 64) for r in range(0, 512, 64)]
    assert GA.chains(512, W, 32) == [(r, r + 32) for r in range(0, 512, 32)]
    assert GA.chains(2080, W, W) == [(0, 1024), (1024, 2048), (2048, 2080)]
    assert GA.chains(4096, 1536, W) == [(0, 1024), (1024, 1536), (1536, 2560), (2560, 3072), (3072, 4096)]  # the cap counts from the GROUP's start
    assert GA.chains(96, 16, 48) == [(r, r + 16) for r in range(0, 96, 16)]
    assert GA.chains(37, 16, 16) == [(0, 16), (16, 32), (32, 37)]
    assert GA.chains(2080, W, W, 1024, 2048) == [(1024, 2048)]
    assert max(r1 - r0 for r0, r1 in GA.chains(131104, W, W)) == 1024 and len(GA.chains(131104, W, W)) == 129


def test_a_full_chain_of_minus_128_is_exactly_2_to_24():
    """All -128 on both sides: a 1024-row chain sums to 1024 * 2^14 = 2^24, which int32 holds and (float) keeps; 1025 rows would give 2^24 + 2^14 -- still a float --
    but a chain of mixed data past 1024 rows can reach an odd integer above 2^24, which no float holds: the cap is part of the contract."""
    case = GA.by_name("chain_cap")
    q, s, x, xs = GA.random_inputs(case)
    d = q[:1024, 0, 0].astype(np.int64) @ x[:1024, 0, 0].astype(np.int64)
    assert d == 2 ** 24 and np.float32(d) == d
    odd = 2 ** 24 + 1  # e.g. 1024 rows of -128 * -128 and one row of 1 * 1
    assert int(np.float32(odd)) != odd
    # without the cap an int32 chain of k = 131104 rows of -128 * -128 overflows
    assert 131104 * 2 ** 14 > 2 ** 31 - 1
    got = GA.model32(q, s, x, xs, case["G"], case["Gx"])
    truth, sabs, nch = GA.truth64(q, s, x, xs, case["G"], case["Gx"])
    assert nch == 3 and (np.abs(got - truth) <= GA.gate(nch, sabs)).all()


def test_power_of_two_operands_are_exact():
    for name in ("one_step", "cols_65", "any_g16"):
        c = GA.by_name(name)
        q, s, x, xs = GA.pow2_inputs(c)
        assert GA.exactness_condition(q, s, x, xs) < 2.0 ** 24
        truth, _, _ = GA.truth64(q, s, x, xs, c["G"], c["Gx"])
        U.assert_bits_equal(GA.model32(q, s, x, xs, c["G"], c["Gx"]), truth.astype(np.float32), name)
    c = GA.by_name("groups_96")
    q, s, x, xs = GA.pow2_inputs(c, w_exps=(-140,), x_exps=(0, 1), salt=2)
    truth, _, _ = GA.truth64(q, s, x, xs, c["G"], c["Gx"])
    want = truth.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), truth) and ((want != 0) & (np.abs(want) < 2.0 ** -126)).mean() > 0.25
    U.assert_bits_equal(GA.model32(q, s, x, xs, c["G"], c["Gx"]), want, "2^-140")


def test_combine_order():
    """The cut's partials are added as the combine pass adds them: wave w takes splits w, w + 4, ..., then ((w0 + w1) + w2) + w3 -- not ascending over all splits."""
    c = GA.by_name("cut")
    q, s, x, xs = GA.random_inputs(c)
    a, b = GA.model32(q, s, x, xs, c["G"], c["Gx"], 1024), GA.model32(q, s, x, xs, c["G"], c["Gx"])
    assert a.shape == b.shape and np.isfinite(a).all()
    assert not np.array_equal(a, b)  # (129 partials of about 2^24 * s * xs each: the two orders round differently)
