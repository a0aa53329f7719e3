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


def cut_plan(case, cus=256):
    """The planner's cut of a case (wg_debug_gemm_q8a8_plan on the query the GPU test's views fill)."""
    import ctypes

    from wgmath_amd import _lib
    q, p = _lib.GemmQ8A8QueryC(), _lib.GemmQ8A8PlanC()
    for key, v in GA.query_kw(case, cus=cus).items():
        setattr(q, key, v)
    tags = ctypes.create_string_buffer(128)
    assert _lib.lib.wg_debug_gemm_q8a8_plan(ctypes.byref(q), ctypes.byref(p), tags, 128) == 0
    return p


@pytest.mark.parametrize("case", GA.CUT_CASES, ids=GA.CUT_IDS)
def test_cut_model_within_the_gate(case):
    """The cut cases under the planner's own cut: every cut boundary is a chain boundary (model32 asserts it), and the model -- the bits the GPU test asks for -- is
    inside gate(nchains, sabs): the combine adds fewer than ns roundings, and an output of C chains is allowed 2 C."""
    plan = cut_plan(case)
    assert plan.nsplit > 1
    q, s, x, xs = GA.random_inputs(case)
    truth, sabs, nch = GA.truth64(q, s, x, xs, case["G"], case["Gx"])
    assert plan.nsplit < nch + 1  # (no split without a chain of its own: the combine's roundings are fewer than the chains')
    got = GA.model32(q, s, x, xs, case["G"], case["Gx"], plan.k_per_split)
    err = np.abs(got.astype(np.float64) - truth)
    tol = GA.gate(nch, sabs)
    assert (err <= tol).all(), f"{case['name']}: worst err / gate = {(err / tol).max():.3g}"
    if case["name"] == "cut_masked":  # the cuts of the 16- and 8-CU contexts
        for cus in (16, 8):
            got = GA.model32(q, s, x, xs, case["G"], case["Gx"], cut_plan(case, cus).k_per_split)
            assert (np.abs(got.astype(np.float64) - truth) <= tol).all(), cus


@pytest.mark.parametrize("case", GA.CUT_CASES, ids=GA.CUT_IDS)
def test_cut_power_of_two_operands_are_exact(case):
    """What test_cut_exact_operands runs (cut_pow2_inputs: x in {-1, 0, 1}, scales 2^0 and 2^1 on both sides): the condition holds and the model under the plan's cut
    gives the float64 truth to the bit."""
    q, s, x, xs = GA.cut_pow2_inputs(case)
    assert (q == -128).any() and (q == 127).any() and np.abs(x).max() == 1
    assert GA.exactness_condition(q, s, x, xs) < 2.0 ** 24 and 4 * 128 * 29696 < 2 ** 24
    truth, _, _ = GA.truth64(q, s, x, xs, case["G"], case["Gx"])
    want = truth.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), truth) and np.count_nonzero(want) > want.size // 2
    U.assert_same_class_bits(GA.model32(q, s, x, xs, case["G"], case["Gx"], cut_plan(case).k_per_split), want, case["name"])


def test_cut_lane_map_inputs_are_exact_and_asymmetric():
    """lane_map_inputs (an asymmetric x over the full int8 range) at k = 1088 is past the sum bound: x is narrowed to [-4, 4] -- 2 * 4 * 1088 * 127 * 4 < 2^24. A k
    permutation applied to the weights in the SECOND split only, and the two splits exchanged, change the integers."""
    case = GA.CUT_LANE_MAP
    k = case["k"]
    q, s, x, xs = GA.cut_lane_map_inputs(case)
    assert 2 * 4 * k * 127 * 4 < 2 ** 24 and GA.exactness_condition(q, s, x, xs) < 2.0 ** 24 and np.abs(x).max() <= 4 and q.min() >= -127
    truth, _, _ = GA.truth64(q, s, x, xs, case["G"], case["Gx"])
    t = truth[:, :, 0]
    assert not np.array_equal(t, t.T), "the product is symmetric: a swapped row / column would pass"
    inside = np.arange(k)
    inside[544:] = 544 + np.arange(544).reshape(-1, 2, 8)[:, ::-1, :].ravel()
    shifted = np.concatenate([np.arange(544), 544 + (np.arange(544) + 32) % 544])
    swapped = np.concatenate([np.arange(544, k), np.arange(544)])
    for what, perm in (("inside a piece", inside), ("steps rotated", shifted), ("splits exchanged", swapped)):
        assert not np.array_equal(GA.truth64(q[perm], s, x, xs, case["G"], case["Gx"])[0], truth), what
    U.assert_same_class_bits(GA.model32(q, s, x, xs, case["G"], case["Gx"], 544), truth.astype(np.float32), "cut_lane_map")


def test_combine_order():
    """The cut's partials are added as the combine pass adds them: wave w takes splits w, w + 4, ..., then ((w0 + w1) + w2) + w3 -- not ascending over all splits."""
    c = GA.by_name("cut")
    q, s, x, xs = GA.random_inputs(c)
    a, b = GA.model32(q, s, x, xs, c["G"], c["Gx"], 1024), GA.model32(q, s, x, xs, c["G"], c["Gx"])
    assert a.shape == b.shape and np.isfinite(a).all()
    assert not np.array_equal(a, b)  # (129 partials of about 2^24 * s * xs each: the two orders round differently)
