"""The yardsticks of tests/test_gpu_gemm_q4.py on the same inputs without a device: the float32 model of the kernel's sum (_gemm_q8.model32 on _q4.unpack of the packed
bytes: the MFMA chain per group, then fmaf(s, d, acc)) in two summation orders stays inside _q4.gate against the float64 truth on the random inputs of every case;
the exact inputs satisfy _q4.exactness_condition for both element types and the model reproduces the truth to the bit on them; the kernel's two f16 unpack identities
and its bf16 magic number hold for all 16 nibbles."""
import numpy as np
import pytest

import _bf16
import _gemm_q4 as GQ
import _q4
import _util as U


@pytest.mark.parametrize("dt", GQ.DTYPES)
@pytest.mark.parametrize("case", GQ.CASES, ids=GQ.CASE_IDS)
def test_model_inside_the_gate(case, dt):
    q, s, x = GQ.random_inputs(case, dt)
    assert q.min() == -8 and q.max() == 7 and np.array_equal(_q4.unpack(_q4.pack(q)), q)
    assert np.array_equal(GQ.round16(dt, x), x), "x is not representable in the 16-bit type"
    truth, sabs = GQ.truth64(q, s, x, case["G"])
    for order in ("sequential", "pairwise"):
        r = _q4.assert_within_gate(GQ.model32(q, s, x, case["G"], order), truth, case["k"], sabs, f"{case['name']} {dt} {order}")
        assert r < 1.0


@pytest.mark.parametrize("dt", GQ.DTYPES)
@pytest.mark.parametrize("case", GQ.EXACT_CASES, ids=[c["name"] for c in GQ.EXACT_CASES])
def test_exact_inputs_are_exact(case, dt):
    q, s, x = GQ.exact_inputs(case, dt)
    assert (q[0::2] == -8).any() and (q[1::2] == -8).any() and (q[0::2] == 7).any() and (q[1::2] == 7).any(), "both ends in even and in odd rows"
    assert np.array_equal(GQ.round16(dt, x), x) and np.abs(x).max() <= 4
    assert _q4.exactness_condition(q, s, x) < 2.0 ** 24
    truth, _ = GQ.truth64(q, s, x, case["G"])
    want = truth.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), truth)
    if case["k"] <= 16384:  # (the float32 model of the cut case is tested on its random inputs above)
        U.assert_same_class_bits(GQ.model32(q, s, x, case["G"]), want, f"{case['name']} {dt}")


def test_lane_map_inputs_are_exact_and_asymmetric():
    case = GQ.LANE_MAP
    q, s, x = GQ.lane_map_inputs(case)
    assert _q4.exactness_condition(q, s, x) < 2.0 ** 24 and np.abs(x).max() <= 4 and q.min() == -8 and q.max() == 7
    truth, _ = GQ.truth64(q, s, x, case["G"])
    t = truth[:, :, 0]
    assert not np.array_equal(t, t.T), "the product is symmetric: a swapped row / column would pass"
    k = case["k"]
    perms = {"nibbles swapped": np.arange(k).reshape(-1, 2)[:, ::-1].ravel(),
             "rows (r, r + 4) in the place of (r, r + 1)": np.arange(k).reshape(-1, 2, 4).transpose(0, 2, 1).ravel(),
             "the dwords of a lane swapped": np.arange(k).reshape(-1, 2, 8)[:, ::-1, :].ravel(),
             "the half-wave exchange crossed": np.arange(k).reshape(-1, 2, 16)[:, ::-1, :].ravel(),
             "no half-wave exchange": np.arange(k).reshape(-1, 2, 2, 16).transpose(0, 2, 1, 3).ravel()}
    for what, perm in perms.items():  # a k permutation applied to the weights only changes the result
        assert not np.array_equal(GQ.truth64(q[perm], s, x, case["G"])[0], truth), what
    U.assert_same_class_bits(GQ.model32(q, s, x, case["G"]), truth.astype(np.float32), "lane_map")


@pytest.mark.parametrize("dt", GQ.DTYPES)
@pytest.mark.parametrize("case", GQ.CUT_CASES, ids=GQ.CUT_IDS)
def test_cut_model_inside_the_gate(case, dt):
    """The cut cases under the SAME gate, f32_gate(2 k, sum |s q x|): the combine pass adds fewer than ns roundings to the 2 k the gate allows. "pairwise" adds the
    groups' scaled sums over halves, as a cut's partial sums are."""
    q, s, x = GQ.random_inputs(case, dt)
    assert q.min() == -8 and q.max() == 7 and np.array_equal(_q4.unpack(_q4.pack(q)), q)
    assert np.array_equal(GQ.round16(dt, x), x), "x is not representable in the 16-bit type"
    truth, sabs = GQ.truth64(q, s, x, case["G"])
    for order in ("sequential", "pairwise"):
        r = _q4.assert_within_gate(GQ.model32(q, s, x, case["G"], order), truth, case["k"], sabs, f"{case['name']} {dt} {order}")
        assert r < 1.0


@pytest.mark.parametrize("dt", GQ.DTYPES)
@pytest.mark.parametrize("case", GQ.CUT_CASES, ids=GQ.CUT_IDS)
def test_cut_exact_inputs_are_exact(case, dt):
    """What test_cut_exact_operands runs: exact_inputs, whose scales are 2^-2 .. 2^2 up to k = 16384 and 2^0 .. 2^1 beyond."""
    q, s, x = GQ.exact_inputs(case, dt)
    assert (q[0::2] == -8).any() and (q[1::2] == -8).any() and (q[0::2] == 7).any() and (q[1::2] == 7).any(), "both ends in even and in odd rows"
    assert np.array_equal(GQ.round16(dt, x), x) and np.abs(x).max() <= 4
    assert _q4.exactness_condition(q, s, x) < 2.0 ** 24
    truth, _ = GQ.truth64(q, s, x, case["G"])
    want = truth.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), truth) and np.count_nonzero(want) > want.size // 2


def test_cut_lane_map_inputs_are_exact_and_asymmetric():
    """lane_map_inputs at k = 1088 (2 splits of 544 rows: the first ends on half a double step, the second starts on the other half) needs no narrower ranges:
    4 * 1088 * 8 * 4 < 2^24. Permutations of the weights' rows in the SECOND split only, a step handed across the cut and the two splits exchanged change the
    integers."""
    case = GQ.CUT_LANE_MAP
    k = case["k"]
    q, s, x = GQ.lane_map_inputs(case)
    assert 4 * k * 8 * 4 < 2 ** 24 and _q4.exactness_condition(q, s, x) < 2.0 ** 24 and np.abs(x).max() <= 4 and q.min() == -8 and q.max() == 7
    truth, _ = GQ.truth64(q, s, x, case["G"])
    t = truth[:, :, 0]
    assert not np.array_equal(t, t.T), "the product is symmetric: a swapped row / column would pass"
    second = lambda p: np.concatenate([np.arange(544), 544 + p])  # noqa: E731
    perms = {"nibbles swapped": second(np.arange(544).reshape(-1, 2)[:, ::-1].ravel()),
             "the dwords of a lane swapped": second(np.arange(544).reshape(-1, 2, 8)[:, ::-1, :].ravel()),
             "the half-wave exchange crossed": second(np.arange(544).reshape(-1, 2, 16)[:, ::-1, :].ravel()),
             "the second split begun on a whole double step": second((np.arange(544) + 32) % 544),
             "the first split's last step read twice": np.concatenate([np.arange(544), np.arange(512, 544), np.arange(576, k)]),
             "the splits exchanged": np.concatenate([np.arange(544, k), np.arange(544)])}
    for what, perm in perms.items():  # a k permutation (or a repeated step) applied to the weights only changes the result
        assert len(perm) == k and not np.array_equal(GQ.truth64(q[perm], s, x, case["G"])[0], truth), what
    U.assert_same_class_bits(GQ.model32(q, s, x, case["G"], "pairwise"), truth.astype(np.float32), "cut_lane_map")


def test_the_f16_unpack_identities_hold_for_all_16_nibbles():
    n = np.arange(16)
    lo = (np.uint16(0x6400) | n.astype(np.uint16)).view(np.float16)            # (b & 0x000f) | 0x6400
    hi = (np.uint16(0x6400) | (16 * n).astype(np.uint16)).view(np.float16)     # (b & 0x00f0) | 0x6400
    assert np.array_equal(lo.astype(np.float64), 1024.0 + n) and np.array_equal(hi.astype(np.float64), 1024.0 + 16 * n)
    assert np.array_equal((lo - np.float16(1032)).astype(np.float64), n - 8.0)  # (1024 + n) - 1032 == n - 8
    # fma(1024 + 16 n, 1/16, -72) == n - 8: the product is exact in float64 and an f16 value, so the single rounding of the fma changes nothing
    prod = hi.astype(np.float64) * float(np.float16(0.0625)) - 72.0
    assert np.array_equal(prod.astype(np.float16).astype(np.float64), prod) and np.array_equal(prod, n - 8.0)
    # ... and with a rounding after the product (no fused form) as well: 64 + n is an f16 value
    assert np.array_equal(((hi * np.float16(0.0625)) - np.float16(72)).astype(np.float64), n - 8.0)
    # the low-half form through the same fma with the constants (1, -1032)
    assert np.array_equal((lo.astype(np.float64) * 1.0 - 1032.0).astype(np.float16).astype(np.float64), n - 8.0)
    # a whole byte at once: {b, 0x64, b, 0x64} & 0x64f0640f is the pair (1024 + n_lo, 1024 + 16 n_hi)
    b = np.arange(256, dtype=np.uint32)
    both = ((b | 0x6400) | ((b | 0x6400) << 16)) & 0x64F0640F
    assert np.array_equal((both & 0xFFFF).astype(np.uint16).view(np.float16).astype(np.float64), 1024.0 + b % 16)
    assert np.array_equal((both >> 16).astype(np.uint16).view(np.float16).astype(np.float64), 1024.0 + 16 * (b // 16))


def test_the_bf16_forms_hold_for_all_16_nibbles():
    n = np.arange(16)
    magic = _bf16.from_bits((np.uint16(0x4300) | n.astype(np.uint16))).astype(np.float64)
    assert np.array_equal(magic.ravel(), 128.0 + n)  # 0x4300 | n is 128 + n in bf16
    # the kernel's route: n as f32, minus 8, the high half -- the low half is zero (4 significant bits)
    f = (n.astype(np.float32) - np.float32(8)).view(np.uint32)
    assert (f & 0xFFFF == 0).all() and np.array_equal(_bf16.from_bits((f >> 16).astype(np.uint16)).astype(np.float64).ravel(), n - 8.0)
