"""The yardsticks of tests/test_gpu_gemm_q8.py on the same inputs without a device: a NumPy float32 model of the kernel's sum -- the MFMA chain per group, then
fmaf(s, d, acc) -- in two summation orders stays inside _q8.gate against the float64 truth for every case; the exact inputs satisfy the exactness condition and the
model reproduces the truth to the bit on them; int8 -> f16 and -> bf16 round-trips all 256 values, by conversion and by the kernel's own bit recipes."""
import numpy as np
import pytest

import _bf16
import _gemm_q8 as GQ
import _q8
import _util as U


@pytest.mark.parametrize("dt", GQ.DTYPES)
@pytest.mark.parametrize("case", GQ.CASES, ids=GQ.CASE_IDS)
def test_model_inside_the_gate(case, dt):
    q, s, x = GQ.random_inputs(case, dt)
    assert np.array_equal(GQ.round16(dt, x), x), "x is not representable in the 16-bit type"
    truth, sabs = GQ.truth64(q, s, x, case["G"])
    for order in ("sequential", "pairwise"):
        r = _q8.assert_within_gate(GQ.model32(q, s, x, case["G"], order), truth, case["k"], sabs, f"{case['name']} {dt} {order}")
        assert r < 1.0


@pytest.mark.parametrize("dt", GQ.DTYPES)
@pytest.mark.parametrize("case", GQ.EXACT_CASES, ids=[c["name"] for c in GQ.EXACT_CASES])
def test_exact_inputs_are_exact(case, dt):
    q, s, x = GQ.exact_inputs(case, dt)
    assert (q == -128).any() and (q == 127).any()
    assert np.array_equal(GQ.round16(dt, x), x)
    assert _q8.exactness_condition(q, s, x, True) < 2.0 ** 24
    truth, _ = GQ.truth64(q, s, x, case["G"])
    want = truth.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), truth)
    for order in ("sequential", "pairwise"):
        U.assert_same_class_bits(GQ.model32(q, s, x, case["G"], order), want, f"{case['name']} {dt} {order}")


def test_lane_map_inputs_are_exact_and_asymmetric():
    case = [c for c in GQ.CASES if c["name"] == "lane_map"][0]
    q, s, x = GQ.lane_map_inputs(case)
    assert _q8.exactness_condition(q, s, x, True) < 2.0 ** 24 and np.abs(x).max() <= 4 and q.min() >= -127
    truth, _ = GQ.truth64(q, s, x, case["G"])
    t = truth[:, :, 0]
    assert not np.array_equal(t, t.T), "the product is symmetric: a swapped row / column would pass"
    # a k permutation applied to one operand only (the two halves of a lane's 16-byte piece swapped) changes the result
    perm = np.arange(case["k"]).reshape(-1, 2, 8)[:, ::-1, :].ravel()
    assert not np.array_equal(GQ.truth64(q[perm], s, x, case["G"])[0], truth)
    U.assert_same_class_bits(GQ.model32(q, s, x, case["G"]), truth.astype(np.float32), "lane_map")


@pytest.mark.parametrize("dt", GQ.DTYPES)
@pytest.mark.parametrize("case", GQ.CUT_CASES, ids=GQ.CUT_IDS)
def test_cut_model_inside_the_gate(case, dt):
    """The cut cases under the SAME gate, f32_gate(2 k, sum |s q x|): the combine pass adds fewer than ns roundings to the 2 k the gate allows. "pairwise" adds the
    groups' scaled sums over halves, as a cut's partial sums are."""
    q, s, x = GQ.random_inputs(case, dt)
    assert np.array_equal(GQ.round16(dt, x), x), "x is not representable in the 16-bit type"
    truth, sabs = GQ.truth64(q, s, x, case["G"])
    for order in ("sequential", "pairwise"):
        r = _q8.assert_within_gate(GQ.model32(q, s, x, case["G"], order), truth, case["k"], sabs, f"{case['name']} {dt} {order}")
        assert r < 1.0


@pytest.mark.parametrize("dt", GQ.DTYPES)
@pytest.mark.parametrize("case", GQ.CUT_CASES, ids=GQ.CUT_IDS)
def test_cut_exact_inputs_are_exact(case, dt):
    """What test_cut_exact_operands runs: exact_inputs up to k = 2048, the narrower variant (x in {-1, 0, 1}, scales 2^0 and 2^1) beyond."""
    q, s, x = GQ.cut_exact_inputs(case, dt)
    assert (q == -128).any() and (q == 127).any()
    assert np.array_equal(GQ.round16(dt, x), x) and np.abs(x).max() == (4 if case["k"] <= 2048 else 1)
    assert _q8.exactness_condition(q, s, x, True) < 2.0 ** 24
    assert 2 * 128 * 18432 < 2 ** 24  # (the narrow variant's worst case at the longest k)
    truth, _ = GQ.truth64(q, s, x, case["G"])
    want = truth.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), truth) and np.count_nonzero(want) > want.size // 2


def test_cut_lane_map_inputs_are_exact_and_asymmetric():
    """lane_map_inputs at k = 1088 (2 splits of 544 rows) needs no narrower ranges: 4 * 1088 * 127 * 4 < 2^24. A k permutation applied to one operand in the SECOND
    split only, and the two splits' rows exchanged on one operand, change the integers."""
    case = GQ.CUT_LANE_MAP
    k = case["k"]
    q, s, x = GQ.lane_map_inputs(case)
    assert 4 * k * 127 * 4 < 2 ** 24 and _q8.exactness_condition(q, s, x, True) < 2.0 ** 24 and np.abs(x).max() <= 4 and q.min() >= -127
    truth, _ = GQ.truth64(q, s, x, case["G"])
    t = truth[:, :, 0]
    assert not np.array_equal(t, t.T), "the product is symmetric: a swapped row / column would pass"
    inside = np.arange(k)
    inside[544:] = 544 + np.arange(544).reshape(-1, 2, 8)[:, ::-1, :].ravel()  # the halves of a lane's 16-byte piece swapped, in the second split
    shifted = np.concatenate([np.arange(544), 544 + (np.arange(544) + 32) % 544])  # the second split's steps rotated by one
    swapped = np.concatenate([np.arange(544, k), np.arange(544)])                  # the two splits' rows exchanged
    for what, perm in (("inside a piece", inside), ("steps rotated", shifted), ("splits exchanged", swapped)):
        assert not np.array_equal(GQ.truth64(q[perm], s, x, case["G"])[0], truth), what
    U.assert_same_class_bits(GQ.model32(q, s, x, case["G"], "pairwise"), truth.astype(np.float32), "cut_lane_map")


def test_int8_round_trips_through_both_16_bit_types():
    v = np.arange(-128, 128).astype(np.int8)
    assert np.array_equal(v.astype(np.float16).astype(np.int32), v.astype(np.int32))
    assert np.array_equal(_bf16.from_bits(_bf16.to_bits(v.astype(np.float32))).astype(np.int32), v.astype(np.int32))
    # the kernel's recipes, restated on the bits. f16: 0x6400 | (q ^ 0x80) is 1024 + u; minus 1152 is q, exactly
    u = (v.view(np.uint8) ^ 0x80).astype(np.uint16)
    magic = (np.uint16(0x6400) | u).view(np.float16)
    assert np.array_equal(magic.astype(np.float32), 1024 + u.astype(np.float32))
    assert np.array_equal((magic - np.float16(1152)).astype(np.int32), v.astype(np.int32))
    # bf16: the high half of (float)q -- the low half is zero for |q| <= 128
    f = v.astype(np.float32).view(np.uint32)
    assert (f & 0xFFFF == 0).all() and np.array_equal(_bf16.from_bits((f >> 16).astype(np.uint16)).astype(np.int32), v.astype(np.int32))
