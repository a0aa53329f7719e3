"""The yardsticks of tests/test_gpu_gemv_q4.py, checked on the CPU: the float32 model of the scaled sum (the scale applied per element and per 16-weight piece,
sequential and pairwise orders) must stay inside the gate f32_gate(2 k, sum |s q v|) against float64 on the GPU tests' own random inputs, and the exact-case inputs
must satisfy their exactness condition and come out of every model to the bit -- so that the GPU tests cannot hide a failure behind a gate the truth itself misses, or
pin bits that depend on the order after all. Then the host helpers: pack_q4 / unpack_q4 and quantize_q4 / dequantize_q4 keep their stated rules."""
import numpy as np
import pytest

import _q4
import _util as U
import wgmath_amd as wg

MODELS = [("element", "sequential"), ("element", "pairwise"), ("piece", "sequential"), ("piece", "pairwise")]
MODEL_CASES = [c for c in _q4.CASES if c[0] != "t4_split"]  # (the same kernel and tile as t4_trips at 64 M weights: the model is a Python loop per term)


@pytest.mark.parametrize("case", MODEL_CASES, ids=[c[0] for c in MODEL_CASES])
def test_models_stay_inside_the_gate_on_the_gpu_tests_inputs(case):
    name, k, C, nrhs, Z, G = case[:6]
    q, s, v = _q4.random_inputs(case)
    assert q.min() == -8 and q.max() == 7, "the random weights should reach both ends"
    q, s, v = q[:, :16, :1], s[:, :16, :1], v[:, :2, :1]  # (16 columns, two right-hand sides of one matrix say what all would)
    truth, sabs = _q4.truth64(q, s, v, G)
    for scale, order in (MODELS if k <= 8192 else [("piece", "sequential"), ("element", "pairwise")]):
        _q4.assert_within_gate(_q4.model32(q, s, v, G, scale, order), truth, k, sabs, f"{name} model {scale}/{order}")
    # the gate is not vacuous either: a few 1e-5 of the sum of magnitudes at most (2 sqrt(2 k) 2^-24 at k = 65536), so a lost term or a lost scale shows
    assert (_q4.gate(k, sabs) <= 1e-4 * sabs + 1e-37).all()


@pytest.mark.parametrize("case", _q4.EXACT_CASES, ids=[c[0] for c in _q4.EXACT_CASES])
def test_exact_inputs_are_exact_in_every_model(case):
    name, k, C, nrhs, Z, G = case[:6]
    q, s, v = _q4.exact_inputs(case)
    assert (q == -8).any() and (q == 7).any()
    assert set(np.unique(s)) <= {0.25, 0.5, 1.0, 2.0, 4.0} and np.abs(v).max() <= 4 and np.array_equal(v, np.rint(v))
    assert _q4.exactness_condition(q, s, v) < 2.0 ** 24
    q, s, v = q[:, :8, :1], s[:, :8, :1], v[:, :2, :1]
    truth, _ = _q4.truth64(q, s, v, G)
    want = truth.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), truth)
    for scale, order in (MODELS if k <= 8192 else [("piece", "sequential"), ("element", "pairwise")]):  # (the long ones: one of each placement and order)
        U.assert_bits_equal(_q4.model32(q, s, v, G, scale, order) + np.float32(0), want + np.float32(0), f"{name} model {scale}/{order}")


def test_subnormal_scale_inputs_are_exact_subnormals():
    case = _q4.CASES[0]  # one load
    q, s, v = _q4.exact_inputs(case, scale_exp=(-140, -140), salt=2)
    truth, _ = _q4.truth64(q, s, v, case[5])
    want = truth.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), truth), "2^-140 times an integer below 2^10 is an f32 value"
    tiny = np.abs(want[want != 0])
    assert tiny.size and (tiny < np.float32(2.0 ** -126)).all(), "every nonzero result is a subnormal"
    for scale, order in MODELS:
        U.assert_bits_equal(_q4.model32(q, s, v, case[5], scale, order) + np.float32(0), want + np.float32(0), f"subnormal model {scale}/{order}")


# ---- pack_q4 / unpack_q4 -----------------------------------------------------------------------------------------------------------------------------------
def test_pack_round_trips_all_16_values_in_both_nibbles():
    lo, hi = np.meshgrid(np.arange(-8, 8), np.arange(-8, 8), indexing="ij")
    q = np.empty((2, 256), np.int8)
    q[0], q[1] = lo.ravel(), hi.ravel()  # row 0: the low nibble, row 1: the high nibble -- every pair once
    m = wg.pack_q4(q)
    assert m.dtype == np.uint8 and m.shape == (1, 256)
    assert np.array_equal(m[0], ((lo.ravel() + 8) + 16 * (hi.ravel() + 8)).astype(np.uint8)), "row 2 j in the LOW nibble, row 2 j + 1 in the HIGH one, n = q + 8"
    assert sorted(m[0]) == list(range(256))
    back = wg.unpack_q4(m)
    assert back.dtype == np.int8 and np.array_equal(back, q)
    assert np.array_equal(_q4.pack(q[:, :, None])[:, :, 0], m) and np.array_equal(_q4.unpack(m), q)  # the tests' own restatement agrees
    # a cube, more rows; the inverse of every byte
    rng = np.random.default_rng(3)
    q3 = rng.integers(-8, 8, (10, 3, 2), dtype=np.int8)
    assert wg.pack_q4(q3).shape == (5, 3, 2) and np.array_equal(wg.unpack_q4(wg.pack_q4(q3)), q3)
    allb = np.arange(256, dtype=np.uint8).reshape(16, 16)
    assert np.array_equal(wg.pack_q4(wg.unpack_q4(allb)), allb)
    assert np.array_equal(wg.pack_q4(q3.astype(np.int64)), wg.pack_q4(q3))


def test_pack_refuses_what_it_cannot_hold():
    with pytest.raises(ValueError, match="even"):
        wg.pack_q4(np.zeros((3, 2), np.int8))
    for bad in (-9, 8):
        with pytest.raises(ValueError):
            wg.pack_q4(np.full((2, 2), bad, np.int8))
    with pytest.raises(TypeError):
        wg.pack_q4(np.zeros((2, 2), np.float32))
    with pytest.raises(TypeError):
        wg.unpack_q4(np.zeros((2, 2), np.int8))
    with pytest.raises(ValueError):
        wg.pack_q4(np.zeros(4, np.int8))


# ---- quantize_q4 / dequantize_q4 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,G", [((128, 5), 32), ((128, 5), 64), ((128, 5), 128), ((100, 7), 32), ((100, 7), 96), ((100, 7), 100), ((100, 7), 4096), ((38, 3), 39),
                                     ((64, 4, 3), 32), ((100, 2, 2), 64)])
def test_quantize_holds_its_rule(shape, G):
    rng = np.random.default_rng(shape[0] + G)
    w = (rng.standard_normal(shape) * rng.choice([1e-3, 1.0, 50.0], shape[1:])).astype(np.float32)
    m, s = wg.quantize_q4(w, G)
    k = shape[0]
    ng = -(-k // G)
    assert m.dtype == np.uint8 and m.shape == (k // 2,) + shape[1:] and s.dtype == np.float32 and s.shape == (ng,) + shape[1:]
    q = _q4.unpack(m)
    assert q.min() >= -7, "-8 was produced"
    gi = np.arange(k) // G
    # per group and column s = fl32(max|w| / 7) and q = clip(rint(w / s), -7, 7): some weight of every group sits at +-7 (a partial last group included)
    for i in range(ng):
        blk = w[i * G:(i + 1) * G]
        assert np.array_equal(s[i], (np.abs(blk).max(axis=0) / np.float32(7)).astype(np.float32))
        assert np.array_equal(q[i * G:(i + 1) * G], np.clip(np.rint(blk / s[i]), -7, 7).astype(np.int8))
        assert (np.abs(q[i * G:(i + 1) * G].astype(np.int32)).max(axis=0) == 7).all()
    d = wg.dequantize_q4(m, s, G)
    assert d.dtype == np.float32 and d.shape == w.shape
    assert np.array_equal(d, (s[gi] * q.astype(np.float32)).astype(np.float32))
    # the round trip is within s / 2 per element (the f32 quotient is off by less than 2^-20 of a step, the product s q by 2^-24 of at most 7 steps)
    err = np.abs(d.astype(np.float64) - w.astype(np.float64))
    assert (err <= s[gi].astype(np.float64) * (0.5 + 2.0 ** -16)).all()


def test_quantize_all_zero_groups_and_errors():
    w = np.ones((128, 3), np.float32)
    w[32:64, 1] = 0  # one all-zero group
    w[:, 2] = 0      # an all-zero column
    m, s = wg.quantize_q4(w, 32)
    q = wg.unpack_q4(m)
    assert s[1, 1] == 0 and (q[32:64, 1] == 0).all() and (s[:, 2] == 0).all() and (q[:, 2] == 0).all()
    assert (m[16:32, 1] == 0x88).all(), "a zero weight is the nibble 8"
    assert (s[:, 0] == np.float32(1) / np.float32(7)).all() and (q[:, 0] == 7).all()
    assert np.array_equal(wg.dequantize_q4(m, s, 32)[:, 2], np.zeros(128, np.float32)) and np.isfinite(wg.dequantize_q4(m, s, 32)).all()
    m2, s2 = wg.quantize_q4(-w, 1000)  # per column
    assert s2.shape == (1, 3) and (wg.unpack_q4(m2)[:, 0] == -7).all()
    for bad in (0, -32, 16, 48, 127):
        with pytest.raises(ValueError):
            wg.quantize_q4(w, bad)
    with pytest.raises(ValueError, match="even"):
        wg.quantize_q4(np.ones((33, 2), np.float32), 64)
    with pytest.raises(TypeError):
        wg.dequantize_q4(m.astype(np.int8), s, 32)
    with pytest.raises(ValueError):
        wg.dequantize_q4(m, s[:2], 32)
