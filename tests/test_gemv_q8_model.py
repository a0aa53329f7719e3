"""The yardsticks of tests/test_gpu_gemv_q8.py, checked on the CPU: a NumPy float32 model of the scaled sum (tests/_q8.py: the scale applied per element and per
piece, sequential and pairwise orders) must stay inside the gate f32_gate(2 k, sum |s q v|) on the GPU tests' own random inputs, and the exact-case inputs must satisfy
their exactness condition and come out of every model to the bit -- so that the GPU tests cannot hide a failure behind a gate the truth itself misses, or pin bits
that depend on the order after all."""
import numpy as np
import pytest

import _q8
import _util as U

MODELS = [("element", "sequential"), ("element", "pairwise"), ("piece", "sequential"), ("piece", "pairwise")]


def _models_for(case):
    k = case[2] if case[1] else case[3]
    return MODELS if k <= 8192 else [("piece", "sequential"), ("element", "pairwise")]  # (the two 65536-term cases: one of each placement and order)


@pytest.mark.parametrize("case", _q8.CASES, ids=_q8.CASE_IDS)
def test_models_stay_inside_the_gate_on_the_gpu_tests_inputs(case):
    name, tr, R, C, nrhs, Z, G = case[:7]
    k = R if tr else C
    q, s, v = _q8.random_inputs(case)
    assert q.min() == -128 or q.size < 2048, "the random weights should reach -128"
    if nrhs > 3:  # (the model is a Python loop per term: three right-hand sides of one matrix say what eleven would)
        v = v[:, :3]
    q, s, v = q[:, :, :1], s[:, :, :1], v[:, :, :1]
    if name in ("t4_3rhs_split", "t4_2mats_split"):  # (t4_split's tile at the same size with more right-hand sides: 512 of the outputs -- they do not interact)
        q, s = q[:, :512], s[:, :512]
    truth, sabs = _q8.truth64(q, s, v, G, tr)
    worst = {}
    for scale, order in _models_for(case):
        got = _q8.model32(q, s, v, G, tr, scale, order)
        worst[scale, order] = _q8.assert_within_gate(got, truth, k, sabs, f"{name} model {scale}/{order}")
    print(name, {f"{a}/{b}": round(w, 3) for (a, b), w in worst.items()})
    # the gate is not vacuous either: it is a few 1e-5 of the sum of magnitudes at most (2 sqrt(2 k) 2^-24 at k = 65536), so a lost term or a lost scale shows
    assert (_q8.gate(k, sabs) <= 1e-4 * sabs + 1e-37).all()


@pytest.mark.parametrize("case", _q8.EXACT_CASES, ids=[c[0] for c in _q8.EXACT_CASES])
def test_exact_inputs_are_exact_in_every_model(case):
    name, tr, R, C, nrhs, Z, G = case[:7]
    q, s, v = _q8.exact_inputs(case)
    assert (q == -128).any() and (q == 127).any()
    assert set(np.unique(s)) <= {0.25, 0.5, 1.0, 2.0, 4.0} and np.abs(v).max() <= 4 and np.array_equal(v, np.rint(v))
    assert _q8.exactness_condition(q, s, v, tr) < 2.0 ** 24
    q, s, v = q[:, :, :1], s[:, :, :1], v[:, :2, :1]
    truth, _ = _q8.truth64(q, s, v, G, tr)
    want = truth.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), truth)
    for scale, order in MODELS:
        U.assert_bits_equal(_q8.model32(q, s, v, G, tr, scale, order) + np.float32(0), want + np.float32(0), f"{name} model {scale}/{order}")


def test_subnormal_scale_inputs_are_exact_subnormals():
    case = _q8.CASES[0]  # one piece
    q, s, v = _q8.exact_inputs(case, scale_exp=(-140, -140), salt=2)
    truth, _ = _q8.truth64(q, s, v, case[6], case[1])
    want = truth.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), truth), "2^-140 times an integer below 2^9 is an f32 value"
    tiny = np.abs(want[want != 0])
    assert tiny.size and (tiny < np.float32(2.0 ** -126)).all(), "every nonzero result is a subnormal"
    for scale, order in MODELS:
        U.assert_bits_equal(_q8.model32(q, s, v, case[6], case[1], scale, order) + np.float32(0), want + np.float32(0), f"subnormal model {scale}/{order}")
