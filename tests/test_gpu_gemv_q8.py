"""wg_gemv_q8 on the GPU, through the C ABI: an int8 matrix with one f32 scale per group of rows, f32 vectors, f32 result. Before the feature the symbol did not exist.

The contract (include/wgebra_hip.h): W[r, c] = scales[r // G, c] * m[r, c]; out = W v or W^T v; int8 widened exactly, nothing narrowed, f32 FMAs and multiplies, the
accumulator stored as it is; deterministic. Cases, inputs, truth and gate are tests/_q8.py's (tests/test_gemv_q8_model.py checks them on the CPU).

  1  every leaf ran (wg_debug_take_path): the streaming kernels at the smallest lengths at which they can go wrong, the element-by-element ones on views that are off
  2  |got - f64 sum s q v| <= f32_gate(2 k, sum |s q v|)                                              test_leaves_truth_and_determinism (1, 2, 6)
  3  exact operands to the bit, -128 included; scale 2^-140: exact subnormals                        test_exact_operands, test_subnormal_scale
  4  against wg_gemv_mixed on the dequantised f16 matrix and wg_gemv on the dequantised f32 one       test_against_the_projects_own_kernels
  5  NaN in out overwritten; NaN / Inf in v or in a scale reach exactly their outputs; 0 * Inf = NaN  test_special_values
  6  the same call twice is bit-identical, the cut contraction included                               (in 1)
     every cut case (1 and 3 right-hand sides, 1 and 2 matrices, per cut leaf) runs on a workspace that a NaN-scaled call of another shape has just filled, in 1,
     3 and 9: an unwritten partial is a NaN in the result                                             dirty_workspace
  7  status codes and messages                                                                       test_status_codes, test_workspace_inside_a_recording
  8  aliasing, on addresses                                                                          test_aliasing
  9  recorded and replayed; a CU-masked context                                                      test_recorded_and_masked
 10  a matrix whose third column starts past 4 GiB of its parent                                     test_far_view
 11  the Python operators with quantize_q8                                                           test_python_operators
No test asserts a time.
"""
import ctypes
import faulthandler

import numpy as np
import pytest

import _q8
import _util as U

pytestmark = pytest.mark.gpu

S_STORAGE = 128 | 4 | 8
NAN32 = np.float32(np.nan)
SENTINEL8 = np.int8(0x5A)
GiB = 1 << 30


def _wg():
    import wgmath_amd as wg
    return wg


def _L():
    from wgmath_amd import _lib
    return _lib


@pytest.fixture(autouse=True)
def _time_limit():
    """No test of this file may hang the run: after 300 s a watchdog thread dumps the tracebacks and ends the process."""
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


# ---- plumbing --------------------------------------------------------------------------------------------------------------------------------------
class Op:
    """X[r, c, z] stored column-major at element `off` with leading dimension r + pad and `gap` elements between matrices, in a poisoned parent: NaN for float32,
    the sentinel byte 0x5A for int8."""

    def __init__(self, gpu, vals, dtype=np.float32, off=0, pad=0, gap=0):
        wg = _wg()
        vals = np.asarray(vals, dtype)
        R, C, Z = vals.shape
        self.gpu, self.dtype = gpu, np.dtype(dtype)
        self.ld = R + pad
        self.batch = self.ld * C + gap
        self.size = off + self.batch * Z + 16
        self.idx = off + np.arange(R)[:, None, None] + np.arange(C)[None, :, None] * self.ld + np.arange(Z)[None, None, :] * self.batch
        self.poison_value = NAN32 if self.dtype == np.float32 else SENTINEL8
        self.init = np.full(self.size, self.poison_value, dtype)
        self.init[self.idx] = vals
        self.buf = wg.TensorBuilder.tensor((self.size,), S_STORAGE).build_init(gpu.device(), self.init, self.init.dtype)
        self.shape = wg.ViewShape((R, C, Z), self.ld, self.batch, off)
        self.outside = np.ones(self.size, bool)
        self.outside[self.idx.ravel()] = False

    def poison(self):
        self.gpu.queue().write_buffer(self.buf, 0, self.init)

    def read(self, what=""):
        flat = self.buf.read(self.gpu.device())
        assert np.isnan(flat[self.outside]).all(), f"{what}: wrote outside the view"
        return np.ascontiguousarray(flat[self.idx])


class View:
    """A view of somebody else's buffer."""

    def __init__(self, buf, shape):
        self.buf, self.shape = buf, shape


def call(inst, tr, G, out, m, s, v, variant=None):
    """(status, message) of wg_gemv_q8."""
    wg, L = _wg(), _L()
    variant = int(wg.GemvVariant.GemvTr if tr else wg.GemvVariant.Gemv) if variant is None else int(variant)
    rc = L.lib.wg_gemv_q8(inst._ctx.handle, variant, int(G), out.buf._h, out.shape.to_c(), m.buf._h, m.shape.to_c(), s.buf._h, s.shape.to_c(), v.buf._h, v.shape.to_c())
    return rc, L.lib.wg_last_error_string().decode()


def run(inst, tr, G, out, m, s, v):
    rc, msg = call(inst, tr, G, out, m, s, v)
    assert rc == 0, msg


def build_case(gpu, case, q, s, v):
    """The operands of a case on the device: the matrix at its byte offset / padding / gap, the scales in a view of their own that no kernel may assume dense (offset
    3, leading dimension + 1, gap 2), v and out at the case's offset (leading dimensions padded by 4 when it is not zero)."""
    name, tr, R, C, nrhs, Z, G, (moff, mpad, gap), voff, tag = case
    vp = 4 if voff else 0
    m = Op(gpu, q, np.int8, off=moff, pad=mpad, gap=gap)
    sc = Op(gpu, s, off=3, pad=1, gap=2)
    vv = Op(gpu, v, off=voff, pad=vp)
    out = Op(gpu, np.full((C if tr else R, nrhs, Z), NAN32), off=voff, pad=vp)
    return m, sc, vv, out


_DIRTY = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_dirty():
    yield
    _DIRTY.clear()


def planned(inst, case, m, sc, vv, out):
    """wg_debug_gemv_q8_plan's plan for the query a call on these views fills, on the context's CU count (a CU-masked context's own)."""
    L = _L()
    name, tr, R, C, nrhs, Z, G = case[:7]
    info = inst.adapter()
    q, p = L.GemvQ8QueryC(), L.GemvQ8PlanC()
    kw = dict(trans=int(tr), rows=R, cols=C, nrhs=nrhs, mats=Z, group_rows=G, ldm=m.ld, lds=sc.ld, ldv=vv.ld, ldo=out.ld, m_batch=m.batch, s_batch=sc.batch, v_batch=vv.batch,
              o_batch=out.batch, cus=info.get("stream_compute_units", info["compute_units"]))
    for key, op, es in (("m_addr16", m, 1), ("v_addr16", vv, 4), ("o_addr16", out, 4)):
        kw[key] = (L.lib.wg_buf_device_ptr(op.buf._h) + es * op.shape.offset) % 16
    for key, v in kw.items():
        setattr(q, key, v)
    tags = ctypes.create_string_buffer(128)
    assert L.lib.wg_debug_gemv_q8_plan(ctypes.byref(q), ctypes.byref(p), tags, 128) == 0
    return p


def dirty_workspace(inst, case, ops):
    """Before a cut case (`ops`: its operands) runs: one call on _q8.DIRTY, a larger cut problem of another shape whose scales are all NaN, so that every f32 partial
    in the context's workspace the case should write holds NaN -- a partial it fails to write shows in its result. Through the planner: the dirtying call is cut and
    its workspace covers the case's; its outputs x right-hand sides is another one, so stale values cannot line up. Nothing happens for a case that is not cut."""
    plan = planned(inst, case, *ops)
    if plan.nsplit == 1:
        return
    d = _q8.DIRTY
    first = id(inst) not in _DIRTY
    if first:
        q, s, v = _q8.random_inputs(d, salt=9)
        _DIRTY[id(inst)] = (inst,) + build_case(inst, d, q, np.full_like(s, NAN32), v)
    dops = _DIRTY[id(inst)][1:]
    dplan = planned(inst, d, *dops)
    assert dplan.nsplit > 1 and dplan.workspace_bytes >= plan.workspace_bytes > 0, (dplan.nsplit, dplan.workspace_bytes, plan.workspace_bytes)
    assert d[2] * d[4] != (case[3] if case[1] else case[2]) * case[4]
    m, sc, vv, out = dops
    run(inst, d[1], d[6], out, m, sc, vv)
    if first:
        assert np.isnan(out.read("dirty")).all(), "NaN scales did not reach every partial of the dirtying call"
    inst.take_path()


# ---- 1, 2, 6 -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", _q8.CASES, ids=_q8.CASE_IDS)
def test_leaves_truth_and_determinism(gpu, case):
    name, tr, R, C, nrhs, Z, G = case[:7]
    k = R if tr else C
    q, s, v = _q8.random_inputs(case)
    m, sc, vv, out = build_case(gpu, case, q, s, v)
    dirty_workspace(gpu, case, (m, sc, vv, out))  # (a cut case: NaN in every partial it should write)
    gpu.take_path()
    run(gpu, tr, G, out, m, sc, vv)
    path = gpu.take_path()
    print(name, "->", path)
    got = out.read(name)  # (out was NaN everywhere: overwritten inside the view, untouched outside)
    # 1: the leaf (the plan on the whole chip: tests/test_gemv_q8_plan_host.py pins the same tags on 256 CUs)
    tags = path.split(" ")
    assert all(t.startswith("gemv_q8/") for t in tags), path
    if gpu.adapter()["compute_units"] == 256:
        assert tags[0] == case[9], f"{name}: expected {case[9]}, the call took '{path}'"
    else:  # (a part with fewer CUs cuts the two *_split cases differently: the kernel and its tile are the same)
        assert tags[0].split(",ns=")[0] == case[9].split(",ns=")[0], f"{name}: expected {case[9]} up to the cut, the call took '{path}'"
    ns = int(tags[0].split("ns=")[1]) if "ns=" in tags[0] else 1
    assert tags[1:] == ([f"gemv_q8/combine,ns={ns}"] if ns > 1 else []), path
    if name.endswith("_split"):
        assert ns > 1, f"{name}: the contraction was not cut ({path})"
    # 2: the truth
    truth, sabs = _q8.truth64(q, s, v, G, tr)
    r = _q8.assert_within_gate(got, truth, k, sabs, name)
    print(f"  worst err / gate = {r:.3g}")
    # 6: the same bits again
    dirty_workspace(gpu, case, (m, sc, vv, out))
    out.poison()
    run(gpu, tr, G, out, m, sc, vv)
    U.assert_bits_equal(out.read(name), got, f"{name}: second call")


# ---- 3 -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", _q8.EXACT_CASES, ids=[c[0] for c in _q8.EXACT_CASES])
def test_exact_operands(gpu, case):
    """q over the full int8 range, integer v in [-4, 4], scales 2^-2 .. 2^2, k <= 2048: (max scale / min scale) * sum |q||v| < 2^24 (asserted), so every partial sum
    in any order and with the scale entering anywhere is exact: the result is fixed by construction."""
    name, tr, R, C, nrhs, Z, G = case[:7]
    q, s, v = _q8.exact_inputs(case)
    assert (q == -128).any() and _q8.exactness_condition(q, s, v, tr) < 2.0 ** 24
    m, sc, vv, out = build_case(gpu, case, q, s, v)
    dirty_workspace(gpu, case, (m, sc, vv, out))
    gpu.take_path()
    run(gpu, tr, G, out, m, sc, vv)
    assert (" gemv_q8/combine,ns=" in gpu.take_path()) == name.endswith("_split"), name
    truth, _ = _q8.truth64(q, s, v, G, tr)
    want = truth.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), truth)
    U.assert_same_class_bits(out.read(name), want, name)  # (zeros as one class: the sign of an exact zero sum is open)


@pytest.mark.parametrize("case", [c for c in _q8.CASES if c[0] in ("t_piece", "n_piece", "t_chunk_plus", "t4_chunk_plus", "any_t", "any_n")], ids=lambda c: c[0])
def test_subnormal_scale(gpu, case):
    """Every scale 2^-140: the results are 2^-140 times an integer -- exact f32 values, most of them subnormal. Nothing is flushed on the way."""
    name, tr, R, C, nrhs, Z, G = case[:7]
    q, s, v = _q8.exact_inputs(case, scale_exp=(-140, -140), salt=2)
    m, sc, vv, out = build_case(gpu, case, q, s, v)
    run(gpu, tr, G, out, m, sc, vv)
    truth, _ = _q8.truth64(q, s, v, G, tr)
    want = truth.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), truth)
    sub = (want != 0) & (np.abs(want) < np.float32(2.0 ** -126))
    assert sub.mean() > 0.25, f"{name}: only {sub.mean():.2f} of the results are subnormal (the case shows nothing)"
    U.assert_same_class_bits(out.read(name), want, name)


# ---- 4 -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr,R,C,nrhs,G", [(True, 1040, 24, 2, 16), (False, 1040, 40, 2, 128), (True, 4096, 8, 1, 128), (True, 528, 8200, 2, 48), (False, 48, 70, 3, 48)],
                         ids=["t", "n", "t_trip", "t_4cols", "n_small"])
def test_against_the_projects_own_kernels(gpu, tr, R, C, nrhs, G):
    """Power-of-two scales in [2^-2, 2^2] and |q| <= 127: the dequantised weight s q is an f16 value (7 bits times a power of two). wg_gemv_mixed on that f16 matrix
    and wg_gemv on the f32 one compute the same product with one rounding per term: each agrees with this call within the sum of the two gates."""
    wg, L = _wg(), _L()
    rng = np.random.default_rng(R + C)
    k, outs = (R, C) if tr else (C, R)
    q = rng.integers(-127, 128, (R, C, 1)).astype(np.int8)
    s = np.ldexp(np.float32(1), rng.integers(-2, 3, (_q8.n_groups(R, G), C, 1))).astype(np.float32)
    v = (rng.random((k, nrhs, 1), dtype=np.float32) * 2 - 1).astype(np.float32)
    W = wg.dequantize_q8(q, s, G)
    assert np.array_equal(W.astype(np.float16).astype(np.float32), W) and np.array_equal(W.astype(np.float64), _q8.dequantized64(q, s, G))
    truth, sabs = _q8.truth64(q, s, v, G, tr)
    m, sc, vv, out = Op(gpu, q, np.int8), Op(gpu, s), Op(gpu, v), Op(gpu, np.full((outs, nrhs, 1), NAN32))
    run(gpu, tr, G, out, m, sc, vv)
    got = out.read("q8").astype(np.float64)
    _q8.assert_within_gate(got, truth, k, sabs, "q8")
    variant = int(wg.GemvVariant.GemvTr if tr else wg.GemvVariant.Gemv)
    both = _q8.gate(k, sabs) + U.f32_gate(k, sabs)
    for fn, dt, wdt in (("wg_gemv_mixed", L.WG_F16, np.float16), ("wg_gemv", L.WG_F32, np.float32)):
        w = View(_raw(gpu, W[:, :, 0].ravel(order="F").astype(wdt)), wg.ViewShape((R, C, 1), R, R * C, 0))  # the dequantised matrix, dense
        o2 = Op(gpu, np.full((outs, nrhs, 1), NAN32))
        rc = getattr(L.lib, fn)(gpu._ctx.handle, variant, dt, o2.buf._h, o2.shape.to_c(), w.buf._h, w.shape.to_c(), vv.buf._h, vv.shape.to_c())
        assert rc == 0, L.lib.wg_last_error_string().decode()
        other = o2.read(fn).astype(np.float64)
        U.assert_close_f64(other, truth, k, sabs, fn)  # (the other call inside its own gate)
        err = np.abs(got - other)
        assert (err <= both).all(), f"{fn}: worst |q8 - other| / (gate + gate) = {(err / both).max():.3g}"


# ---- 5 -------------------------------------------------------------------------------------------------------------------------------------------------
SPECIAL = [c for c in _q8.CASES if c[0] in ("t_chunk_plus", "t_2mats", "t_8rhs", "t4_trips", "n_rows_plus", "n_2mats", "n_8rhs", "any_t", "any_n")]


@pytest.mark.parametrize("what", ["v_nan", "v_inf", "scale_nan", "scale_inf", "zero_scale_inf_v"])
@pytest.mark.parametrize("case", SPECIAL, ids=lambda c: c[0])
def test_special_values(gpu, case, what):
    """`out` starts as NaN and is overwritten. ONE special entry -- in v (right-hand side 1 of matrix 0) or in the scales (one group of one column of matrix 0) --
    reaches exactly the outputs whose sums contain it. Weights are nonzero and v is nonzero, so an Inf term is an Inf, never 0 * Inf, except where the case asks."""
    name, tr, R, C, nrhs, Z, G = case[:7]
    rng = _q8.rng_of(name, 5)
    k, outs = (R, C) if tr else (C, R)
    q = (rng.integers(1, 4, (R, C, Z)) * rng.choice([-1, 1], (R, C, Z))).astype(np.int8)
    s = np.ldexp(np.float32(1), rng.integers(-1, 2, (_q8.n_groups(R, G), C, Z))).astype(np.float32)
    v = (rng.integers(1, 4, (k, nrhs, Z)) * rng.choice([-1, 1], (k, nrhs, Z))).astype(np.float32)
    ng = _q8.n_groups(R, G)
    g0, c0, y0, k0 = ng - 1, C // 2, min(1, nrhs - 1), k - 1  # the last group (a partial one where the case has it), a middle column, the last contracted entry
    hit = np.zeros((outs, nrhs, Z), bool)      # outputs that must be non-finite
    nan_only = np.zeros((outs, nrhs, Z), bool)  # ... of which those that must be NaN
    rows_g0 = np.arange(R) // G == g0
    if what in ("v_nan", "v_inf"):
        v[k0, y0, 0] = np.nan if what == "v_nan" else np.inf
        hit[:, y0, 0] = True
        nan_only[:, y0, 0] = what == "v_nan"
    elif what in ("scale_nan", "scale_inf"):
        s[g0, c0, 0] = np.nan if what == "scale_nan" else np.inf
        if tr:
            hit[c0, :, 0] = True  # the column's dot product contains the group
        else:
            hit[rows_g0, :, 0] = True  # the rows of the group, through column c0
        nan_only[hit] = what == "scale_nan"
    else:  # a zero scale against an Inf in v: 0 * Inf = NaN where the two meet, +-Inf wherever another (nonzero) scale meets the Inf
        if tr:
            r0 = int(np.flatnonzero(rows_g0)[0])
            s[g0, c0, 0], v[r0, y0, 0] = 0, np.inf
            hit[:, y0, 0] = True
            nan_only[c0, y0, 0] = True
        else:
            s[g0, c0, 0], v[c0, y0, 0] = 0, np.inf
            hit[:, y0, 0] = True
            nan_only[rows_g0, y0, 0] = True
    m, sc, vv, out = build_case(gpu, case, q, s, v)
    run(gpu, tr, G, out, m, sc, vv)
    got = out.read(f"{name} {what}")
    assert np.isfinite(got[~hit]).all(), f"{name} {what}: {np.count_nonzero(~np.isfinite(got[~hit]))} outputs outside the special entry's reach are not finite"
    assert not np.isfinite(got[hit]).any(), f"{name} {what}: {np.count_nonzero(np.isfinite(got[hit]))} outputs the special entry reaches are finite"
    assert np.isnan(got[nan_only]).all(), f"{name} {what}: an output that must be NaN is {got[nan_only][~np.isnan(got[nan_only])][:1]}"
    if what in ("v_inf", "zero_scale_inf_v"):
        inf = hit & ~nan_only
        W = _q8.dequantized64(q, s, G)
        A = np.transpose(W, (1, 0, 2)) if tr else W
        kk = k0 if what == "v_inf" else (r0 if tr else c0)
        want_sign = np.sign(A[:, kk, 0])  # one Inf term per output: its sign is the weight's
        assert np.array_equal(np.sign(got[:, y0, 0][inf[:, y0, 0]]), want_sign[inf[:, y0, 0]]) and inf.any(), f"{name} {what}: the sign of an Inf"
    # the finite outputs are the exact product (small integers times powers of two)
    truth, _ = _q8.truth64(q, np.where(np.isfinite(s), s, 1), np.where(np.isfinite(v), v, 1), G, tr)
    assert np.array_equal(got[~hit].astype(np.float64), truth[~hit])


# ---- 7 -------------------------------------------------------------------------------------------------------------------------------------------------
def _raw(gpu, arr):
    """A buffer of exactly arr.nbytes bytes."""
    wg = _wg()
    arr = np.ascontiguousarray(arr)
    return wg.TensorBuilder.tensor((arr.size,), S_STORAGE).build_init(gpu.device(), arr, arr.dtype)


def test_status_codes(gpu):
    wg, L = _wg(), _L()
    V = wg.GemvVariant
    R, C, G = 64, 32, 16
    q = np.ones((R, C), np.int8)
    mb, sb, vb, ob, vtb, otb = (_raw(gpu, q.ravel()), _raw(gpu, np.ones(R // G * C, np.float32)), _raw(gpu, np.ones(C, np.float32)), _raw(gpu, np.zeros(R, np.float32)),
                                _raw(gpu, np.ones(R, np.float32)), _raw(gpu, np.zeros(C, np.float32)))
    sh = wg.ViewShape
    m, s, v, out = View(mb, sh((R, C, 1), R, R * C, 0)), View(sb, sh((R // G, C, 1), R // G, R // G * C, 0)), View(vb, sh((C, 1, 1), C, C, 0)), View(ob, sh((R, 1, 1), R, R, 0))
    vt, ot = View(vtb, sh((R, 1, 1), R, R, 0)), View(otb, sh((C, 1, 1), C, C, 0))
    gpu.take_path()
    # an m buffer sized in bytes is fine, for either variant
    rc, msg = call(gpu, False, G, out, m, s, v)
    assert rc == 0, msg
    assert np.array_equal(ob.read(gpu.device()), np.full(R, C, np.float32))
    assert call(gpu, True, G, ot, m, s, vt)[0] == 0 and np.array_equal(otb.read(gpu.device()), np.full(C, R, np.float32))
    assert gpu.take_path() != ""
    # group_rows
    for bad in (0, 8, 24, 63):
        rc, msg = call(gpu, False, bad, out, m, s, v)
        assert rc == L.WG_ERR_INVALID_ARG and msg == f"Gemv: group_rows {bad} is neither a positive multiple of 16 nor at least the {R} rows of m", (rc, msg)
    # the scales' shape: one row of scales short, a column short, one row for a per-column call is right
    rc, msg = call(gpu, False, G, out, m, View(sb, sh((R // G - 1, C, 1), R // G, R // G * C, 0)), v)
    assert rc == L.WG_ERR_DIM_MISMATCH and msg == f"Gemv: dimension mismatch. (m [{R},{C},1], group_rows {G}, scales [{R // G - 1},{C},1], expected [{R // G},{C},1])", (rc, msg)
    rc, msg = call(gpu, True, G, ot, m, View(sb, sh((R // G, C - 1, 1), R // G, R // G * C, 0)), vt)
    assert rc == L.WG_ERR_DIM_MISMATCH and f"scales [{R // G},{C - 1},1], expected [{R // G},{C},1]" in msg, (rc, msg)
    rc, msg = call(gpu, False, 32, out, m, s, v)  # (the scales of groups of 16 under groups of 32)
    assert rc == L.WG_ERR_DIM_MISMATCH and f"expected [{R // 32},{C},1]" in msg
    assert call(gpu, False, 1000, out, m, View(sb, sh((1, C, 1), 1, C, 0)), v)[0] == 0
    assert np.array_equal(ob.read(gpu.device()), np.full(R, C, np.float32))
    # wg_gemv's dimension check and message come first
    rc, msg = call(gpu, False, G, out, m, s, vt)
    assert rc == L.WG_ERR_DIM_MISMATCH and msg == f"Gemv: dimension mismatch. (out [{R},1,1], m [{R},{C},1], v [{R},1,1])", (rc, msg)
    rc, msg = call(gpu, True, 8, out, m, s, v)  # (before the group_rows check)
    assert rc == L.WG_ERR_DIM_MISMATCH and "]^T, v [" in msg
    # each operand out of bounds at its own element size
    rc, msg = call(gpu, False, G, out, View(_raw(gpu, q.ravel()[:-1]), m.shape), s, v)
    assert rc == L.WG_ERR_OUT_OF_BOUNDS and msg == f"Gemv: view `m` addresses {R * C} elements but its buffer holds {R * C - 1}", (rc, msg)
    rc, msg = call(gpu, False, G, out, m, View(_raw(gpu, np.ones(R // G * C - 1, np.float32)), s.shape), v)
    assert rc == L.WG_ERR_OUT_OF_BOUNDS and msg == f"Gemv: view `scales` addresses {R // G * C} elements but its buffer holds {R // G * C - 1}", (rc, msg)
    rc, msg = call(gpu, False, G, out, m, s, View(_raw(gpu, np.ones(C - 1, np.float32)), v.shape))
    assert rc == L.WG_ERR_OUT_OF_BOUNDS and msg == f"Gemv: view `v` addresses {C} elements but its buffer holds {C - 1}", (rc, msg)
    rc, msg = call(gpu, False, G, View(_raw(gpu, np.zeros(R, np.int8)), out.shape), m, s, v)  # an `out` sized as if it held bytes
    assert rc == L.WG_ERR_OUT_OF_BOUNDS and msg == f"Gemv: view `out` addresses {R} elements but its buffer holds {R // 4}", (rc, msg)
    # the Fast precondition, the silent fallback of GemvTrFast, the variant
    m6, s6 = View(_raw(gpu, np.ones(6 * 16, np.int8)), sh((6, 16, 1), 6, 96, 0)), View(_raw(gpu, np.ones(16, np.float32)), sh((1, 16, 1), 1, 16, 0))
    v16, o6 = View(_raw(gpu, np.ones(16, np.float32)), sh((16, 1, 1), 16, 16, 0)), View(_raw(gpu, np.zeros(6, np.float32)), sh((6, 1, 1), 6, 6, 0))
    rc, msg = call(gpu, False, 16, o6, m6, s6, v16, V.GemvFast)
    assert rc == L.WG_ERR_PRECONDITION and msg == "Gemv: assertion `left == right` failed (out_nrows % 4 == 0, gemv.rs:122): out has 6 rows", (rc, msg)
    m6t, s6t = View(m6.buf, sh((16, 6, 1), 16, 96, 0)), View(s6.buf, sh((1, 6, 1), 1, 6, 0))
    rc, msg = call(gpu, True, 16, o6, m6t, s6t, v16, V.GemvTrFast)  # 16 rows % 128 != 0: silently GemvTr, which takes 6 outputs
    assert rc == 0 and np.array_equal(o6.buf.read(gpu.device()), np.full(6, 16, np.float32)), (rc, msg)
    rc, msg = call(gpu, False, G, out, m, s, v, 7)
    assert rc == L.WG_ERR_INVALID_ARG and msg == "Gemv: unknown variant 7"
    # empty operands: WG_OK, nothing launched, nothing written
    before = ob.read(gpu.device()).copy()
    gpu.take_path()
    assert call(gpu, False, G, View(ob, sh((R, 0, 1), R, R, 0)), m, s, v)[0] == 0
    h0 = ctypes.c_void_p()
    L.check(L.lib.wg_buf_create(gpu._ctx.handle, 0, S_STORAGE, ctypes.byref(h0)))
    try:
        for which in range(4):
            hs = [h0 if i == which else b.buf._h for i, b in enumerate((out, m, s, v))]
            rc = L.lib.wg_gemv_q8(gpu._ctx.handle, 0, G, hs[0], out.shape.to_c(), hs[1], m.shape.to_c(), hs[2], s.shape.to_c(), hs[3], v.shape.to_c())
            assert rc == 0, (which, L.lib.wg_last_error_string().decode())
    finally:
        L.check(L.lib.wg_buf_destroy(h0))
    assert gpu.take_path() == "" and ob.read(gpu.device()).tobytes() == before.tobytes()
    # nmats * ceil(nrhs / 8) > 65535: wg_gemv_mixed's limit and message
    many = View(_raw(gpu, np.zeros(4 * 65536, np.float32)), sh((4, 1, 65536), 4, 4, 0))
    m4, s4, v4 = View(m6.buf, sh((16, 4, 1), 16, 0, 0)), View(s6.buf, sh((1, 4, 1), 1, 0, 0)), View(v16.buf, sh((16, 1, 1), 16, 0, 0))
    rc, msg = call(gpu, True, 16, many, m4, s4, v4)
    assert rc == L.WG_ERR_UNSUPPORTED and msg == "Gemv: nmats * ceil(nrhs/8) = 65536 exceeds 65535", (rc, msg)


def test_workspace_inside_a_recording():
    """The partials of a cut contraction live in the context's workspace: on a fresh context it cannot grow inside a recording (WG_ERR_WORKSPACE, as wg_gemv); after
    one eager call the same call records, and the replay has the eager bits."""
    wg, L = _wg(), _L()
    inst = wg.GpuInstance.new(0)
    try:
        case = [c for c in _q8.CASES if c[0] == "t_split"][0]
        q, s, v = _q8.exact_inputs(case, scale_exp=(0, 0))  # (k = 65536 with |q v| <= 512: below 2^25, not exact -- the replay is compared with the eager bits)
        m, sc, vv, out = build_case(inst, case, q, s, v)
        enc = inst.device().create_command_encoder(record=True)
        try:
            rc, msg = call(inst, True, case[6], out, m, sc, vv)
        finally:
            cb = enc.finish()
        assert rc == L.WG_ERR_WORKSPACE, (rc, msg)
        del cb
        run(inst, True, case[6], out, m, sc, vv)
        want = out.read()
        truth, sabs = _q8.truth64(q, s, v, case[6], True)
        _q8.assert_within_gate(want, truth, case[2], sabs, "eager")
        out.poison()
        enc = inst.device().create_command_encoder(record=True)
        try:
            rc, msg = call(inst, True, case[6], out, m, sc, vv)
        finally:
            cb = enc.finish()
        assert rc == 0, msg
        inst.queue().submit([cb])
        U.assert_bits_equal(out.read(), want, "cut contraction, replayed")
        del cb
    finally:
        inst.sync()


# ---- 8 -------------------------------------------------------------------------------------------------------------------------------------------------
def test_aliasing(gpu):
    """Decided on addresses, `out` (f32) against `m` (1 byte) in 1-byte units; nothing is launched, logged or written by a refused call."""
    wg, L = _wg(), _L()
    sh = wg.ViewShape
    rng = np.random.default_rng(31)
    R, C, G = 64, 256, 32
    q = rng.integers(-128, 128, (R, C, 1)).astype(np.int8)
    s = np.ldexp(np.float32(1), rng.integers(-2, 3, (R // G, C, 1))).astype(np.float32)
    v = rng.integers(-4, 5, (C, 1, 1)).astype(np.float32)
    truth = _q8.truth64(q, s, v, G, False)[0]
    sc, vv = Op(gpu, s), Op(gpu, v)
    # one buffer: R floats of `out` at byte 0, then the matrix from byte 4 R on
    raw = np.zeros(4 * R + R * C + 16, np.int8)
    raw[: 4 * R] = np.full(R, NAN32).view(np.int8)
    raw[4 * R: 4 * R + R * C] = q.ravel(order="F")
    buf = _raw(gpu, raw)
    o, mm = View(buf, sh((R, 1, 1), R, R, 0)), View(buf, sh((R, C, 1), R, R * C, 4 * R))  # the matrix begins exactly where out ends
    gpu.take_path()
    rc, msg = call(gpu, False, G, o, mm, sc, vv)
    assert rc == 0, msg
    after = buf.read(gpu.device())
    assert np.array_equal(after[: 4 * R].view(np.float32).astype(np.float64), truth.ravel()), "touching views: wrong result"
    assert np.array_equal(after[4 * R:], raw[4 * R:]), "touching views: the matrix changed"
    # the matrix one byte earlier: the last byte of out is shared -> refused, nothing written, nothing logged
    gpu.queue().write_buffer(buf, 0, raw)
    gpu.take_path()
    rc, msg = call(gpu, False, G, o, View(buf, sh((R, C, 1), R, R * C, 4 * R - 1)), sc, vv)
    assert rc == L.WG_ERR_ALIASED and msg == "Gemv: `out` overlaps `m` (the written view shares memory with a view the call reads)", (rc, msg)
    assert gpu.take_path() == "" and buf.read(gpu.device()).tobytes() == raw.tobytes()
    # ... and through a second handle over the same allocation that starts at the last byte of out
    base = L.lib.wg_buf_device_ptr(buf._h)
    h = ctypes.c_void_p()
    L.check(L.lib.wg_buf_wrap(gpu._ctx.handle, ctypes.c_void_p(base + 4 * R - 1), R * C, ctypes.byref(h)))
    try:
        rc = L.lib.wg_gemv_q8(gpu._ctx.handle, 0, G, buf._h, o.shape.to_c(), h, sh((R, C, 1), R, R * C, 0).to_c(), sc.buf._h, sc.shape.to_c(), vv.buf._h, vv.shape.to_c())
        assert rc == L.WG_ERR_ALIASED and "`out` overlaps `m`" in L.lib.wg_last_error_string().decode()
    finally:
        L.check(L.lib.wg_buf_destroy(h))
    assert gpu.take_path() == ""

    # out interleaved between the columns of a strided matrix (GemvTr): m is 16 x 8 bytes with leading dimension 48; the 32 bytes of padding behind column j are
    # 8 floats = out[:, j] for j < 3 (f32 offset 4 + 12 j)
    R2, C2, ld, nrhs = 16, 8, 48, 3
    q2 = rng.integers(-128, 128, (R2, C2, 1)).astype(np.int8)
    s2 = np.ldexp(np.float32(1), rng.integers(-2, 3, (1, C2, 1))).astype(np.float32)
    v2 = rng.integers(-4, 5, (R2, nrhs, 1)).astype(np.float32)
    raw2 = np.zeros(ld * C2 + 16, np.int8)
    midx = np.arange(R2)[:, None] + np.arange(C2)[None, :] * ld
    raw2[midx] = q2[:, :, 0]
    buf2 = _raw(gpu, raw2)
    sc2, vv2 = Op(gpu, s2), Op(gpu, v2)
    o2, m2 = View(buf2, sh((C2, nrhs, 1), ld // 4, 0, R2 // 4)), View(buf2, sh((R2, C2, 1), ld, 0, 0))
    rc, msg = call(gpu, True, 16, o2, m2, sc2, vv2)
    assert rc == 0, msg
    after2 = buf2.read(gpu.device())
    oidx = R2 // 4 + np.arange(C2)[:, None] + np.arange(nrhs)[None, :] * (ld // 4)
    assert np.array_equal(after2.view(np.float32)[oidx].astype(np.float64), _q8.truth64(q2, s2, v2, 16, True)[0][:, :, 0]), "interleaved views: wrong result"
    assert np.array_equal(after2[midx], raw2[midx]), "interleaved views: the matrix changed"
    o2.shape = sh((C2, nrhs, 1), ld // 4, 0, R2 // 4 - 1)  # one float earlier: the last four bytes of every column of m
    rc, msg = call(gpu, True, 16, o2, m2, sc2, vv2)
    assert rc == L.WG_ERR_ALIASED and "`out` overlaps `m`" in msg

    # out inside scales; out inside v
    R3, C3 = 32, 64
    m3 = Op(gpu, rng.integers(-3, 4, (R3, C3, 1)).astype(np.int8), np.int8)
    s3, v3 = Op(gpu, np.ones((2, C3, 1), np.float32)), Op(gpu, np.ones((C3, 3, 1), np.float32))
    before_s, before_v = s3.buf.read(gpu.device()).copy(), v3.buf.read(gpu.device()).copy()
    gpu.take_path()
    rc, msg = call(gpu, False, 16, View(s3.buf, sh((R3, 1, 1), R3, R3, 8)), m3, s3, View(v3.buf, sh((C3, 1, 1), C3, C3, 0)))
    assert rc == L.WG_ERR_ALIASED and msg == "Gemv: `out` overlaps `scales` (the written view shares memory with a view the call reads)", (rc, msg)
    rc, msg = call(gpu, False, 16, View(v3.buf, sh((R3, 2, 1), C3, 2 * C3, C3)), m3, s3, View(v3.buf, sh((C3, 2, 1), C3, 2 * C3, 0)))  # out in columns 1 .. 2 of v, v columns 0 .. 1
    assert rc == L.WG_ERR_ALIASED and msg == "Gemv: `out` overlaps `v` (the written view shares memory with a view the call reads)", (rc, msg)
    assert gpu.take_path() == "" and s3.buf.read(gpu.device()).tobytes() == before_s.tobytes() and v3.buf.read(gpu.device()).tobytes() == before_v.tobytes()

    # the read operands may overlap each other: the scales ARE the first bytes of the matrix (2^e as bytes: 0, 0, 0x80 or 0, 0x3f .. 0x40)
    R4, C4, G4 = 64, 16, 16
    sc4 = np.ldexp(np.float32(1), rng.integers(-2, 3, R4 // G4 * C4)).astype(np.float32)
    raw4 = rng.integers(-128, 128, R4 * C4).astype(np.int8)
    raw4[: sc4.nbytes] = sc4.view(np.int8)
    buf4 = _raw(gpu, raw4)
    q4, s4 = raw4.reshape(R4, C4, 1, order="F"), sc4.reshape(R4 // G4, C4, 1, order="F")
    v4 = rng.integers(-4, 5, (C4, 1, 1)).astype(np.float32)
    o4, vv4 = Op(gpu, np.full((R4, 1, 1), NAN32)), Op(gpu, v4)
    rc, msg = call(gpu, False, G4, o4, View(buf4, sh((R4, C4, 1), R4, R4 * C4, 0)), View(buf4, sh((R4 // G4, C4, 1), R4 // G4, R4 // G4 * C4, 0)), vv4)
    assert rc == 0, msg
    assert _q8.exactness_condition(q4, s4, v4, False) < 2.0 ** 24
    assert np.array_equal(o4.read("m over scales").astype(np.float64), _q8.truth64(q4, s4, v4, G4, False)[0])


# ---- 9 -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def masked():
    wg = _wg()
    inst = wg.GpuInstance.new(0, cu_count=248, one_xcd=True)
    yield inst
    inst.sync()


REPLAY = [c for c in _q8.CASES if c[0] in ("t_trips", "t_8rhs", "t_split", "t4_8rhs", "t4_split", "n_rows_plus", "n_split", "any_t", "any_n", "t_3rhs_split", "t_2mats_split",
                                           "t4_3rhs_split", "t4_2mats_split", "n_3rhs_split", "n_2mats_split")]


@pytest.mark.parametrize("where", ["whole", "masked"])
def test_recorded_and_masked(gpu, masked, where):
    """Eager, then recorded once and replayed twice into a re-poisoned output (a cut case: on a workspace dirtied before the eager call and before each replay): the
    eager bits each time. On the whole chip and on a CU-masked context (248 CUs: the
    plan reads the context's CU count), where the truth gate and determinism hold."""
    inst = gpu if where == "whole" else masked
    for case in REPLAY:
        name, tr, R, C, nrhs, Z, G = case[:7]
        q, s, v = _q8.random_inputs(case, salt=3)
        m, sc, vv, out = build_case(inst, case, q, s, v)
        dirty_workspace(inst, case, (m, sc, vv, out))
        inst.take_path()
        run(inst, tr, G, out, m, sc, vv)
        log = inst.take_path()
        assert (" gemv_q8/combine,ns=" in log) == name.endswith("_split"), (name, log)
        eager = out.read(name)
        truth, sabs = _q8.truth64(q, s, v, G, tr)
        _q8.assert_within_gate(eager, truth, R if tr else C, sabs, f"{name} {where}")
        out.poison()
        enc = inst.device().create_command_encoder(record=True)
        try:
            run(inst, tr, G, out, m, sc, vv)
        finally:
            cb = enc.finish()
        assert inst.take_path() == log
        for rep in range(2):
            dirty_workspace(inst, case, (m, sc, vv, out))
            out.poison()
            inst.queue().submit([cb])
            U.assert_bits_equal(out.read(name), eager, f"{name} {where}: replay {rep}")
        del cb


# ---- 10 ------------------------------------------------------------------------------------------------------------------------------------------------
def test_far_view(gpu):
    """An int8 matrix of 512 rows x 3 columns with leading dimension 2^31 + 16: the third column starts past 4 GiB of its parent. Only the columns are written (the
    parent is uninitialised). GemvTr and Gemv on exact operands, to the bit: a column offset formed in 32 bits reads the wrong bytes."""
    wg, L = _wg(), _L()
    R, C, G, ld = 512, 3, 128, 2 ** 31 + 16
    nbytes = -(-(2 * ld + R + 4096) // 65536) * 65536
    free, _ = gpu.mem_info()
    if free < nbytes + 2 * GiB:
        pytest.skip(f"{free / GiB:.1f} GiB of device memory free, the case needs {nbytes / GiB:.1f} + 2")
    case = ("far", True, R, C, 2, 1, G)
    q, s, _ = _q8.exact_inputs(case)
    big = wg.TensorBuilder.tensor((65536, nbytes // 65536), S_STORAGE).build(gpu.device(), np.int8)
    try:
        for c in range(C):
            col = np.ascontiguousarray(q[:, c, 0])
            L.check(L.lib.wg_buf_write(gpu._ctx.handle, big._h, c * ld, col.ctypes.data_as(ctypes.c_void_p), col.nbytes))
        m = View(big, wg.ViewShape((R, C, 1), ld, 2 ** 32 - 16, 0))
        sc = Op(gpu, s)
        for tr in (True, False):
            k, outs = (R, C) if tr else (C, R)
            v = _q8.rng_of("far", int(tr)).integers(-4, 5, (k, 2, 1)).astype(np.float32)
            assert _q8.exactness_condition(q, s, v, tr) < 2.0 ** 24
            vv, out = Op(gpu, v), Op(gpu, np.full((outs, 2, 1), NAN32))
            gpu.take_path()
            run(gpu, tr, G, out, m, sc, vv)
            assert gpu.take_path().startswith("gemv_q8/t," if tr else "gemv_q8/n,")
            truth, _ = _q8.truth64(q, s, v, G, tr)
            U.assert_same_class_bits(out.read("far"), truth.astype(np.float32), f"far view, {'GemvTr' if tr else 'Gemv'}")
    finally:
        gpu.sync()
        big.destroy()


# ---- 11 ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [32, 128, 4096])
def test_python_operators(gpu, G):
    """Gemv.dispatch_q8 / dispatch_q8_tr / dispatch_q8_generic on tensors, through a compute pass: a random f32 matrix quantised with quantize_q8, against the f64
    truth of the DEQUANTISED matrix within the gate of item 2; int8 tensors build, upload and read back."""
    wg = _wg()
    dev, shapes = gpu.device(), wg.ViewShapeBuffers()
    rng = np.random.default_rng(41 + G)
    R, C = 1040, 72
    w = rng.standard_normal((R, C)).astype(np.float32)
    q, s = wg.quantize_q8(w, G)
    tq = wg.TensorBuilder.matrix(R, C, S_STORAGE).build_init(dev, q)
    ts = wg.TensorBuilder.matrix(s.shape[0], C, S_STORAGE).build_init(dev, s)
    assert tq.dtype == np.int8 and np.array_equal(tq.read(dev), q.ravel(order="F"))
    op = wg.Gemv.from_device(dev)
    V = wg.GemvVariant
    for method, tr, extra in (("dispatch_q8", False, ()), ("dispatch_q8_tr", True, ()), ("dispatch_q8_generic", False, (V.Gemv,)), ("dispatch_q8_generic", True, (V.GemvTr,))):
        k, outs = (R, C) if tr else (C, R)
        v = (rng.random((k, 1, 1), dtype=np.float32) * 2 - 1).astype(np.float32)
        tv = wg.TensorBuilder.vector(k, S_STORAGE).build_init(dev, v.ravel())
        to = wg.TensorBuilder.vector(outs, S_STORAGE).build_init(dev, np.full(outs, NAN32))
        gpu.take_path()
        enc = dev.create_command_encoder()
        p = enc.compute_pass("q8", None)
        getattr(op, method)(dev, shapes, p, to, tq, ts, tv, G, *extra)
        p.end()
        gpu.queue().submit([enc.finish()])
        got = to.read(dev)
        assert gpu.take_path().startswith("gemv_q8/t," if tr else "gemv_q8/n,"), method
        truth, sabs = _q8.truth64(q[:, :, None], s[:, :, None], v, G, tr)
        _q8.assert_within_gate(got, truth, k, sabs, f"{method} G = {G}")
        # ... and the quantisation error itself is what it should be: each weight within s / 2, so the product within sum (s / 2) |v|
        W64 = _q8.dequantized64(q[:, :, None], s[:, :, None], G)[:, :, 0]
        A, Aw = (W64.T, w.T.astype(np.float64)) if tr else (W64, w.astype(np.float64))
        half = (s.astype(np.float64)[np.arange(R) // G] * (0.5 + 2.0 ** -16))
        bound = (half.T if tr else half) @ np.abs(v[:, 0, 0].astype(np.float64))
        assert (np.abs(A @ v[:, 0, 0].astype(np.float64) - Aw @ v[:, 0, 0].astype(np.float64)) <= bound + 1e-30).all()
