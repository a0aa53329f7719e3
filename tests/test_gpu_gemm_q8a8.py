"""wg_gemm_q8a8 on the GPU, through the C ABI: wg_gemm_q8's int8 matrix and f32 group scales against int8 columns with f32 group scales of their own on the i8 matrix
cores, f32 result. Before the feature the symbol did not exist.

The contract (include/wgebra_hip.h; restated in tests/_gemm_q8a8.py, whose model tests/test_gemm_q8a8_model.py checks on the CPU): integer chains of at most 1024
rows, exact; u = x_scale * (float)d, acc = fmaf(w_scale, u, acc), chains ascending; a cut adds f32 partials in a fixed order. The chains are integers, so the result
must EQUAL the float32 model to the bit: there is no tolerance. The shapes are the smallest at which the kernel can still go wrong.

  1  per case: the tags logged are the planner's for the query the call fills, the first one is the case's; random full-range operands equal the model (under the
     plan's cut) to the bit; `out` prefilled with NaN inside a guard pattern; two calls, identical bits                test_cases_equal_the_model
  2  the lane map on structured exact integer data, the identity and an asymmetric matrix as x                        test_lane_map
  3  power-of-two scales against the exact f64 truth, 2^-140 and subnormal results included                            test_power_of_two_scales, test_subnormal_scale
  4  agreement with wg_gemm_q8 on exact operands                                                                        test_agrees_with_gemm_q8
  5  Inf / NaN scales reach exactly the outputs whose chains hold them; 0 * Inf = NaN                                   test_non_finite_scales
  6  status codes and messages in the contract's order; aliasing on addresses                                           test_status_codes, test_aliasing
  7  WG_ERR_WORKSPACE inside a recording, success after wg_ctx_reserve_workspace; replayed = the eager bits             test_workspace_inside_a_recording
  8  the Python operators                                                                                               test_python_operators
  9  the cut contraction on GA.CUT_CASES (more than one matrix and pass, T = 2, strided `out`, odd / short / group-straddling splits, every threshold of the
     combine's two loops; chains of 1024 + 512 inside a split, G != Gx, one side grouped), each call on a workspace a NaN-scaled call of another shape has just
     filled: tags, the model's bits, the gate; exact operands; the lane map on 2 splits   test_cut_truth_on_a_dirty_workspace, test_cut_exact_operands, test_cut_lane_map
 10  the cut recorded and replayed on dirtied workspaces, on the whole chip and on contexts of 16 and 8 CUs (three different ns)   test_cut_recorded_and_masked
No test asserts a time.
"""
import ctypes
import faulthandler

import numpy as np
import pytest

import _gemm_q8a8 as GA
import _util as U

pytestmark = pytest.mark.gpu

S_STORAGE = 128 | 4 | 8
NAN32 = np.float32(np.nan)
POISON = {np.dtype(np.float32): NAN32, np.dtype(np.int8): np.int8(0x5A), np.dtype(np.uint16): np.uint16(0x7FC1)}


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
        self.init = np.full(self.size, POISON[self.dtype], dtype)
        self.init[self.idx] = vals
        self.buf = wg.TensorBuilder.tensor((self.size,), S_STORAGE).build_init(gpu.device(), self.init, self.init.dtype)
        self.shape = wg.ViewShape((R, C, Z), self.ld, self.batch, off)
        self.outside = np.ones(self.size, bool)
        self.outside[self.idx.ravel()] = False

    def poison(self):
        self.gpu.queue().write_buffer(self.buf, 0, self.init)

    def read(self, what=""):
        """The view's elements; asserts that the guard around them still holds its pattern (float32 operands: `out`)."""
        flat = self.buf.read(self.gpu.device())
        assert np.isnan(flat[self.outside]).all(), f"{what}: wrote outside the view"
        return np.ascontiguousarray(flat[self.idx])


class View:
    """A view of somebody else's buffer."""

    def __init__(self, buf, shape):
        self.buf, self.shape = buf, shape


def call(inst, G, Gx, out, m, s, x, xs, variant=None):
    """(status, message) of wg_gemm_q8a8."""
    wg, L = _wg(), _L()
    variant = int(wg.GemmVariant.GemmTr) if variant is None else int(variant)
    rc = L.lib.wg_gemm_q8a8(inst._ctx.handle, variant, int(G), int(Gx), out.buf._h, out.shape.to_c(), m.buf._h, m.shape.to_c(), s.buf._h, s.shape.to_c(), x.buf._h,
                            x.shape.to_c(), xs.buf._h, xs.shape.to_c())
    return rc, L.lib.wg_last_error_string().decode()


def run(inst, G, Gx, out, m, s, x, xs):
    rc, msg = call(inst, G, Gx, out, m, s, x, xs)
    assert rc == 0, msg


def build_case(gpu, c, q, s, x, xs):
    """The operands of a case on the device: the matrix and x at their byte offsets / paddings, both scales in views of their own that no kernel may assume dense,
    `out` at the case's offset and padding, NaN inside a NaN guard."""
    (moff, mpad, gap), (xoff, xpad), (ooff, opad, ogap) = c["m"], c["x"], GA.out_view(c)
    m = Op(gpu, q, np.int8, off=moff, pad=mpad, gap=gap)
    sc = Op(gpu, s, off=3, pad=1, gap=2)
    xx = Op(gpu, x, np.int8, off=xoff, pad=xpad)
    xsc = Op(gpu, xs, off=5, pad=2, gap=3)
    out = Op(gpu, np.full((c["outputs"], c["n"], c["Z"]), NAN32), off=ooff, pad=opad, gap=ogap)
    return m, sc, xx, xsc, out


def cus_of(inst):
    """The CU count the launcher plans with: a CU-masked context's own."""
    info = inst.adapter()
    return info.get("stream_compute_units", info["compute_units"])


def planned(gpu, c, m, sc, xx, xsc, out, cus=None):
    """wg_debug_gemm_q8a8_plan's (plan, tags) for the query the call fills: the views' own strides and addresses, the context's CU count (or `cus`)."""
    L = _L()
    q, p = L.GemmQ8A8QueryC(), L.GemmQ8A8PlanC()
    kw = dict(k=c["k"], outputs=c["outputs"], n=c["n"], mats=c["Z"], group_rows=c["G"], x_group_rows=c["Gx"], ldm=m.ld, lds=sc.ld, ldx=xx.ld, ldxs=xsc.ld, ldo=out.ld,
              m_batch=m.batch, s_batch=sc.batch, x_batch=xx.batch, xs_batch=xsc.batch, o_batch=out.batch, cus=cus or cus_of(gpu))
    for name, op, es in (("m_addr16", m, 1), ("x_addr16", xx, 1), ("o_addr16", out, 4)):
        kw[name] = (L.lib.wg_buf_device_ptr(op.buf._h) + es * op.shape.offset) % 16
    for key, v in kw.items():
        setattr(q, key, v)
    tags = ctypes.create_string_buffer(128)
    assert L.lib.wg_debug_gemm_q8a8_plan(ctypes.byref(q), ctypes.byref(p), tags, 128) == 0
    return p, tags.value.decode()


# ---- 1 -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GA.CASES, ids=GA.CASE_IDS)
def test_cases_equal_the_model(gpu, case):
    name, G, Gx = case["name"], case["G"], case["Gx"]
    q, s, x, xs = GA.random_inputs(case)
    m, sc, xx, xsc, out = build_case(gpu, case, q, s, x, xs)
    gpu.take_path()
    run(gpu, G, Gx, out, m, sc, xx, xsc)
    path = gpu.take_path()
    got = out.read(name)  # (no byte outside the view changed)
    print(name, "->", path)
    plan, tags = planned(gpu, case, m, sc, xx, xsc, out)
    assert path == tags, f"{name}: the call logged '{path}', the planner says '{tags}'"
    first = path.split(" ")[0]
    if gpu.adapter()["compute_units"] == 256:
        assert first == case["tag"], f"{name}: expected {case['tag']}, the call took '{path}'"
    else:  # (a part with fewer CUs cuts differently: the kernel and its tile are the same)
        assert first.split(",ns=")[0] == case["tag"].split(",ns=")[0], f"{name}: expected {case['tag']} up to the cut, the call took '{path}'"
    assert path.split(" ")[1:] == ([f"gemm_q8a8/combine,ns={plan.nsplit}"] if plan.nsplit > 1 else []), path
    if name == "cut":
        assert plan.nsplit > 1, f"the contraction was not cut ({path})"
    assert not np.isnan(got).any(), f"{name}: {np.isnan(got).sum()} elements of the view were not written"
    want = GA.model32(q, s, x, xs, G, Gx, plan.k_per_split if plan.nsplit > 1 else None)
    truth, sabs, nch = GA.truth64(q, s, x, xs, G, Gx)
    print(f"  worst |got - truth| / gate = {(np.abs(got - truth) / GA.gate(nch, sabs)).max():.3g}")
    U.assert_bits_equal(got, want, f"{name}: against the float32 model")
    out.poison()
    run(gpu, G, Gx, out, m, sc, xx, xsc)
    U.assert_bits_equal(out.read(name), got, f"{name}: second call")


# ---- 2 -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("identity", [True, False], ids=["identity", "asymmetric"])
def test_lane_map(gpu, identity):
    """Exact integer data (the kernel guide's check of an i8 operand map): with the identity as x the result is the scaled weight matrix itself; with an asymmetric
    x a row / column slip in the store, or a k permutation applied to one MFMA operand only, gives other integers."""
    case = GA.by_name("lane_map")
    q, s, x, xs = GA.lane_map_inputs(case, identity)
    m, sc, xx, xsc, out = build_case(gpu, case, q, s, x, xs)
    gpu.take_path()
    run(gpu, case["G"], case["Gx"], out, m, sc, xx, xsc)
    assert gpu.take_path().startswith("gemm_q8a8/mfma,")
    truth, _, _ = GA.truth64(q, s, x, xs, case["G"], case["Gx"])
    want = truth.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), truth)
    if identity:
        assert np.array_equal(truth[:, :, 0], (s[0, :, 0][:, None] * xs[0, :, 0][None, :]).astype(np.float64) * q[:32, :, 0].T)
    U.assert_same_class_bits(out.read("lane_map"), want, f"lane_map identity={identity}")


# ---- 3 -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [GA.by_name(n) for n in ("one_step", "cols_65", "any_g16")], ids=lambda c: c["name"])
def test_power_of_two_scales(gpu, case):
    """Scales 2^-2 and 2^2 on both sides, q over the full range, integer x in [-4, 4], k <= 64: (largest / smallest scale product) * sum |q||x| < 2^24 (asserted), so
    every partial sum is exact and the result is the f64 truth to the bit."""
    q, s, x, xs = GA.pow2_inputs(case)
    assert (q == -128).any() and (q == 127).any() and GA.exactness_condition(q, s, x, xs) < 2.0 ** 24
    m, sc, xx, xsc, out = build_case(gpu, case, q, s, x, xs)
    run(gpu, case["G"], case["Gx"], out, m, sc, xx, xsc)
    truth, _, _ = GA.truth64(q, s, x, xs, case["G"], case["Gx"])
    want = truth.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), truth)
    U.assert_same_class_bits(out.read(case["name"]), want, case["name"])


@pytest.mark.parametrize("case", [GA.by_name(n) for n in ("one_step", "groups_96", "two_mats", "any_m")], ids=lambda c: c["name"])
def test_subnormal_scale(gpu, case):
    """Every weight scale 2^-140, activation scales 1 and 2: the results are 2^-140 times an integer below 2^24 -- exact f32 values, most of them subnormal. The tiny
    scale enters last (fmaf(w_scale, x_scale * d, acc)): nothing is flushed or lost in an intermediate product."""
    q, s, x, xs = GA.pow2_inputs(case, w_exps=(-140,), x_exps=(0, 1), salt=2)
    assert GA.exactness_condition(q, s, x, xs) < 2.0 ** 24
    m, sc, xx, xsc, out = build_case(gpu, case, q, s, x, xs)
    run(gpu, case["G"], case["Gx"], out, m, sc, xx, xsc)
    truth, _, _ = GA.truth64(q, s, x, xs, case["G"], case["Gx"])
    want = truth.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), truth)
    sub = (want != 0) & (np.abs(want) < np.float32(2.0 ** -126))
    assert sub.mean() > 0.25, f"only {sub.mean():.2f} of the results are subnormal (the case shows nothing)"
    U.assert_same_class_bits(out.read(case["name"]), want, case["name"])


# ---- 4 -------------------------------------------------------------------------------------------------------------------------------------------------
def test_agrees_with_gemm_q8(gpu):
    """The same `m` and `scales` through wg_gemm_q8 with f16 columns equal to x_scales * x: on exact operands (power-of-two scales, small integers; the condition is
    asserted) both calls give the exact product, hence the same bits."""
    wg, L = _wg(), _L()
    case = GA.by_name("groups_64_128")
    q, s, x, xs = GA.pow2_inputs(case, w_exps=(-2, 0, 2), x_exps=(0, 1), salt=3)
    cols = (xs[np.arange(case["k"]) // case["Gx"]] * x.astype(np.float32)).astype(np.float32)  # |.| <= 8: f16 values
    assert GA.exactness_condition(q, s, x, xs) < 2.0 ** 24 and np.array_equal(cols.astype(np.float16).astype(np.float32), cols)
    m, sc, xx, xsc, out = build_case(gpu, case, q, s, x, xs)
    run(gpu, case["G"], case["Gx"], out, m, sc, xx, xsc)
    got = out.read("q8a8")
    x16 = Op(gpu, cols.astype(np.float16).view(np.uint16), np.uint16)
    out8 = Op(gpu, np.full(got.shape, NAN32))
    rc = L.lib.wg_gemm_q8(gpu._ctx.handle, int(wg.GemmVariant.GemmTr), case["G"], L.WG_F16, out8.buf._h, out8.shape.to_c(), m.buf._h, m.shape.to_c(), sc.buf._h,
                          sc.shape.to_c(), x16.buf._h, x16.shape.to_c())
    assert rc == 0, L.lib.wg_last_error_string().decode()
    U.assert_same_class_bits(got, out8.read("q8"), "wg_gemm_q8a8 against wg_gemm_q8")


# ---- 5 -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [GA.by_name(n) for n in ("groups_64_128", "cols_65", "any_g16_48")], ids=lambda c: c["name"])
def test_non_finite_scales(gpu, case):
    """An Inf weight scale (group g0 of output o0) and a NaN activation scale (group g1 of column n1) reach exactly row o0 and column n1 of `out`; a zero activation
    scale against the Inf (column n2, the x group that holds g0's rows) gives 0 * Inf = NaN. Everything else equals the model of the finite operands to the bit."""
    k, outs, n, G, Gx = case["k"], case["outputs"], case["n"], case["G"], case["Gx"]
    q, s, x, xs = GA.random_inputs(case, salt=5)
    q[q == 0], x[x == 0] = 1, 1
    s0, xs0 = s.copy(), xs.copy()
    o0, n1, n2 = outs // 2, n - 1, 0
    g0, g1 = s.shape[0] - 1, 0
    s[g0, o0, 0] = np.inf
    xs[g1, n1, 0] = np.nan
    xs[(g0 * min(G, k)) // min(Gx, k), n2, 0] = 0
    m, sc, xx, xsc, out = build_case(gpu, case, q, s, x, xs)
    run(gpu, G, Gx, out, m, sc, xx, xsc)
    got = out.read(case["name"])[:, :, 0]
    hit = np.zeros((outs, n), bool)
    hit[o0, :] = True
    hit[:, n1] = True
    assert np.isfinite(got[~hit]).all() and not np.isfinite(got[hit]).any(), "the non-finite scales reached other outputs than their own"
    assert np.isnan(got[:, n1]).all() and np.isnan(got[o0, n2]), "NaN scale / 0 * Inf"
    rest = [j for j in range(n) if j not in (n1, n2)]
    assert np.isinf(got[o0, rest]).all()
    want = GA.model32(q, s, x, xs, G, Gx)[:, :, 0]
    U.assert_same_class_bits(got, want, "against the model on the same scales")
    xs0[(g0 * min(G, k)) // min(Gx, k), n2, 0] = 0
    fin = GA.model32(q, s0, x, xs0, G, Gx)[:, :, 0]
    U.assert_bits_equal(got[~hit], fin[~hit], "the outputs no non-finite scale reaches")


# ---- 6 -------------------------------------------------------------------------------------------------------------------------------------------------
def _raw(gpu, arr):
    """A buffer of exactly arr.nbytes bytes."""
    wg = _wg()
    arr = np.ascontiguousarray(arr)
    return wg.TensorBuilder.tensor((arr.size,), S_STORAGE).build_init(gpu.device(), arr, arr.dtype)


def test_status_codes(gpu):
    wg, L = _wg(), _L()
    V, sh = wg.GemmVariant, wg.ViewShape
    K, O, N, G = 64, 32, 8, 32
    NG = K // G
    mb, sb = _raw(gpu, np.ones(K * O, np.int8)), _raw(gpu, np.ones(NG * O, np.float32))
    xb, xsb, ob = _raw(gpu, np.ones(K * N, np.int8)), _raw(gpu, np.ones(NG * N, np.float32)), _raw(gpu, np.zeros(O * N, np.float32))
    m, s = View(mb, sh((K, O, 1), K, K * O, 0)), View(sb, sh((NG, O, 1), NG, NG * O, 0))
    x, xs, out = View(xb, sh((K, N, 1), K, K * N, 0)), View(xsb, sh((NG, N, 1), NG, NG * N, 0)), View(ob, sh((O, N, 1), O, O * N, 0))
    gpu.take_path()
    for variant in (V.GemmTr, V.GemmTrFast):  # the same call
        gpu.queue().write_buffer(ob, 0, np.full(O * N, NAN32))
        rc, msg = call(gpu, G, G, out, m, s, x, xs, variant)
        assert rc == 0, msg
        assert np.array_equal(ob.read(gpu.device()), np.full(O * N, K, np.float32))
    assert gpu.take_path() == "gemm_q8a8/mfma,nt=2,ns=1 gemm_q8a8/mfma,nt=2,ns=1"
    # NULL context, NULL buffer, the variant's range
    a = (out.buf._h, out.shape.to_c(), m.buf._h, m.shape.to_c(), s.buf._h, s.shape.to_c(), x.buf._h, x.shape.to_c(), xs.buf._h, xs.shape.to_c())
    assert L.lib.wg_gemm_q8a8(None, 2, G, G, *a) == L.WG_ERR_INVALID_ARG and L.lib.wg_last_error_string() == b"Gemm: ctx is NULL"
    b = list(a)
    b[8] = None
    assert L.lib.wg_gemm_q8a8(gpu._ctx.handle, 2, G, G, *b) == L.WG_ERR_INVALID_ARG and L.lib.wg_last_error_string() == b"Gemm: buffer argument 4 is NULL"
    rc, msg = call(gpu, G, G, out, m, s, x, xs, 7)
    assert rc == L.WG_ERR_INVALID_ARG and msg == "Gemm: unknown variant 7", (rc, msg)
    # out = W x is not this call's -- before any dimension is looked at (a mismatched x)
    bad_x = View(xb, sh((K - 1, N, 1), K, K * N, 0))
    for variant in (V.Gemm, V.GemmFast):
        for xv in (x, bad_x):
            rc, msg = call(gpu, G, G, out, m, s, xv, xs, variant)
            assert rc == L.WG_ERR_UNSUPPORTED and "wg_gemv_q8" in msg and msg.startswith("Gemm: wg_gemm_q8a8 computes out = W^T x only"), (rc, msg)
    # the Gemm dimension check comes first, with its message -- before the group sizes
    rc, msg = call(gpu, 8, 8, out, m, s, bad_x, xs)
    assert rc == L.WG_ERR_DIM_MISMATCH and msg == f"Gemm: dimension mismatch. (out [{O},{N},1], m1 [{K},{O},1]^T, m2 [{K - 1},{N},1])", (rc, msg)
    for bad_out in (sh((O - 1, N, 1), O, O * N, 0), sh((O, N - 1, 1), O, O * N, 0), sh((O, N, 2), O, 0, 0)):
        assert call(gpu, G, G, View(ob, bad_out), m, s, x, xs)[0] == L.WG_ERR_DIM_MISMATCH
    # the group sizes
    for bad in (0, 8, 24, 63):
        rc, msg = call(gpu, bad, G, out, m, s, x, xs)
        assert rc == L.WG_ERR_INVALID_ARG and msg == f"Gemm: group_rows {bad} is neither a positive multiple of 16 nor at least the {K} rows of m", (rc, msg)
        rc, msg = call(gpu, G, bad, out, m, s, x, xs)
        assert rc == L.WG_ERR_INVALID_ARG and msg == f"Gemm: x_group_rows {bad} is neither a positive multiple of 16 nor at least the {K} rows of x", (rc, msg)
    rc, msg = call(gpu, 32, 48, out, m, s, x, xs)  # both below k, neither divides the other
    assert rc == L.WG_ERR_INVALID_ARG and "neither divides the other" in msg, (rc, msg)
    # the scales' shape, then the activation scales' shape
    rc, msg = call(gpu, G, G, out, m, View(sb, sh((NG - 1, O, 1), NG, NG * O, 0)), x, View(xsb, sh((NG - 1, N, 1), NG, NG * N, 0)))
    assert rc == L.WG_ERR_DIM_MISMATCH and msg == f"Gemm: dimension mismatch. (m [{K},{O},1], group_rows {G}, scales [{NG - 1},{O},1], expected [{NG},{O},1])", (rc, msg)
    rc, msg = call(gpu, G, G, out, m, s, x, View(xsb, sh((NG - 1, N, 1), NG, NG * N, 0)))
    assert rc == L.WG_ERR_DIM_MISMATCH and msg == f"Gemm: dimension mismatch. (x [{K},{N},1], x_group_rows {G}, x_scales [{NG - 1},{N},1], expected [{NG},{N},1])", (rc, msg)
    assert call(gpu, 1000, 2000, out, m, View(sb, sh((1, O, 1), 1, O, 0)), x, View(xsb, sh((1, N, 1), 1, N, 0)))[0] == 0  # one row of scales for a whole side
    # each operand out of bounds at its own element size
    for name, view, arr, have in (("m", m, np.ones(K * O - 1, np.int8), K * O - 1), ("scales", s, np.ones(NG * O - 1, np.float32), NG * O - 1),
                                  ("x", x, np.ones(K * N - 1, np.int8), K * N - 1), ("x_scales", xs, np.ones(NG * N - 1, np.float32), NG * N - 1),
                                  ("out", out, np.zeros(O * N, np.uint16), O * N // 2)):
        ops = dict(out=out, m=m, s=s, x=x, xs=xs)
        ops[{"scales": "s", "x_scales": "xs"}.get(name, name)] = View(_raw(gpu, arr), view.shape)
        rc, msg = call(gpu, G, G, ops["out"], ops["m"], ops["s"], ops["x"], ops["xs"])
        need = have + 1 if name != "out" else O * N
        assert rc == L.WG_ERR_OUT_OF_BOUNDS and msg == f"Gemm: view `{name}` addresses {need} elements but its buffer holds {have}", (name, rc, msg)
    # empty operands: WG_OK, nothing launched, nothing written
    before = ob.read(gpu.device()).copy()
    gpu.take_path()
    assert call(gpu, G, G, View(ob, sh((O, 0, 1), O, O * N, 0)), m, s, View(xb, sh((K, 0, 1), K, K * N, 0)), View(xsb, sh((NG, 0, 1), NG, NG * N, 0)))[0] == 0
    h0 = ctypes.c_void_p()
    L.check(L.lib.wg_buf_create(gpu._ctx.handle, 0, S_STORAGE, ctypes.byref(h0)))
    try:
        for which in range(5):
            c = list(a)
            c[2 * which] = h0
            rc = L.lib.wg_gemm_q8a8(gpu._ctx.handle, 2, G, G, *c)
            assert rc == 0, (which, L.lib.wg_last_error_string().decode())
    finally:
        L.check(L.lib.wg_buf_destroy(h0))
    assert gpu.take_path() == "" and ob.read(gpu.device()).tobytes() == before.tobytes()
    # k == 0: an empty sum, zeros
    gpu.queue().write_buffer(ob, 0, np.full(O * N, NAN32))
    rc, msg = call(gpu, G, G, out, View(mb, sh((0, O, 1), 16, 16 * O, 0)), View(sb, sh((0, O, 1), 1, O, 0)), View(xb, sh((0, N, 1), 16, 16 * N, 0)),
                   View(xsb, sh((0, N, 1), 1, N, 0)))
    assert rc == 0 and gpu.take_path() == "gemm_q8a8/any" and np.array_equal(ob.read(gpu.device()), np.zeros(O * N, np.float32)), (rc, msg)
    # mats * column passes past grid.z
    rc, msg = call(gpu, G, G, View(ob, sh((O, N, 70000), O, 0, 0)), View(mb, sh((K, O, 70000), K, 0, 0)), View(sb, sh((NG, O, 70000), NG, 0, 0)),
                   View(xb, sh((K, N, 70000), K, 0, 0)), View(xsb, sh((NG, N, 70000), NG, 0, 0)))
    assert rc in (L.WG_ERR_UNSUPPORTED, L.WG_ERR_ALIASED), (rc, msg)  # (a matrix stride of 0 on `out` would also be refused)


def test_aliasing(gpu):
    """Decided on addresses: `out` (f32) against `m` and `x` in 1-byte units, against both scales; nothing is launched, logged or written by a refused call. One
    buffer: out | scales | x_scales | m | x, touching."""
    wg, L = _wg(), _L()
    sh = wg.ViewShape
    K, O, N, G = 64, 16, 8, 32
    case = dict(name="alias", k=K, outputs=O, n=N, G=G, Gx=G, Z=1)
    q, s, x, xs = GA.pow2_inputs(case)
    want = GA.model32(q, s, x, xs, G, G)[:, :, 0]
    OUT, SC, XSC, M, X, END = 0, 512, 640, 704, 1728, 2240  # byte offsets
    raw = np.zeros(4096, np.uint8)
    raw[OUT:SC] = np.full(O * N, NAN32).view(np.uint8)
    raw[SC:XSC] = s[:, :, 0].ravel(order="F").view(np.uint8)
    raw[XSC:M] = xs[:, :, 0].ravel(order="F").view(np.uint8)
    raw[M:X] = q[:, :, 0].ravel(order="F").view(np.uint8)
    raw[X:END] = x[:, :, 0].ravel(order="F").view(np.uint8)
    buf = _raw(gpu, raw)
    out = lambda off: View(buf, sh((O, N, 1), O, O * N, off))  # noqa: E731  (off in floats)
    sc, xsc = View(buf, sh((2, O, 1), 2, 2 * O, SC // 4)), View(buf, sh((2, N, 1), 2, 2 * N, XSC // 4))
    m, xx = View(buf, sh((K, O, 1), K, K * O, M)), View(buf, sh((K, N, 1), K, K * N, X))
    gpu.take_path()
    rc, msg = call(gpu, G, G, out(0), m, sc, xx, xsc)  # touching
    assert rc == 0, msg
    assert gpu.take_path() == "gemm_q8a8/mfma,nt=2,ns=1"
    after = buf.read(gpu.device())
    U.assert_bits_equal(after[:512].view(np.float32).reshape(O, N, order="F"), want, "touching views")
    assert np.array_equal(after[512:], raw[512:]), "touching views: a read operand changed"
    rc, msg = call(gpu, G, G, out(END // 4), m, sc, xx, xsc)  # `out` directly behind x
    assert rc == 0, msg
    gpu.queue().write_buffer(buf, 0, raw)
    gpu.take_path()
    refused = [(out(1), m, sc, xx, xsc, "scales"),                                          # the last float of out is the first scale
               (out(0), View(buf, sh((K, O, 1), K, K * O, SC - 1)), View(buf, sh((2, O, 1), 2, 2 * O, 3000 // 4)), xx, xsc, "m"),  # m's first byte is out's last
               (out((X + K * N) // 4 - 1), m, sc, xx, xsc, "x"),                             # the first float of out is x's last four bytes
               (out(XSC // 4 - O * N + 1), m, View(buf, sh((2, O, 1), 2, 2 * O, 3000 // 4)), xx, xsc, "x_scales")]  # the last float of out is the first x scale
    for o_, m_, s_, x_, xs_, name in refused:
        rc, msg = call(gpu, G, G, o_, m_, s_, x_, xs_)
        assert rc == L.WG_ERR_ALIASED and msg == f"Gemm: `out` overlaps `{name}` (the written view shares memory with a view the call reads)", (name, rc, msg)
    assert gpu.take_path() == "" and buf.read(gpu.device()).tobytes() == raw.tobytes()
    # the read operands may overlap each other: x IS the first bytes of the matrix
    o2 = Op(gpu, np.full((O, N, 1), NAN32))
    rc, msg = call(gpu, G, G, o2, m, sc, View(buf, sh((K, N, 1), K, K * N, M)), xsc)
    assert rc == 0, msg
    U.assert_bits_equal(o2.read("x over m")[:, :, 0], GA.model32(q, s, q[:, :N], xs, G, G)[:, :, 0], "x over m")


# ---- 7 -------------------------------------------------------------------------------------------------------------------------------------------------
def test_workspace_inside_a_recording():
    """The partials of a cut contraction live in the context's workspace: on a fresh context it cannot grow inside a recording (WG_ERR_WORKSPACE); after
    wg_ctx_reserve_workspace the same call records, and the replay has the eager bits."""
    wg, L = _wg(), _L()
    inst = wg.GpuInstance.new(0)
    try:
        case = GA.by_name("chain_cap")
        q, s, x, xs = GA.random_inputs(case, salt=3)
        m, sc, xx, xsc, out = build_case(inst, case, q, s, x, xs)
        plan, _ = planned(inst, case, m, sc, xx, xsc, out)
        assert plan.nsplit > 1
        enc = inst.device().create_command_encoder(record=True)
        try:
            rc, msg = call(inst, case["G"], case["Gx"], out, m, sc, xx, xsc)
        finally:
            cb = enc.finish()
        assert rc == L.WG_ERR_WORKSPACE, (rc, msg)
        del cb
        inst.device().reserve_workspace(plan.workspace_bytes)
        enc = inst.device().create_command_encoder(record=True)
        try:
            rc, msg = call(inst, case["G"], case["Gx"], out, m, sc, xx, xsc)
        finally:
            cb = enc.finish()
        assert rc == 0, msg
        inst.queue().submit([cb])
        replayed = out.read("replayed")
        U.assert_bits_equal(replayed, GA.model32(q, s, x, xs, case["G"], case["Gx"], plan.k_per_split), "replayed against the model")
        out.poison()
        run(inst, case["G"], case["Gx"], out, m, sc, xx, xsc)
        U.assert_bits_equal(out.read("eager"), replayed, "cut contraction: eager against replayed")
        out.poison()
        inst.queue().submit([cb])
        U.assert_bits_equal(out.read("replayed again"), replayed, "cut contraction: second replay")
        del cb
    finally:
        inst.sync()


# ---- 8 -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,Gx", [(32, 32), (128, 4096), (4096, 4096)])
def test_python_operators(gpu, G, Gx):
    """Gemm.dispatch_q8a8_tr / dispatch_q8a8_generic on tensors, through a compute pass, on operands the NumPy quantize_q8 made: the model's bits."""
    wg = _wg()
    dev, shapes = gpu.device(), wg.ViewShapeBuffers()
    rng = np.random.default_rng(47 + G)
    K, O, N = 544, 72, 12
    q, s = wg.quantize_q8(rng.standard_normal((K, O)).astype(np.float32), G)
    x, xs = wg.quantize_q8(rng.standard_normal((K, N)).astype(np.float32), Gx)
    tq, ts = wg.TensorBuilder.matrix(K, O, S_STORAGE).build_init(dev, q), wg.TensorBuilder.matrix(s.shape[0], O, S_STORAGE).build_init(dev, s)
    tx, txs = wg.TensorBuilder.matrix(K, N, S_STORAGE).build_init(dev, x), wg.TensorBuilder.matrix(xs.shape[0], N, S_STORAGE).build_init(dev, xs)
    want = GA.model32(q[:, :, None], s[:, :, None], x[:, :, None], xs[:, :, None], G, Gx)[:, :, 0]
    op = wg.Gemm.from_device(dev)
    for method, extra in (("dispatch_q8a8_tr", ()), ("dispatch_q8a8_generic", (wg.GemmVariant.GemmTr,)), ("dispatch_q8a8_generic", (wg.GemmVariant.GemmTrFast,))):
        to = wg.TensorBuilder.matrix(O, N, S_STORAGE).build_init(dev, np.full((O, N), NAN32))
        gpu.take_path()
        enc = dev.create_command_encoder()
        p = enc.compute_pass("gemm_q8a8", None)
        getattr(op, method)(dev, shapes, p, to, tq, ts, tx, txs, G, Gx, *extra)
        p.end()
        gpu.queue().submit([enc.finish()])
        assert gpu.take_path() == "gemm_q8a8/mfma,nt=2,ns=1", method
        U.assert_bits_equal(to.read(dev).reshape(O, N, order="F"), want, f"{method} G = {G}, Gx = {Gx}")
    with pytest.raises(_L().WgError, match="wg_gemv_q8"):
        enc = dev.create_command_encoder()
        p = enc.compute_pass("gemm_q8a8", None)
        try:
            op.dispatch_q8a8_generic(dev, shapes, p, to, tq, ts, tx, txs, G, Gx, wg.GemmVariant.Gemm)  # out = W x: refused by the library
        finally:
            p.end()
            gpu.queue().submit([enc.finish()])


# ---- 9 -------------------------------------------------------------------------------------------------------------------------------------------------
_DIRTY, _SHARED = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _drop_shared():
    yield
    _DIRTY.clear()
    _SHARED.clear()


def shared(case, kind):
    """(q, s, x, xs, truth, sabs, chains) of a cut case, drawn and summed in float64 once for all the tests that use them (read-only)."""
    key = (case["name"], kind)
    if key not in _SHARED:
        ins = GA.random_inputs(case) if kind == "random" else GA.cut_pow2_inputs(case)
        truth, sabs, nch = GA.truth64(*ins, case["G"], case["Gx"])
        for a in ins + (truth, sabs):
            a.setflags(write=False)
        _SHARED[key] = ins + (truth, sabs, nch)
    return _SHARED[key]


def model_of(case, kps, kind="random"):
    """GA.model32 of the shared inputs under a cut of `kps` rows per split, once per cut."""
    key = (case["name"], kind, "model", kps)
    if key not in _SHARED:
        _SHARED[key] = GA.model32(*shared(case, kind)[:4], case["G"], case["Gx"], kps)
        _SHARED[key].setflags(write=False)
    return _SHARED[key]


def dirty_workspace(inst, plan, case):
    """One call on GA.DIRTY (k 4096, 256 outputs, 192 columns) whose weight scales are all NaN: every f32 partial it writes into the context's workspace is NaN, so a
    partial the next call fails to write shows in that call's result. Through the planner: the dirtying call is cut, and its workspace covers `plan`'s; its
    outputs x n is another one than the case's, so stale values cannot line up."""
    d = GA.DIRTY
    first = id(inst) not in _DIRTY
    if first:
        q, s, x, xs = GA.random_inputs(d, salt=9)
        _DIRTY[id(inst)] = (inst,) + build_case(inst, d, q, np.full_like(s, NAN32), x, xs)
    m, sc, xx, xsc, out = _DIRTY[id(inst)][1:]
    dplan, _ = planned(inst, d, m, sc, xx, xsc, out)
    assert dplan.nsplit > 1 and dplan.workspace_bytes >= plan.workspace_bytes > 0, (dplan.nsplit, dplan.workspace_bytes, plan.workspace_bytes)
    assert d["outputs"] * d["n"] != case["outputs"] * case["n"]
    run(inst, d["G"], d["Gx"], out, m, sc, xx, xsc)
    if first:
        assert np.isnan(out.read("dirty")).all(), "NaN scales did not reach every partial of the dirtying call"
    inst.take_path()


def assert_cut_tags(inst, case, path, plan, tags):
    """The logged tags are the planner's, the first is the case's (on 256 CUs; up to the cut elsewhere), the combine's tag follows; the ns logged."""
    assert path == tags, f"{case['name']}: the call logged '{path}', the planner says '{tags}'"
    first, want = path.split(" ")[0], case["tag"]
    if cus_of(inst) == 256:
        assert first == want, f"{case['name']}: expected {want}, the call took '{path}'"
    else:
        assert first.split(",ns=")[0] == want.split(",ns=")[0], f"{case['name']}: expected {want} up to the cut, the call took '{path}'"
    ns = int(first.split("ns=")[1])
    assert ns == plan.nsplit > 1 and path.split(" ")[1:] == [f"gemm_q8a8/combine,ns={ns}"], path
    return ns


@pytest.mark.parametrize("case", GA.CUT_CASES, ids=GA.CUT_IDS)
def test_cut_truth_on_a_dirty_workspace(gpu, case):
    """A cut contraction whose workspace holds NaN in every partial the call should write: tags, every element written, nothing outside, the gate (2 rounded terms per
    chain, not widened for the cut), the bits of the model under the plan's cut, and the same bits after dirtying again."""
    name, G, Gx = case["name"], case["G"], case["Gx"]
    q, s, x, xs, truth, sabs, nch = shared(case, "random")
    m, sc, xx, xsc, out = build_case(gpu, case, q, s, x, xs)
    plan, tags = planned(gpu, case, m, sc, xx, xsc, out)
    dirty_workspace(gpu, plan, case)
    run(gpu, G, Gx, out, m, sc, xx, xsc)
    path = gpu.take_path()
    got = out.read(name)  # (no byte outside the view changed)
    ns = assert_cut_tags(gpu, case, path, plan, tags)
    print(f"{name} -> {path}: ns {ns} x {plan.k_per_split} rows")
    assert not np.isnan(got).any(), f"{name}: {np.isnan(got).sum()} elements of the view are NaN: not written, or summed from a partial the call did not write"
    err, tol = np.abs(got.astype(np.float64) - truth), GA.gate(nch, sabs)
    print(f"  worst |got - truth| / gate = {(err / tol).max():.3g}")
    assert (err <= tol).all(), f"{name}: {(err > tol).sum()} elements outside gate({nch} chains); worst err / gate = {(err / tol).max():.3g}"
    U.assert_bits_equal(got, model_of(case, plan.k_per_split), f"{name}: against the float32 model")
    dirty_workspace(gpu, plan, case)
    out.poison()
    run(gpu, G, Gx, out, m, sc, xx, xsc)
    U.assert_bits_equal(out.read(name), got, f"{name}: second call")


@pytest.mark.parametrize("case", GA.CUT_CASES, ids=GA.CUT_IDS)
def test_cut_exact_operands(gpu, case):
    """Exact operands under a cut (GA.cut_pow2_inputs: x in {-1, 0, 1}, scales 2^0 and 2^1 on both sides; the condition is asserted): every partial sum in any order is
    exact, so the result is fixed by construction -- the float64 truth, which is also the model's bits. A dropped, doubled or misplaced split gives other integers."""
    name = case["name"]
    q, s, x, xs, truth, _, _ = shared(case, "exact")
    assert (q == -128).any() and (q == 127).any() and GA.exactness_condition(q, s, x, xs) < 2.0 ** 24
    m, sc, xx, xsc, out = build_case(gpu, case, q, s, x, xs)
    plan, tags = planned(gpu, case, m, sc, xx, xsc, out)
    dirty_workspace(gpu, plan, case)
    run(gpu, case["G"], case["Gx"], out, m, sc, xx, xsc)
    assert_cut_tags(gpu, case, gpu.take_path(), plan, tags)
    want = truth.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), truth)
    got = out.read(name)
    U.assert_same_class_bits(got, want, name)
    U.assert_same_class_bits(got, model_of(case, plan.k_per_split, "exact"), f"{name}: against the float32 model")


def test_cut_lane_map(gpu):
    """test_lane_map's asymmetric operands, x narrowed to [-4, 4] for the sum bound at this k (asserted), on 2 splits of 544 rows: a k permutation applied to one
    operand in the second split only, or a row / column slip in the partials, gives other integers."""
    case = GA.CUT_LANE_MAP
    q, s, x, xs = GA.cut_lane_map_inputs(case)
    assert GA.exactness_condition(q, s, x, xs) < 2.0 ** 24
    m, sc, xx, xsc, out = build_case(gpu, case, q, s, x, xs)
    plan, tags = planned(gpu, case, m, sc, xx, xsc, out)
    dirty_workspace(gpu, plan, case)
    run(gpu, case["G"], case["Gx"], out, m, sc, xx, xsc)
    assert_cut_tags(gpu, case, gpu.take_path(), plan, tags)
    truth, _, _ = GA.truth64(q, s, x, xs, case["G"], case["Gx"])
    want = truth.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), truth)
    U.assert_same_class_bits(out.read("cut_lane_map"), want, "cut_lane_map")


# ---- 10 ------------------------------------------------------------------------------------------------------------------------------------------------
SMALL = {"cus16": 16, "cus8": 8}


@pytest.fixture(scope="module")
def small():
    wg = _wg()
    made = {where: wg.GpuInstance.new(0, cu_count=n) for where, n in SMALL.items()}
    yield made
    for inst in made.values():
        inst.sync()


@pytest.mark.parametrize("where", ["whole", "cus16", "cus8"])
def test_cut_recorded_and_masked(gpu, small, where):
    """The cut on the whole chip and on contexts of 16 and 8 CUs (want_blocks = 4 x CUs decides ns): eagerly on a dirtied workspace -- the planner's tags for that CU
    count, the gate, the model's bits under that context's cut -- then recorded once and replayed twice, the workspace dirtied and `out` poisoned before each replay:
    the eager bits. cut_masked is cut differently on each of the three contexts, and on exact operands gives the same bits on all of them (the truth's)."""
    inst = gpu if where == "whole" else small[where]
    cus = dict(SMALL, whole=cus_of(gpu))
    assert cus_of(inst) == cus[where]
    for name in ("cut_masked", "cut_g96_partial", "cut_passes"):
        case = GA.by_name(name)
        G, Gx = case["G"], case["Gx"]
        q, s, x, xs, truth, sabs, nch = shared(case, "random")
        m, sc, xx, xsc, out = build_case(inst, case, q, s, x, xs)
        plan, tags = planned(inst, case, m, sc, xx, xsc, out)
        dirty_workspace(inst, plan, case)
        run(inst, G, Gx, out, m, sc, xx, xsc)
        log = inst.take_path()
        assert_cut_tags(inst, case, log, plan, tags)
        print(f"{name} {where} -> {log}: {plan.k_per_split} rows per split")
        if name == "cut_masked":
            ns = {w: planned(inst, case, m, sc, xx, xsc, out, cus=n)[0].nsplit for w, n in cus.items()}
            assert len(set(ns.values())) == 3 and plan.nsplit == ns[where], ns
            assert cus["whole"] != 256 or ns == {"whole": 8, "cus16": 6, "cus8": 3}, ns
        eager = out.read(name)
        assert not np.isnan(eager).any()
        assert (np.abs(eager.astype(np.float64) - truth) <= GA.gate(nch, sabs)).all(), f"{name} {where}: outside the gate"
        U.assert_bits_equal(eager, model_of(case, plan.k_per_split), f"{name} {where}: against the float32 model")
        inst.device().reserve_workspace(plan.workspace_bytes)
        out.poison()
        enc = inst.device().create_command_encoder(record=True)
        try:
            run(inst, G, Gx, out, m, sc, xx, xsc)
        finally:
            cb = enc.finish()
        assert inst.take_path() == log
        for rep in range(2):
            dirty_workspace(inst, plan, case)
            out.poison()
            inst.queue().submit([cb])
            U.assert_bits_equal(out.read(name), eager, f"{name} {where}: replay {rep}")
        del cb
        if name == "cut_masked":  # exact operands: the same bits whatever the cut
            q, s, x, xs, truth, _, _ = shared(case, "exact")
            assert GA.exactness_condition(q, s, x, xs) < 2.0 ** 24
            m, sc, xx, xsc, out = build_case(inst, case, q, s, x, xs)
            dirty_workspace(inst, plan, case)
            run(inst, G, Gx, out, m, sc, xx, xsc)
            assert inst.take_path() == log
            U.assert_same_class_bits(out.read(name), truth.astype(np.float32), f"{name} {where}: exact operands")
