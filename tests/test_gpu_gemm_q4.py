"""wg_gemm_q4 on the GPU, through the C ABI: wg_gemv_q4's packed 4-bit matrix and f32 group scales against f16 / bf16 columns on the matrix cores, f32 result. Before
the feature the symbol did not exist.

The contract (include/wgebra_hip.h): out = W^T x, W[r, c] = scales[r // G, c] * q[r, c], byte j of a column = rows 2 j (low nibble) and 2 j + 1 (high nibble), q = n - 8
formed exactly in the 16-bit type; every product exact in f32, per group d = the MFMA chain from zero, acc = fmaf(s, d, acc); nothing narrowed, the accumulator stored
as it is; deterministic. Cases and inputs are tests/_gemm_q4.py's, packing, truth and gate tests/_q4.py's (tests/test_gemm_q4_model.py checks them on the CPU). The
shapes are the smallest at which the kernel can still go wrong; the plan's step is 32 rows.

  1  per case and element type: the first tag logged is the planner's for the query the call fills; random inputs inside _q4.gate; `m`'s padding bytes, x's padding
     (NaN patterns) and `out` (NaN inside a NaN guard) poisoned -- every element of the view overwritten, no byte outside it changed; two calls, identical bits
                                                                                                                           test_leaves_truth_and_determinism
  2  exact operands to the bit on every case (the cut one with scales 2^0 .. 2^1): against the float64 truth, against wg_gemm_q4 on the unpacked int8 with the same
     scales and x buffers, against wg_gemv_q4 on the same m and scales (N <= 8); nibble order and lane map                  test_exact_operands, test_identity, test_lane_map
  3  scale 2^-140: exact subnormal results; Inf in x against a nibble of 8 / a zero scale                                  test_subnormal_scale, test_inf_*
  4  status codes and messages                                                                                             test_status_codes
  5  aliasing, on addresses                                                                                                test_aliasing
  6  WG_ERR_WORKSPACE inside a recording, success after wg_ctx_reserve_workspace; recorded + replayed = the eager bits, for a cut and for an element-by-element call
                                                                                                                           test_workspace_inside_a_recording, test_replay_any
  7  the Python operators with quantize_q4                                                                                 test_python_operators
  8  the cut contraction on GQ.CUT_CASES (splits of 17 steps: half a double step in the middle of k, a split that starts at byte 16 mod 32; more than one matrix and
     pass, T = 2, strided `out`, short / group-straddling splits, every threshold of the combine's two loops), each call on a workspace a NaN-scaled call of another
     shape has just filled: tags, truth, bits; exact operands; the lane map on 2 splits           test_cut_truth_on_a_dirty_workspace, test_cut_exact_operands, test_cut_lane_map
  9  the cut recorded and replayed on dirtied workspaces, on the whole chip and on contexts of 16 and 8 CUs (three different ns)   test_cut_recorded_and_masked
No test asserts a time.
"""
import ctypes
import faulthandler

import numpy as np
import pytest

import _gemm_q4 as GQ
import _q4
import _util as U

pytestmark = pytest.mark.gpu

S_STORAGE = 128 | 4 | 8
NAN32 = np.float32(np.nan)
POISON = {np.dtype(np.float32): NAN32, np.dtype(np.int8): np.int8(0x5A), np.dtype(np.uint8): np.uint8(0x5A), np.dtype(np.uint16): np.uint16(0x7FC1)}  # (0x7FC1: a NaN in f16 and in bf16)


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
    """X[r, c, z] stored column-major at element `off` with leading dimension r + pad and `gap` elements between matrices, in a poisoned parent: NaN for float32 and
    for the 16-bit patterns, the sentinel byte 0x5A for the packed bytes and for int8."""

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


def dtype_of(dt):
    return _L().WG_F16 if dt == "f16" else _L().WG_BF16


def call(inst, G, dt, out, m, s, x, variant=None):
    """(status, message) of wg_gemm_q4."""
    wg, L = _wg(), _L()
    variant = int(wg.GemmVariant.GemmTr) if variant is None else int(variant)
    xd = dtype_of(dt) if isinstance(dt, str) else int(dt)
    rc = L.lib.wg_gemm_q4(inst._ctx.handle, variant, int(G), xd, out.buf._h, out.shape.to_c(), m.buf._h, m.shape.to_c(), s.buf._h, s.shape.to_c(), x.buf._h, x.shape.to_c())
    return rc, L.lib.wg_last_error_string().decode()


def call_q8(inst, G, dt, out, m8, s, x):
    """(status, message) of wg_gemm_q8 on the unpacked int8 matrix."""
    wg, L = _wg(), _L()
    rc = L.lib.wg_gemm_q8(inst._ctx.handle, int(wg.GemmVariant.GemmTr), int(G), dtype_of(dt), out.buf._h, out.shape.to_c(), m8.buf._h, m8.shape.to_c(), s.buf._h, s.shape.to_c(),
                          x.buf._h, x.shape.to_c())
    return rc, L.lib.wg_last_error_string().decode()


def call_gemv_q4(inst, G, out, m, s, v):
    """(status, message) of wg_gemv_q4 on the same packed matrix and scales, f32 right-hand sides."""
    wg, L = _wg(), _L()
    rc = L.lib.wg_gemv_q4(inst._ctx.handle, int(wg.GemvVariant.GemvTr), int(G), out.buf._h, out.shape.to_c(), m.buf._h, m.shape.to_c(), s.buf._h, s.shape.to_c(), v.buf._h,
                          v.shape.to_c())
    return rc, L.lib.wg_last_error_string().decode()


def run(inst, G, dt, out, m, s, x):
    rc, msg = call(inst, G, dt, out, m, s, x)
    assert rc == 0, msg


def build_case(gpu, c, dt, q, s, x):
    """The operands of a case on the device: the packed matrix (_q4.pack of q) at its byte offset / padding / gap, the scales in a view of their own that no kernel may assume dense (offset
    3, leading dimension + 1, gap 2), x and out at the case's offsets and paddings; `out` starts as NaN inside a NaN guard."""
    (moff, mpad, gap), (xoff, xpad), (ooff, opad, ogap) = c["m"], c["x"], GQ.out_view(c)
    m = Op(gpu, _q4.pack(q), np.uint8, off=moff, pad=mpad, gap=gap)
    sc = Op(gpu, s, off=3, pad=1, gap=2)
    xx = Op(gpu, GQ.bits16(dt, x), np.uint16, off=xoff, pad=xpad)
    out = Op(gpu, np.full((c["outputs"], c["n"], c["Z"]), NAN32), off=ooff, pad=opad, gap=ogap)
    return m, sc, xx, out


def planned_tags(gpu, c, dt, m, sc, xx, out):
    """wg_debug_gemm_q4_plan's tags for the query the call fills: the views' own strides and addresses, the context's CU count."""
    return planned(gpu, c, dt, m, sc, xx, out)[1]


def cus_of(inst):
    """The CU count the launcher plans with: a CU-masked context's own."""
    info = inst.adapter()
    return info.get("stream_compute_units", info["compute_units"])


def planned(gpu, c, dt, m, sc, xx, out, cus=None):
    """(plan, tags) of wg_debug_gemm_q4_plan for the query the call fills; `cus`: another CU count than the context's."""
    L = _L()
    q, p = L.GemmQ4QueryC(), L.GemmQ4PlanC()
    kw = dict(k=c["k"], outputs=c["outputs"], n=c["n"], mats=c["Z"], group_rows=c["G"], x_bf16=int(dt == "bf16"), ldm=m.ld, lds=sc.ld, ldx=xx.ld, ldo=out.ld, m_batch=m.batch,
              s_batch=sc.batch, x_batch=xx.batch, o_batch=out.batch, cus=cus or cus_of(gpu))
    for name, op, es in (("m_addr16", m, 1), ("x_addr16", xx, 2), ("o_addr16", out, 4)):
        kw[name] = (L.lib.wg_buf_device_ptr(op.buf._h) + es * op.shape.offset) % 16
    for key, v in kw.items():
        setattr(q, key, v)
    tags = ctypes.create_string_buffer(128)
    assert L.lib.wg_debug_gemm_q4_plan(ctypes.byref(q), ctypes.byref(p), tags, 128) == 0
    return p, tags.value.decode()


# ---- 1 -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", GQ.DTYPES)
@pytest.mark.parametrize("case", GQ.CASES, ids=GQ.CASE_IDS)
def test_leaves_truth_and_determinism(gpu, case, dt):
    name, k, G = case["name"], case["k"], case["G"]
    q, s, x = GQ.random_inputs(case, dt)
    m, sc, xx, out = build_case(gpu, case, dt, q, s, x)
    gpu.take_path()
    run(gpu, G, dt, out, m, sc, xx)
    path = gpu.take_path()
    got = out.read(name)  # (no byte outside the view changed)
    print(name, dt, "->", path)
    # the leaf: what the launcher logged is what the planner says for the query the call filled -- a planner / launcher divergence fails here
    assert path == planned_tags(gpu, case, dt, m, sc, xx, out), f"{name}: the call logged '{path}'"
    tags = path.split(" ")
    want = case["tag"].format(dt=dt)
    if gpu.adapter()["compute_units"] == 256:
        assert tags[0] == want, f"{name}: expected {want}, the call took '{path}'"
    else:  # (a part with fewer CUs cuts differently: the kernel and its tile are the same)
        assert tags[0].split(",ns=")[0] == want.split(",ns=")[0], f"{name}: expected {want} up to the cut, the call took '{path}'"
    ns = int(tags[0].split("ns=")[1]) if "ns=" in tags[0] else 1
    assert tags[1:] == ([f"gemm_q4/combine,ns={ns}"] if ns > 1 else []), path
    if name == "cut":
        assert ns > 1, f"the contraction was not cut ({path})"
    # every element of the view overwritten
    assert not np.isnan(got).any(), f"{name}: {np.isnan(got).sum()} elements of the view were not written"
    # the truth
    truth, sabs = GQ.truth64(q, s, x, G)
    r = _q4.assert_within_gate(got, truth, k, sabs, f"{name} {dt}")
    print(f"  worst err / gate = {r:.3g}")
    # the same bits again
    out.poison()
    run(gpu, G, dt, out, m, sc, xx)
    U.assert_bits_equal(out.read(name), got, f"{name} {dt}: second call")


# ---- 2 -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", GQ.DTYPES)
@pytest.mark.parametrize("case", GQ.EXACT_CASES, ids=[c["name"] for c in GQ.EXACT_CASES])
def test_exact_operands(gpu, case, dt):
    """q over all 16 values with -8 and 7 planted in even and in odd rows, integer x in [-4, 4], scales 2^-2 .. 2^2 (2^0 .. 2^1 on the cut case):
    (max scale / min scale) * sum |q||x| < 2^24 (asserted), so every partial sum in any order is exact: the result is fixed by construction -- the float64 truth,
    wg_gemm_q8 on the unpacked int8 (same scales and x buffers) and wg_gemv_q4 on the same m and scales (x widened to f32, N <= 8) give the same bits."""
    name, G = case["name"], case["G"]
    q, s, x = GQ.exact_inputs(case, dt)
    assert (q[0::2] == -8).any() and (q[1::2] == -8).any() and (q[0::2] == 7).any() and (q[1::2] == 7).any() and _q4.exactness_condition(q, s, x) < 2.0 ** 24
    m, sc, xx, out = build_case(gpu, case, dt, q, s, x)
    run(gpu, G, dt, out, m, sc, xx)
    truth, _ = GQ.truth64(q, s, x, G)
    want = truth.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), truth)
    got = out.read(name)
    U.assert_same_class_bits(got, want, f"{name} {dt}")  # (zeros as one class: the sign of an exact zero sum is open)
    # wg_gemm_q8 on _q4.unpack of the same bytes, the same scales and x buffers
    m8 = Op(gpu, _q4.unpack(_q4.pack(q)), np.int8)
    out8 = Op(gpu, np.full(got.shape, NAN32))
    rc, msg = call_q8(gpu, G, dt, out8, m8, sc, xx)
    assert rc == 0, msg
    U.assert_same_class_bits(out8.read(name + " q8"), got, f"{name} {dt}: wg_gemm_q8 on the unpacked int8")
    if case["n"] <= 8:  # wg_gemv_q4 on the same m and scales
        v = Op(gpu, x)
        outv = Op(gpu, np.full(got.shape, NAN32))
        rc, msg = call_gemv_q4(gpu, G, outv, m, sc, v)
        assert rc == 0, msg
        U.assert_same_class_bits(outv.read(name + " gemv_q4"), got, f"{name} {dt}: wg_gemv_q4 on the same m and scales")


@pytest.mark.parametrize("dt", GQ.DTYPES)
def test_identity(gpu, dt):
    """Nibble order and lane map: N = k and x the identity, so out[o, r] = s[r // G, o] * q[r, o] for every r, to the bit -- a swapped nibble, a permutation applied
    to one operand only or a crossed half-wave exchange puts a weight into another column."""
    case = GQ.IDENTITY
    k, outs, G = case["k"], case["outputs"], case["G"]
    rng = _q4.rng_of("identity", 7)
    q = rng.integers(-8, 8, (k, outs, 1), dtype=np.int8)
    q[:16, 0, 0] = np.arange(-8, 8)  # every nibble value, in both positions
    q[16:32, 1, 0] = np.arange(-8, 8)[::-1]
    s = np.ldexp(np.float32(1), rng.integers(-3, 4, (_q4.n_groups(k, G), outs, 1))).astype(np.float32)
    x = np.eye(k, dtype=np.float32)[:, :, None]
    m, sc, xx, out = build_case(gpu, case, dt, q, s, x)
    gpu.take_path()
    run(gpu, G, dt, out, m, sc, xx)
    assert gpu.take_path() == case["tag"].format(dt=dt)
    want = (s[np.arange(k) // G, :, 0] * q[:, :, 0].astype(np.float32)).T  # [outputs, k]
    got = out.read("identity")[:, :, 0]
    wrong = np.argwhere(got != want)
    assert wrong.size == 0, f"identity {dt}: {len(wrong)} wrong elements, first (output, row) = {tuple(wrong[0])}: got {got[tuple(wrong[0])]}, expected {want[tuple(wrong[0])]}"


@pytest.mark.parametrize("dt", GQ.DTYPES)
def test_lane_map(gpu, dt):
    """Structured operands whose value depends asymmetrically on (row, output) and (row, column): a row / column slip in the store, or a k permutation applied to one
    MFMA operand only, gives other integers."""
    case = GQ.LANE_MAP
    q, s, x = GQ.lane_map_inputs(case)
    m, sc, xx, out = build_case(gpu, case, dt, q, s, x)
    gpu.take_path()
    run(gpu, case["G"], dt, out, m, sc, xx)
    assert gpu.take_path().startswith("gemm_q4/mfma,")
    truth, _ = GQ.truth64(q, s, x, case["G"])
    U.assert_same_class_bits(out.read("lane_map"), truth.astype(np.float32), f"lane_map {dt}")


# ---- 3 -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", GQ.DTYPES)
@pytest.mark.parametrize("case", [c for c in GQ.CASES if c["name"] in ("one_step", "groups_96", "two_mats", "any_m")], ids=lambda c: c["name"])
def test_subnormal_scale(gpu, case, dt):
    """Every scale 2^-140: the results are 2^-140 times an integer -- exact f32 values, most of them subnormal. Nothing is flushed on the way."""
    q, s, x = GQ.exact_inputs(case, dt, scale_exp=(-140, -140), salt=2)
    m, sc, xx, out = build_case(gpu, case, dt, q, s, x)
    run(gpu, case["G"], dt, out, m, sc, xx)
    truth, _ = GQ.truth64(q, s, x, case["G"])
    want = truth.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), truth)
    sub = (want != 0) & (np.abs(want) < np.float32(2.0 ** -126))
    assert sub.mean() > 0.25, f"only {sub.mean():.2f} of the results are subnormal (the case shows nothing)"
    U.assert_same_class_bits(out.read(case["name"]), want, f"{case['name']} {dt}")


@pytest.mark.parametrize("dt", GQ.DTYPES)
@pytest.mark.parametrize("what", ["zero_weight", "zero_scale"])
@pytest.mark.parametrize("case", [c for c in GQ.CASES if c["name"] in ("groups_64", "cols_65", "any_rows")], ids=lambda c: c["name"])
def test_inf_against_zero(gpu, case, dt, what):
    """ONE Inf in x (row r0 of column n0) against nonzero weights gives +-Inf in every output of that column -- except output o0, whose nibble at r0 is 8 (q = 0: a
    true zero) or whose scale of r0's group is zero: 0 * Inf = NaN there, and nowhere else. Every other column stays the exact finite product."""
    name, k, outs, n, G = case["name"], case["k"], case["outputs"], case["n"], case["G"]
    rng = _q4.rng_of(name, 5)
    q = (rng.integers(1, 4, (k, outs, 1)) * rng.choice([-1, 1], (k, outs, 1))).astype(np.int8)
    s = np.ldexp(np.float32(1), rng.integers(-1, 2, (_q4.n_groups(k, G), outs, 1))).astype(np.float32)
    x = (rng.integers(1, 4, (k, n, 1)) * rng.choice([-1, 1], (k, n, 1))).astype(np.float32)
    r0, n0, o0 = k - 3, n - 1, outs // 2
    x[r0, n0, 0] = np.inf
    if what == "zero_weight":
        q[r0, o0, 0] = 0
    else:
        s[r0 // G, o0, 0] = 0
    m, sc, xx, out = build_case(gpu, case, dt, q, s, x)
    run(gpu, G, dt, out, m, sc, xx)
    got = out.read(f"{name} {what}")[:, :, 0]
    hit = np.zeros((outs, n), bool)
    hit[:, n0] = True
    assert np.isfinite(got[~hit]).all(), f"{np.count_nonzero(~np.isfinite(got[~hit]))} outputs outside the Inf's reach are not finite"
    assert np.isnan(got[o0, n0]) and np.count_nonzero(np.isnan(got)) == 1, f"0 * Inf gave {got[o0, n0]}; {np.count_nonzero(np.isnan(got))} NaN in all"
    others = np.arange(outs) != o0
    assert np.isinf(got[others, n0]).all() and np.array_equal(np.sign(got[others, n0]), np.sign(q[r0, others, 0].astype(np.float32))), "the Inf column"
    truth, _ = GQ.truth64(q, s, np.where(np.isfinite(x), x, 1), G)
    assert np.array_equal(got[~hit].astype(np.float64), truth[:, :, 0][~hit])


# ---- 4 -------------------------------------------------------------------------------------------------------------------------------------------------
def _raw(gpu, arr):
    """A buffer of exactly arr.nbytes bytes."""
    wg = _wg()
    arr = np.ascontiguousarray(arr)
    return wg.TensorBuilder.tensor((arr.size,), S_STORAGE).build_init(gpu.device(), arr, arr.dtype)


def test_status_codes(gpu):
    wg, L = _wg(), _L()
    V, sh = wg.GemmVariant, wg.ViewShape
    K, O, N, G = 64, 32, 8, 32
    B = K // 2  # rows of bytes
    mb, sb = _raw(gpu, np.full(B * O, 0x99, np.uint8)), _raw(gpu, np.ones(K // G * O, np.float32))  # every nibble 9: q = 1
    xb, ob = _raw(gpu, np.ones(K * N, np.float16).view(np.uint16)), _raw(gpu, np.zeros(O * N, np.float32))
    m, s = View(mb, sh((B, O, 1), B, B * O, 0)), View(sb, sh((K // G, O, 1), K // G, K // G * O, 0))
    x, out = View(xb, sh((K, N, 1), K, K * N, 0)), View(ob, sh((O, N, 1), O, O * N, 0))
    gpu.take_path()
    for variant in (V.GemmTr, V.GemmTrFast):  # the same call
        gpu.queue().write_buffer(ob, 0, np.full(O * N, NAN32))
        rc, msg = call(gpu, G, "f16", out, m, s, x, variant)
        assert rc == 0, msg
        assert np.array_equal(ob.read(gpu.device()), np.full(O * N, K, np.float32))
    assert gpu.take_path() == "gemm_q4/mfma,f16,nt=2,ns=1 gemm_q4/mfma,f16,nt=2,ns=1"
    # out = W x is not this call's; f32 columns are not; both messages name the call that is. Both come before any dimension is looked at
    x_bad = View(xb, sh((K - 2, N, 1), K, K * N, 0))
    for variant in (V.Gemm, V.GemmFast):
        for xv in (x, x_bad):
            rc, msg = call(gpu, G, "f16", out, m, s, xv, variant)
            assert rc == L.WG_ERR_UNSUPPORTED and "wg_gemv_q8" in msg and msg.startswith("Gemm: wg_gemm_q4 computes out = W^T x only"), (rc, msg)
        assert call(gpu, 0, "f16", View(ob, sh((O, 0, 1), O, O * N, 0)), m, s, View(xb, sh((K, 0, 1), K, K * N, 0)), variant)[0] == L.WG_ERR_UNSUPPORTED  # zero-sized too
    for xv in (x, x_bad):
        rc, msg = call(gpu, G, L.WG_F32, out, m, s, xv)
        assert rc == L.WG_ERR_UNSUPPORTED and "wg_gemv_q4" in msg and msg.startswith("Gemm: wg_gemm_q4 takes f16 or bf16 columns"), (rc, msg)
    rc, msg = call(gpu, G, 3, out, m, s, x)
    assert rc == L.WG_ERR_INVALID_ARG and msg == "Gemm: unknown dtype 3", (rc, msg)
    rc, msg = call(gpu, G, "f16", out, m, s, x, 7)
    assert rc == L.WG_ERR_INVALID_ARG and msg == "Gemm: unknown variant 7", (rc, msg)
    rc = L.lib.wg_gemm_q4(gpu._ctx.handle, 2, G, L.WG_F16, out.buf._h, out.shape.to_c(), None, m.shape.to_c(), s.buf._h, s.shape.to_c(), x.buf._h, x.shape.to_c())
    assert rc == L.WG_ERR_INVALID_ARG and L.lib.wg_last_error_string() == b"Gemm: buffer argument 1 is NULL"
    # group_rows: wg_gemv_q4's rule
    for bad in (0, 16, 48, 63):
        rc, msg = call(gpu, bad, "f16", out, m, s, x)
        assert rc == L.WG_ERR_INVALID_ARG and msg == f"Gemm: group_rows {bad} is neither a positive multiple of 32 nor at least the {K} logical rows of m", (rc, msg)
    # the scales' shape; one row for a per-output call is right
    rc, msg = call(gpu, G, "f16", out, m, View(sb, sh((K // G - 1, O, 1), K // G, K // G * O, 0)), x)
    assert rc == L.WG_ERR_DIM_MISMATCH and msg == (f"Gemm: dimension mismatch. (m [{B},{O},1] packed: k {K}, group_rows {G}, scales [{K // G - 1},{O},1], "
                                                   f"expected [{K // G},{O},1])"), (rc, msg)
    rc, msg = call(gpu, 64, "f16", out, m, s, x)  # (the scales of groups of 32 under groups of 64)
    assert rc == L.WG_ERR_DIM_MISMATCH and f"expected [1,{O},1]" in msg
    assert call(gpu, 1000, "f16", out, m, View(sb, sh((1, O, 1), 1, O, 0)), x)[0] == 0
    # the Gemm dimension check comes first, with its message: x.rows == 2 * m.rows
    rc, msg = call(gpu, 16, "f16", out, m, s, x_bad)
    assert rc == L.WG_ERR_DIM_MISMATCH and msg == f"Gemm: dimension mismatch. (out [{O},{N},1], m1 [{B},{O},1]^T packed: k {K}, m2 [{K - 2},{N},1])", (rc, msg)
    assert call(gpu, G, "f16", out, m, s, View(xb, sh((B, N, 1), K, K * N, 0)))[0] == L.WG_ERR_DIM_MISMATCH  # x with as many rows as m has BYTES
    for bad_out in (sh((O - 1, N, 1), O, O * N, 0), sh((O, N - 1, 1), O, O * N, 0), sh((O, N, 2), O, 0, 0)):
        assert call(gpu, G, "f16", View(ob, bad_out), m, s, x)[0] == L.WG_ERR_DIM_MISMATCH
    # each operand out of bounds at its own element size
    rc, msg = call(gpu, G, "f16", out, View(_raw(gpu, np.ones(B * O - 1, np.uint8)), m.shape), s, x)
    assert rc == L.WG_ERR_OUT_OF_BOUNDS and msg == f"Gemm: view `m` addresses {B * O} elements but its buffer holds {B * O - 1}", (rc, msg)
    rc, msg = call(gpu, G, "f16", out, m, View(_raw(gpu, np.ones(K // G * O - 1, np.float32)), s.shape), x)
    assert rc == L.WG_ERR_OUT_OF_BOUNDS and msg == f"Gemm: view `scales` addresses {K // G * O} elements but its buffer holds {K // G * O - 1}", (rc, msg)
    rc, msg = call(gpu, G, "f16", out, m, s, View(_raw(gpu, np.ones(K * N - 1, np.uint16)), x.shape))
    assert rc == L.WG_ERR_OUT_OF_BOUNDS and msg == f"Gemm: view `x` addresses {K * N} elements but its buffer holds {K * N - 1}", (rc, msg)
    rc, msg = call(gpu, G, "f16", View(_raw(gpu, np.zeros(O * N, np.uint16)), out.shape), m, s, x)  # an `out` sized as if it held 16-bit elements
    assert rc == L.WG_ERR_OUT_OF_BOUNDS and msg == f"Gemm: view `out` addresses {O * N} elements but its buffer holds {O * N // 2}", (rc, msg)
    # mats * column passes past grid.z: refused before anything is launched (one output; the read views fit: every matrix and every column of theirs is the same memory)
    gpu.take_path()
    NZ, Nw = 40000, 65
    rc, msg = call(gpu, G, "f16", View(_raw(gpu, np.zeros(Nw * NZ, np.float32)), sh((1, Nw, NZ), 1, Nw, 0)), View(mb, sh((16, 1, NZ), 16, 0, 0)),
                   View(sb, sh((1, 1, NZ), 1, 0, 0)), View(xb, sh((32, Nw, NZ), 0, 0, 0)))
    assert rc == L.WG_ERR_UNSUPPORTED and msg == f"Gemm: nmats * column passes = {2 * NZ} exceeds 65535" and gpu.take_path() == "", (rc, msg)
    # empty operands: WG_OK, nothing launched, nothing written
    before = ob.read(gpu.device()).copy()
    gpu.take_path()
    assert call(gpu, G, "f16", View(ob, sh((O, 0, 1), O, O * N, 0)), m, s, View(xb, sh((K, 0, 1), K, K * N, 0)))[0] == 0
    h0 = ctypes.c_void_p()
    L.check(L.lib.wg_buf_create(gpu._ctx.handle, 0, S_STORAGE, ctypes.byref(h0)))
    try:
        for which in range(4):
            hs = [h0 if i == which else b.buf._h for i, b in enumerate((out, m, s, x))]
            rc = L.lib.wg_gemm_q4(gpu._ctx.handle, 2, G, L.WG_F16, hs[0], out.shape.to_c(), hs[1], m.shape.to_c(), hs[2], s.shape.to_c(), hs[3], x.shape.to_c())
            assert rc == 0, (which, L.lib.wg_last_error_string().decode())
    finally:
        L.check(L.lib.wg_buf_destroy(h0))
    assert gpu.take_path() == "" and ob.read(gpu.device()).tobytes() == before.tobytes()
    # k == 0: an empty sum, zeros
    gpu.queue().write_buffer(ob, 0, np.full(O * N, NAN32))
    rc, msg = call(gpu, G, "f16", out, View(mb, sh((0, O, 1), 16, 16 * O, 0)), View(sb, sh((0, O, 1), 1, O, 0)), View(xb, sh((0, N, 1), 16, 16 * N, 0)))
    assert rc == 0 and gpu.take_path() == "gemm_q4/any" and np.array_equal(ob.read(gpu.device()), np.zeros(O * N, np.float32)), (rc, msg)


# ---- 5 -------------------------------------------------------------------------------------------------------------------------------------------------
def test_aliasing(gpu):
    """Decided on addresses: `out` (f32) against `m` in 1-byte units, against `scales`, against `x` in 2-byte units; nothing is launched, logged or written by a refused
    call. The layout is tests/cpp/overlap_gemm_q4_check.cpp's: out | m | scales | x touching in ONE buffer (out: bytes 256 .. 511)."""
    wg, L = _wg(), _L()
    sh = wg.ViewShape
    K, O, N, G = 128, 16, 4, 64
    B = K // 2
    case = dict(name="alias", k=K, outputs=O, n=N, G=G, Z=1)
    q, s, x = GQ.exact_inputs(case, "f16")
    truth = GQ.truth64(q, s, x, G)[0][:, :, 0]
    raw = np.zeros(4096, np.uint8)
    raw[256:512] = np.full(O * N, NAN32).view(np.uint8)
    raw[512:1536] = _q4.pack(q)[:, :, 0].ravel(order="F")
    raw[1536:1664] = s[:, :, 0].ravel(order="F").view(np.uint8)
    raw[1664:2688] = GQ.bits16("f16", x[:, :, 0]).ravel(order="F").view(np.uint8)
    buf = _raw(gpu, raw)
    out = lambda off: View(buf, sh((O, N, 1), O, O * N, off))  # noqa: E731
    m, sc, xx = View(buf, sh((B, O, 1), B, B * O, 512)), View(buf, sh((K // G, O, 1), K // G, K // G * O, 384)), View(buf, sh((K, N, 1), K, K * N, 832))
    gpu.take_path()
    rc, msg = call(gpu, G, "f16", out(64), m, sc, xx)  # `out` ends where m begins
    assert rc == 0, msg
    assert gpu.take_path() == "gemm_q4/mfma,f16,nt=2,ns=1"
    after = buf.read(gpu.device())
    assert np.array_equal(after[256:512].view(np.float32).reshape(O, N, order="F").astype(np.float64), truth), "touching views: wrong result"
    assert np.array_equal(after[512:], raw[512:]) and np.array_equal(after[:256], raw[:256]), "touching views: a byte outside `out` changed"
    rc, msg = call(gpu, G, "f16", out((1664 + 1024) // 4), m, sc, xx)  # `out` directly behind x
    assert rc == 0, msg
    assert np.array_equal(buf.read(gpu.device())[2688:2944].view(np.float32).reshape(O, N, order="F").astype(np.float64), truth), "out behind x: wrong result"
    gpu.queue().write_buffer(buf, 0, raw)
    gpu.take_path()
    refused = [(out(64), View(buf, sh((B, O, 1), B, B * O, 511)), sc, xx, "m"),   # the matrix one byte earlier: the last byte of out is shared
               (out(384 - O * N + 1), View(buf, sh((B, O, 1), B, B * O, 2688)), sc, xx, "scales"),  # the last float of out is the first scale (m elsewhere)
               (out(384 + 2 * O), m, sc, xx, "x"),                              # out begins where the scales end: on x's first two elements
               (out((1664 + 1024) // 4 - 1), m, sc, xx, "x")]                   # the first float of out is x's last two elements
    for o_, m_, s_, x_, name in refused:
        rc, msg = call(gpu, G, "f16", o_, m_, s_, x_)
        assert rc == L.WG_ERR_ALIASED and msg == f"Gemm: `out` overlaps `{name}` (the written view shares memory with a view the call reads)", (name, rc, msg)
    assert gpu.take_path() == "" and buf.read(gpu.device()).tobytes() == raw.tobytes()
    # the read operands may overlap each other: x IS the first bytes of the matrix
    o2 = Op(gpu, np.full((O, N, 1), NAN32))
    rc, msg = call(gpu, G, "f16", o2, m, sc, View(buf, sh((K, N, 1), K, K * N, 256)))
    assert rc == 0, msg
    o2.read("x over m")  # (the guard: the values are whatever the weights' bytes spell as f16)


# ---- 6 -------------------------------------------------------------------------------------------------------------------------------------------------
def test_workspace_inside_a_recording():
    """The partials of a cut contraction live in the context's workspace: on a fresh context it cannot grow inside a recording (WG_ERR_WORKSPACE); after
    wg_ctx_reserve_workspace the same call records, and the replay has the eager bits."""
    wg, L = _wg(), _L()
    inst = wg.GpuInstance.new(0)
    try:
        case = [c for c in GQ.CASES if c["name"] == "cut"][0]
        q, s, x = GQ.random_inputs(case, "bf16", salt=3)
        m, sc, xx, out = build_case(inst, case, "bf16", q, s, x)
        enc = inst.device().create_command_encoder(record=True)
        try:
            rc, msg = call(inst, case["G"], "bf16", out, m, sc, xx)
        finally:
            cb = enc.finish()
        assert rc == L.WG_ERR_WORKSPACE, (rc, msg)
        del cb
        inst.device().reserve_workspace(4 * 65535 * case["n"] * case["outputs"])  # (whatever the cut on this part is)
        enc = inst.device().create_command_encoder(record=True)
        try:
            rc, msg = call(inst, case["G"], "bf16", out, m, sc, xx)
        finally:
            cb = enc.finish()
        assert rc == 0, msg
        inst.queue().submit([cb])
        replayed = out.read("replayed")
        truth, sabs = GQ.truth64(q, s, x, case["G"])
        _q4.assert_within_gate(replayed, truth, case["k"], sabs, "replayed")
        out.poison()
        run(inst, case["G"], "bf16", out, m, sc, xx)
        U.assert_bits_equal(out.read("eager"), replayed, "cut contraction: eager against replayed")
        out.poison()
        inst.queue().submit([cb])
        U.assert_bits_equal(out.read("replayed again"), replayed, "cut contraction: second replay")
        del cb
    finally:
        inst.sync()


def test_replay_any(gpu):
    """An element-by-element call recorded and replayed: the eager bits."""
    case = [c for c in GQ.CASES if c["name"] == "any_m"][0]
    q, s, x = GQ.random_inputs(case, "f16", salt=4)
    m, sc, xx, out = build_case(gpu, case, "f16", q, s, x)
    run(gpu, case["G"], "f16", out, m, sc, xx)
    eager = out.read("eager")
    out.poison()
    gpu.take_path()
    enc = gpu.device().create_command_encoder(record=True)
    try:
        rc, msg = call(gpu, case["G"], "f16", out, m, sc, xx)
    finally:
        cb = enc.finish()
    assert rc == 0, msg
    assert gpu.take_path() == "gemm_q4/any"
    for i in range(2):
        gpu.queue().submit([cb])
        U.assert_bits_equal(out.read(f"replay {i}"), eager, f"any: replay {i} against eager")
        out.poison()
    del cb


# ---- 7 -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,G", [("f16", 32), ("bf16", 128), ("f16", 4096)])
def test_python_operators(gpu, dt, G):
    """Gemm.dispatch_q4_tr / dispatch_q4_generic on tensors, through a compute pass: a random f32 matrix quantised with quantize_q4, against the f64 truth of the
    DEQUANTISED matrix within the gate; the same packed / scale tensors serve Gemv.dispatch_q4_tr, whose result (on the widened column) agrees within both gates."""
    wg = _wg()
    dev, shapes = gpu.device(), wg.ViewShapeBuffers()
    rng = np.random.default_rng(47 + G)
    K, O, N = 544, 72, 12
    w = rng.standard_normal((K, O)).astype(np.float32)
    packed, s = wg.quantize_q4(w, G)
    assert packed.dtype == np.uint8 and packed.shape == (K // 2, O)
    q = _q4.unpack(packed)
    x = GQ.round16(dt, rng.random((K, N), dtype=np.float32) * 2 - 1)
    tq = wg.TensorBuilder.matrix(K // 2, O, S_STORAGE).build_init(dev, packed)
    ts = wg.TensorBuilder.matrix(s.shape[0], O, S_STORAGE).build_init(dev, s)
    tx = wg.TensorBuilder.matrix(K, N, S_STORAGE).build_init(dev, x.ravel(order="F").astype(np.float16) if dt == "f16" else wg.to_bfloat16(x.ravel(order="F")))
    truth, sabs = GQ.truth64(q[:, :, None], s[:, :, None], x[:, :, None], G)
    op = wg.Gemm.from_device(dev)
    for method, extra in (("dispatch_q4_tr", ()), ("dispatch_q4_generic", (wg.GemmVariant.GemmTr,)), ("dispatch_q4_generic", (wg.GemmVariant.GemmTrFast,))):
        to = wg.TensorBuilder.matrix(O, N, S_STORAGE).build_init(dev, np.full((O, N), NAN32))
        gpu.take_path()
        enc = dev.create_command_encoder()
        p = enc.compute_pass("gemm_q4", None)
        getattr(op, method)(dev, shapes, p, to, tq, ts, tx, G, *extra)
        p.end()
        gpu.queue().submit([enc.finish()])
        got = to.read(dev).reshape(O, N, order="F")
        assert gpu.take_path() == f"gemm_q4/mfma,{dt},nt=2,ns=1", method
        _q4.assert_within_gate(got, truth[:, :, 0], K, sabs[:, :, 0], f"{method} {dt} G = {G}")
    with pytest.raises(_L().WgError, match="wg_gemv_q8"):
        enc = dev.create_command_encoder()
        p = enc.compute_pass("gemm_q4", None)
        try:
            op.dispatch_q4_generic(dev, shapes, p, to, tq, ts, tx, G, wg.GemmVariant.Gemm)  # out = W x: refused by the library
        finally:
            p.end()
            gpu.queue().submit([enc.finish()])
    # the Gemv on the same weights, one column
    tv = wg.TensorBuilder.vector(K, S_STORAGE).build_init(dev, np.ascontiguousarray(x[:, 0]))
    tov = wg.TensorBuilder.vector(O, S_STORAGE).build_init(dev, np.full(O, NAN32))
    enc = dev.create_command_encoder()
    p = enc.compute_pass("gemv_q4", None)
    wg.Gemv.from_device(dev).dispatch_q4_tr(dev, shapes, p, tov, tq, ts, tv, G)
    p.end()
    gpu.queue().submit([enc.finish()])
    err = np.abs(tov.read(dev).astype(np.float64) - got[:, 0].astype(np.float64))
    assert (err <= 2 * _q4.gate(K, sabs[:, 0, 0])).all(), f"wg_gemv_q4 on the same weights: worst / (gate + gate) = {(err / (2 * _q4.gate(K, sabs[:, 0, 0]))).max():.3g}"


# ---- 8 -------------------------------------------------------------------------------------------------------------------------------------------------
_DIRTY, _SHARED = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _drop_shared():
    yield
    _DIRTY.clear()
    _SHARED.clear()


def shared(case, dt, kind):
    """(q, s, x, truth, sabs) of a cut case, drawn and summed in float64 once for all the tests that use them (read-only)."""
    key = (case["name"], dt, kind)
    if key not in _SHARED:
        q, s, x = GQ.random_inputs(case, dt) if kind == "random" else GQ.exact_inputs(case, dt)
        _SHARED[key] = (q, s, x) + tuple(GQ.truth64(q, s, x, case["G"]))
        for a in _SHARED[key]:
            a.setflags(write=False)
    return _SHARED[key]


def dirty_workspace(inst, dt, plan, case):
    """One call on GQ.DIRTY (k 4096, 256 outputs, 192 columns) whose scales are all NaN: every f32 partial it writes into the context's workspace is NaN, so a partial
    the next call fails to write shows in that call's result. Through the planner: the dirtying call is cut, and its workspace covers `plan`'s; its outputs x n is
    another one than the case's, so stale values cannot line up."""
    d = GQ.DIRTY
    first = (id(inst), dt) not in _DIRTY
    if first:
        q, s, x = GQ.random_inputs(d, dt, salt=9)
        _DIRTY[(id(inst), dt)] = (inst,) + build_case(inst, d, dt, q, np.full_like(s, NAN32), x)
    m, sc, xx, out = _DIRTY[(id(inst), dt)][1:]
    dplan, _ = planned(inst, d, dt, m, sc, xx, out)
    assert dplan.nsplit > 1 and dplan.workspace_bytes >= plan.workspace_bytes > 0, (dplan.nsplit, dplan.workspace_bytes, plan.workspace_bytes)
    assert d["outputs"] * d["n"] != case["outputs"] * case["n"]
    run(inst, d["G"], dt, out, m, sc, xx)
    if first:
        assert np.isnan(out.read("dirty")).all(), "NaN scales did not reach every partial of the dirtying call"
    inst.take_path()


def assert_cut_tags(inst, case, dt, path, plan, tags):
    """The logged tags are the planner's, the first is the case's (on 256 CUs; up to the cut elsewhere), the combine's tag follows; the ns logged."""
    assert path == tags, f"{case['name']}: the call logged '{path}', the planner says '{tags}'"
    first, want = path.split(" ")[0], case["tag"].format(dt=dt)
    if cus_of(inst) == 256:
        assert first == want, f"{case['name']}: expected {want}, the call took '{path}'"
    else:
        assert first.split(",ns=")[0] == want.split(",ns=")[0], f"{case['name']}: expected {want} up to the cut, the call took '{path}'"
    ns = int(first.split("ns=")[1])
    assert ns == plan.nsplit > 1 and path.split(" ")[1:] == [f"gemm_q4/combine,ns={ns}"], path
    return ns


@pytest.mark.parametrize("dt", GQ.DTYPES)
@pytest.mark.parametrize("case", GQ.CUT_CASES, ids=GQ.CUT_IDS)
def test_cut_truth_on_a_dirty_workspace(gpu, case, dt):
    """A cut contraction whose workspace holds NaN in every partial the call should write: tags, every element written, nothing outside, the truth gate (the project's
    f32_gate(2 k, sum |s q x|), not widened for the cut), and the same bits after dirtying again."""
    name, k, G = case["name"], case["k"], case["G"]
    q, s, x, truth, sabs = shared(case, dt, "random")
    m, sc, xx, out = build_case(gpu, case, dt, q, s, x)
    plan, tags = planned(gpu, case, dt, m, sc, xx, out)
    dirty_workspace(gpu, dt, plan, case)
    run(gpu, G, dt, out, m, sc, xx)
    path = gpu.take_path()
    got = out.read(name)  # (no byte outside the view changed)
    ns = assert_cut_tags(gpu, case, dt, path, plan, tags)
    print(f"{name} {dt} -> {path}: ns {ns} x {plan.k_per_split} rows")
    assert not np.isnan(got).any(), f"{name}: {np.isnan(got).sum()} elements of the view are NaN: not written, or summed from a partial the call did not write"
    r = _q4.assert_within_gate(got, truth, k, sabs, f"{name} {dt}")
    print(f"  worst err / gate = {r:.3g}")
    dirty_workspace(gpu, dt, plan, case)
    out.poison()
    run(gpu, G, dt, out, m, sc, xx)
    U.assert_bits_equal(out.read(name), got, f"{name} {dt}: second call")


@pytest.mark.parametrize("dt", GQ.DTYPES)
@pytest.mark.parametrize("case", GQ.CUT_CASES, ids=GQ.CUT_IDS)
def test_cut_exact_operands(gpu, case, dt):
    """Exact operands under a cut (GQ.exact_inputs: scales 2^0, 2^1 past k = 16384; the condition is asserted): every partial sum in any order
    is exact, so the result is fixed by construction -- a dropped, doubled or misplaced split gives other integers."""
    name = case["name"]
    q, s, x, truth, _ = shared(case, dt, "exact")
    assert (q[0::2] == -8).any() and (q[1::2] == -8).any() and (q[0::2] == 7).any() and (q[1::2] == 7).any() and _q4.exactness_condition(q, s, x) < 2.0 ** 24
    m, sc, xx, out = build_case(gpu, case, dt, q, s, x)
    plan, tags = planned(gpu, case, dt, m, sc, xx, out)
    dirty_workspace(gpu, dt, plan, case)
    run(gpu, case["G"], dt, out, m, sc, xx)
    assert_cut_tags(gpu, case, dt, gpu.take_path(), plan, tags)
    want = truth.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), truth)
    U.assert_same_class_bits(out.read(name), want, f"{name} {dt}")


@pytest.mark.parametrize("dt", GQ.DTYPES)
def test_cut_lane_map(gpu, dt):
    """test_lane_map's structured operands on 2 splits of 544 rows: a k permutation applied to one operand in the second split only, or a row / column slip in the
    partials, gives other integers. The sum bound holds at this k without narrower ranges (asserted)."""
    case = GQ.CUT_LANE_MAP
    q, s, x = GQ.lane_map_inputs(case)
    assert _q4.exactness_condition(q, s, x) < 2.0 ** 24
    m, sc, xx, out = build_case(gpu, case, dt, q, s, x)
    plan, tags = planned(gpu, case, dt, m, sc, xx, out)
    dirty_workspace(gpu, dt, plan, case)
    run(gpu, case["G"], dt, out, m, sc, xx)
    assert_cut_tags(gpu, case, dt, gpu.take_path(), plan, tags)
    truth, _ = GQ.truth64(q, s, x, case["G"])
    U.assert_same_class_bits(out.read("cut_lane_map"), truth.astype(np.float32), f"cut_lane_map {dt}")


# ---- 9 -------------------------------------------------------------------------------------------------------------------------------------------------
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
    count, the truth gate -- then recorded once and replayed twice, the workspace dirtied and `out` poisoned before each replay: the eager bits. cut_masked is cut
    differently on each of the three contexts, and on exact operands gives the same bits on all of them (the truth's)."""
    inst = gpu if where == "whole" else small[where]
    cus = dict(SMALL, whole=gpu.adapter()["compute_units"])
    assert cus_of(inst) == cus[where]
    for name, dt in (("cut_masked", "f16"), ("cut_masked", "bf16"), ("cut_g96_partial", "bf16"), ("cut_passes", "f16")):
        case = GQ.by_name(name)
        q, s, x, truth, sabs = shared(case, dt, "random")
        m, sc, xx, out = build_case(inst, case, dt, q, s, x)
        plan, tags = planned(inst, case, dt, m, sc, xx, out)
        dirty_workspace(inst, dt, plan, case)
        run(inst, case["G"], dt, out, m, sc, xx)
        log = inst.take_path()
        assert_cut_tags(inst, case, dt, log, plan, tags)
        print(f"{name} {dt} {where} -> {log}: {plan.k_per_split} rows per split")
        if name == "cut_masked":
            ns = {w: planned(inst, case, dt, m, sc, xx, out, cus=n)[0].nsplit for w, n in cus.items()}
            assert len(set(ns.values())) == 3 and plan.nsplit == ns[where], ns
            assert cus["whole"] != 256 or ns == {"whole": 8, "cus16": 6, "cus8": 3}, ns
        eager = out.read(name)
        assert not np.isnan(eager).any()
        _q4.assert_within_gate(eager, truth, case["k"], sabs, f"{name} {dt} {where}")
        inst.device().reserve_workspace(plan.workspace_bytes)
        out.poison()
        enc = inst.device().create_command_encoder(record=True)
        try:
            run(inst, case["G"], dt, out, m, sc, xx)
        finally:
            cb = enc.finish()
        assert inst.take_path() == log
        for rep in range(2):
            dirty_workspace(inst, dt, plan, case)
            out.poison()
            inst.queue().submit([cb])
            U.assert_bits_equal(out.read(name), eager, f"{name} {dt} {where}: replay {rep}")
        del cb
        if name == "cut_masked":  # exact operands: the same bits whatever the cut
            q, s, x, truth, _ = shared(case, dt, "exact")
            assert _q4.exactness_condition(q, s, x) < 2.0 ** 24
            m, sc, xx, out = build_case(inst, case, dt, q, s, x)
            dirty_workspace(inst, dt, plan, case)
            run(inst, case["G"], dt, out, m, sc, xx)
            assert inst.take_path() == log
            U.assert_same_class_bits(out.read(name), truth.astype(np.float32), f"{name} {dt} {where}: exact operands")
