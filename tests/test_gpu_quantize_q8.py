"""wg_quantize_q8 on the GPU, through the C ABI: the device-side quantiser of the q8 family. Before the feature the symbol did not exist.

The rule (include/wgebra_hip.h) is the NumPy helper quantize_q8's on the source widened exactly to f32: per group s = fl32(max|x| / 127),
q = clip(rint(fl32(x / s)), -127, 127) -- a true division, ties to even --, s == 0 gives q = 0; a group holding a NaN or an Inf gets s = NaN and q = 0. Bytes and scales
must EQUAL NumPy's: there is no tolerance.

  1  per case and source type: the tag; q and scales equal quantize_q8 to the bit; the guards around both views untouched; twice the same bytes   test_cases
  2  planted values: ties, clamping, an all-zero group, subnormals whose scale rounds to zero                                                  test_planted_values
  3  groups holding a NaN / an Inf                                                                                                             test_non_finite_groups
  4  statuses and aliasing; inside a recording                                                                                                 test_status_codes, test_aliasing, test_inside_a_recording
  5  end to end: quantise f16 activations on the device, feed wg_gemm_q8a8, compare with the f64 product of the unquantised X                   test_end_to_end
No test asserts a time.
"""
import ctypes
import faulthandler

import numpy as np
import pytest

import _gemm_q8a8 as GA

pytestmark = pytest.mark.gpu

S_STORAGE = 128 | 4 | 8
NAN32 = np.float32(np.nan)
DTYPES = ("f32", "f16", "bf16")
WHOLE = 1 << 30


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


# name, rows, cols, mats, group_rows, (q: byte offset, ld padding, gap), (src: element offset, ld padding, gap), leaf
CASES = [
    ("g32", 64, 17, 1, 32, (0, 0, 0), (0, 0, 0), "vec"),
    ("g32_one_col", 96, 1, 1, 32, (0, 0, 0), (0, 0, 0), "vec"),
    ("g32_65_cols", 32, 65, 1, 32, (16, 16, 0), (8, 8, 0), "vec"),
    ("g128_two_blocks", 4112, 3, 2, 128, (0, 0, 32), (0, 0, 16), "vec"),      # 257 lanes per column: a second workgroup with one live lane; a partial last group of 16 rows
    ("g1024", 2048, 2, 1, 1024, (0, 0, 0), (0, 0, 0), "vec"),                # 64 lanes per group: a whole wave
    ("g64_partial", 160, 5, 1, 64, (0, 0, 0), (0, 0, 0), "vec"),             # a partial last group of 32 rows: lanes past the last row take part with zeros
    ("g96_partial", 200, 17, 1, 96, (0, 0, 0), (0, 0, 0), "any"),            # 96: 6 lanes are no power of two; 200 rows: a partial last group of 8
    ("g16", 48, 3, 1, 16, (0, 0, 0), (0, 0, 0), "any"),
    ("whole", 200, 65, 1, WHOLE, (0, 0, 0), (0, 0, 0), "any"),               # one scale per column, a wave per column
    ("whole_long", 4100, 2, 2, 5000, (0, 0, 0), (0, 0, 0), "any"),           # past 1024 rows per group: a workgroup of 4 waves per column
    ("odd_views", 64, 5, 2, 32, (1, 3, 5), (1, 3, 7), "any"),                # everything else would be vec: the views are not 16-byte aligned
    ("odd_src_only", 64, 5, 1, 32, (0, 0, 0), (1, 0, 0), "any"),
]
CASE_IDS = [c[0] for c in CASES]


def representable(dt, x32):
    """float32 values after one rounding to `dt`, as float32."""
    wg = _wg()
    x32 = np.asarray(x32, np.float32)
    if dt == "f32":
        return x32
    if dt == "f16":
        with np.errstate(over="ignore"):
            return x32.astype(np.float16).astype(np.float32)
    return np.asarray(wg.from_bfloat16(wg.to_bfloat16(x32)), np.float32).reshape(x32.shape)


def stored(dt, x32):
    """The array to upload for values representable in `dt`."""
    wg = _wg()
    if dt == "f32":
        return np.ascontiguousarray(x32, np.float32)
    if dt == "f16":
        return np.ascontiguousarray(x32.astype(np.float16)).view(np.uint16)
    return np.ascontiguousarray(np.asarray(wg.to_bfloat16(x32))).view(np.uint16).reshape(x32.shape)


class Op:
    """X[r, c, z] column-major at element `off`, leading dimension r + pad, `gap` elements between matrices, inside a parent filled with `fill`."""

    def __init__(self, gpu, vals, off=0, pad=0, gap=0, fill=0):
        wg = _wg()
        vals = np.ascontiguousarray(vals)
        R, C, Z = vals.shape
        self.gpu = gpu
        self.ld, self.batch = R + pad, (R + pad) * C + gap
        self.size = off + self.batch * Z + 16
        self.idx = off + np.arange(R)[:, None, None] + np.arange(C)[None, :, None] * self.ld + np.arange(Z)[None, None, :] * self.batch
        self.init = np.full(self.size, fill, vals.dtype)
        self.init[self.idx] = vals
        self.buf = wg.TensorBuilder.tensor((self.size,), S_STORAGE).build_init(gpu.device(), self.init, self.init.dtype)
        self.shape = wg.ViewShape((R, C, Z), self.ld, self.batch, off)
        self.outside = np.ones(self.size, bool)
        self.outside[self.idx.ravel()] = False

    def poison(self):
        self.gpu.queue().write_buffer(self.buf, 0, self.init)

    def read(self, what=""):
        flat = self.buf.read(self.gpu.device())
        assert flat[self.outside].tobytes() == self.init[self.outside].tobytes(), f"{what}: wrote outside the view"
        return np.ascontiguousarray(flat[self.idx])


class View:
    def __init__(self, buf, shape):
        self.buf, self.shape = buf, shape


def wg_dt(dt):
    L = _L()
    return {"f32": L.WG_F32, "f16": L.WG_F16, "bf16": L.WG_BF16}[dt] if isinstance(dt, str) else int(dt)


def call(inst, dt, G, q, s, src):
    L = _L()
    rc = L.lib.wg_quantize_q8(inst._ctx.handle, wg_dt(dt), int(G), q.buf._h, q.shape.to_c(), s.buf._h, s.shape.to_c(), src.buf._h, src.shape.to_c())
    return rc, L.lib.wg_last_error_string().decode()


def n_groups(rows, G):
    return -(-rows // min(G, rows))


def operands(gpu, dt, x32, G, qv=(0, 0, 0), sv=(0, 0, 0)):
    """src (values of x32, representable in dt), q prefilled with the sentinel 0x5A, scales prefilled with a NaN of payload 0x5A5A -- all inside guards."""
    R, C, Z = x32.shape
    src = Op(gpu, stored(dt, x32), off=sv[0], pad=sv[1], gap=sv[2], fill=0)
    q = Op(gpu, np.full((R, C, Z), 0x5A, np.int8), off=qv[0], pad=qv[1], gap=qv[2], fill=0x5A)
    s = Op(gpu, np.full((n_groups(R, G), C, Z), 0x7FC05A5A, np.uint32).view(np.float32), off=3, pad=1, gap=2, fill=np.uint32(0x7FC05A5A).view(np.float32))
    return q, s, src


def expected(x32, G):
    """NumPy's quantize_q8, with the one case it leaves undefined defined: a group whose max|x| is not finite gets s = NaN, q = 0."""
    wg = _wg()
    q, s = wg.quantize_q8(np.where(np.isfinite(x32), x32, np.float32(0)), G)
    g = min(G, x32.shape[0])
    for i in range(s.shape[0]):
        bad = ~np.isfinite(x32[i * g:(i + 1) * g]).all(axis=0)
        s[i][bad] = np.nan
        q[i * g:(i + 1) * g][:, bad] = 0
    return q, s


def check(gpu, dt, x32, G, qv=(0, 0, 0), sv=(0, 0, 0), leaf=None, what=""):
    q, s, src = operands(gpu, dt, x32, G, qv, sv)
    gpu.take_path()
    rc, msg = call(gpu, dt, G, q, s, src)
    assert rc == 0, msg
    path = gpu.take_path()
    if leaf:
        assert path == f"quantize_q8/{leaf},{dt}", f"{what}: the call took '{path}'"
    got_q, got_s = q.read(what + " q"), s.read(what + " scales")
    want_q, want_s = expected(x32, G)
    bad = np.flatnonzero(got_s.view(np.uint32).ravel() != want_s.view(np.uint32).ravel()) if not np.isnan(want_s).any() else \
        np.flatnonzero((np.isnan(got_s) != np.isnan(want_s)).ravel() | (~np.isnan(want_s) & (got_s.view(np.uint32) != want_s.view(np.uint32))).ravel())
    assert bad.size == 0, f"{what}: {bad.size} scales differ; first at {bad[0]}: got {got_s.ravel()[bad[0]]!r}, expected {want_s.ravel()[bad[0]]!r}"
    badq = np.flatnonzero(got_q.ravel() != want_q.ravel())
    assert badq.size == 0, (f"{what}: {badq.size} of {got_q.size} bytes differ; first at {np.unravel_index(badq[0], got_q.shape)}: got {got_q.ravel()[badq[0]]}, "
                            f"expected {want_q.ravel()[badq[0]]}")
    return q, s, src, got_q, got_s


# ---- 1 -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_cases(gpu, case, dt):
    name, R, C, Z, G, qv, sv, leaf = case
    if dt != "f32" and leaf == "vec" and (sv[0] or sv[1]):  # (the case's source offsets are in f32 elements of 4 bytes: 16-byte multiples for 2-byte elements too)
        sv = (2 * sv[0], 2 * sv[1], 2 * sv[2])
    rng = np.random.default_rng(sum(map(ord, name)) + len(dt))
    x = representable(dt, rng.standard_normal((R, C, Z)).astype(np.float32) * np.float32(3))
    q, s, src, got_q, got_s = check(gpu, dt, x, G, qv, sv, leaf, f"{name} {dt}")
    assert (got_q == 127).any() or (got_q == -127).any()
    q.poison()
    s.poison()
    assert call(gpu, dt, G, q, s, src)[0] == 0
    assert q.read().tobytes() == got_q.tobytes() and s.read().tobytes() == got_s.tobytes(), f"{name} {dt}: second call"


# ---- 2 -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,leaf", [(32, "vec"), (16, "any")])
@pytest.mark.parametrize("dt", DTYPES)
def test_planted_values(gpu, dt, G, leaf):
    """Column 0: max 127, so s = 1 exactly and x / s = n + 1/2 are true ties (to even: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, -0.5 -> -0, ...). Column 1: max 1, s = fl(1 / 127):
    x = s * (n + 1/2) rounded -- quotients next to ties, where x / s and x * (1 / s) differ. Column 2: all zero (s = 0, q = 0). f32 only -- columns 3 .. 5 hold
    subnormals: max 3 * 2^-149 (s rounds to 0: q = 0), max 190 * 2^-149 (s = 2^-149: 190 clamps to 127, -190 to -127), max 100 * 2^-149 (s = 2^-149: q = x)."""
    R = 64
    ncols = 6 if dt == "f32" else 3
    x = np.zeros((R, ncols, 1), np.float32)
    n = np.arange(R, dtype=np.float32) - 32
    r = np.arange(R)
    first, sign = r % G == 0, np.where((r // G) % 2, -1, 1).astype(np.float32)  # the first row of every group carries the group's max, with alternating sign
    x[:, 0, 0] = np.where(first, 127 * sign, n + np.float32(0.5))
    s1 = np.float32(1) / np.float32(127)
    x[:, 1, 0] = np.where(first, sign, (s1 * (np.arange(R, dtype=np.float32) + np.float32(0.5))).astype(np.float32))
    if dt == "f32":
        sub = np.float32(2.0 ** -149)
        x[:, 3, 0] = sub * (np.arange(R) % 4).astype(np.float32) * np.where(np.arange(R) % 2, 1, -1)
        x[:, 4, 0] = sub * (np.arange(R) * 3 % 191).astype(np.float32)
        x[1, 4, 0], x[2, 4, 0], x[G + 1, 4, 0], x[G + 2, 4, 0] = 190 * sub, -190 * sub, -190 * sub, 190 * sub
        x[:, 5, 0] = sub * (np.arange(R) % 101).astype(np.float32)
        x[3, 5, 0], x[G + 3, 5, 0] = 100 * sub, -100 * sub
    x = representable(dt, x)
    _, _, _, got_q, got_s = check(gpu, dt, x, G, leaf=leaf, what=f"planted {dt} G {G}")
    assert (got_s[:, 0, 0] == 1).all() and (got_s[:, 2, 0] == 0).all() and (got_q[:, 2, 0] == 0).all()
    ties = ~first
    assert np.array_equal(got_q[ties, 0, 0], np.rint(n[ties] + 0.5).astype(np.int8)) and (got_q[ties, 0, 0] % 2 == 0).all()
    if dt == "f32":
        assert (got_s[:, 3, 0] == 0).all() and (got_q[:, 3, 0] == 0).all(), "a scale that rounds to zero"
        assert got_s[0, 4, 0] == np.float32(2.0 ** -149) and got_q[1, 4, 0] == 127 and got_q[2, 4, 0] == -127, "clamping"
        assert got_s[0, 5, 0] == np.float32(2.0 ** -149) and got_q[3, 5, 0] == 100


# ---- 3 -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,R,leaf", [(32, 128, "vec"), (48, 144, "any"), (WHOLE, 100, "any")])
@pytest.mark.parametrize("dt", DTYPES)
def test_non_finite_groups(gpu, dt, G, R, leaf):
    """One group holds a NaN, one +Inf, one -Inf next to a NaN: s = NaN and q = 0 throughout those groups and nowhere else (the max instructions drop NaNs: the
    kernel has to look)."""
    rng = np.random.default_rng(7)
    x = representable(dt, rng.standard_normal((R, 4, 1)).astype(np.float32))
    g = min(G, R)
    x[5, 0, 0] = np.nan
    x[R - 1, 1, 0] = np.inf
    x[g // 2, 2, 0], x[g // 2 + 1, 2, 0] = -np.inf, np.nan
    _, _, _, got_q, got_s = check(gpu, dt, x, G, leaf=leaf, what=f"non-finite {dt} G {G}")
    want_nan = np.zeros(got_s.shape, bool)
    want_nan[0, 0, 0] = want_nan[-1, 1, 0] = want_nan[0, 2, 0] = True
    assert np.array_equal(np.isnan(got_s), want_nan)
    assert (got_q[:g, 0, 0] == 0).all() and (got_q[R - 1 - (R - 1) % g:, 1, 0] == 0).all() and (got_q[:g, 2, 0] == 0).all() and (got_q[:, 3, 0] != 0).any()


# ---- 4 -------------------------------------------------------------------------------------------------------------------------------------------------
def _raw(gpu, arr):
    wg = _wg()
    arr = np.ascontiguousarray(arr)
    return wg.TensorBuilder.tensor((arr.size,), S_STORAGE).build_init(gpu.device(), arr, arr.dtype)


def test_status_codes(gpu):
    wg, L = _wg(), _L()
    sh = wg.ViewShape
    R, C, G = 64, 8, 32
    NG = R // G
    qb, sb, xb = _raw(gpu, np.zeros(R * C, np.int8)), _raw(gpu, np.zeros(NG * C, np.float32)), _raw(gpu, np.ones(R * C, np.float32))
    q, s, x = View(qb, sh((R, C, 1), R, R * C, 0)), View(sb, sh((NG, C, 1), NG, NG * C, 0)), View(xb, sh((R, C, 1), R, R * C, 0))
    gpu.take_path()
    rc, msg = call(gpu, "f32", G, q, s, x)
    assert rc == 0 and gpu.take_path() == "quantize_q8/vec,f32", (rc, msg)
    assert (qb.read(gpu.device()) == 127).all() and (sb.read(gpu.device()) == np.float32(1) / np.float32(127)).all()
    a = (q.buf._h, q.shape.to_c(), s.buf._h, s.shape.to_c(), x.buf._h, x.shape.to_c())
    assert L.lib.wg_quantize_q8(None, L.WG_F32, G, *a) == L.WG_ERR_INVALID_ARG and L.lib.wg_last_error_string() == b"Quantize: ctx is NULL"
    rc, msg = call(gpu, 3, G, q, s, x)
    assert rc == L.WG_ERR_INVALID_ARG and msg == "Quantize: unknown dtype 3", (rc, msg)
    b = list(a)
    b[4] = None
    assert L.lib.wg_quantize_q8(gpu._ctx.handle, L.WG_F32, G, *b) == L.WG_ERR_INVALID_ARG and L.lib.wg_last_error_string() == b"Quantize: buffer argument 2 is NULL"
    rc, msg = call(gpu, "f32", 8, q, s, View(xb, sh((R - 1, C, 1), R, R * C, 0)))  # q against src first
    assert rc == L.WG_ERR_DIM_MISMATCH and msg == f"Quantize: dimension mismatch. (q [{R},{C},1], src [{R - 1},{C},1])", (rc, msg)
    for bad in (0, 8, 24, 63):
        rc, msg = call(gpu, "f32", bad, q, s, x)
        assert rc == L.WG_ERR_INVALID_ARG and msg == f"Quantize: group_rows {bad} is neither a positive multiple of 16 nor at least the {R} rows of src", (rc, msg)
    rc, msg = call(gpu, "f32", 16, q, s, x)
    assert rc == L.WG_ERR_DIM_MISMATCH and msg == f"Quantize: dimension mismatch. (q [{R},{C},1], group_rows 16, scales [{NG},{C},1], expected [{R // 16},{C},1])", (rc, msg)
    assert call(gpu, "f32", 1000, q, View(sb, sh((1, C, 1), 1, C, 0)), x)[0] == 0
    for name, arr, which, need, have in (("q", np.zeros(R * C - 1, np.int8), 0, R * C, R * C - 1), ("scales", np.zeros(NG * C - 1, np.float32), 1, NG * C, NG * C - 1),
                                         ("src", np.zeros(R * C, np.float16), 2, R * C, R * C // 2)):
        ops = [q, s, x]
        ops[which] = View(_raw(gpu, arr), ops[which].shape)
        rc, msg = call(gpu, "f32", G, *ops)
        assert rc == L.WG_ERR_OUT_OF_BOUNDS and msg == f"Quantize: view `{name}` addresses {need} elements but its buffer holds {have}", (rc, msg)
    assert call(gpu, "f16", G, q, s, View(_raw(gpu, np.zeros(R * C, np.float16)), x.shape))[0] == 0  # (the same buffer holds f16 elements)
    gpu.take_path()
    assert call(gpu, "f32", G, View(qb, sh((R, 0, 1), R, 0, 0)), View(sb, sh((NG, 0, 1), NG, 0, 0)), View(xb, sh((R, 0, 1), R, 0, 0)))[0] == 0
    assert gpu.take_path() == ""


def test_aliasing(gpu):
    """On addresses, in bytes: q | scales | src touching in one buffer is legal; one shared byte between q and src, scales and src, or q and scales is refused."""
    wg, L = _wg(), _L()
    sh = wg.ViewShape
    R, C, G = 64, 4, 32
    rng = np.random.default_rng(3)
    x = rng.standard_normal((R, C)).astype(np.float32)
    raw = np.zeros(4096, np.uint8)
    Q, SC, SRC = 0, 256, 288  # bytes: q 256, scales 2 * 4 * 4 = 32, src 1024
    raw[SRC:SRC + 1024] = x.ravel(order="F").view(np.uint8)
    buf = _raw(gpu, raw)
    q = lambda off: View(buf, sh((R, C, 1), R, R * C, off))  # noqa: E731
    s = lambda off: View(buf, sh((2, C, 1), 2, 2 * C, off))  # noqa: E731
    src = View(buf, sh((R, C, 1), R, R * C, SRC // 4))
    gpu.take_path()
    rc, msg = call(gpu, "f32", G, q(Q), s(SC // 4), src)
    assert rc == 0, msg
    after = buf.read(gpu.device())
    wq, ws = wg.quantize_q8(x, G)
    assert after[:256].view(np.int8).tobytes() == wq.ravel(order="F").tobytes() and after[SC:SRC].tobytes() == ws.ravel(order="F").tobytes()
    assert after[SRC:].tobytes() == raw[SRC:].tobytes()
    gpu.queue().write_buffer(buf, 0, raw)
    gpu.take_path()
    for qv, sv, w, r in ((q(SRC - 255), s(3000 // 4), "q", "src"), (q(Q), s(SRC // 4 - 7), "scales", "src"), (q(SC - 255), s(SC // 4), "q", "scales"),
                         (q(SRC + 1023), s(SC // 4), "q", "src")):
        rc, msg = call(gpu, "f32", G, qv, sv, src)
        assert rc == L.WG_ERR_ALIASED and msg == f"Quantize: `{w}` overlaps `{r}` (the written view shares memory with a view the call reads)", (w, r, rc, msg)
    assert gpu.take_path() == "" and buf.read(gpu.device()).tobytes() == raw.tobytes()


def test_inside_a_recording():
    """No workspace: the call records on a fresh context, and the replay writes NumPy's bytes."""
    wg = _wg()
    inst = wg.GpuInstance.new(0)
    try:
        rng = np.random.default_rng(11)
        x = rng.standard_normal((96, 5, 1)).astype(np.float32)
        q, s, src = operands(inst, "f32", x, 32)
        enc = inst.device().create_command_encoder(record=True)
        try:
            rc, msg = call(inst, "f32", 32, q, s, src)
        finally:
            cb = enc.finish()
        assert rc == 0, msg
        inst.queue().submit([cb])
        wq, ws = wg.quantize_q8(x, 32)
        assert q.read().tobytes() == wq.tobytes() and s.read().tobytes() == ws.tobytes()
        del cb
    finally:
        inst.sync()


# ---- 5 -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,Gx", [(64, 32), (128, WHOLE)])
def test_end_to_end(gpu, G, Gx):
    """Random f16 activations quantised ON THE DEVICE (QuantizeQ8), fed to Gemm.dispatch_q8a8_tr, against the f64 product of the dequantised weights with the
    UNQUANTISED X. The bound is derived: an activation is off by at most half a step of its group, |x - x_scale q| <= x_scale / 2, so the product is off by at most
    sum_r |W[r, o]| x_scale[g(r), j] / 2; on top, the gate of the q8a8 arithmetic itself."""
    wg = _wg()
    dev, shapes = gpu.device(), wg.ViewShapeBuffers()
    rng = np.random.default_rng(5 + G)
    K, O, N = 512, 33, 20
    q, s = wg.quantize_q8(rng.standard_normal((K, O)).astype(np.float32), G)
    X = (rng.standard_normal((K, N)).astype(np.float32)).astype(np.float16)
    NGx = n_groups(K, Gx)
    tq, ts = wg.TensorBuilder.matrix(K, O, S_STORAGE).build_init(dev, q), wg.TensorBuilder.matrix(s.shape[0], O, S_STORAGE).build_init(dev, s)
    tX = wg.TensorBuilder.matrix(K, N, S_STORAGE).build_init(dev, X)
    tx = wg.TensorBuilder.matrix(K, N, S_STORAGE).build_init(dev, np.zeros((K, N), np.int8))
    txs = wg.TensorBuilder.matrix(NGx, N, S_STORAGE).build_init(dev, np.zeros((NGx, N), np.float32))
    to = wg.TensorBuilder.matrix(O, N, S_STORAGE).build_init(dev, np.full((O, N), NAN32))
    gpu.take_path()
    enc = dev.create_command_encoder()
    p = enc.compute_pass("w8a8", None)
    wg.QuantizeQ8.from_device(dev).dispatch(dev, shapes, p, tx, txs, tX, Gx)
    wg.Gemm.from_device(dev).dispatch_q8a8_tr(dev, shapes, p, to, tq, ts, tx, txs, G, Gx)
    p.end()
    gpu.queue().submit([enc.finish()])
    assert gpu.take_path() == f"quantize_q8/{'vec' if Gx == 32 else 'any'},f16 gemm_q8a8/mfma,nt=2,ns=1"
    got = to.read(dev).reshape(O, N, order="F").astype(np.float64)
    xq, xs = tx.read(dev).reshape(K, N, order="F"), txs.read(dev).reshape(NGx, N, order="F")
    wq, ws = wg.quantize_q8(X.astype(np.float32), Gx)
    assert np.array_equal(xq, wq) and xs.tobytes() == ws.tobytes()
    W = s.astype(np.float64)[np.arange(K) // G] * q
    truth = W.T @ X.astype(np.float64)
    xs_rows = xs.astype(np.float64)[np.arange(K) // min(Gx, K)]
    _, sabs, nch = GA.truth64(q[:, :, None], s[:, :, None], xq[:, :, None], xs[:, :, None], G, Gx)
    bound = np.abs(W).T @ xs_rows / 2 + GA.gate(nch, sabs[:, :, 0])
    err = np.abs(got - truth)
    print(f"worst err / bound = {(err / bound).max():.3g}")
    assert (err <= bound).all(), f"worst err / bound = {(err / bound).max():.3g}"
