"""wg_gemv_mixed on the GPU: a 16-bit matrix (f16 / bf16) with f32 vectors and an f32 result. Before the feature the symbol did not exist.

The contract (include/wgebra_hip.h): matrix elements widened exactly, `v` never narrowed, f32 FMAs, the f32 accumulator stored as it is; the kernels and the summation
order of the 16-bit wg_gemv for the same shape, views and context; never the Gemm kernels.

  1  every leaf ran (wg_debug_take_path), also with two matrices and with 11 right-hand sides            test_leaves_truth_order_and_determinism
  2  |got - f64 product| <= f32_gate(k, sum|m||v|): no half-ulp term, nothing is narrowed                 (same test)
  3  RNE16(mixed out) == the 16-bit wg_gemv's output, bit for bit, wherever that call stays on Gemv      (same test)
  4  odd integers above 2048 in `v` and in the results come out exactly                                   test_nothing_is_narrowed
  5  NaN in `out` is overwritten; Inf / NaN in the last column / row reach only their rows                test_special_values
  6  status codes and messages: wg_gemv's for the same mistake                                            test_status_codes, test_workspace_inside_a_recording
  7  `out` and `m` in one buffer: touching, one byte of overlap, interleaved; `out` inside `v`            test_aliasing
  8  recorded and replayed; a CU-masked context                                                           test_recorded_and_masked
  9  m_dtype = WG_F32 forwards to wg_gemv                                                                 test_f32_forwards
 10  the Python operators Gemv.dispatch_mixed / _tr / _generic on the real library                        test_python_operators
No test asserts a time.
"""
import ctypes
import faulthandler
import re

import numpy as np
import pytest

import _util as U

pytestmark = pytest.mark.gpu

S_STORAGE = 128 | 4 | 8
NAN32 = np.float32(np.nan)


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
def store(kind, flat32):
    """float32 values -> the stored element type (one RNE; exact for values that are already of that type)."""
    wg = _wg()
    flat32 = np.ascontiguousarray(flat32, np.float32)
    with np.errstate(over="ignore"):  # (a value past the largest f16 becomes Inf: that is the rounding)
        return flat32 if kind == "f32" else flat32.astype(np.float16) if kind == "f16" else wg.to_bfloat16(flat32)


def widen(kind, arr):
    wg = _wg()
    return arr.astype(np.float32) if kind != "bf16" else wg.from_bfloat16(arr)


def rne16(kind, x32):
    """f32 -> the 16-bit type -> f32: NumPy's RNE for f16, wg.to_bfloat16 for bf16."""
    return widen(kind, store(kind, x32))


def dtype_of(kind):
    L = _L()
    return {"f32": L.WG_F32, "f16": L.WG_F16, "bf16": L.WG_BF16}[kind]


class Op:
    """X[r, c, z] (float32 values) stored column-major as `kind` elements at `off`, leading dimension r + pad, `gap` elements between matrices; NaN elsewhere."""

    def __init__(self, gpu, vals, kind, off=0, pad=0, gap=0):
        wg = _wg()
        vals = np.asarray(vals, np.float32)
        R, C, Z = vals.shape
        self.kind, self.gpu = kind, gpu
        self.ld = R + pad
        self.batch = self.ld * C + gap
        self.size = off + self.batch * Z + 8
        self.idx = off + np.arange(R)[:, None, None] + np.arange(C)[None, :, None] * self.ld + np.arange(Z)[None, None, :] * self.batch
        flat = np.full(self.size, NAN32, np.float32)
        flat[self.idx] = vals
        self.init = store(kind, flat)
        self.buf = wg.TensorBuilder.tensor((self.size,), S_STORAGE).build_init(gpu.device(), self.init, self.init.dtype)
        self.shape = wg.ViewShape((R, C, Z), self.ld, self.batch, off)
        self.outside = np.ones(self.size, bool)
        self.outside[self.idx.ravel()] = False

    def poison(self):
        self.gpu.queue().write_buffer(self.buf, 0, self.init)

    def read(self, what=""):
        flat = self.buf.read(self.gpu.device())
        assert np.isnan(widen(self.kind, flat[self.outside])).all(), f"{what}: wrote outside the view"
        return np.ascontiguousarray(flat[self.idx])


def call(inst, fn_name, tr, dt, out, m, v, variant=None):
    """(status, message) of wg_gemv_mixed / wg_gemv through the C ABI."""
    wg, L = _wg(), _L()
    variant = int(wg.GemvVariant.GemvTr if tr else wg.GemvVariant.Gemv) if variant is None else int(variant)
    rc = getattr(L.lib, fn_name)(inst._ctx.handle, variant, dt, out.buf._h, out.shape.to_c(), m.buf._h, m.shape.to_c(), v.buf._h, v.shape.to_c())
    return rc, L.lib.wg_last_error_string().decode()


def mixed(inst, tr, kind, out, m, v):
    rc, msg = call(inst, "wg_gemv_mixed", tr, dtype_of(kind), out, m, v)
    assert rc == 0, msg


def tags(path):
    """The tags of a launch log: space-separated, a wrapper tag ends in '>' and the next one follows it directly."""
    return [t for t in re.split(r"[ >]", path) if t]


def product64(M, V, tr):
    """(op(M) V, |op(M)| |V|) per matrix in float64: [rows_out, nrhs, Z]."""
    M, V = np.asarray(M, np.float64), np.asarray(V, np.float64)
    A = np.transpose(M, (1, 0, 2)) if tr else M
    return np.einsum("rkz,kyz->ryz", A, V), np.einsum("rkz,kyz->ryz", np.abs(A), np.abs(V))


# ---- the leaves (plan_nsplit on 256 CUs; the tags are what wg_gemv logs for the 16-bit call of the same shape) ----------------------------------------------
# name, GemvTr, stored rows, stored columns, right-hand sides, matrices, matrix (offset, ld padding), vector offset, tags that must appear after the element prefix
CASES = [
    ("small", False, 1024, 1024, 1, 1, (0, 0), 0, ["gemv.small/rl=2"]),
    ("n_split", False, 64, 256, 1, 1, (0, 0), 0, ["gemv.n/t=1,ns=4", "gemv.combine/ns=4"]),
    ("n_split_2mats", False, 64, 256, 2, 2, (4, 4), 0, ["gemv.n/t=2,ns=", "gemv.combine/ns="]),
    ("n_11rhs", False, 64, 256, 11, 1, (0, 0), 0, ["gemv.n/t=8,ns=", "gemv.combine/ns="]),
    ("t_3rhs", True, 512, 256, 3, 1, (0, 0), 0, ["gemv.t/t=4,ns=1"]),
    ("t_11rhs", True, 512, 256, 11, 1, (0, 0), 0, ["gemv.t/t=8,ns=1"]),
    ("tcols_e8", True, 1024, 512, 1, 1, (0, 0), 0, ["gemv.tcols/e=8,u=4,v=1,ns=1"]),
    ("tcols_e8_2mats", True, 1024, 512, 1, 2, (8, 8), 0, ["gemv.tcols/e=8,u=4,v=1,ns=1"]),
    ("tcols_e4", True, 1024, 512, 1, 1, (0, 4), 0, ["gemv.tcols/e=4,u=4,v=1,ns=1"]),  # leading dimension 1028 = 4 mod 8: 8-byte loads
    ("tcols_u8", True, 4096, 4096, 1, 1, (0, 0), 0, ["gemv.tcols/e=8,u=8,v=1,ns=1"]),  # 16 chunks of 256 rows: whole trips of 8 loads (the smallest matrix that takes them)
    ("tcols_v2", True, 256, 2048, 2, 1, (0, 0), 0, ["gemv.tcols/e=8,u=4,v=2,ns=1"]),
    ("tcols_v2_e4", True, 260, 2048, 2, 1, (4, 0), 0, ["gemv.tcols/e=4,u=4,v=2,ns=1"]),  # (an 8-byte-aligned matrix)
    ("any_n", False, 130, 70, 1, 1, (1, 3), 0, ["gemv_any/n,ns="]),
    ("any_t", True, 130, 70, 2, 1, (1, 3), 0, ["gemv_any/t,ns="]),
    ("staged_vectors", False, 64, 256, 1, 1, (0, 0), 1, ["stage>", "gemv.n/t=1,ns=4"]),  # v and out at offset 1: f32 copies, the matrix on the vec4 kernels
]
KINDS = ["f16", "bf16"]


def build_case(gpu, case, kind, rng, v16=False, integers=False):
    name, tr, R, C, nrhs, Z, (moff, mpad), voff, tags = case
    k, ro = (R, C) if tr else (C, R)
    if integers:
        Mv = rng.integers(-2, 3, (R, C, Z)).astype(np.float32)
        Vv = ((2049 + 2 * rng.integers(0, 500, (k, nrhs, Z))) * rng.choice([-1, 1], (k, nrhs, Z))).astype(np.float32)
    else:
        Mv = widen(kind, store(kind, rng.random((R, C, Z), dtype=np.float32) * 2 - 1))
        Vv = rng.random((k, nrhs, Z), dtype=np.float32) * 2 - 1
        if v16:
            Vv = rne16(kind, Vv)
    m = Op(gpu, Mv, kind, off=moff, pad=mpad, gap=mpad)
    v = Op(gpu, Vv, "f32", off=voff, pad=voff, gap=0)
    out = Op(gpu, np.full((ro, nrhs, Z), NAN32), "f32", off=voff, pad=voff, gap=0)
    return tr, k, Mv, Vv, m, v, out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_leaves_truth_order_and_determinism(gpu, case, kind):
    """Items 1, 2, 3 and the determinism clause: v is drawn in the 16-bit type and widened, so that the 16-bit wg_gemv sees the same operands."""
    wg = _wg()
    rng = np.random.default_rng(sum(map(ord, case[0])) + len(kind))
    tr, k, Mv, Vv, m, v, out = build_case(gpu, case, kind, rng, v16=True)
    gpu.take_path()
    mixed(gpu, tr, kind, out, m, v)
    path = gpu.take_path()
    print(case[0], kind, "->", path)
    got = out.read(case[0])  # (out was NaN everywhere: overwritten inside the view, untouched outside)
    # 1: the leaf
    pos = 0
    for tag in case[8]:
        assert tag in path[pos:], f"{case[0]}: expected {case[8]} in order, the call took '{path}'"
        pos = path.index(tag, pos)
    if "gemv_any" not in path:
        assert f"{kind}w.gemv" in tags(path) and f"{kind}.gemv" not in tags(path), path
    assert "gemm" not in path and ".m16" not in path and "skinny" not in path, f"the mixed call took a Gemm kernel: {path}"
    # 2: the truth, with the f32 gate alone
    truth, sabs = product64(Mv, Vv, tr)
    r = U.assert_close_f64(got, truth, k, sabs, f"{case[0]} {kind}")
    print(f"  worst err / gate = {r:.3g}")
    # determinism: the same bits again
    out.poison()
    mixed(gpu, tr, kind, out, m, v)
    U.assert_bits_equal(out.read(), got, f"{case[0]} {kind}: second call")
    # 3: the order pin against the unchanged 16-bit call, where that call stays on the Gemv kernels
    v16 = Op(gpu, Vv, kind, off=v.shape.offset, pad=v.shape.offset)
    o16 = Op(gpu, np.full(got.shape, NAN32), kind, off=out.shape.offset, pad=out.shape.offset)
    gpu.take_path()
    rc, msg = call(gpu, "wg_gemv", tr, dtype_of(kind), o16, m, v16)
    assert rc == 0, msg
    p16 = gpu.take_path()
    if f"{kind}.gemv" in tags(p16):
        assert p16.replace(f"{kind}.gemv", f"{kind}w.gemv") == path, (p16, path)
        U.assert_bits_equal(store(kind, got), o16.read(), f"{case[0]} {kind}: RNE16(mixed) against the 16-bit wg_gemv ({p16})")
    else:
        print(f"  the 16-bit call left the Gemv kernels ({p16}): no order pin")
        assert case[0] in ("n_11rhs", "t_11rhs", "any_n", "any_t"), (case[0], p16)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", [c for c in CASES if c[0] in ("small", "n_split_2mats", "n_11rhs", "t_3rhs", "tcols_e8", "tcols_e4", "tcols_v2", "any_n", "any_t", "staged_vectors")],
                         ids=lambda c: c[0])
def test_nothing_is_narrowed(gpu, case, kind):
    """Integer operands whose every partial sum stays below 2^24 (|m| <= 2, |v| < 3049, k <= 1024: 6.3e6): any order gives the exact sum. v holds odd integers above
    2048 -- not f16 values, not bf16 values --, and so do results: a pass of v or of out through 16 bits anywhere changes them."""
    rng = np.random.default_rng(7 + sum(map(ord, case[0])))
    tr, k, Mv, Vv, m, v, out = build_case(gpu, case, kind, rng, integers=True)
    assert (np.abs(Vv) > 2048).all() and (Vv % 2 == 1).all() and not np.array_equal(rne16(kind, Vv), Vv)
    truth, sabs = product64(Mv, Vv, tr)
    assert sabs.max() < 2 ** 24
    odd_big = (np.abs(truth) > 2048) & (truth % 2 == 1)
    assert odd_big.any() and not np.array_equal(rne16(kind, truth.astype(np.float32)), truth.astype(np.float32))
    mixed(gpu, tr, kind, out, m, v)
    got = out.read(case[0])
    assert np.array_equal(got.astype(np.float64), truth), f"{case[0]} {kind}: {np.count_nonzero(got != truth)} of {got.size} results are not the exact integer product"


# k is not a multiple of 64: the last trip of every kernel is a partial one
SPECIAL = [("n_split", False, 64, 100), ("small", False, 256, 100), ("t", True, 100, 64), ("tcols", True, 100, 256), ("tcols_wide_tail", True, 1000, 256), ("any_n", False, 66, 101), ("any_t", True, 101, 66)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,tr,R,C", SPECIAL, ids=[s[0] for s in SPECIAL])
def test_special_values(gpu, name, tr, R, C, kind):
    """out is pre-filled with NaN (Op) and must be overwritten; Inf and NaN sit in the last valid column (Gemv) / row (GemvTr) of the matrix and reach exactly the
    results the mathematics gives them (load slots past the end contribute an exact zero, not (last column) x 0)."""
    rng = np.random.default_rng(R * 3 + C)
    k, ro = (R, C) if tr else (C, R)
    nrhs = 2 if name == "t" else 1
    Mv = rng.integers(-3, 4, (R, C, 1)).astype(np.float32)
    Vv = rng.integers(1, 5, (k, nrhs, 1)).astype(np.float32)
    i_inf, i_nan, i_ninf = 1, ro // 2, ro - 1
    for i, val in ((i_inf, np.inf), (i_nan, np.nan), (i_ninf, -np.inf)):
        if tr:
            Mv[k - 1, i, 0] = val
        else:
            Mv[i, k - 1, 0] = val
    m, v, out = Op(gpu, Mv, kind), Op(gpu, Vv, "f32"), Op(gpu, np.full((ro, nrhs, 1), NAN32), "f32")
    gpu.take_path()
    mixed(gpu, tr, kind, out, m, v)
    print(name, kind, "->", gpu.take_path())
    got = out.read(name)
    A = np.transpose(Mv, (1, 0, 2)) if tr else Mv
    want = U.special_product(A, Vv, np.float32)
    U.assert_same_class_bits(got, want, f"{name} {kind}")
    assert np.isnan(got[i_nan]).all() and (got[i_inf] == np.inf).all() and (got[i_ninf] == -np.inf).all()
    assert np.isfinite(np.delete(got, [i_inf, i_nan, i_ninf], axis=0)).all()


def test_status_codes(gpu):
    """Each status of the C ABI, with wg_gemv's message for the same mistake (the 16-bit call on 16-bit vectors of the same shapes)."""
    wg, L = _wg(), _L()
    kind = "f16"
    rng = np.random.default_rng(3)
    R, C = 64, 128
    Mv = rng.integers(-2, 3, (R, C, 1)).astype(np.float32)
    m = Op(gpu, Mv, kind)
    ops = {}
    for vk in ("f32", kind):  # f32 vectors for the mixed call, 16-bit ones for wg_gemv
        ops[vk] = dict(v=Op(gpu, np.ones((C, 1, 1)), vk), out=Op(gpu, np.zeros((R, 1, 1)), vk), v_bad=Op(gpu, np.ones((C + 4, 1, 1)), vk),
                       out_bad=Op(gpu, np.zeros((R + 4, 1, 1)), vk), out6=Op(gpu, np.zeros((6, 1, 1)), vk), vt=Op(gpu, np.ones((R, 1, 1)), vk))
    m6 = Op(gpu, np.ones((6, 8, 1)), kind)
    m6t = Op(gpu, np.ones((8, 6, 1)), kind)
    v8 = {vk: Op(gpu, np.ones((8, 1, 1)), vk) for vk in ("f32", kind)}
    V = wg.GemvVariant

    def both(tr, o, mm, vv, variant=None):
        a = call(gpu, "wg_gemv_mixed", tr, dtype_of(kind), ops["f32"][o] if isinstance(o, str) else o["f32"], mm, ops["f32"][vv] if isinstance(vv, str) else vv["f32"], variant)
        b = call(gpu, "wg_gemv", tr, dtype_of(kind), ops[kind][o] if isinstance(o, str) else o[kind], mm, ops[kind][vv] if isinstance(vv, str) else vv[kind], variant)
        assert a == b, (a, b)
        return a

    gpu.take_path()
    rc, msg = both(False, "out", m, "v_bad")
    assert rc == L.WG_ERR_DIM_MISMATCH and msg == f"Gemv: dimension mismatch. (out [{R},1,1], m [{R},{C},1], v [{C + 4},1,1])"
    rc, msg = both(False, "out_bad", m, "v")
    assert rc == L.WG_ERR_DIM_MISMATCH and "dimension mismatch" in msg
    rc, msg = both(True, "v", m, "vt")  # the transposed product of the same matrix is fine ...
    assert rc == 0
    rc, msg = both(True, "out", m, "v")  # ... and its mismatch names the transpose
    assert rc == L.WG_ERR_DIM_MISMATCH and "]^T, v [" in msg
    o6 = {vk: ops[vk]["out6"] for vk in ops}
    rc, msg = both(False, o6, m6, v8, V.GemvFast)
    assert rc == L.WG_ERR_PRECONDITION and msg == "Gemv: assertion `left == right` failed (out_nrows % 4 == 0, gemv.rs:122): out has 6 rows"
    rc, msg = both(True, o6, m6t, v8, V.GemvTrFast)  # 8 rows % 128 != 0: silently GemvTr, which takes 6 outputs
    assert rc == 0, msg
    assert np.array_equal(o6["f32"].read(), np.full((6, 1, 1), 8, np.float32))
    rc, msg = call(gpu, "wg_gemv_mixed", False, dtype_of(kind), ops["f32"]["out"], m, ops["f32"]["v"], 9)
    assert rc == L.WG_ERR_INVALID_ARG and msg == "Gemv: unknown variant 9"
    rc, msg = call(gpu, "wg_gemv_mixed", False, 7, ops["f32"]["out"], m, ops["f32"]["v"])
    assert rc == L.WG_ERR_INVALID_ARG and msg == "Gemv: unknown dtype 7"
    # zero-sized views are skipped
    z_out, z_v = Op(gpu, np.zeros((R, 1, 1)), "f32"), Op(gpu, np.ones((C, 1, 1)), "f32")
    z_out.shape = wg.ViewShape((R, 0, 1), R, R, 0)
    before = z_out.buf.read(gpu.device()).copy()
    assert call(gpu, "wg_gemv_mixed", False, dtype_of(kind), z_out, m, z_v)[0] == 0
    assert z_out.buf.read(gpu.device()).tobytes() == before.tobytes()
    # ... and so are zero-sized BUFFERS: each operand in turn is a buffer of 0 bytes under a view that a bounds check would refuse -- WG_OK, nothing launched or written
    h0 = ctypes.c_void_p()
    L.check(L.lib.wg_buf_create(gpu._ctx.handle, 0, S_STORAGE, ctypes.byref(h0)))
    try:
        o_ok, v_ok = ops["f32"]["out"], ops["f32"]["v"]
        before = o_ok.buf.read(gpu.device()).copy()
        gpu.take_path()
        for which in range(3):
            hs = [h0 if i == which else b.buf._h for i, b in enumerate((o_ok, m, v_ok))]
            for fn in ("wg_gemv_mixed", "wg_gemv"):  # (wg_gemv skips before it looks at element sizes: the same rule)
                rc = getattr(L.lib, fn)(gpu._ctx.handle, 0, dtype_of(kind), hs[0], o_ok.shape.to_c(), hs[1], m.shape.to_c(), hs[2], v_ok.shape.to_c())
                assert rc == 0, (fn, which, L.lib.wg_last_error_string().decode())
        assert gpu.take_path() == "" and o_ok.buf.read(gpu.device()).tobytes() == before.tobytes()
    finally:
        L.check(L.lib.wg_buf_destroy(h0))
    # bounds use each operand's own element size: a `v` buffer sized as if it held 16-bit elements (C * 2 bytes = C / 2 floats)
    half_v = Op(gpu, np.ones((C // 2 - 8, 1, 1)), "f32")  # (Op adds 8 elements of margin: the buffer holds C / 2 floats)
    assert half_v.size == C // 2
    half_v.shape = wg.ViewShape((C, 1, 1), C, C, 0)
    rc, msg = call(gpu, "wg_gemv_mixed", False, dtype_of(kind), ops["f32"]["out"], m, half_v)
    assert rc == L.WG_ERR_OUT_OF_BOUNDS and msg == f"Gemv: view `v` addresses {C} elements but its buffer holds {C // 2}"
    small_m = Op(gpu, np.ones((R, C // 2, 1)), kind)
    small_m.shape = wg.ViewShape((R, C, 1), R, R * C, 0)
    rc, msg = call(gpu, "wg_gemv_mixed", False, dtype_of(kind), ops["f32"]["out"], small_m, ops["f32"]["v"])
    assert rc == L.WG_ERR_OUT_OF_BOUNDS and msg == f"Gemv: view `m` addresses {R * C} elements but its buffer holds {small_m.size}"
    # nmats * ceil(nrhs / 8) > 65535: the limit of the launcher stays
    many = Op(gpu, np.zeros((4, 1, 65536)), "f32")
    m4, v4 = Op(gpu, np.ones((4, 4, 1)), kind), Op(gpu, np.ones((4, 1, 1)), "f32")
    m4.shape, v4.shape = wg.ViewShape((4, 4, 1), 4, 0, 0), wg.ViewShape((4, 1, 1), 4, 0, 0)
    rc, msg = call(gpu, "wg_gemv_mixed", False, dtype_of(kind), many, m4, v4)
    assert rc == L.WG_ERR_UNSUPPORTED and msg == "Gemv: nmats * ceil(nrhs/8) = 65536 exceeds 65535"


def test_workspace_inside_a_recording():
    """Vectors that are off are staged as f32 copies in a context scratch: on a fresh context that scratch cannot grow inside a recording (WG_ERR_WORKSPACE, as
    wg_gemv); after one eager call the same call records."""
    wg, L = _wg(), _L()
    inst = wg.GpuInstance.new(0)
    try:
        rng = np.random.default_rng(5)
        Mv, Vv = rng.integers(-2, 3, (64, 64, 1)).astype(np.float32), rng.integers(-2, 3, (64, 1, 1)).astype(np.float32)
        m, v, out = Op(inst, Mv, "bf16"), Op(inst, Vv, "f32", off=1), Op(inst, np.full((64, 1, 1), NAN32), "f32", off=3)
        enc = inst.device().create_command_encoder(record=True)
        try:
            rc, msg = call(inst, "wg_gemv_mixed", False, L.WG_BF16, out, m, v)
        finally:
            cb = enc.finish()
        assert rc == L.WG_ERR_WORKSPACE, (rc, msg)
        del cb
        mixed(inst, False, "bf16", out, m, v)
        want = out.read()
        assert np.array_equal(want.astype(np.float64), product64(Mv, Vv, False)[0])
        out.poison()
        enc = inst.device().create_command_encoder(record=True)
        try:
            rc, msg = call(inst, "wg_gemv_mixed", False, L.WG_BF16, out, m, v)
        finally:
            cb = enc.finish()
        assert rc == 0, msg
        inst.queue().submit([cb])
        U.assert_bits_equal(out.read(), want, "staged vectors, replayed")
        del cb
    finally:
        inst.sync()


@pytest.mark.parametrize("kind", KINDS)
def test_aliasing(gpu, kind):
    """`out` (f32) and `m` (16-bit) in ONE buffer, decided on addresses in 2-byte units."""
    wg, L = _wg(), _L()
    rng = np.random.default_rng(11)
    R, C = 64, 256
    Mv = rng.integers(-2, 3, (R, C, 1)).astype(np.float32)
    Vv = rng.integers(-3, 4, (C, 1, 1)).astype(np.float32)
    truth = product64(Mv, Vv, False)[0]
    v = Op(gpu, Vv, "f32")

    class Shared:  # one buffer: R floats of `out` at byte 0, then the matrix from byte 4 R on (16-bit element 2 R)
        pass
    raw = np.zeros(2 * R + R * C + 8, np.uint16)
    raw[: 2 * R] = np.full(R, NAN32).view(np.uint16)
    raw[2 * R: 2 * R + R * C] = store(kind, Mv.ravel(order="F")).view(np.uint16)
    buf = wg.TensorBuilder.tensor((raw.size,), S_STORAGE).build_init(gpu.device(), raw, raw.dtype)
    o, mm = Shared(), Shared()
    o.buf = mm.buf = buf
    o.shape = wg.ViewShape((R, 1, 1), R, R, 0)           # f32 elements 0 .. R
    mm.shape = wg.ViewShape((R, C, 1), R, R * C, 2 * R)  # 16-bit elements from 2 R on: begins exactly where out ends
    gpu.take_path()
    rc, msg = call(gpu, "wg_gemv_mixed", False, dtype_of(kind), o, mm, v)
    assert rc == 0, msg
    after = buf.read(gpu.device())
    assert np.array_equal(after[: 2 * R].view(np.float32).astype(np.float64), truth.ravel()), "touching views: wrong result"
    assert np.array_equal(after[2 * R:], raw[2 * R:]), "touching views: the matrix changed"
    # the matrix one 16-bit element earlier: the last two bytes of out are shared -> refused, nothing written, nothing logged
    gpu.queue().write_buffer(buf, 0, raw)
    gpu.take_path()
    mm.shape = wg.ViewShape((R, C, 1), R, R * C, 2 * R - 1)
    rc, msg = call(gpu, "wg_gemv_mixed", False, dtype_of(kind), o, mm, v)
    assert rc == L.WG_ERR_ALIASED and msg == "Gemv: `out` overlaps `m` (the written view shares memory with a view the call reads)", (rc, msg)
    assert gpu.take_path() == "" and buf.read(gpu.device()).tobytes() == raw.tobytes()
    # ONE byte of overlap: a second handle over the same allocation (wg_buf_wrap) that starts at the last byte of out -- refused on addresses before anything is read
    base = L.lib.wg_buf_device_ptr(buf._h)
    h = ctypes.c_void_p()
    L.check(L.lib.wg_buf_wrap(gpu._ctx.handle, ctypes.c_void_p(base + 4 * R - 1), 2 * R * C, ctypes.byref(h)))
    try:
        rc = L.lib.wg_gemv_mixed(gpu._ctx.handle, 0, dtype_of(kind), buf._h, o.shape.to_c(), h, wg.ViewShape((R, C, 1), R, R * C, 0).to_c(), v.buf._h, v.shape.to_c())
        assert rc == L.WG_ERR_ALIASED and "`out` overlaps `m`" in L.lib.wg_last_error_string().decode()
        L.check(L.lib.wg_buf_wrap(gpu._ctx.handle, ctypes.c_void_p(base + 4 * R), 2 * R * C, ctypes.byref(h2 := ctypes.c_void_p())))
        rc = L.lib.wg_gemv_mixed(gpu._ctx.handle, 0, dtype_of(kind), buf._h, o.shape.to_c(), h2, wg.ViewShape((R, C, 1), R, R * C, 0).to_c(), v.buf._h, v.shape.to_c())
        assert rc == 0, L.lib.wg_last_error_string().decode()  # (one byte further: touching again)
        L.check(L.lib.wg_buf_destroy(h2))
    finally:
        L.check(L.lib.wg_buf_destroy(h))
    assert gpu.take_path() != "" and np.array_equal(buf.read(gpu.device())[: 2 * R].view(np.float32).astype(np.float64), truth.ravel())

    # out interleaved between the columns of a strided matrix: m is 8 x 16 with leading dimension 24 (16-bit elements); the 16 elements of padding behind column j
    # are 8 floats = out[:, j] for j < 3 (f32 offset 4 + 12 j)
    R2, C2, ld, nrhs = 8, 16, 24, 3
    M2 = rng.integers(-2, 3, (R2, C2, 1)).astype(np.float32)
    V2 = rng.integers(-3, 4, (C2, nrhs, 1)).astype(np.float32)
    raw2 = np.zeros(ld * C2 + 8, np.uint16)
    midx = (np.arange(R2)[:, None] + np.arange(C2)[None, :] * ld)
    raw2[midx] = store(kind, M2[:, :, 0]).view(np.uint16)
    buf2 = wg.TensorBuilder.tensor((raw2.size,), S_STORAGE).build_init(gpu.device(), raw2, raw2.dtype)
    o2, m2, v2 = Shared(), Shared(), Op(gpu, V2, "f32")
    o2.buf = m2.buf = buf2
    o2.shape = wg.ViewShape((R2, nrhs, 1), ld // 2, 0, R2 // 2)
    m2.shape = wg.ViewShape((R2, C2, 1), ld, 0, 0)
    rc, msg = call(gpu, "wg_gemv_mixed", False, dtype_of(kind), o2, m2, v2)
    assert rc == 0, msg
    after2 = buf2.read(gpu.device())
    oidx = R2 // 2 + np.arange(R2)[:, None] + np.arange(nrhs)[None, :] * (ld // 2)
    assert np.array_equal(after2.view(np.float32)[oidx].astype(np.float64), product64(M2, V2, False)[0][:, :, 0]), "interleaved views: wrong result"
    assert np.array_equal(after2[midx], raw2[midx]), "interleaved views: the matrix changed"
    o2.shape = wg.ViewShape((R2, nrhs, 1), ld // 2, 0, R2 // 2 - 1)  # one float earlier: the last two elements of every column of m
    rc, msg = call(gpu, "wg_gemv_mixed", False, dtype_of(kind), o2, m2, v2)
    assert rc == L.WG_ERR_ALIASED and "`out` overlaps `m`" in msg

    # out = a column range of v
    k = 64
    M3 = rng.integers(-2, 3, (k, k, 1)).astype(np.float32)
    m3, v3 = Op(gpu, M3, kind), Op(gpu, rng.integers(-3, 4, (k, 3, 1)).astype(np.float32), "f32")
    before = v3.buf.read(gpu.device()).copy()
    o3 = Shared()
    o3.buf = v3.buf
    o3.shape = wg.ViewShape((k, 2, 1), k, 2 * k, k)  # columns 1 and 2 of v
    v3.shape = wg.ViewShape((k, 2, 1), k, 2 * k, 0)  # columns 0 and 1
    gpu.take_path()
    rc, msg = call(gpu, "wg_gemv_mixed", False, dtype_of(kind), o3, m3, v3)
    assert rc == L.WG_ERR_ALIASED and msg == "Gemv: `out` overlaps `v` (the written view shares memory with a view the call reads)", (rc, msg)
    assert gpu.take_path() == "" and v3.buf.read(gpu.device()).tobytes() == before.tobytes()


@pytest.fixture(scope="module")
def masked():
    wg = _wg()
    inst = wg.GpuInstance.new(0, cu_count=248, one_xcd=True)
    yield inst
    inst.sync()


REPLAY = [c for c in CASES if c[0] in ("n_split", "tcols_e8", "small")]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("where", ["whole", "masked"])
def test_recorded_and_masked(gpu, masked, where, kind):
    """Eager, then recorded once and replayed twice into a re-poisoned output: the eager bits each time. On the whole chip and on a CU-masked context (248 CUs: the
    plan reads compute_units), where the truth gate and determinism hold."""
    inst = gpu if where == "whole" else masked
    for case in REPLAY:
        rng = np.random.default_rng(len(case[0]) + len(kind))
        tr, k, Mv, Vv, m, v, out = build_case(inst, case, kind, rng)
        inst.take_path()
        mixed(inst, tr, kind, out, m, v)
        log = inst.take_path()
        eager = out.read(case[0])
        truth, sabs = product64(Mv, Vv, tr)
        U.assert_close_f64(eager, truth, k, sabs, f"{case[0]} {kind} {where}")
        out.poison()
        enc = inst.device().create_command_encoder(record=True)
        try:
            mixed(inst, tr, kind, out, m, v)
        finally:
            cb = enc.finish()
        assert inst.take_path() == log
        for rep in range(2):
            out.poison()
            inst.queue().submit([cb])
            U.assert_bits_equal(out.read(case[0]), eager, f"{case[0]} {kind} {where}: replay {rep}")
        del cb


@pytest.mark.parametrize("tr", [False, True])
def test_f32_forwards(gpu, tr):
    """m_dtype = WG_F32: wg_gemv(WG_F32) unchanged -- the same log, the same bits."""
    L = _L()
    rng = np.random.default_rng(17)
    R, C = (512, 256)
    k, ro = (R, C) if tr else (C, R)
    Mv, Vv = rng.random((R, C, 1), dtype=np.float32) * 2 - 1, rng.random((k, 2, 1), dtype=np.float32) * 2 - 1
    m, v = Op(gpu, Mv, "f32"), Op(gpu, Vv, "f32")
    res, logs = [], []
    for fn in ("wg_gemv", "wg_gemv_mixed"):
        out = Op(gpu, np.full((ro, 2, 1), NAN32), "f32")
        gpu.take_path()
        rc, msg = call(gpu, fn, tr, L.WG_F32, out, m, v)
        assert rc == 0, msg
        logs.append(gpu.take_path())
        res.append(out.read(fn))
    assert logs[0] == logs[1] and "f32.gemv" in tags(logs[0])
    U.assert_bits_equal(res[1], res[0], "wg_gemv_mixed(WG_F32) against wg_gemv(WG_F32)")


@pytest.mark.parametrize("kind", KINDS + ["f32"])
def test_python_operators(gpu, kind):
    """Gemv.dispatch_mixed / dispatch_mixed_tr / dispatch_mixed_generic on tensors, through a compute pass: the exact integer product of test_nothing_is_narrowed (odd
    integers above 2048 in `v` and in results), the mixed element prefix in the launch log (a float32 matrix forwards to the f32 call), NaN in `out` overwritten."""
    wg = _wg()
    dev, shapes = gpu.device(), wg.ViewShapeBuffers()
    rng = np.random.default_rng(23)
    R, C = 64, 256
    Mv = rng.integers(-2, 3, (R, C, 1)).astype(np.float32)
    m16 = store(kind, Mv.ravel(order="F"))
    tm = wg.TensorBuilder.tensor((R, C), S_STORAGE).build_init(dev, m16, m16.dtype)
    op = wg.Gemv.from_device(dev)
    V = wg.GemvVariant
    for method, tr, extra in (("dispatch_mixed", False, ()), ("dispatch_mixed_tr", True, ()), ("dispatch_mixed_generic", False, (V.Gemv,)),
                              ("dispatch_mixed_generic", True, (V.GemvTr,))):
        k, ro = (R, C) if tr else (C, R)
        Vv = ((2049 + 2 * rng.integers(0, 500, (k, 1, 1))) * rng.choice([-1, 1], (k, 1, 1))).astype(np.float32)
        truth = product64(Mv, Vv, tr)[0]
        assert ((np.abs(truth) > 2048) & (truth % 2 == 1)).any()
        tv = wg.TensorBuilder.tensor((k,), S_STORAGE).build_init(dev, Vv.ravel(), np.float32)
        to = wg.TensorBuilder.tensor((ro,), S_STORAGE).build_init(dev, np.full(ro, NAN32), np.float32)
        gpu.take_path()
        enc = dev.create_command_encoder()
        p = enc.compute_pass("mixed", None)
        getattr(op, method)(dev, shapes, p, to, tm, tv, *extra)
        p.end()
        gpu.queue().submit([enc.finish()])
        got = to.read(dev)
        path = gpu.take_path()
        assert (f"{kind}w.gemv" if kind != "f32" else "f32.gemv") in tags(path), (method, path)
        assert np.array_equal(np.asarray(got, np.float64).ravel(), truth.ravel()), f"{method} {kind}: not the exact integer product"
