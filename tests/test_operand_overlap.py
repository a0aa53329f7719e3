"""Operand views that share memory (include/wgebra_hip.h, "the aliasing rule"): a call whose written footprint shares a byte with a footprint it reads is refused with
WG_ERR_ALIASED before anything is launched; views of one buffer with disjoint footprints -- touching, interleaved -- are legal; OpAssign and Axpy take the identical
view on both sides.

CPU   test_predicate_matches_brute_force   wg_debug_views_overlap against the intersection of the two byte sets built with NumPy, a few thousand seeded pairs of small
                                           views; zero-sized views; a pair above the run bound (exact == 0). (tests/test_cpp_overlap.py: the same under the sanitizers.)
GPU   test_in_place_elementwise            OpAssign (five ops) and Axpy with `a` and `b` the same view: bit-equal to NumPy's x (op) x, NaN as a class
      test_refused_*                       every entry point, every (written, read) pair, identical views and views that share exactly one element: AliasedOperands
                                           naming both views, an empty launch log, the buffer bit-unchanged, a valid call right afterwards; one refusal inside a recording
      test_packed_*                        all operands of a call back to back in one buffer, the first at element 1: the result within the dense tests' bound of the
                                           f64 product (no NaN: an over-read brings one in), every input element and guard bit-unchanged (an over-write corrupts one)
      test_interleaved_gemm                the output's columns in the leading-dimension padding of m1
      test_refused_sharded_gemm_one_launch the one-launch M-sharded Gemm (wg_gemm_f16_panels) with an operand in the staging cube; wg_gemm_sharded's own `out` check
      test_prod_keeps_the_sign_of_an_exact_zero   the kernel fault these tests found (a 16-bit Prod whose f32 product is -0 came out as +0), on every Reduce entry
CPU   test_reduce_rounds_its_f32_result_not_a_fused_product   the same fault seen in the ISA
"""
import ctypes

import numpy as np
import pytest

import _bf16 as B
import _util as U

S_STORAGE = 128 | 4 | 8  # STORAGE | COPY_SRC | COPY_DST


def _wg():
    import wgmath_amd as wg
    return wg


def _L():
    from wgmath_amd import _lib
    return _lib


# ========================================================================================================
# CPU: the predicate
# ========================================================================================================
def _predicate(a, base_a, b, base_b, es):
    L = _L()
    exact = ctypes.c_int(-1)
    r = L.lib.wg_debug_views_overlap(L.ViewShapeC((ctypes.c_uint32 * 3)(*a[:3]), a[3], a[4], a[5]), base_a,
                                     L.ViewShapeC((ctypes.c_uint32 * 3)(*b[:3]), b[3], b[4], b[5]), base_b, es, ctypes.byref(exact))
    return r, exact.value


def _elements(v):
    """Element indices t*stride_mat + offset + i + j*stride of the view (rows, cols, mats, stride, stride_mat, offset)."""
    rows, cols, mats, stride, stride_mat, offset = v
    i, j, t = np.arange(rows, dtype=np.int64)[:, None, None], np.arange(cols, dtype=np.int64)[None, :, None], np.arange(mats, dtype=np.int64)[None, None, :]
    return (t * stride_mat + offset + i + j * stride).ravel()


def _byte_set(v, base, es):
    return np.unique((base + _elements(v)[:, None] * es + np.arange(es, dtype=np.int64)[None, :]).ravel())


def _random_view(rng):
    rows, cols, mats = int(rng.choice([0, 1, 3, 4, 5, 8])), int(rng.choice([0, 1, 3, 4, 5, 8])), int(rng.integers(1, 4))
    stride = int(rng.choice([rows, rows + 1, rows + 3, 2 * rows]))
    mat = stride * max(cols, 1)
    stride_mat = int(rng.choice([rows * cols, mat, mat + 3, 2 * mat, 1]))  # dense, whole columns, a gap, room for another view between, GpuCubeView::matrix's 1
    return (rows, cols, mats, stride, stride_mat, int(rng.choice([0, 1, 3, 4, 7])))


def _extent(v):
    e = _elements(v)
    return int(e.max()) + 1 if e.size else 0


def test_predicate_matches_brute_force():
    rng = np.random.default_rng(20250)
    base_a = 1 << 20
    seen = {"overlap": 0, "disjoint": 0, "empty": 0, "touching": 0, "interleaved": 0}
    for it in range(4000):
        a, b, es = _random_view(rng), _random_view(rng), int(rng.choice([2, 4]))
        ea, eb = _extent(a), _extent(b)
        kind = it % 7
        if kind == 0:    # disjoint: b wholly behind a
            base_b = base_a + (ea + 16) * es
        elif kind == 1:  # touching: b's first byte is the byte behind a's last
            base_b = base_a + (ea - b[5]) * es
        elif kind == 2:  # shifted by one element, either way
            base_b = base_a + es
        elif kind == 3:
            base_b = base_a - es
        elif kind == 4:  # anywhere from wholly in front to wholly behind: views that interleave
            base_b = base_a + (int(rng.integers(0, ea + eb + 1)) - eb) * es
        elif kind == 5:  # identical bases: two views of one buffer
            base_b = base_a
        else:            # the same view one column height further: in the leading-dimension padding where there is enough of it, across a column end otherwise
            b, eb, base_b = a, ea, base_a + a[0] * es
        sa, sb = _byte_set(a, base_a, es), _byte_set(b, base_b, es)
        want = int(np.intersect1d(sa, sb, assume_unique=True).size > 0)
        got, exact = _predicate(a, base_a, b, base_b, es)
        assert exact == 1, f"{a} @ {base_a}, {b} @ {base_b}, es {es}: a small pair answered conservatively"
        assert got == want, f"{a} @ {base_a}, {b} @ {base_b}, es {es}: predicate {got}, the byte sets {'intersect' if want else 'are disjoint'}"
        assert _predicate(b, base_b, a, base_a, es) == (got, exact)
        if not sa.size or not sb.size:
            assert got == 0  # a zero-sized view overlaps nothing
            seen["empty"] += 1
        else:
            seen["overlap" if want else "disjoint"] += 1
            if not want and sa[0] < sb[-1] and sb[0] < sa[-1]:
                seen["interleaved"] += 1  # the intervals intersect, the footprints do not: decided by the walk
            if not want and (sa[-1] + 1 == sb[0] or sb[-1] + 1 == sa[0]):
                seen["touching"] += 1
    assert min(seen.values()) >= 50, f"the pairs do not cover every kind: {seen}"
    # zero-sized views, whatever their other fields, at the very address of the other view
    dense = (8, 8, 2, 8, 64, 0)
    for empty in ((0, 8, 2, 8, 64, 0), (8, 0, 2, 8, 64, 0), (8, 8, 0, 8, 64, 0)):
        assert _predicate(empty, base_a, dense, base_a, 4) == (0, 1) and _predicate(dense, base_a, empty, base_a, 4) == (0, 1)
    # above the run bound: 3000 + 3000 single-element columns two elements apart, shifted by one element -- they interleave without touching, and the answer is
    # "overlaps", marked as not exact; with disjoint intervals the same views are disjoint, exactly
    L = _L()
    comb = (1, 3000, 1, 2, 6000, 0)
    assert 2 * 3000 > L.WG_VIEWS_OVERLAP_MAX_RUNS and f"#define WG_VIEWS_OVERLAP_MAX_RUNS {L.WG_VIEWS_OVERLAP_MAX_RUNS}\n" in open(L.HEADER_PATH).read()
    assert np.intersect1d(_byte_set(comb, 4096, 4), _byte_set(comb, 4100, 4)).size == 0
    assert _predicate(comb, 4096, comb, 4100, 4) == (1, 0)
    assert _predicate(comb, 4096, comb, 4096 + 6000 * 4, 4) == (0, 1)
    # just under it the walk decides: 2048 + 2047 runs
    c1, c2 = (1, 2048, 1, 2, 4096, 0), (1, 2047, 1, 2, 4096, 0)
    assert _predicate(c1, 4096, c2, 4100, 4) == (0, 1) and _predicate(c1, 4096, c2, 4104, 4) == (1, 1)
    # a dense cube is one run however many columns it has
    cube, one = (64, 100000, 7, 64, 6400000, 5), (1, 1, 1, 1, 1, 0)
    assert _predicate(cube, 0, one, (5 + 44799999) * 2, 2) == (1, 1) and _predicate(cube, 0, one, (5 + 44800000) * 2, 2) == (0, 1)


def test_status_and_exception_are_mirrored():
    wg, L = _wg(), _L()
    hdr = open(L.HEADER_PATH).read()
    assert L.WG_ERR_ALIASED == 9 and "WG_ERR_ALIASED = 9 " in hdr and "WG_ERR_WORKSPACE = 8," in hdr  # appended: no existing value moved
    assert issubclass(wg.AliasedOperands, wg.WgError) and L._EXC[L.WG_ERR_ALIASED] is wg.AliasedOperands


def test_reduce_rounds_its_f32_result_not_a_fused_product():
    """Found by test_packed_reduce (Prod of 4097 f16 values in [-1, 1): the product underflows to -0 in f32): hipcc fused the LAST multiplication of a 16-bit
    Prod with the store's conversion into `v_fma_mixlo_f16 a, b, 0` -- the exact product rounded straight to 16 bits, plus +0, so an exact -0 came out as +0 where
    the reference order in f32, rounded once more, gives -0. reduce.hip fences the folded value before it converts it; the ISA must hold no such instruction."""
    import os
    import shutil
    import subprocess
    import tempfile
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "wgmath_amd", "csrc", "reduce.hip")
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math", "-ffp-contract=on",
                        "-I", os.path.join(root, "include"), "-I", os.path.dirname(src), "-S", "--cuda-device-only", src, "-o", out], check=True, capture_output=True)
        text = open(out).read()
    assert "reduce_rows4" in text and "reduce_long" in text and "reduce_fast_pass2" in text
    bad = [l.strip() for l in text.splitlines() if "_mixlo_" in l or "_mixhi_" in l]
    assert not bad, f"reduce.hip: a multiplication fused with the conversion of the result: {bad[:4]}"


# ========================================================================================================
# GPU
# ========================================================================================================
class DT:
    """An element type of the kernels: storage arrays <-> float32, bit views, half an ulp of a result and the epilogue tests' ulp (relative)."""

    def __init__(self, name):
        self.name = name
        self.es = 4 if name == "f32" else 2
        self.uint = np.uint32 if name == "f32" else np.uint16
        self.half_ulp = {"f32": 0.0, "f16": 2.0 ** -11, "bf16": 2.0 ** -8}[name]  # tests/_util.py, tests/test_gpu_bf16.py
        self.floor = {"f32": 0.0, "f16": 2.0 ** -25, "bf16": 2.0 ** -126}[name]
        self.eps = {"f32": 2.0 ** -23, "f16": 2.0 ** -10, "bf16": 2.0 ** -7}[name]     # tests/test_gpu_epilogue.py: one ulp, for alpha acc + beta c

    def __repr__(self):
        return self.name

    @property
    def np_dtype(self):
        return {"f32": np.dtype(np.float32), "f16": np.dtype(np.float16), "bf16": _wg().bfloat16}[self.name]

    def round(self, x):
        """float array -> the float32 values of its roundings to this type (one RNE)."""
        x = np.asarray(x, np.float32)
        with np.errstate(over="ignore"):
            return x if self.name == "f32" else x.astype(np.float16).astype(np.float32) if self.name == "f16" else B.round_f32(x)

    def bits(self, x32):
        """float32 values (representable in this type, or to be rounded once) -> the type's bit patterns."""
        x32 = np.asarray(x32, np.float32)
        with np.errstate(over="ignore"):
            return x32.view(np.uint32).copy() if self.name == "f32" else x32.astype(np.float16).view(np.uint16) if self.name == "f16" else B.to_bits(x32)

    def f32(self, bits):
        bits = np.asarray(bits, self.uint)
        return bits.view(np.float32) if self.name == "f32" else bits.view(np.float16).astype(np.float32) if self.name == "f16" else B.from_bits(bits)

    def upload(self, gpu, bits):
        wg = _wg()
        bits = np.ascontiguousarray(bits, self.uint).ravel()
        return wg.TensorBuilder.tensor((bits.size,), S_STORAGE).build_init(gpu.device(), bits.view(self.np_dtype), self.np_dtype)

    def read(self, gpu, t):
        return t.read(gpu.device()).view(self.uint)

    def nan_bits(self):
        return self.uint({"f32": 0x7FC5A5A5, "f16": 0x7E5A, "bf16": 0x7FC5}[self.name])  # a quiet NaN with a payload no kernel writes


F32, F16, BF16 = DT("f32"), DT("f16"), DT("bf16")
DTYPES = [F32, F16, BF16]


def _run(gpu, fn, record=False):
    enc = gpu.device().create_command_encoder(record=record)
    with enc.compute_pass("overlap", None) as p:
        fn(p)
    cb = enc.finish()
    if not record:
        gpu.queue().submit([cb])
    return cb


def _view(t, rows, cols=1, mats=1, stride=None, stride_mat=None, offset=0, dim=None):
    wg = _wg()
    stride = rows if stride is None else stride
    stride_mat = stride * cols if stride_mat is None else stride_mat
    return wg.GpuTensorView(wg.ViewShape((rows, cols, mats), stride, stride_mat, offset), t, dim or (1 if cols == 1 and mats == 1 else 3))


def _assert_bits_nan_class(dt, got_bits, want_bits, what):
    """Bit equality, NaN compared as a class (any payload, either sign)."""
    g, w = dt.f32(got_bits), dt.f32(want_bits)
    gn, wn = np.isnan(g), np.isnan(w)
    bad = (gn != wn) | (~gn & (np.asarray(got_bits) != np.asarray(want_bits)))
    if bad.any():
        i = np.flatnonzero(bad)[0]
        raise AssertionError(f"{what}: {bad.sum()} of {bad.size} elements differ; first at {i}: got {g[i]!r}, expected {w[i]!r}")


def _elementwise_want(dt, op, x32, y32, alpha=None):
    """a (op) b as the header states it: computed in f32 on the widened elements, rounded once to the type. Returns bit patterns."""
    with np.errstate(all="ignore"):
        if op == "Axpy":
            r = U.fmaf_f32(np.float32(alpha), y32, x32)  # y[i] = fma(alpha, x[i], y[i]) with (y, x) = (a, b)
        else:
            r = {"Add": lambda: x32 + y32, "Sub": lambda: x32 - y32, "Mul": lambda: x32 * y32, "Div": lambda: x32 / y32, "Copy": lambda: y32.copy()}[op]()
    return dt.bits(r.astype(np.float32))


ELEMENTWISE = [("Add", None), ("Sub", None), ("Mul", None), ("Div", None), ("Copy", None), ("Axpy", 1.0), ("Axpy", -1.0), ("Axpy", 0.3)]


def _elementwise_call(gpu, op, alpha, a, b):
    wg, dev, shapes = _wg(), gpu.device(), _wg().ViewShapeBuffers()
    if op == "Axpy":
        _run(gpu, lambda p: wg.Axpy.from_device(dev).dispatch(dev, shapes, p, alpha, a, b))
    else:
        _run(gpu, lambda p: wg.OpAssign.new(dev, wg.OpAssignVariant[op]).dispatch(dev, shapes, p, a, b))


@pytest.mark.gpu
@pytest.mark.parametrize("offset", [0, 1, 3, 5])
@pytest.mark.parametrize("n", [1, 3, 1757, 100003])
@pytest.mark.parametrize("dt", DTYPES, ids=repr)
def test_in_place_elementwise(gpu, dt, n, offset):
    """`a` and `b` the same view (the one exception of the aliasing rule): x (op) x to the bit -- every lane loads its a[i] and b[i] before it stores a[i], in the
    16-byte body and the scalar head and tail (offsets 1, 3, 5 put the view's ends off the 16-byte grid). A zero and an Inf in the data: 0 / 0, Inf / Inf and
    Inf - Inf are NaN, as a class. The elements before and behind the view are bit-unchanged."""
    rng = np.random.default_rng(n * 8 + offset)
    x = dt.round(rng.standard_normal(n).astype(np.float32) * 3)
    x[0] = 0.0
    if n >= 3:
        x[n - 1], x[n // 2] = np.inf, -0.0
    if n > 100:
        x[7], x[n - 9] = -np.inf, 0.0
    tail = 5
    guard = dt.bits(dt.round(rng.standard_normal(offset + tail).astype(np.float32)))
    before = np.concatenate([guard[:offset], dt.bits(x), guard[offset:]])
    for op, alpha in ELEMENTWISE:
        t = dt.upload(gpu, before)
        v = _view(t, n, offset=offset)
        gpu.take_path()
        _elementwise_call(gpu, op, alpha, v, v)
        got = dt.read(gpu, t)
        what = f"{op}{'' if alpha is None else f'({alpha})'} in place, {dt} n={n} offset={offset}"
        assert np.array_equal(got[:offset], before[:offset]) and np.array_equal(got[offset + n:], before[offset + n:]), f"{what}: wrote outside the view"
        want = _elementwise_want(dt, op, x, x, alpha)
        if op == "Div":
            assert np.isnan(dt.f32(want)[0]) and (n < 3 or np.isnan(dt.f32(want)[n - 1])), "0 / 0 and Inf / Inf must be NaN in the expected values"
        _assert_bits_nan_class(dt, got[offset:offset + n], want, what)


# --------------------------------------------------------------------------------------------------------
# refusals
# --------------------------------------------------------------------------------------------------------
def _valid_call_gives_the_right_bits(gpu):
    """A valid OpAssign Add on the same context: the context works as before, to the bit."""
    rng = np.random.default_rng(5)
    x, y = rng.standard_normal(37).astype(np.float32), rng.standard_normal(37).astype(np.float32)
    ta, tb = F32.upload(gpu, F32.bits(x)), F32.upload(gpu, F32.bits(y))
    _elementwise_call(gpu, "Add", None, _view(ta, 37), _view(tb, 37))
    assert np.array_equal(F32.read(gpu, ta), F32.bits(x + y)), "a valid call after a refused one gave wrong bits"
    gpu.take_path()


def _refused(gpu, dt, t, before, call, written, read, what, op=None):
    wg = _wg()
    gpu.take_path()
    with pytest.raises(wg.AliasedOperands) as e:
        _run(gpu, call)
    msg = str(e.value)
    assert e.value.status == _L().WG_ERR_ALIASED and f"`{written}`" in msg and f"`{read}`" in msg and "overlap" in msg, f"{what}: {msg!r}"
    assert op is None or msg.startswith(op + ":"), f"{what}: the message names another operator than the call that was made: {msg!r}"
    log = gpu.take_path()
    assert log == "", f"{what}: a refused call left {log!r} in the launch log"
    assert np.array_equal(dt.read(gpu, t), before), f"{what}: a refused call changed memory"


def _wrap(gpu, dt, t, first, count):
    """A second handle over `count` elements of t's memory from element `first` on (overlap is decided on addresses, not on handles)."""
    wg = _wg()
    return wg.GpuTensor.wrap(gpu.device(), t.device_ptr() + first * dt.es, (count,), dt.np_dtype, keepalive=t)


def _noise(dt, n, seed=1):
    return dt.bits(dt.round(np.random.default_rng(seed).standard_normal(n).astype(np.float32)))


@pytest.fixture
def knobs(gpu):
    saved = {}

    def set_(d):
        for k, v in d.items():
            saved.setdefault(k, gpu.set_tuning(k, v))

    yield set_
    for k, v in saved.items():
        gpu.set_tuning(k, v)


GEMM_APIS = ["gemm", "gemm_tr", "gemm_ex", "rm_gemm", "rm_gemm_tr_native", "rm_gemm_tr_copy"]


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["identical", "one_element"])
@pytest.mark.parametrize("read", ["m1", "m2"])
@pytest.mark.parametrize("api", GEMM_APIS)
@pytest.mark.parametrize("dt", [F32, F16], ids=repr)
def test_refused_gemm(gpu, knobs, dt, api, read, how):
    """wg_gemm / wg_gemm_ex / wg_gemm_rm (the forwarded Gemm, the native GemmTr, the GemmTr that copies m1 first): `out` against `m1` and against `m2`."""
    wg, dev, shapes = _wg(), gpu.device(), _wg().ViewShapeBuffers()
    n, e = 8, 64  # 8 x 8 x 8: every view has the same shape, row-major or not
    before = _noise(dt, 4 * e)
    t = dt.upload(gpu, before)
    o_off = e
    r_off = o_off if how == "identical" else o_off + e - 1  # the last element of `out` is the first of the view that is read
    other = 3 * e
    out, rd, free = _view(t, n, n, offset=o_off, dim=3), _view(t, n, n, offset=r_off, dim=3), _view(t, n, n, offset=other, dim=3)
    m1, m2 = (rd, free) if read == "m1" else (free, rd)
    if api.startswith("rm_gemm_tr"):
        knobs({"rm_tr_native": 1 if api.endswith("native") else 0})
    rm = wg.Gemm.from_device(dev, wg.row_major_shader_defs())
    cm = wg.Gemm.from_device(dev)
    call = {"gemm": lambda p: cm.dispatch(dev, shapes, p, out, m1, m2),
            "gemm_tr": lambda p: cm.dispatch_tr(dev, shapes, p, out, m1, m2),
            "gemm_ex": lambda p: cm.dispatch_ex(dev, shapes, p, 0.5, 1.0, out, m1, m2),
            "rm_gemm": lambda p: rm.dispatch(dev, shapes, p, out, m1, m2),
            "rm_gemm_tr_native": lambda p: rm.dispatch_tr(dev, shapes, p, out, m1, m2),
            "rm_gemm_tr_copy": lambda p: rm.dispatch_tr(dev, shapes, p, out, m1, m2)}[api]
    _refused(gpu, dt, t, before, call, "out", read, f"{api} {dt} out / {read} {how}")
    _valid_call_gives_the_right_bits(gpu)


# (a matrix shaped like four right-hand sides would be the `one_element` case again: no identical (out, m) pair for rm_gemv_many)
REFUSED_GEMV = [pytest.param(dt, api, read, how, id=f"{dt}-{api}-{read}-{how}") for dt in (F32, BF16) for api in ("gemv", "gemv_tr", "rm_gemv", "rm_gemv_many")
                for read in ("m", "v") for how in ("identical", "one_element", "column") if not (api == "rm_gemv_many" and read == "m" and how == "identical")]


@pytest.mark.gpu
@pytest.mark.parametrize("dt,api,read,how", REFUSED_GEMV)
def test_refused_gemv(gpu, dt, api, read, how):
    """wg_gemv / wg_gemv_rm (one right-hand side: the forwarded Gemv; four: the row-major Gemm it becomes): `out` against `m` and against `v`. `column`: the
    output is a column of the matrix (the last element of the vector, for `v`)."""
    wg, dev, shapes = _wg(), gpu.device(), _wg().ViewShapeBuffers()
    n = 8
    nrhs = 4 if api == "rm_gemv_many" else 1
    before = _noise(dt, 512)
    t = dt.upload(gpu, before)
    rm = api.startswith("rm_")
    # row-major right-hand sides: n x nrhs with `stride` elements between rows
    vec = (lambda off: _view(t, n, nrhs, stride=nrhs, offset=off, dim=3)) if rm else (lambda off: _view(t, n, nrhs, offset=off, dim=3))
    span = n * nrhs
    o_off = 256
    if read == "m":
        # identical: an n x 1 matrix (one right-hand side of length 1) where `out` is; `column`: `out` is column 3 of the n x n matrix
        if how == "identical":
            m = _view(t, n, 1, offset=o_off, dim=3) if not rm else _view(t, n, 1, stride=1, offset=o_off, dim=3)
            if api == "gemv_tr":
                m = _view(t, 1, n, stride=1, offset=o_off, dim=3)
            v = _view(t, 1, 1, offset=0, dim=3)
        else:
            m_off = o_off + span - 1 if how == "one_element" else o_off - 3 * n
            m, v = _view(t, n, n, offset=m_off, dim=3), vec(0)
    else:
        m = _view(t, n, n, offset=64, dim=3)
        v = vec(o_off if how == "identical" else o_off + span - 1 if how == "one_element" else o_off - span + 1)
    out = vec(o_off)
    op = wg.Gemv.from_device(dev, wg.row_major_shader_defs() if rm else None)
    variant = wg.GemvVariant.GemvTr if api == "gemv_tr" else wg.GemvVariant.Gemv
    _refused(gpu, dt, t, before, lambda p: op.dispatch_generic(dev, shapes, p, out, m, v, variant), "out", read, f"{api} {dt} out / {read} {how}", op="Gemv")
    _valid_call_gives_the_right_bits(gpu)


# (gemv_reduce_fused_m: a shape of the one-launch Gemv + Reduce, which is f32 only and needs 128 rows: no identical pair)
REFUSED_REDUCE = [pytest.param(dt, api, how, id=f"{dt}-{api}-{how}") for dt in (F32, F16)
                  for api in ("reduce", "reduce_fast", "reduce_batched", "gemv_reduce_m", "gemv_reduce_v", "gemv_reduce_fused_m")
                  for how in ("identical", "one_element", "inside") if not (api == "gemv_reduce_fused_m" and (dt is not F32 or how == "identical"))]


@pytest.mark.gpu
@pytest.mark.parametrize("dt,api,how", REFUSED_REDUCE)
def test_refused_reduce(gpu, dt, api, how):
    """wg_reduce / wg_reduce_fast / wg_reduce_batched / wg_gemv_reduce: the result (a second handle over the same memory: the result is a whole buffer) against
    the vector, the matrix of vectors, and the matrix and the vector of the fused product. `inside`: the result lies in the middle of what is read."""
    wg, dev, shapes = _wg(), gpu.device(), _wg().ViewShapeBuffers()
    fused = api == "gemv_reduce_fused_m"
    R, C = (128, 8) if fused else (8, 8)
    before = _noise(dt, 2048)
    t = dt.upload(gpu, before)
    off = 64
    red = wg.Reduce.new(dev, wg.ReduceOp.Sum)
    if api in ("reduce", "reduce_fast"):
        n = 1 if how == "identical" else 100
        res = _wrap(gpu, dt, t, off + {"identical": 0, "one_element": n - 1, "inside": 41}[how], 1)
        val = _view(t, n, offset=off)
        fn = red.dispatch if api == "reduce" else red.dispatch_fast
        call, names = (lambda p: fn(dev, shapes, p, val, res)), ("result", "value")
    elif api == "reduce_batched":
        rows, cols = (1, 4) if how == "identical" else (10, 4)  # identical: four vectors of one element, the four results in their place
        first = {"identical": off, "one_element": off - 3, "inside": off + 17}[how]  # one_element: the last result is the first element of the first vector
        res = _wrap(gpu, dt, t, first, 4)
        val = _view(t, rows, cols, offset=off, dim=3)
        call, names = (lambda p: red.dispatch_batched(dev, shapes, p, val, res)), ("results", "values")
    else:
        rd = "v" if api == "gemv_reduce_v" else "m"
        if how == "identical":  # a 1 x 1 matrix and a one-element vector
            m, v = _view(t, 1, 1, offset=off, dim=3), _view(t, 1, offset=off if rd == "v" else 0)
            if rd == "v":
                m = _view(t, 1, 1, offset=8, dim=3)
            res = _wrap(gpu, dt, t, off, 1)
        else:
            m, v = _view(t, R, C, offset=off, dim=3), _view(t, C, offset=0)
            span = C if rd == "v" else R * C
            res = _wrap(gpu, dt, t, (0 if rd == "v" else off) + (span - 1 if how == "one_element" else span // 2), 1)
        call, names = (lambda p: wg.gemv_reduce(p, wg.ReduceOp.Sum, res, m, v)), ("result", rd)
    _refused(gpu, dt, t, before, call, names[0], names[1], f"{api} {dt} {how}")
    _valid_call_gives_the_right_bits(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["one_element", "one_element_front", "shifted_by_one"])
@pytest.mark.parametrize("op,alpha", [("Add", None), ("Copy", None), ("Axpy", 0.3)])
@pytest.mark.parametrize("dt", DTYPES, ids=repr)
def test_refused_elementwise(gpu, dt, op, alpha, how):
    """wg_op_assign / wg_axpy: a partial overlap of `a` and `b` (the identical view is legal: test_in_place_elementwise) -- one shared element at either end, and
    a.rows(0, n) against a.rows(1, n)."""
    n = 100
    before = _noise(dt, 400)
    t = dt.upload(gpu, before)
    a_off = 150
    b_off = {"one_element": a_off + n - 1, "one_element_front": a_off - n + 1, "shifted_by_one": a_off + 1}[how]
    a, b = _view(t, n, offset=a_off), _view(t, n, offset=b_off)
    w, r = ("y", "x") if op == "Axpy" else ("a", "b")
    wg = _wg()
    gpu.take_path()
    with pytest.raises(wg.AliasedOperands) as e:
        _elementwise_call(gpu, op, alpha, a, b)
    assert f"`{w}`" in str(e.value) and f"`{r}`" in str(e.value) and e.value.status == 9, str(e.value)
    assert gpu.take_path() == "" and np.array_equal(dt.read(gpu, t), before), f"{op} {dt} {how}: a refused call launched something"
    _valid_call_gives_the_right_bits(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["identical", "one_element", "shifted_by_one_row"])
@pytest.mark.parametrize("dt", DTYPES, ids=repr)
def test_refused_copy_view(gpu, dt, how):
    """wg_copy_view: `dst` against `src` -- the same view (no exception here), one shared element, and the same block one row further down."""
    wg, dev, shapes = _wg(), gpu.device(), _wg().ViewShapeBuffers()
    rows, cols, ld = 5, 6, 9
    before = _noise(dt, 400)
    t = dt.upload(gpu, before)
    d_off = 100
    span = (cols - 1) * ld + rows
    s_off = {"identical": d_off, "one_element": d_off + span - 1, "shifted_by_one_row": d_off + 1}[how]
    dst, src = _view(t, rows, cols, stride=ld, offset=d_off, dim=3), _view(t, rows, cols, stride=ld, offset=s_off, dim=3)
    _refused(gpu, dt, t, before, lambda p: wg.CopyView.from_device(dev).dispatch(dev, shapes, p, dst, src), "dst", "src", f"copy_view {dt} {how}")
    _valid_call_gives_the_right_bits(gpu)
    # the same block one COLUMN further is disjoint when shifted past the rows (rows of dst and src interleave in the leading-dimension gap): legal, and exact
    src2 = _view(t, 4, cols, stride=ld, offset=d_off + rows, dim=3)
    dst2 = _view(t, 4, cols, stride=ld, offset=d_off, dim=3)
    _run(gpu, lambda p: wg.CopyView.from_device(dev).dispatch(dev, shapes, p, dst2, src2))
    want = before.copy()
    idx = np.arange(4)[:, None] + np.arange(cols)[None, :] * ld
    want[d_off + idx] = before[d_off + rows + idx]
    assert np.array_equal(dt.read(gpu, t), want), "copy_view between interleaved views of one buffer"
    gpu.take_path()


@pytest.mark.gpu
def test_refusal_inside_a_recording(gpu):
    """A refused call inside an open recording: the recording goes on, finishes, and its replay holds the valid calls only."""
    wg, dev, shapes = _wg(), gpu.device(), _wg().ViewShapeBuffers()
    dt = F32
    rng = np.random.default_rng(9)
    x0 = rng.standard_normal(300).astype(np.float32)
    t = dt.upload(gpu, dt.bits(x0))
    a, b, c = _view(t, 64, offset=0), _view(t, 64, offset=64), _view(t, 64, offset=200)
    o, m1 = _view(t, 8, 8, offset=128, dim=3), _view(t, 8, 8, offset=128 + 63, dim=3)
    gpu.sync()
    gpu.take_path()
    enc = dev.create_command_encoder(record=True)
    try:
        with enc.compute_pass("rec", None) as p:
            wg.OpAssign.new(dev, wg.OpAssignVariant.Add).dispatch(dev, shapes, p, a, b)        # a += b
            with pytest.raises(wg.AliasedOperands, match="`out` overlaps `m1`"):
                wg.Gemm.from_device(dev).dispatch(dev, shapes, p, o, m1, _view(t, 8, 8, offset=0, dim=3))
            with pytest.raises(wg.AliasedOperands, match="`a` overlaps `b`"):
                wg.OpAssign.new(dev, wg.OpAssignVariant.Mul).dispatch(dev, shapes, p, a, _view(t, 64, offset=1))
            wg.Axpy.from_device(dev).dispatch(dev, shapes, p, -1.0, c, a)                       # c -= a (the new a)
    finally:
        cb = enc.finish()
    assert gpu.take_path() == "", "element-wise calls log nothing, and the refused Gemm must not"
    assert np.array_equal(dt.read(gpu, t), dt.bits(x0)), "recording executed something, or a refused call wrote"
    want = x0.copy()
    for rep in (1, 2):
        gpu.queue().submit([cb])
        want[0:64] = want[0:64] + want[64:128]
        want[200:264] = U.fmaf_f32(np.float32(-1.0), want[0:64], want[200:264])
        assert np.array_equal(dt.read(gpu, t), dt.bits(want)), f"replay {rep}: the recording does not hold exactly the two valid calls"
    del cb
    _valid_call_gives_the_right_bits(gpu)


@pytest.mark.gpu
def test_refused_sharded_gemm_one_launch(gpu):
    """wg_gemm_sharded on one rank, staged engine, one launch per step (wg_gemm_f16_panels: the rank's whole f16 product as ONE kernel that writes its N-panels into
    the communicator's staging cube). wg_comm_stage_reserve hands that cube out, so `a_rows` or `b` can be a view of it. The cube has two halves, at elements 0 and
    `half`; step s (1, 2, ...; a refused call is no step) writes its panels -- 3 of 1024 columns and a tail of 1024, M x N elements back to back -- from element
    (s & 1) * half on. Refused: an operand that starts where panel 0 starts, and one whose first 4 elements are the last 4 of the tail panel (vec4 views: 4 elements is
    the smallest overlap there is) -- `out` against `m1` / `m2`, nothing launched, cube and result unchanged. Then a valid step: the f64 bound; then `b` inside the cube,
    directly behind that step's panels: accepted, bit-equal to the valid step, `b` unchanged. Last, wg_gemm_sharded's own check: `out` against `a_rows` and `b`."""
    wg, L, dev = _wg(), _L(), gpu.device()
    from wgmath_amd.sharded import Comm, GatherMode
    dt = F16
    M, K, N, panel = 4096, 256, 4096, 1024  # 16 x 16 tiles of 256 x 256: one round of the chip's 256 CUs, the least the one-launch form takes
    half = M * N + K * N + 64                # room for a K x N operand behind a step's panels in either half
    rng = np.random.default_rng(77)
    A, Bm = _rand(dt, rng, (M, K, 1)), _rand(dt, rng, (K, N, 1))
    ta, tb = dt.upload(gpu, dt.bits(A.ravel(order="F"))), dt.upload(gpu, dt.bits(Bm.ravel(order="F")))
    tc = dt.upload(gpu, np.full(M * N, dt.nan_bits(), dt.uint))
    comm = Comm(gpu, 1, 0, None)
    try:
        st, _ = comm.stage_reserve(2 * half * dt.es)
        cube = wg.GpuTensor.wrap(dev, L.lib.wg_buf_device_ptr(st), (2 * half,), dt.np_dtype)  # a second handle over the cube's memory
        cube0 = dt.bits(_rand(dt, rng, (2 * half,)))
        cube0[M * N:M * N + K * N] = dt.bits(Bm.ravel(order="F"))  # the operand of the accepted call
        fill = dt.upload(gpu, cube0)
        L.check(L.lib.wg_buf_copy(gpu._ctx.handle, fill._h, 0, cube._h, 0, 2 * half * dt.es))
        comm.set_one_launch(True)
        a_sep, b_sep, out = _view(ta, M, K, dim=3), _view(tb, K, N, dim=3), _view(tc, M, N, dim=3)
        steps = 0

        def sharded(o, a, b):
            comm.sharded_gemm(o, a, b, 0, GatherMode.PEER_STAGED, panel)
            comm.join()
            gpu.sync()

        base = ((steps + 1) & 1) * half
        for read, off in (("m1", base), ("m1", base + M * N - 4), ("m2", base), ("m2", base + M * N - 4)):
            what = f"one-launch sharded Gemm, {read} in the staging cube at element {off} (panels from {base} on)"
            a = _view(cube, M, K, offset=off, dim=3) if read == "m1" else a_sep
            b = _view(cube, K, N, offset=off, dim=3) if read == "m2" else b_sep
            gpu.take_path()
            with pytest.raises(wg.AliasedOperands) as e:
                sharded(out, a, b)
            msg = str(e.value)
            assert "`out`" in msg and f"`{read}`" in msg and "overlap" in msg and e.value.status == L.WG_ERR_ALIASED, f"{what}: {msg!r}"
            log = gpu.take_path()
            assert log == "", f"{what}: a refused call left {log!r} in the launch log"
            gpu.sync()
            assert np.array_equal(dt.read(gpu, cube), cube0), f"{what}: a refused call changed the staging cube"
        assert np.array_equal(dt.read(gpu, tc), np.full(M * N, dt.nan_bits(), dt.uint)), "a refused call wrote `out`"
        # a valid step on the same communicator
        sharded(out, a_sep, b_sep)
        steps += 1
        log = gpu.take_path()
        print(f"one-launch sharded Gemm: [{log}]")
        assert log.count("f16.") == 1, f"expected ONE Gemm launch over the four panels, the call took {log!r}"
        valid = dt.read(gpu, tc).copy()
        rows = np.unique(rng.integers(0, M, 64))
        A64, B64 = A[rows, :, 0].astype(np.float64), Bm[:, :, 0].astype(np.float64)
        _check_product(dt, dt.f32(valid).reshape(N, M).T[rows], A64 @ B64, np.abs(A64) @ np.abs(B64), K, None, "one-launch sharded Gemm after the refusals")
        # `b` in the cube, directly behind this step's panels (or, were the step odd, in the other half): legal
        base = ((steps + 1) & 1) * half
        assert base == 0, "the second step writes the lower half: `b` at element M * N touches its tail panel"
        tc2 = dt.upload(gpu, np.full(M * N, dt.nan_bits(), dt.uint))
        sharded(_view(tc2, M, N, dim=3), a_sep, _view(cube, K, N, offset=M * N, dim=3))
        steps += 1
        assert gpu.take_path().count("f16.") == 1
        assert np.array_equal(dt.read(gpu, tc2), valid), "`b` read from the staging cube: not the bits of the same step with `b` in a buffer of its own"
        after = dt.read(gpu, cube)
        assert np.array_equal(after[M * N:half], cube0[M * N:half]), "the step wrote behind its panels in the staging cube"
        # wg_gemm_sharded's own check, in a gathered mode and in WG_GATHER_NONE: `out` against `a_rows` and `b`, before anything is launched
        big = dt.upload(gpu, cube0[:M * N + K * N])
        before = dt.read(gpu, big).copy()
        for mode in (GatherMode.PEER_STAGED, GatherMode.NONE):
            for read, o, a, b in (("a_rows", _view(big, M, N, dim=3), _view(big, M, K, offset=M * N - 4, dim=3), b_sep),
                                  ("b", _view(big, M, N, dim=3), a_sep, _view(big, K, N, offset=M * N - 4, dim=3))):
                gpu.take_path()
                with pytest.raises(wg.AliasedOperands) as e:
                    comm.sharded_gemm(o, a, b, 0, mode, panel)
                assert "`out`" in str(e.value) and f"`{read}`" in str(e.value) and str(e.value).startswith("Gemm (sharded):"), str(e.value)
                gpu.sync()
                assert gpu.take_path() == "" and np.array_equal(dt.read(gpu, big), before), f"sharded Gemm, mode {mode}, out / {read}: a refused call launched something"
        sharded(out, a_sep, b_sep)
        assert np.array_equal(dt.read(gpu, tc), valid), "a valid step after the refusals: not the bits of the first one"
        gpu.take_path()
    finally:
        comm.close()
    _valid_call_gives_the_right_bits(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("api", ["reduce", "reduce_fast", "reduce_batched"])
@pytest.mark.parametrize("dt", DTYPES, ids=repr)
def test_prod_keeps_the_sign_of_an_exact_zero(gpu, dt, api):
    """Prod of +1 / -1 values and one +0: the f32 product is an exact zero whose sign is the parity of the negative factors, in whatever order it is folded, and the
    result is that f32 value rounded to the element type: -0 stays -0. (A multiplication fused with the store's conversion adds a +0 and turns -0 into +0: what
    test_packed_reduce found in the 16-bit Prod.) Two vectors that differ in one sign, so that no kernel passes by always answering one of the two."""
    wg, dev, shapes = _wg(), gpu.device(), _wg().ViewShapeBuffers()
    red = wg.Reduce.new(dev, wg.ReduceOp.Prod)
    for n in (5, 4097) if api == "reduce_batched" else (5, 4097, 100003):
        rng = np.random.default_rng(n)
        x = np.where(rng.random(n) < 0.5, -1.0, 1.0).astype(np.float32)
        x[n // 2] = 0.0
        if np.count_nonzero(x < 0) % 2 == 0:
            x[0] = -x[0]
        y = x.copy()
        y[1] = -y[1]  # an even number of negative factors: +0
        want = dt.bits(np.array([-0.0, 0.0], np.float32))
        assert want[0] == dt.uint(1) << (8 * dt.es - 1) and want[1] == 0
        if api == "reduce_batched":
            t = dt.upload(gpu, dt.bits(np.concatenate([x, y])))
            res = dt.upload(gpu, np.full(2, dt.nan_bits(), dt.uint))
            _run(gpu, lambda p: red.dispatch_batched(dev, shapes, p, _view(t, n, 2, dim=3), res))
            got = dt.read(gpu, res)
        else:
            got = np.zeros(2, dt.uint)
            for i, v in enumerate((x, y)):
                t = dt.upload(gpu, dt.bits(v))
                res = dt.upload(gpu, np.full(1, dt.nan_bits(), dt.uint))
                fn = red.dispatch if api == "reduce" else red.dispatch_fast
                _run(gpu, lambda p: fn(dev, shapes, p, _view(t, n), res))
                got[i] = dt.read(gpu, res)[0]
        log = gpu.take_path()
        assert np.array_equal(got, want), f"Prod {dt} n={n} {api} [{log}]: got bits {[hex(int(g)) for g in got]}, expected -0 then +0 ({[hex(int(w)) for w in want]})"


# --------------------------------------------------------------------------------------------------------
# packed neighbours
# --------------------------------------------------------------------------------------------------------
class Packed:
    """Views stored back to back in one buffer from element `first` on: add(name, rows, cols, mats, ld) places the next one; the elements in front of the first
    view, GUARD elements behind the last and the leading-dimension padding hold a NaN."""
    GUARD = 64

    def __init__(self, dt, first=1):
        self.dt, self.at, self.views = dt, first, {}

    def add(self, name, rows, cols=1, mats=1, ld=None):
        ld = rows if ld is None else ld
        batch = ld * cols
        span = (mats - 1) * batch + (cols - 1) * ld + rows
        idx = self.at + np.arange(rows)[:, None, None] + np.arange(cols)[None, :, None] * ld + np.arange(mats)[None, None, :] * batch
        self.views[name] = (rows, cols, mats, ld, batch, self.at, idx)
        self.at += span
        return self

    def build(self, gpu, values):
        """values[name]: float32 (rows x cols x mats), already representable in the type; elements no view holds: NaN."""
        self.flat = np.full(self.at + self.GUARD, self.dt.nan_bits(), self.dt.uint)
        for name, x in values.items():
            self.flat[self.views[name][6]] = self.dt.bits(np.asarray(x, np.float32).ravel()).reshape(x.shape)
        self.t = self.dt.upload(gpu, self.flat)
        return self

    def view(self, name, dim=3):
        rows, cols, mats, ld, batch, off, _ = self.views[name]
        return _view(self.t, rows, cols, mats, stride=ld, stride_mat=batch, offset=off, dim=dim)

    def result(self, gpu, name, what):
        """The written view's values; everything else in the buffer must be bit-unchanged."""
        got = self.dt.read(gpu, self.t)
        idx = self.views[name][6]
        keep = np.ones(got.size, bool)
        keep[idx.ravel()] = False
        changed = np.flatnonzero(keep & (got != self.flat))
        assert changed.size == 0, f"{what}: {changed.size} elements outside `{name}` changed, first at element {changed[0]} (`{name}` starts at {self.views[name][5]})"
        return self.dt.f32(got[idx])


def _rand(dt, rng, shape):
    return dt.round(rng.random(shape, dtype=np.float32) * 2 - 1)


def _check_product(dt, got, truth, sabs, k, c0, what):
    """The dense tests' bound: f32_gate (+ half an ulp of the result) for beta = 0; with a seeded output the epilogue tests' gate + ulp (|truth| + |c0|)."""
    assert not np.isnan(got).any(), f"{what}: {np.isnan(got).sum()} NaN in the result (read outside a view, or did not write)"
    gate = U.f32_gate(k, sabs)
    if c0 is None:
        want, tol = truth, gate + dt.half_ulp * np.abs(truth) + dt.floor
    else:
        want, tol = truth + c0, gate + dt.eps * (np.abs(truth) + np.abs(c0)) + dt.floor
    err = np.abs(got.astype(np.float64) - want)
    print(f"{what}: worst err/tol {(err / tol).max():.3g}")
    assert (err <= tol).all(), f"{what}: worst err/tol {(err / tol).max():.3g} at {np.unravel_index((err / tol).argmax(), err.shape)}"


def _took(tags, log):
    return all(any(t in log for t in ((alt,) if isinstance(alt, str) else alt)) for alt in tags)


# (M, K, N, mats), knobs, and the launch-log tags of the Gemm and the GemmTr call (every entry: a tag, or a tuple of alternatives of which one must appear;
# 16-bit tags without the element prefix). The shapes are the smallest of each kernel family in tests/test_gpu_parity.py's and tests/test_gpu_epilogue.py's tables.
# The f32 shapes come from a table without leaves (test_gpu_parity.py GEMM_SHAPES): their families are asserted by the tags tests/test_gpu_epilogue.py uses for them
# (Gemm, GemmTr); None: printed only.
PACKED_F32 = [
    ((36, 20, 28, 1), {}, None, None),
    ((260, 264, 132, 1), {}, None, None),
    ((256, 4096, 128, 1), {}, ("splitk.reduce/",), ("splitk.reduce/",)),                              # split-K
    ((520, 132, 4, 1), {}, ("f32.skinny/",), None),                                                   # few columns
    ((8, 128, 516, 1), {}, (("f32.fewrow>", "f32.skinnyT/"),), (("f32.fewrow>", "f32.skinnyT/"),)),   # few rows
]
PACKED_16 = [
    ((61, 30, 19, 1), {}, ("stage/c",)),                              # lengths that are no multiple of 4: staged copies around the generic kernel
    ((384, 320, 264, 2), {"f16_tile": 128}, (".t128",)),
    ((512, 256, 512, 1), {"f16_tile": 256}, ((".m16", ".cont"),)),
    ((512, 256, 384, 1), {"f16_tile": 256128}, (".t256x128",)),
    ((1028, 512, 1028, 1), {}, (".pad/c",)),
]
# first: the element the first view starts at. From element 1 on no boundary is 16-byte aligned (the 16-bit tile kernels then read zero-padded copies of m1 and m2 --
# "pad>" -- and write the packed output where it lies); from element 8 on the 16-bit tile shapes, whose sizes are multiples of 8, have every boundary ON the 16-byte
# grid and the tile kernels read the packed operands themselves, LDS-DMA pieces included, right up to the neighbour.
PACKED_GEMM = ([pytest.param(F32, s, k, ttr if tr else tnn, tr, 1, id=f"f32-{'x'.join(map(str, s))}-{'tr' if tr else 'nn'}") for s, k, tnn, ttr in PACKED_F32
                for tr in (False, True)]
               + [pytest.param(dt, s, k, tags, tr, first, id=f"{dt}-{'x'.join(map(str, s))}-{'tr' if tr else 'nn'}-at{first}") for dt in (F16, BF16)
                  for s, k, tags in PACKED_16 for tr in (False, True) for first in ((1, 8) if k else (1,))])


@pytest.mark.gpu
@pytest.mark.parametrize("dt,shape,kn,tags,tr,first", PACKED_GEMM)
def test_packed_gemm(gpu, knobs, dt, shape, kn, tags, tr, first):
    """[NaN][m1][out][m2][NaN ...], no gap, m1 from element 1 (or 8) on: Gemm into a NaN output (beta = 0) and gemm_ex(1, 1) on a seeded one."""
    wg, dev, shapes = _wg(), gpu.device(), _wg().ViewShapeBuffers()
    M, K, N, Z = shape
    knobs(kn)
    rng = np.random.default_rng(M * 7 + K * 5 + N * 3 + Z + int(tr))
    A, Bm, C0 = _rand(dt, rng, (M, K, Z)), _rand(dt, rng, (K, N, Z)), _rand(dt, rng, (M, N, Z))
    A64, B64 = A.astype(np.float64), Bm.astype(np.float64)
    truth = np.einsum("mkz,knz->mnz", A64, B64, optimize=True)
    sabs = np.einsum("mkz,knz->mnz", np.abs(A64), np.abs(B64), optimize=True)
    stored_a = np.transpose(A, (1, 0, 2)) if tr else A
    gemm = wg.Gemm.from_device(dev)
    variant = wg.GemmVariant.GemmTr if tr else wg.GemmVariant.Gemm
    for beta in (0.0, 1.0):
        pk = Packed(dt, first).add("m1", *stored_a.shape).add("out", M, N, Z).add("m2", K, N, Z)
        pk.build(gpu, {"m1": stored_a, "m2": Bm, **({"out": C0} if beta else {})})
        gpu.take_path()
        if beta:
            _run(gpu, lambda p: gemm.dispatch_ex(dev, shapes, p, 1.0, beta, pk.view("out"), pk.view("m1"), pk.view("m2"), variant))
        else:
            _run(gpu, lambda p: gemm.dispatch_generic(dev, shapes, p, pk.view("out"), pk.view("m1"), pk.view("m2"), variant))
        what = f"packed {'GemmTr' if tr else 'Gemm'} {dt} {M}x{K}x{N}x{Z} from element {first}, beta={beta:g}"
        got = pk.result(gpu, "out", what)
        log = gpu.take_path()
        print(f"{what}: [{log}]")
        assert log, f"{what}: nothing was launched"
        if tags is not None and (beta == 0.0 or M > 64 or dt is not F32):  # (the f32 few-row forms take beta = 0 only: tests/test_gpu_epilogue.py's `not_ab`)
            assert _took(tags, log), f"{what}: expected {tags!r}, the call took {log!r}"
        if first == 8:
            assert "pad" not in log and "stage" not in log, f"{what}: expected the tile kernels on the packed operands themselves, the call took {log!r}"
        _check_product(dt, got, truth, sabs, K, C0.astype(np.float64) if beta else None, f"{what} [{log}]")


PACKED_GEMV = [pytest.param(dt, R, C, ld, nrhs, tr, first, id=f"{dt}-{R}x{C}-ld{ld}-{nrhs}rhs-{'tr' if tr else 'n'}-at{first}")
               for dt in DTYPES for (R, C, ld) in ((301, 203, 305), (1024, 512, 1024), (64, 4096, 64)) for nrhs in (1, 3) for tr in (False, True)
               for first in ((1,) if ld != R else (1, 4))]


@pytest.mark.gpu
@pytest.mark.parametrize("dt,R,C,ld,nrhs,tr,first", PACKED_GEMV)
def test_packed_gemv(gpu, dt, R, C, ld, nrhs, tr, first):
    """[NaN][m][out][v][NaN ...], no gap. From element 1 on every view is off the vec4 grid (the any-alignment kernels: 16-byte loads at element-aligned
    addresses right up to a neighbour); from element 4 on the aligned shapes run on the tuned vec4 kernels, whose last 16-byte access of a vector ends at the
    neighbour's first element."""
    wg, dev, shapes = _wg(), gpu.device(), _wg().ViewShapeBuffers()
    k, ro = (R, C) if tr else (C, R)
    rng = np.random.default_rng(R + C * 3 + nrhs + int(tr) + first)
    Mx, V = _rand(dt, rng, (R, C, 1)), _rand(dt, rng, (k, nrhs, 1))
    op_m = np.transpose(Mx, (1, 0, 2)) if tr else Mx
    truth = np.einsum("rkz,knz->rnz", op_m.astype(np.float64), V.astype(np.float64), optimize=True)
    sabs = np.einsum("rkz,knz->rnz", np.abs(op_m).astype(np.float64), np.abs(V).astype(np.float64), optimize=True)
    pk = Packed(dt, first)
    pk.add("m", R, C, 1, ld).add("out", ro, nrhs).add("v", k, nrhs)
    pk.build(gpu, {"m": Mx, "v": V})
    gemv = wg.Gemv.from_device(dev)
    gpu.take_path()
    _run(gpu, lambda p: gemv.dispatch_generic(dev, shapes, p, pk.view("out"), pk.view("m"), pk.view("v"), wg.GemvVariant.GemvTr if tr else wg.GemvVariant.Gemv))
    what = f"packed {'GemvTr' if tr else 'Gemv'} {dt} {R}x{C} ld {ld}, {nrhs} rhs, from element {first}"
    got = pk.result(gpu, "out", what)
    log = gpu.take_path()
    print(f"{what}: [{log}]")
    if first == 1:  # tests/test_gpu_operands.py GRow.odd: the leaf of views at odd offsets
        assert f"gemv_any/{'t' if tr else 'n'},ns=" in log, f"{what}: expected the any-alignment kernel, the call took {log!r}"
    else:
        assert log and "gemv_any" not in log and "stage" not in log, f"{what}: expected the vec4 kernels where the views lie, the call took {log!r}"
    _check_product(dt, got, truth, sabs, k, None, f"{what} [{log}]")


@pytest.mark.gpu
@pytest.mark.parametrize("n,leaf", [(4097, "reduce.rows4/al=0"), (300007, "reduce.long")])  # tests/test_gpu_operands.py REDUCE_PATHS at an odd offset
@pytest.mark.parametrize("dt", DTYPES, ids=repr)
def test_packed_reduce(gpu, oracle_c, dt, n, leaf):
    """[NaN][vector][result][NaN ...]: the result scalar is the element directly behind the vector (a handle of its own over that element). The oracle's bits."""
    wg, dev, shapes = _wg(), gpu.device(), _wg().ViewShapeBuffers()
    from oracle import wgsl_oracle as wo
    rng = np.random.default_rng(n)
    x = _rand(dt, rng, (n, 1, 1))
    for op, wop in ((wg.ReduceOp.Min, wo.MIN), (wg.ReduceOp.Max, wo.MAX), (wg.ReduceOp.Sum, wo.SUM), (wg.ReduceOp.SqNorm, wo.SQNORM), (wg.ReduceOp.Prod, wo.PROD)):
        pk = Packed(dt).add("value", n).add("result", 1).build(gpu, {"value": x})
        res = _wrap(gpu, dt, pk.t, pk.views["result"][5], 1)
        gpu.take_path()
        _run(gpu, lambda p: wg.Reduce.new(dev, op).dispatch(dev, shapes, p, pk.view("value", dim=1), res))
        what = f"packed Reduce {op.name} {dt} n={n}"
        got = pk.result(gpu, "result", what)
        log = gpu.take_path()
        want_leaf = "reduce.fast/" if n >= 65536 and op in (wg.ReduceOp.Min, wg.ReduceOp.Max) else leaf  # (Min / Max of a long vector: the two-pass kernels)
        assert want_leaf in log, f"{what}: expected {want_leaf!r}, took {log!r}"
        with np.errstate(over="ignore", invalid="ignore"):
            want = dt.bits(np.array([oracle_c.reduce(int(wop), x.ravel(), wo.Shape(n, 1, 1, n, n, 0))], np.float32))
        _assert_bits_nan_class(dt, dt.bits(got.ravel()), want, f"{what} [{log}]")
        assert not np.isnan(got).any(), f"{what}: NaN (read past the vector)"


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=repr)
def test_packed_elementwise(gpu, dt):
    """[NaN][a][b][NaN ...], n = 1757: `b` directly behind `a`."""
    n = 1757
    rng = np.random.default_rng(n)
    x, y = _rand(dt, rng, (n, 1, 1)), _rand(dt, rng, (n, 1, 1))
    y[y == 0] = 1.0
    for op, alpha in ELEMENTWISE:
        pk = Packed(dt).add("a", n).add("b", n).build(gpu, {"a": x, "b": y})
        _elementwise_call(gpu, op, alpha, pk.view("a", dim=1), pk.view("b", dim=1))
        what = f"packed {op}{'' if alpha is None else f'({alpha})'} {dt}"
        got = pk.result(gpu, "a", what)
        want = _elementwise_want(dt, op, x.ravel(), y.ravel(), alpha)
        assert np.array_equal(dt.bits(got.ravel()), want), f"{what}: not bit-equal to NumPy"
    gpu.take_path()


# --------------------------------------------------------------------------------------------------------
# interleaved
# --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dt,M,K,N", [(F32, 260, 72, 72), (F16, 264, 96, 264)], ids=["f32-260x72x72", "f16-264x96x264"])
def test_interleaved_gemm(gpu, dt, M, K, N):
    """The output's columns live in the leading-dimension padding of m1: both views have ld = 2 M, m1 at offset 0, the output at offset M. Disjoint footprints
    whose byte intervals intersect (the predicate walks their column runs): legal, the usual bound, m1 unchanged."""
    wg, dev, shapes = _wg(), gpu.device(), _wg().ViewShapeBuffers()
    rng = np.random.default_rng(M + K + N)
    A, Bm = _rand(dt, rng, (M, K, 1)), _rand(dt, rng, (K, N, 1))
    truth = A[:, :, 0].astype(np.float64) @ Bm[:, :, 0].astype(np.float64)
    sabs = np.abs(A[:, :, 0]).astype(np.float64) @ np.abs(Bm[:, :, 0]).astype(np.float64)
    ld, cols = 2 * M, max(K, N)
    flat = np.full(ld * cols + K * N + 64, dt.nan_bits(), dt.uint)
    a_idx = np.arange(M)[:, None] + np.arange(K)[None, :] * ld
    o_idx = M + np.arange(M)[:, None] + np.arange(N)[None, :] * ld
    b_off = ld * cols
    flat[a_idx] = dt.bits(A[:, :, 0].ravel()).reshape(M, K)
    flat[b_off:b_off + K * N] = dt.bits(Bm[:, :, 0].reshape(-1, order="F"))
    t = dt.upload(gpu, flat)
    L = _L()
    assert L.lib.wg_debug_views_overlap(wg.ViewShape((M, N, 1), ld, ld * N, M).to_c(), 0, wg.ViewShape((M, K, 1), ld, ld * K, 0).to_c(), 0, dt.es, None) == 0
    out, m1, m2 = _view(t, M, N, stride=ld, offset=M, dim=3), _view(t, M, K, stride=ld, offset=0, dim=3), _view(t, K, N, offset=b_off, dim=3)
    gpu.take_path()
    _run(gpu, lambda p: wg.Gemm.from_device(dev).dispatch(dev, shapes, p, out, m1, m2))
    got = dt.read(gpu, t)
    log = gpu.take_path()
    keep = np.ones(flat.size, bool)
    keep[o_idx.ravel()] = False
    assert np.array_equal(got[keep], flat[keep]), f"interleaved Gemm [{log}]: m1, m2 or the padding changed"
    _check_product(dt, dt.f32(got[o_idx]), truth, sabs, K, None, f"interleaved Gemm {dt} {M}x{K}x{N} [{log}]")
    # and the same output one element lower shares a row with m1: refused
    bad = _view(t, M, N, stride=ld, offset=M - 1, dim=3)
    with pytest.raises(wg.AliasedOperands, match="`out` overlaps `m1`"):
        _run(gpu, lambda p: wg.Gemm.from_device(dev).dispatch(dev, shapes, p, bad, m1, m2))
    assert gpu.take_path() == "" and np.array_equal(dt.read(gpu, t), got)
