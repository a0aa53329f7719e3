"""wg_gemm_out32 on the GPU: Gemm on f16 / bf16 operands with an f32 result. Before the feature the symbol did not exist.

The contract (include/wgebra_hip.h): operands widened exactly, the f32 accumulator of the 16-bit wg_gemm_ex on the same leaf, r = alpha * acc rounded to f32,
fmaf(beta, c, r) with c read as f32, r stored as it is; the 16-bit planner's plan without the continuous walk; never the Gemv kernels.

  1  every leaf, both variants, dense and odd output views: the exact integer product, bit for bit, for (1, 0) and (-0.375, 0.5)   test_exact_by_construction
  2  RNE16(out32) == the 16-bit wg_gemm_ex's output, bit for bit, on the same leaf                                                test_one_rounding_from_the_16_bit_call
  3  |got - f64 product| <= the f32 gate alone (no 16-bit term)                                                                   test_truth
  4  results past the f16 range; K-chunked accumulation through beta = 1                                                          test_past_the_16_bit_range
  5  NaN in `out` overwritten (item 1's prefill); Inf in the last row / column of m1 / m2                                         test_special_values
  6  status codes and messages: wg_gemm_ex's for the same mistake; WG_F32 forwards; WG_ERR_WORKSPACE inside a recording           test_status_codes, test_f32_forwards, ...
  7  `out` and `m1` in one buffer: touching, one byte of overlap; `out` interleaved between the columns of `m2`                   test_aliasing
  8  recorded and replayed twice; a CU-masked context (64 CUs)                                                                    test_recorded, test_cu_masked
  9  the Python operators Gemm.dispatch_out32 / _tr / _generic                                                                    test_python_operators
No test asserts a time.

Item 1's operands are integers in [-8, 8] chosen so that a 16-bit store cannot pass: magnitudes uniform in 0 .. 8 (7 or 8 where K < 256), one sign per row of op(m1)
and per column of m2, so the products pile up instead of cancelling and at least a quarter of the expected values of a row are odd integers above 2048 (asserted:
`unstorable`). The one row where that is arithmetically out of reach is `staged`: K = 30 and |a|, |b| <= 8 bound every product by 1920. There the share is asserted
for the (-0.375, 0.5) expectation only (old `out`: odd integers of magnitude 8193 .. 16383, so beta * c ends in .5 above 4096), where the same property reads
"above 2048 in magnitude and not a multiple of 2", i.e. on neither 16-bit grid; the (1, 0) result of that row is still compared bit for bit.
"""
import ctypes
import faulthandler
import functools
import re

import numpy as np
import pytest

import _util as U

pytestmark = pytest.mark.gpu

S_STORAGE = 128 | 4 | 8
NAN32 = np.float32(np.nan)
AB = (-0.375, 0.5)
KINDS = ["f16", "bf16"]


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


def dtype_of(kind):
    L = _L()
    return {"f32": L.WG_F32, "f16": L.WG_F16, "bf16": L.WG_BF16}[kind]


class Op:
    """X[r, c, z] (float32 values) stored column-major as `kind` elements at `off`, leading dimension r + pad, `gap` elements between matrices; NaN elsewhere.
    (Strided views instead of index arrays: the largest output here has 33 M elements.)"""

    def __init__(self, gpu, vals, kind, off=0, pad=0, gap=0):
        wg = _wg()
        vals = np.asarray(vals, np.float32)
        R, C, Z = vals.shape
        self.kind, self.gpu, self.dims = kind, gpu, (R, C, Z)
        self.ld = R + pad
        self.batch = self.ld * C + gap
        self.size = off + self.batch * Z + 8
        self.off = off
        flat = store(kind, np.full(self.size, NAN32, np.float32))
        self._view(flat)[...] = store(kind, vals.ravel()).reshape(vals.shape)
        self.init = flat
        self.buf = wg.TensorBuilder.tensor((self.size,), S_STORAGE).build_init(gpu.device(), self.init, self.init.dtype)
        self.shape = wg.ViewShape((R, C, Z), self.ld, self.batch, off)

    def _view(self, flat):
        R, C, Z = self.dims
        s = flat.itemsize
        return np.lib.stride_tricks.as_strided(flat[self.off:], (R, C, Z), (s, s * self.ld, s * self.batch))

    def set(self, vals):
        flat = self.init.copy()
        self._view(flat)[...] = store(self.kind, np.asarray(vals, np.float32).ravel()).reshape(self.dims)
        self.gpu.queue().write_buffer(self.buf, 0, flat)

    def poison(self):
        self.gpu.queue().write_buffer(self.buf, 0, self.init)

    def _outside(self, flat):
        """The elements of the buffer that are not the view's, as views (no copies): in front of it, below every column, behind every matrix, behind the last one."""
        R, C, Z = self.dims
        s, pad, gap = flat.itemsize, self.ld - R, self.batch - self.ld * C
        parts = [flat[:self.off], flat[self.off + self.batch * Z - gap:]]
        if pad:
            parts.append(np.lib.stride_tricks.as_strided(flat[self.off + R:], (pad, C, Z), (s, s * self.ld, s * self.batch)))
        if gap and Z > 1:
            parts.append(np.lib.stride_tricks.as_strided(flat[self.off + self.ld * C:], (gap, Z - 1), (s, s * self.batch)))
        return parts

    def read(self, what=""):
        flat = self.buf.read(self.gpu.device())
        assert sum(int(x.size) for x in self._outside(flat)) + int(np.prod(self.dims)) == self.size
        assert all(np.isnan(widen(self.kind, np.ascontiguousarray(x).ravel())).all() for x in self._outside(flat)), f"{what}: wrote outside the view"
        return self._view(flat).copy()


def out_view(gpu, kind, M, N, Z, dense, fill=NAN32):
    """The output of a row: dense, or at an odd offset with an odd leading dimension and an odd gap between matrices."""
    vals = np.full((M, N, Z), fill, np.float32)
    return Op(gpu, vals, kind) if dense else Op(gpu, vals, kind, off=1, pad=3, gap=7)


def call(inst, fn_name, tr, dt, alpha, beta, out, m1, m2, variant=None):
    """(status, message) of wg_gemm_out32 / wg_gemm_ex through the C ABI."""
    wg, L = _wg(), _L()
    variant = int(wg.GemmVariant.GemmTr if tr else wg.GemmVariant.Gemm) if variant is None else int(variant)
    rc = getattr(L.lib, fn_name)(inst._ctx.handle, variant, dt, float(alpha), float(beta), out.buf._h, out.shape.to_c(), m1.buf._h, m1.shape.to_c(),
                                 m2.buf._h, m2.shape.to_c())
    return rc, L.lib.wg_last_error_string().decode()


def out32(inst, tr, kind, alpha, beta, out, m1, m2):
    rc, msg = call(inst, "wg_gemm_out32", tr, dtype_of(kind), alpha, beta, out, m1, m2)
    assert rc == 0, msg


def stored(A, tr):
    """op(m1) = A (M x K x Z) as m1 is stored: M x K (Gemm) or K x M (GemmTr)."""
    return np.ascontiguousarray(np.transpose(A, (1, 0, 2))) if tr else A


# ---- the leaves: the rows and knobs of LEAVES in tests/test_gpu_epilogue.py. {p} = the element prefix "f16o32" / "bf16o32" ---------------------------
class Row:
    def __init__(self, name, M, K, N, mats, leaf, knobs=None, ab=None, without=None, variants=(False, True), dense_only=False):
        self.name, self.M, self.K, self.N, self.mats = name, M, K, N, mats
        self.leaf, self.knobs, self.ab, self.without, self.variants, self.dense_only = leaf, knobs or {}, ab or leaf, without, variants, dense_only

    def took(self, kind, log, beta, prefix=None):
        p = prefix or f"{kind}o32"
        want = (self.leaf if beta == 0 else self.ab).format(p=p)
        return want in log and (self.without is None or self.without not in log)


ROWS = [
    Row("skinny", 32768, 256, 8, 1, "{p}.skinny/ns=1", variants=(True,), dense_only=True),
    Row("skinny_split", 4096, 2048, 8, 1, "{p}.skinny/ns=8 splitk.reduce/ns=8", variants=(True,), dense_only=True),
    Row("t128", 512, 512, 512, 1, "{p}.t128/ns=1", {"f16_tile": 128}),
    Row("t128_split", 512, 4096, 512, 1, "{p}.t128/ns=4 splitk.reduce/ns=4", {"f16_tile": 128}),
    Row("t256x128", 1024, 512, 1024, 1, "{p}.t256x128", {"f16_tile": 256128}),
    Row("m16_static", 4096, 512, 4096, 1, "{p}.m16/ns=1", {"f16_tile": 256, "f16_sched": 0}),
    Row("m16_queues", 4096, 512, 4096, 1, "{p}.m16q/ns=1", {"f16_tile": 256, "f16_sched": 1}),
    Row("m16_balance", 4096, 1024, 4096, 1, "{p}.m16bal/ns=1", {"f16_tile": 256, "f16_balance": 1}),
    Row("m16_splitk", 1024, 4096, 1024, 1, "{p}.m16/ns=16 splitk.reduce/ns=16", {"f16_tile": 256, "f16_cont": 0}),
    Row("m16_tail", 4352, 1024, 4096, 1, "{p}.m16/ns=1 {p}.m16tail/ns=4 {p}.tail_reduce", {"f16_tile": 256, "f16_cont": 0}),
    # (a row of this file's own: tiles that are ragged in M and in N keep per-lane guards and the plain stores; whole tiles exchange halves between lanes first)
    Row("m16_ragged", 1032, 256, 520, 1, "{p}.m16/ns=1", {"f16_tile": 256, "f16_cont": 0}),
    Row("pad_c", 1028, 512, 1028, 1, "{p}.pad/c>", ab="{p}.pad/c=seed>"),
    Row("pad_k", 1024, 1028, 1024, 1, "{p}.pad>"),
    Row("generic", 72, 36, 40, 3, "{p}.generic"),
    Row("staged", 61, 30, 19, 1, "stage/c>{p}.", ab="stage/c=seed>{p}."),
    Row("few_columns", 512, 256, 3, 1, "{p}.", without="gemv"),
    Row("walk_requested", 4096, 256, 8192, 1, "{p}.m16", {"f16_tile": 256, "f16_cont": 1}, without="cont"),
]
ROW = {r.name: r for r in ROWS}
CASES = [pytest.param(r, tr, id=f"{r.name}-{'tr' if tr else 'nn'}") for r in ROWS for tr in r.variants]


@pytest.fixture
def knobs(gpu):
    """Sets a row's knobs (wg_ctx_set_tuning) and restores them afterwards."""
    saved = {}

    def set_(d):
        for k, v in d.items():
            saved.setdefault(k, gpu.set_tuning(k, v))

    yield set_
    for k, v in saved.items():
        gpu.set_tuning(k, v)


def unstorable(x):
    """The share of values no 16-bit store can hold: above 2048 in magnitude and not a multiple of 2 (integers: odd) -- off the f16 grid there, and off bf16's."""
    x = np.asarray(x, np.float32)
    h = x * np.float32(0.5)  # (x is a multiple of 2 exactly when x / 2 is an integer)
    return float(np.mean((np.abs(x) > 2048) & (h != np.rint(h))))


@functools.lru_cache(maxsize=2)
def _integer_case(M, K, N, Z, tr):
    rng = np.random.default_rng((M * 7 + K * 5 + N * 3 + Z) * 2 + int(tr))
    mags = np.arange(9) if K >= 256 else np.array([7, 8, 8, 8])  # (K < 256: only 7s and 8s reach 2048 -- 36 x 64 = 2304)
    A = mags[rng.integers(0, mags.size, (M, K, Z))].astype(np.float32) * rng.choice([-1, 1], (M, 1, Z)).astype(np.float32)
    B = mags[rng.integers(0, mags.size, (K, N, Z))].astype(np.float32) * rng.choice([-1, 1], (1, N, Z)).astype(np.float32)
    v = rng.integers(0, 8192, (M, N, Z), dtype=np.int32)
    C0 = ((8193 + (v & ~1)) * (1 - 2 * (v & 1))).astype(np.float32)  # odd integers of magnitude 8193 .. 16383, either sign
    P = U.int_product(A, B).astype(np.float32)
    # both terms and the sum are exact in f32: 3 P < 2^24, so -0.375 P = -3 P / 8 is exact; 0.5 C0 is; their sum is a multiple of 1/8 below 2^20, i.e. 23 bits
    pmax = float(np.abs(P).max())
    assert 3 * pmax < 2 ** 24 and 0.375 * pmax + 8192 < 2 ** 20
    E = np.float32(AB[0]) * P + np.float32(AB[1]) * C0
    for x in (A, B, C0, P, E):
        x.setflags(write=False)
    return A, B, C0, P, E, unstorable(P), unstorable(E)


def integer_case(name, tr, shares=False):
    """(A, B, C0, P, E): integer operands of a row (A = op(m1), M x K x Z; B; the old `out` C0), the exact product P and the exact -0.375 P + 0.5 C0, as float32.
    Computed once per shape and variant, shared by the rows of that shape, both element types and both views, and never written to."""
    r = ROW[name]
    c = _integer_case(r.M, r.K, r.N, r.mats, bool(tr))
    return c if shares else c[:5]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("row,tr", CASES)
def test_exact_by_construction(gpu, knobs, row, tr, kind):
    """Item 1 (and item 5's first clause: `out` starts as NaN for beta = 0 and is overwritten)."""
    A, B, C0, P, E, share_p, share_e = integer_case(row.name, tr, shares=True)
    print(f"{row.name}: unstorable share of P {share_p:.3f}, of -0.375 P + 0.5 C0 {share_e:.3f}")
    if row.name != "staged":  # (K = 30: |P| <= 1920, see the module docstring)
        assert share_p >= 0.25, share_p
    assert share_e >= 0.25, share_e
    assert np.array_equal(widen(kind, store(kind, A.ravel())), A.ravel()) and np.array_equal(widen(kind, store(kind, B.ravel())), B.ravel())
    knobs(row.knobs)
    m1, m2 = Op(gpu, stored(A, tr), kind), Op(gpu, B, kind)
    for dense in ((True,) if row.dense_only else (True, False)):
        view = "dense" if dense else "odd"
        out = out_view(gpu, "f32", row.M, row.N, row.mats, dense)
        gpu.take_path()
        out32(gpu, tr, kind, 1.0, 0.0, out, m1, m2)
        log = gpu.take_path()
        print(f"  {kind} {view} (1, 0): {log}")
        assert row.took(kind, log, 0.0), f"{row.name} {view}: expected {row.leaf!r}, the call took {log!r}"
        U.assert_bits_equal(out.read(f"{row.name} {view}"), P, f"{row.name} {kind} {view} (1, 0) [{log}]")
        out.set(C0)
        out32(gpu, tr, kind, AB[0], AB[1], out, m1, m2)
        log = gpu.take_path()
        print(f"  {kind} {view} {AB}: {log}")
        assert row.took(kind, log, AB[1]), f"{row.name} {view} {AB}: expected {row.ab!r}, the call took {log!r}"
        U.assert_bits_equal(out.read(f"{row.name} {view} {AB}"), E, f"{row.name} {kind} {view} {AB} [{log}]")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("row,tr", CASES)
def test_one_rounding_from_the_16_bit_call(gpu, knobs, row, tr, kind):
    """Item 2: U[-1, 1) operands stored in the 16-bit type, the old `out` representable in it. Wherever the two logs name the same leaf apart from the prefix -- every
    row but few_columns, whose 16-bit call is a Gemv -- one RNE of the out32 result is the 16-bit result, bit for bit."""
    M, K, N, Z = row.M, row.K, row.N, row.mats
    rng = np.random.default_rng(sum(map(ord, row.name)) * 4 + int(tr) * 2 + len(kind))
    a16, b16 = store(kind, rng.random(M * K * Z, dtype=np.float32) * 2 - 1), store(kind, rng.random(K * N * Z, dtype=np.float32) * 2 - 1)
    c16 = widen(kind, store(kind, rng.random(M * N * Z, dtype=np.float32) * 2 - 1)).reshape(M, N, Z)
    knobs(row.knobs)
    m1 = Op(gpu, widen(kind, a16).reshape(((K, M) if tr else (M, K)) + (Z,)), kind)
    m2 = Op(gpu, widen(kind, b16).reshape(K, N, Z), kind)
    for dense in ((True,) if row.dense_only else (True, False)):
        o16, o32 = out_view(gpu, kind, M, N, Z, dense), out_view(gpu, "f32", M, N, Z, dense)
        for alpha, beta in ((1.0, 0.0), AB):
            if beta != 0.0:
                o16.set(c16)
                o32.set(c16)
            gpu.take_path()
            rc, msg = call(gpu, "wg_gemm_ex", tr, dtype_of(kind), alpha, beta, o16, m1, m2)
            assert rc == 0, msg
            log16 = gpu.take_path()
            out32(gpu, tr, kind, alpha, beta, o32, m1, m2)
            log32 = gpu.take_path()
            print(f"  {row.name} {kind} {'dense' if dense else 'odd'} ({alpha}, {beta}): {log16} | {log32}")
            same = log16.replace(f"{kind}.", f"{kind}o32.") == log32
            if row.name == "few_columns" and not same:
                assert "gemv" in log16 and "gemv" not in log32, (log16, log32)
                continue
            if row.name == "walk_requested" and beta == 0.0:  # (the 16-bit call takes the walk; the tiles, k order and accumulation chains are m16_tile's)
                assert log16 == f"{kind}.cont" and "cont" not in log32, (log16, log32)
            else:
                assert same, f"{row.name}: the logs name different leaves: {log16!r} | {log32!r}"
            got = o32.read(row.name)
            U.assert_bits_equal(store(kind, got.ravel()), np.ascontiguousarray(o16.read(row.name)).ravel(), f"{row.name} {kind} ({alpha}, {beta}): RNE16(out32) against the 16-bit call [{log32}]")


TRUTH_ROWS = [pytest.param(ROW[n], tr, id=f"{n}-{'tr' if tr else 'nn'}") for n in ("t128", "m16_static", "m16_splitk", "generic") for tr in (False, True)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("row,tr", TRUTH_ROWS)
def test_truth(gpu, knobs, row, tr, kind):
    """Item 3: against the f64 product with the f32 gate alone; (alpha, beta): two more f32 roundings of at most 2^-24 relative each, with a factor 2 of slack."""
    M, K, N, Z = row.M, row.K, row.N, row.mats
    rng = np.random.default_rng(sum(map(ord, row.name)) * 8 + int(tr) * 2 + len(kind))
    A = widen(kind, store(kind, rng.random(M * K * Z, dtype=np.float32) * 2 - 1)).reshape(M, K, Z)
    B = widen(kind, store(kind, rng.random(K * N * Z, dtype=np.float32) * 2 - 1)).reshape(K, N, Z)
    C0 = (rng.random((M, N, Z), dtype=np.float32) * 2 - 1) * np.float32(K ** 0.5)
    truth = np.stack([A[:, :, z].astype(np.float64) @ B[:, :, z].astype(np.float64) for z in range(Z)], -1)
    sabs = np.stack([np.abs(A[:, :, z]).astype(np.float64) @ np.abs(B[:, :, z]).astype(np.float64) for z in range(Z)], -1)
    gate = U.f32_gate(K, sabs)
    knobs(row.knobs)
    m1, m2 = Op(gpu, stored(A, tr), kind), Op(gpu, B, kind)
    out = out_view(gpu, "f32", M, N, Z, True)
    gpu.take_path()
    out32(gpu, tr, kind, 1.0, 0.0, out, m1, m2)
    assert row.took(kind, gpu.take_path(), 0.0)
    err = np.abs(out.read(row.name).astype(np.float64) - truth)
    print(f"{row.name} {kind}: worst err / gate = {(err / gate).max():.3g}")
    assert (err <= gate).all(), f"{row.name} {kind}: worst err / gate = {(err / gate).max():.3g}"
    out.set(C0)
    out32(gpu, tr, kind, AB[0], AB[1], out, m1, m2)
    want = AB[0] * truth + AB[1] * C0.astype(np.float64)
    tol = abs(AB[0]) * gate + 2.0 ** -23 * (np.abs(AB[0] * truth) + np.abs(AB[1] * C0.astype(np.float64)))
    err = np.abs(out.read(row.name).astype(np.float64) - want)
    print(f"{row.name} {kind} {AB}: worst err / tol = {(err / tol).max():.3g}")
    assert (err <= tol).all(), f"{row.name} {kind} {AB}: worst err / tol = {(err / tol).max():.3g}"


def test_past_the_16_bit_range(gpu, knobs):
    """Item 4: f16 512^3 of 16.0: every result is exactly 131072 where wg_gemm_ex(WG_F16) gives +Inf. Then 512 x 4096 x 512 as four calls of K = 1024 with beta = 1 on
    integer operands: the one-call result bit for bit, which the same chain through a 16-bit `out` does not reach."""
    wg = _wg()
    n = 512
    ones = np.full((n, n, 1), 16.0, np.float32)
    m1, m2 = Op(gpu, ones, "f16"), Op(gpu, ones, "f16")
    o32, o16 = out_view(gpu, "f32", n, n, 1, True), out_view(gpu, "f16", n, n, 1, True)
    out32(gpu, False, "f16", 1.0, 0.0, o32, m1, m2)
    assert (o32.read() == np.float32(131072.0)).all()
    rc, msg = call(gpu, "wg_gemm_ex", False, dtype_of("f16"), 1.0, 0.0, o16, m1, m2)
    assert rc == 0, msg
    assert np.isposinf(o16.read()).all()

    M, K, N, kc = 512, 4096, 512, 1024
    A, B, _, P, _ = integer_case("t128_split", False)
    for kind in KINDS:
        a, b = Op(gpu, A, kind), Op(gpu, B, kind)
        whole = out_view(gpu, "f32", M, N, 1, True)
        out32(gpu, False, kind, 1.0, 0.0, whole, a, b)
        one_call = whole.read()
        U.assert_bits_equal(one_call, P, f"{kind}: the one-call product")

        class Chunk:
            pass
        res = {}
        for okind, fn in (("f32", "wg_gemm_out32"), (kind, "wg_gemm_ex")):
            acc = out_view(gpu, okind, M, N, 1, True)
            for j in range(K // kc):
                ca, cb = Chunk(), Chunk()
                ca.buf, cb.buf = a.buf, b.buf
                ca.shape = wg.ViewShape((M, kc, 1), M, M * K, j * kc * M)  # columns j kc .. of m1
                cb.shape = wg.ViewShape((kc, N, 1), K, K * N, j * kc)      # rows j kc .. of m2
                rc, msg = call(gpu, fn, False, dtype_of(kind), 1.0, 0.0 if j == 0 else 1.0, acc, ca, cb)
                assert rc == 0, msg
            res[okind] = widen(okind, acc.read())
        U.assert_bits_equal(res["f32"], one_call, f"{kind}: four chunks of K = 1024 through an f32 `out`")
        assert not np.array_equal(res[kind], one_call), f"{kind}: the chain through a 16-bit `out` cannot reach the f32 result"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["t128", "pad_c", "pad_k"])
@pytest.mark.parametrize("tr", [False, True], ids=["nn", "tr"])
def test_special_values(gpu, knobs, name, tr, kind):
    """Item 5: +Inf in the last row and last k of op(m1), -Inf and NaN in the last k of m2 (its last column and column 1): exactly the results the mathematics gives
    them -- load slots past the end of a ragged tile and the zero padding of the padded copies contribute an exact zero, not (last row) x 0."""
    row = ROW[name]
    M, K, N = row.M, row.K, row.N
    rng = np.random.default_rng(M + K * 3 + int(tr))
    A, B = rng.integers(-3, 4, (M, K, 1)).astype(np.float32), rng.integers(1, 4, (K, N, 1)).astype(np.float32)
    A[M - 1, K - 1, 0] = np.inf
    B[K - 1, N - 1, 0] = -np.inf
    B[K - 1, 1, 0] = np.nan
    knobs(row.knobs)
    m1, m2, out = Op(gpu, stored(A, tr), kind), Op(gpu, B, kind), out_view(gpu, "f32", M, N, 1, True)
    gpu.take_path()
    out32(gpu, tr, kind, 1.0, 0.0, out, m1, m2)
    assert row.took(kind, gpu.take_path(), 0.0)
    got = out.read(name)
    U.assert_same_class_bits(got, U.special_product(A, B, np.float32), f"{name} {kind}")
    assert np.isnan(got[:, 1, 0]).all() and (got[M - 1, 2:N - 1, 0] == np.inf).all() and got[M - 1, N - 1, 0] == -np.inf
    assert np.isfinite(got[:M - 1, 2:N - 1, 0]).all() and np.isfinite(got[:M - 1, 0, 0]).all()


def test_status_codes(gpu):
    """Item 6: each status with wg_gemm_ex's message for the same mistake (the 16-bit call on a 16-bit `out` of the same shapes)."""
    wg, L = _wg(), _L()
    kind = "f16"
    M, K, N = 64, 128, 32
    rng = np.random.default_rng(3)
    A, B = rng.integers(-2, 3, (M, K, 1)).astype(np.float32), rng.integers(-2, 3, (K, N, 1)).astype(np.float32)
    m1, m2, m2_bad = Op(gpu, A, kind), Op(gpu, B, kind), Op(gpu, np.ones((K + 4, N, 1)), kind)
    outs = {ok: dict(out=out_view(gpu, ok, M, N, 1, True), out_bad=out_view(gpu, ok, M + 4, N, 1, True), out_t=out_view(gpu, ok, K, N, 1, True)) for ok in ("f32", kind)}

    def both(tr, o, a, b, variant=None):
        x = call(gpu, "wg_gemm_out32", tr, dtype_of(kind), 1.0, 0.0, outs["f32"][o], a, b, variant)
        y = call(gpu, "wg_gemm_ex", tr, dtype_of(kind), 1.0, 0.0, outs[kind][o], a, b, variant)
        assert x == y, (x, y)
        return x

    gpu.take_path()
    rc, msg = both(False, "out", m1, m2_bad)
    assert rc == L.WG_ERR_DIM_MISMATCH and msg == f"Gemm: dimension mismatch. (out [{M},{N},1], m1 [{M},{K},1], m2 [{K + 4},{N},1])"
    rc, msg = both(False, "out_bad", m1, m2)
    assert rc == L.WG_ERR_DIM_MISMATCH and "dimension mismatch" in msg
    rc, msg = both(True, "out", m1, m2)  # m1^T is K x M: the mismatch names the transpose
    assert rc == L.WG_ERR_DIM_MISMATCH and "]^T, m2 [" in msg
    rc, msg = both(False, "out", m1, m2, 9)
    assert rc == L.WG_ERR_INVALID_ARG and msg == "Gemm: unknown variant 9"
    rc, msg = call(gpu, "wg_gemm_out32", False, 7, 1.0, 0.0, outs["f32"]["out"], m1, m2)
    assert rc == L.WG_ERR_INVALID_ARG and msg == "Gemm: unknown dtype 7"
    assert gpu.take_path() == ""
    # each view exceeding its buffer, with wg_gemm_ex's words; bounds use each operand's own element size
    for which in ("m1", "m2"):
        small = Op(gpu, np.ones((M, K // 2, 1)) if which == "m1" else np.ones((K, N // 2, 1)), kind)
        small.shape = m1.shape if which == "m1" else m2.shape
        need = M * K if which == "m1" else K * N
        rc, msg = both(False, "out", small if which == "m1" else m1, small if which == "m2" else m2)
        assert rc == L.WG_ERR_OUT_OF_BOUNDS and msg == f"Gemm: view `{which}` addresses {need} elements but its buffer holds {small.size}", msg
    half = Op(gpu, np.zeros((M * N // 2 - 8, 1, 1)), "f32")  # a buffer sized for M x N two-byte elements: M N / 2 floats (Op adds 8 elements of margin)
    assert half.size == M * N // 2
    half.shape = outs["f32"]["out"].shape
    rc, msg = call(gpu, "wg_gemm_out32", False, dtype_of(kind), 1.0, 0.0, half, m1, m2)
    assert rc == L.WG_ERR_OUT_OF_BOUNDS and msg == f"Gemm: view `out` addresses {M * N} elements but its buffer holds {half.size}", msg
    out_small = {ok: out_view(gpu, ok, M, N // 2, 1, True) for ok in ("f32", kind)}
    for ok in out_small:
        out_small[ok].shape = outs["f32"]["out"].shape
    x = call(gpu, "wg_gemm_out32", False, dtype_of(kind), 1.0, 0.0, out_small["f32"], m1, m2)
    y = call(gpu, "wg_gemm_ex", False, dtype_of(kind), 1.0, 0.0, out_small[kind], m1, m2)
    assert x == y and x[0] == L.WG_ERR_OUT_OF_BOUNDS and "view `out`" in x[1], (x, y)
    # zero-sized views are skipped with WG_OK: nothing launched, nothing written
    z_out = out_view(gpu, "f32", M, N, 1, True)
    before = z_out.buf.read(gpu.device()).copy()
    for shape_out, shape_m2 in ((wg.ViewShape((M, 0, 1), M, M, 0), wg.ViewShape((K, 0, 1), K, K, 0)), (wg.ViewShape((M, N, 0), M, M * N, 0), None)):
        class V:
            pass
        zo, zb, za = V(), V(), V()
        zo.buf, zb.buf, za.buf = z_out.buf, m2.buf, m1.buf
        zo.shape = shape_out
        zb.shape = shape_m2 or wg.ViewShape((K, N, 0), K, K * N, 0)
        za.shape = m1.shape if shape_m2 else wg.ViewShape((M, K, 0), M, M * K, 0)
        gpu.take_path()
        assert call(gpu, "wg_gemm_out32", False, dtype_of(kind), 1.0, 0.0, zo, za, zb)[0] == 0
        assert gpu.take_path() == "" and z_out.buf.read(gpu.device()).tobytes() == before.tobytes()
    # ... and so are zero-sized BUFFERS under views a bounds check would refuse
    h0 = ctypes.c_void_p()
    L.check(L.lib.wg_buf_create(gpu._ctx.handle, 0, S_STORAGE, ctypes.byref(h0)))
    try:
        o_ok = outs["f32"]["out"]
        for which in range(3):
            hs = [h0 if i == which else b.buf._h for i, b in enumerate((o_ok, m1, m2))]
            rc = L.lib.wg_gemm_out32(gpu._ctx.handle, 0, dtype_of(kind), 1.0, 0.0, hs[0], o_ok.shape.to_c(), hs[1], m1.shape.to_c(), hs[2], m2.shape.to_c())
            assert rc == 0, (which, L.lib.wg_last_error_string().decode())
        assert gpu.take_path() == ""
    finally:
        L.check(L.lib.wg_buf_destroy(h0))


@pytest.mark.parametrize("tr", [False, True], ids=["nn", "tr"])
def test_f32_forwards(gpu, tr):
    """in_dtype = WG_F32: wg_gemm_ex(WG_F32) unchanged -- the same log, the same bits."""
    L = _L()
    rng = np.random.default_rng(17)
    M, K, N = 256, 128, 64
    A, B = rng.random((M, K, 1), dtype=np.float32) * 2 - 1, rng.random((K, N, 1), dtype=np.float32) * 2 - 1
    C0 = rng.random((M, N, 1), dtype=np.float32)
    m1, m2 = Op(gpu, stored(A, tr), "f32"), Op(gpu, B, "f32")
    res, logs = [], []
    for fn in ("wg_gemm_ex", "wg_gemm_out32"):
        out = out_view(gpu, "f32", M, N, 1, True)
        out.set(C0)
        gpu.take_path()
        rc, msg = call(gpu, fn, tr, L.WG_F32, AB[0], AB[1], out, m1, m2)
        assert rc == 0, msg
        logs.append(gpu.take_path())
        res.append(out.read(fn))
    assert logs[0] == logs[1] and "f32." in logs[0] and "o32" not in logs[0], logs
    U.assert_bits_equal(res[1], res[0], "wg_gemm_out32(WG_F32) against wg_gemm_ex(WG_F32)")


@pytest.mark.parametrize("name", ["pad_c", "pad_k", "staged"])
def test_workspace_inside_a_recording(name):
    """The padding and staging scratch cannot grow inside a recording: WG_ERR_WORKSPACE on a fresh context, as wg_gemm_ex; after one eager call the same call
    records, and the replay gives the eager bits."""
    wg, L = _wg(), _L()
    row = ROW[name]
    inst = wg.GpuInstance.new(0)
    try:
        A, B, _, P, _ = integer_case(name, False)
        m1, m2, out = Op(inst, A, "bf16"), Op(inst, B, "bf16"), out_view(inst, "f32", row.M, row.N, row.mats, True)
        enc = inst.device().create_command_encoder(record=True)
        try:
            rc, msg = call(inst, "wg_gemm_out32", False, L.WG_BF16, 1.0, 0.0, out, m1, m2)
        finally:
            cb = enc.finish()
        assert rc == L.WG_ERR_WORKSPACE, (rc, msg)
        del cb
        out32(inst, False, "bf16", 1.0, 0.0, out, m1, m2)
        U.assert_bits_equal(out.read(name), P, f"{name}: eager")
        out.poison()
        enc = inst.device().create_command_encoder(record=True)
        try:
            rc, msg = call(inst, "wg_gemm_out32", False, L.WG_BF16, 1.0, 0.0, out, m1, m2)
        finally:
            cb = enc.finish()
        assert rc == 0, msg
        inst.queue().submit([cb])
        U.assert_bits_equal(out.read(name), P, f"{name}: replayed")
        del cb
    finally:
        inst.sync()


@pytest.mark.parametrize("kind", KINDS)
def test_aliasing(gpu, kind):
    """Item 7: `out` (f32) and a 16-bit operand in ONE buffer, decided on addresses in 2-byte units."""
    wg, L = _wg(), _L()
    rng = np.random.default_rng(11)
    M, K, N = 64, 128, 32
    A, B = rng.integers(-2, 3, (M, K, 1)).astype(np.float32), rng.integers(-3, 4, (K, N, 1)).astype(np.float32)
    P = U.int_product(A, B)[:, :, 0]
    m2 = Op(gpu, B, kind)

    class Shared:  # one buffer: M x N floats of `out` at byte 0, then m1 from byte 4 M N on (16-bit element 2 M N)
        pass
    raw = np.zeros(2 * M * N + M * K + 8, np.uint16)
    raw[: 2 * M * N] = np.full(M * N, NAN32).view(np.uint16)
    raw[2 * M * N: 2 * M * N + M * K] = store(kind, A.ravel(order="F")).view(np.uint16)
    buf = wg.TensorBuilder.tensor((raw.size,), S_STORAGE).build_init(gpu.device(), raw, raw.dtype)
    o, a = Shared(), Shared()
    o.buf = a.buf = buf
    o.shape = wg.ViewShape((M, N, 1), M, M * N, 0)
    a.shape = wg.ViewShape((M, K, 1), M, M * K, 2 * M * N)  # begins exactly where out ends
    gpu.take_path()
    rc, msg = call(gpu, "wg_gemm_out32", False, dtype_of(kind), 1.0, 0.0, o, a, m2)
    assert rc == 0, msg
    after = buf.read(gpu.device())
    assert np.array_equal(after[: 2 * M * N].view(np.float32).reshape(N, M).T.astype(np.float64), P), "touching views: wrong result"
    assert np.array_equal(after[2 * M * N:], raw[2 * M * N:]), "touching views: m1 changed"
    # m1 one 16-bit element earlier: the last two bytes of out are shared -> refused, nothing written, nothing logged
    gpu.queue().write_buffer(buf, 0, raw)
    gpu.take_path()
    a.shape = wg.ViewShape((M, K, 1), M, M * K, 2 * M * N - 1)
    rc, msg = call(gpu, "wg_gemm_out32", False, dtype_of(kind), 1.0, 0.0, o, a, m2)
    assert rc == L.WG_ERR_ALIASED and msg == "Gemm: `out` overlaps `m1` (the written view shares memory with a view the call reads)", (rc, msg)
    assert gpu.take_path() == "" and buf.read(gpu.device()).tobytes() == raw.tobytes()
    # ONE byte of overlap: a second handle over the same allocation that starts at the last byte of out
    base = L.lib.wg_buf_device_ptr(buf._h)
    h, h2 = ctypes.c_void_p(), ctypes.c_void_p()
    L.check(L.lib.wg_buf_wrap(gpu._ctx.handle, ctypes.c_void_p(base + 4 * M * N - 1), 2 * M * K, ctypes.byref(h)))
    try:
        a0 = wg.ViewShape((M, K, 1), M, M * K, 0).to_c()
        rc = L.lib.wg_gemm_out32(gpu._ctx.handle, 0, dtype_of(kind), 1.0, 0.0, buf._h, o.shape.to_c(), h, a0, m2.buf._h, m2.shape.to_c())
        assert rc == L.WG_ERR_ALIASED and "`out` overlaps `m1`" in L.lib.wg_last_error_string().decode()
        assert gpu.take_path() == "" and buf.read(gpu.device()).tobytes() == raw.tobytes()
        L.check(L.lib.wg_buf_wrap(gpu._ctx.handle, ctypes.c_void_p(base + 4 * M * N), 2 * M * K, ctypes.byref(h2)))
        rc = L.lib.wg_gemm_out32(gpu._ctx.handle, 0, dtype_of(kind), 1.0, 0.0, buf._h, o.shape.to_c(), h2, a0, m2.buf._h, m2.shape.to_c())
        assert rc == 0, L.lib.wg_last_error_string().decode()  # (one byte further: touching again)
        L.check(L.lib.wg_buf_destroy(h2))
    finally:
        L.check(L.lib.wg_buf_destroy(h))
    assert np.array_equal(buf.read(gpu.device())[: 2 * M * N].view(np.float32).reshape(N, M).T.astype(np.float64), P)

    # out interleaved between the columns of m2: m2 is 8 x 16 with leading dimension 24 (16-bit elements); the 16 elements of padding behind column j are 8 floats
    # = out[:, j] for j < 16 (f32 offset 4 + 12 j): an 8 x 16 result of an 8 x 8 m1
    R2, K2, N2, ld = 8, 8, 16, 24
    A2, B2 = rng.integers(-2, 3, (R2, K2, 1)).astype(np.float32), rng.integers(-3, 4, (K2, N2, 1)).astype(np.float32)
    raw2 = np.zeros(ld * N2 + 8, np.uint16)
    bidx = np.arange(K2)[:, None] + np.arange(N2)[None, :] * ld
    raw2[bidx] = store(kind, B2[:, :, 0].ravel()).reshape(K2, N2).view(np.uint16)
    buf2 = wg.TensorBuilder.tensor((raw2.size,), S_STORAGE).build_init(gpu.device(), raw2, raw2.dtype)
    o2, b2, a2 = Shared(), Shared(), Op(gpu, A2, kind)
    o2.buf = b2.buf = buf2
    o2.shape = wg.ViewShape((R2, N2, 1), ld // 2, 0, K2 // 2)
    b2.shape = wg.ViewShape((K2, N2, 1), ld, 0, 0)
    rc, msg = call(gpu, "wg_gemm_out32", False, dtype_of(kind), 1.0, 0.0, o2, a2, b2)
    assert rc == 0, msg
    after2 = buf2.read(gpu.device())
    oidx = K2 // 2 + np.arange(R2)[:, None] + np.arange(N2)[None, :] * (ld // 2)
    assert np.array_equal(after2.view(np.float32)[oidx].astype(np.float64), U.int_product(A2, B2)[:, :, 0]), "interleaved views: wrong result"
    assert np.array_equal(after2[bidx], raw2[bidx]), "interleaved views: m2 changed"
    o2.shape = wg.ViewShape((R2, N2, 1), ld // 2, 0, K2 // 2 - 1)  # one float earlier: the last two elements of every column of m2
    rc, msg = call(gpu, "wg_gemm_out32", False, dtype_of(kind), 1.0, 0.0, o2, a2, b2)
    assert rc == L.WG_ERR_ALIASED and "`out` overlaps `m2`" in msg


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["t128", "m16_splitk"])
def test_recorded(gpu, knobs, name, kind):
    """Item 8: eager, then recorded once and replayed twice into a re-poisoned output: the eager bits each time, the same log."""
    row = ROW[name]
    A, B, C0, P, E = integer_case(name, False)
    knobs(row.knobs)
    m1, m2, out = Op(gpu, A, kind), Op(gpu, B, kind), out_view(gpu, "f32", row.M, row.N, row.mats, False)
    out.set(C0)
    gpu.take_path()
    out32(gpu, False, kind, AB[0], AB[1], out, m1, m2)
    log = gpu.take_path()
    assert row.took(kind, log, AB[1]), log
    U.assert_bits_equal(out.read(name), E, f"{name} {kind}: eager")
    enc = gpu.device().create_command_encoder(record=True)
    try:
        out32(gpu, False, kind, AB[0], AB[1], out, m1, m2)
    finally:
        cb = enc.finish()
    assert gpu.take_path() == log
    for rep in range(2):
        out.set(C0)
        gpu.queue().submit([cb])
        U.assert_bits_equal(out.read(name), E, f"{name} {kind}: replay {rep}")
    del cb


@pytest.fixture(scope="module")
def masked():
    wg = _wg()
    inst = wg.GpuInstance.new(0, cu_count=64)
    yield inst
    inst.sync()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["m16_static", "t128"])
def test_cu_masked(masked, name, kind):
    """Item 8: a context on a CU-masked stream (64 CUs: the plan reads compute_units) against the integer product."""
    row = ROW[name]
    A, B, C0, P, E = integer_case(name, True)
    old = {k: masked.set_tuning(k, v) for k, v in row.knobs.items()}
    try:
        m1, m2, out = Op(masked, stored(A, True), kind), Op(masked, B, kind), out_view(masked, "f32", row.M, row.N, row.mats, True)
        masked.take_path()
        out32(masked, True, kind, 1.0, 0.0, out, m1, m2)
        log = masked.take_path()
        print(name, kind, "on 64 CUs ->", log)
        assert f"{kind}o32." in log and f"{kind}." not in log
        U.assert_bits_equal(out.read(name), P, f"{name} {kind} on 64 CUs [{log}]")
        out.set(C0)
        out32(masked, True, kind, AB[0], AB[1], out, m1, m2)
        U.assert_bits_equal(out.read(name), E, f"{name} {kind} on 64 CUs {AB}")
    finally:
        for k, v in old.items():
            masked.set_tuning(k, v)


@pytest.mark.parametrize("kind", KINDS + ["f32"])
def test_python_operators(gpu, kind):
    """Item 9: Gemm.dispatch_out32 / dispatch_out32_tr / dispatch_out32_generic on tensors, through a compute pass: the exact integer product of item 1 (odd integers
    above 2048), the out32 element prefix in the launch log (float32 operands forward to the f32 call), NaN in `out` overwritten; alpha and beta reach the call."""
    wg = _wg()
    dev, shapes = gpu.device(), wg.ViewShapeBuffers()
    A, B, C0, P, E = integer_case("t128", False)
    M, K, N = 512, 512, 512
    op = wg.Gemm.from_device(dev)
    V = wg.GemmVariant
    tb = wg.TensorBuilder.tensor((K, N), S_STORAGE).build_init(dev, store(kind, B[:, :, 0].ravel(order="F")), store(kind, B[:1, 0, 0]).dtype)
    for method, tr, extra, kw, want in (("dispatch_out32", False, (), {}, P), ("dispatch_out32_tr", True, (), {}, P), ("dispatch_out32_generic", False, (V.Gemm,), {}, P),
                                        ("dispatch_out32_generic", True, (V.GemmTr,), dict(alpha=AB[0], beta=AB[1]), E)):
        a = stored(A, tr)[:, :, 0]
        ta = wg.TensorBuilder.tensor(a.shape, S_STORAGE).build_init(dev, store(kind, a.ravel(order="F")), store(kind, B[:1, 0, 0]).dtype)
        to = wg.TensorBuilder.tensor((M, N), S_STORAGE).build_init(dev, C0[:, :, 0].ravel(order="F") if kw else np.full(M * N, NAN32), np.float32)
        gpu.take_path()
        enc = dev.create_command_encoder()
        p = enc.compute_pass("out32", None)
        getattr(op, method)(dev, shapes, p, to, ta, tb, *extra, **kw)
        p.end()
        gpu.queue().submit([enc.finish()])
        got = np.asarray(to.read(dev), np.float32).reshape(N, M).T
        path = gpu.take_path()
        assert (f"{kind}o32." if kind != "f32" else "f32.") in path, (method, path)
        U.assert_bits_equal(np.ascontiguousarray(got), np.ascontiguousarray(want[:, :, 0]), f"{method} {kind}")
    with pytest.raises(TypeError):
        wg.Gemm.from_device(dev, wg.row_major_shader_defs()).dispatch_out32(dev, shapes, None, to, ta, tb)
    t16 = wg.TensorBuilder.tensor((M, N), S_STORAGE).build_init(dev, np.zeros(M * N, np.float16), np.float16)
    with pytest.raises(TypeError):
        op.dispatch_out32(dev, shapes, None, t16, ta, tb)
