"""Huge leading dimensions and far views: the address range a leaf works in, which no other GPU test varies (their parents are a few MiB).

B1, test_guard_*: both sides of every leading-dimension guard of the LDS-DMA kernels (tests/test_far_views_host.py GUARDS: the table, its thresholds T found by
    bisection on the planners, the protected 32-bit expressions and their maxima). Per guard, case and variant, at ld = T - 8 (the largest leading dimension the
    fast kernel admits: the largest per-lane byte offset is really formed, on whole and on ragged tiles) and at ld = T (what runs past the guard: the generic
    16-bit kernel, behind the PAD leaf with nothing to pad where the product is large enough; the f32 256 x 128 kernel with dma_ok == 0; the few-row form on
    transposed copies; the plain Gemv kernels). ONE operand carries the huge leading dimension, in a sparse parent of up to 12 GiB; the other operand and the
    output are small dense parents (test_gpu_operands.Stored), whose sentinel checks are as strong as everywhere else. Asserted: WG_OK, the launch log equal to
    the pure planner's tags for this exact query (the fast leaf at T - 8, not it at T -- except behind the kernel-argument guards of gemm_f32.hip, whose log
    cannot differ), the bits of the exact model, and the same bits from a second call.
B2, test_far_*: 64-bit addressing, independent of the guards, one case per Gemm leaf: each of m1, m2, out in turn is a view that starts past the 4 GiB byte mark
    of its parent and whose second matrix starts past 2^32 ELEMENTS of it (16-bit: offset = stride_mat = 2^31 + 8, a parent just over 8 GiB; f32: offset =
    stride_mat = 2^30 + 4 passes 4 GiB of bytes only -- 2^32 elements of f32 would need 16 GiB). A far output also checks 4 KiB around every column and, poisoned
    beforehand, 4 KiB at every address `true address - k * 4 GiB` inside the parent: where a 32-bit wrap would land.

Operands are test_gpu_operands._operands (integers in [-8, 8], f16 edge rows; bf16: test_gpu_bf16._small_ints), the expectation U.special_product, compared to the
bit: no tolerance anywhere. At most 13 GiB of device memory are live in a test, freed before the next; a case skips if the device has less than its need + 4 GiB
free, which on an idle MI355X never happens (the run of record has 0 skips).

Out of reach under the 13 GiB cap (the guards are not shrunk; the host file proves their constants all the same):
  * the 16-bit few-column kernel with the huge leading dimension on GemmTr m1 (512 columns x 2^25 x 2 B = 32 GiB);
  * the f32 few-column kernel on GemmTr m1 (32 GiB), and its Gemv form (9 .. 64 right-hand sides) on GemvTr's matrix;
  * the f32 transposed few-column form on m2 (N >= 512 columns x 2^24 x 4 B = 32 GiB);
  * the 16-bit N-contiguous kernels (K >= 256 rows x 2^25 x 2 B = 16 GiB, either operand).
B2 also runs one row of every Gemv kernel (test_gpu_operands.GEMV_LEAVES) on a far matrix, and f32 Gemv / GemvTr on a matrix whose leading dimension puts its last
column past 4 GiB; wg_copy_view from and into a far view with a huge leading dimension; wg_reduce (rows4, long), wg_reduce_fast and wg_reduce_batched on f16 vectors that end
at element 2^32 - 8 (and three columns 2^31 - 8 apart) against the C oracle; wg_op_assign (Add, Div, Copy) and wg_axpy with `a` or `b` at the far end of an 8 GiB parent.
test_far_out_columns_past_2_32_elements: a 16-bit output whose last columns lie past 2^32 elements of the view's start, on five leaves.
wg_gemv_mixed runs on one N and one T row with the 16-bit matrix far; the few-row form (f32.fewrow>: a transpose of op(m1) into the workspace, the product, a
transpose of the result into the output) runs with m1, m2 and the output in turn far AND with a huge leading dimension, so both transposes meet a far source and a
far destination.
"""
import ctypes
import time

import numpy as np
import pytest

import _bf16 as B
import _util as U
import test_far_views_host as H
from test_gpu_bf16 import Mat, _small_ints
from test_gpu_epilogue import F16, F32, LEAVES, SENTINEL, Row, _lib, _wg, knobs  # noqa: F401  (knobs: the fixture)
from test_gpu_operands import EXTRA_LEAVES, GEMV_LEAVES, RM_LEAVES, GRow, Stored, _gemm_call, _gemv_call, _operands, _reduce_data

pytestmark = pytest.mark.gpu

GiB = 1 << 30
MARGIN = 4096  # bytes of quiet NaN before and after every column run, and the size of a wrap window
S_STORAGE = 128 | 4 | 8
# element type -> (storage dtype of the buffer, bit pattern type, the sentinel outside the views, the NaN an output view starts as)
KINDS = {"f16": (np.float16, np.uint16, 0x7E5A, 0x7E00), "bf16": (np.float16, np.uint16, 0x7FC5, 0x7FC0), "f32": (np.float32, np.uint32, 0x7FC5A5A5, 0x7FC00000)}
assert SENTINEL[F16] == KINDS["f16"][2] and SENTINEL[F32] == KINDS["f32"][2]


def _encode(kind, X):
    with np.errstate(over="ignore", invalid="ignore"):
        return B.to_bits(X) if kind == "bf16" else np.ascontiguousarray(X.astype(KINDS[kind][0])).view(KINDS[kind][1])


def _merge(iv):
    iv = sorted(iv)
    out, (lo, hi) = [], iv[0]
    for a, b in iv[1:]:
        if a <= hi:
            hi = max(hi, b)
        else:
            out.append((lo, hi))
            lo, hi = a, b
    out.append((lo, hi))
    return out


class Far:
    """The sparse sibling of test_gpu_operands.Stored: bit patterns `bits` (rows x columns x matrices) stored column-major at `off` with leading dimension `ld` and
    `batch` elements between matrices, in an UNINITIALISED parent of any size. Only the column runs are written (wg_buf_write: no code under test), each with
    4 KiB of the sentinel NaN before and after it, clipped to the buffer; `out`: also 4 KiB of sentinel at every `address of a run - k * 4 GiB` inside the parent.
    read() returns the view's bits and asserts every sentinel element bit-unchanged."""

    def __init__(self, gpu, kind, bits, ld, off=0, batch=None, out=False):
        wg = _wg()
        st, ut, self.sentinel, _ = KINDS[kind]
        rs, cs, z = bits.shape
        es = np.dtype(ut).itemsize
        m = MARGIN // es
        batch = min(ld * cs, 2 ** 32 - 8) if batch is None else batch  # (one matrix: its stride is never used, and a view carries 32 bits of it)
        assert ld >= rs and (z == 1 or batch >= ld * (cs - 1) + rs) and max(ld, batch, off) < 2 ** 32
        self.size = -(-(off + (z - 1) * batch + (cs - 1) * ld + rs + m) // 65536) * 65536  # (a tensor's dimensions are 32-bit: 65536 x n elements)
        self.nbytes = self.size * es
        free, _ = gpu.mem_info()
        assert self.nbytes <= H.CAP_BYTES, f"{self.nbytes / GiB:.2f} GiB"
        if free < self.nbytes + 4 * GiB:
            pytest.skip(f"{free / GiB:.1f} GiB of device memory free, the case needs {self.nbytes / GiB:.1f} + 4")
        self.gpu, self.kind, self.ut, self.es, self.bits, self.ld, self.off, self.batch = gpu, kind, ut, es, bits, ld, off, batch
        self.buf = wg.TensorBuilder.tensor((65536, self.size // 65536), S_STORAGE).build(gpu.device(), st)
        self.cm = wg.ViewShape((rs, cs, z), ld, batch, off)
        self.rm = wg.ViewShape((cs, rs, z), ld, batch, off)
        self.starts = [(off + t * batch + c * ld, c, t) for t in range(z) for c in range(cs)]  # ascending
        iv = [(max(0, s - m), min(self.size, s + rs + m)) for s, _, _ in self.starts]
        if out:
            for s, _, _ in self.starts:
                for k in range(1, 1 + (s * es >> 32)):
                    w = (s * es - (k << 32)) // es
                    iv.append((w, min(self.size, w + m)))
        self.iv = _merge(iv)
        los = np.array([lo for lo, _ in self.iv], np.int64)
        self.where = np.searchsorted(los, np.array([s for s, _, _ in self.starts], np.int64), side="right") - 1  # the interval of every run
        self._each(write=True)

    def _each(self, write):
        """Per interval: the host image (sentinel, the runs over it) written, or read back and checked against the sentinel outside the runs."""
        L, h, b = _lib(), self.gpu._ctx.handle, self.buf._h
        rs = self.bits.shape[0]
        got = None if write else np.empty_like(self.bits)
        runs = {}
        for (s, c, t), i in zip(self.starts, self.where):
            runs.setdefault(int(i), []).append((s, c, t))
        for i, (lo, hi) in enumerate(self.iv):
            img = np.full(hi - lo, self.sentinel, self.ut)
            if write:
                for s, c, t in runs.get(i, ()):
                    img[s - lo:s - lo + rs] = self.bits[:, c, t]
                L.check(L.lib.wg_buf_write(h, b, lo * self.es, img.ctypes.data_as(ctypes.c_void_p), img.nbytes))
            else:
                back = np.empty(hi - lo, self.ut)
                L.check(L.lib.wg_buf_read(h, b, lo * self.es, back.ctypes.data_as(ctypes.c_void_p), back.nbytes))
                for s, c, t in runs.get(i, ()):
                    got[:, c, t] = back[s - lo:s - lo + rs]
                    back[s - lo:s - lo + rs] = self.sentinel
                bad = np.flatnonzero(back != img)
                assert bad.size == 0, (f"wrote outside the output view: {bad.size} elements of the window at byte {lo * self.es:#x} .. {hi * self.es:#x} changed, "
                                       f"the first at byte {(lo + int(bad[0])) * self.es:#x}")
        return got

    def read(self, what=""):
        return self._each(write=False)

    def repoison(self):
        """Every window written again as at the start: an output's runs are the NaN pattern again (a later call has the whole view to write)."""
        self._each(write=True)

    def free(self):
        self.buf.destroy()


class Near:
    """A small dense parent with NaN sentinels everywhere outside the view -- test_gpu_operands.Stored in its `aligned` layout (f16, f32), test_gpu_bf16.Mat (bf16) --
    behind Far's interface. X: rows x columns x matrices as stored (already transposed where the API stores a transpose)."""

    def __init__(self, gpu, kind, X, out=False):
        wg = _wg()
        self.kind, self.gpu = kind, gpu
        if kind == "bf16":
            bits = np.full(X.shape, KINDS[kind][3], np.uint16) if out else B.to_bits(X)
            self.s = Mat(gpu, bits, off=8, pad=8, gap=8)
            self.buf, self.cm, self.ld, self.batch = self.s.buf, self.s.shape, self.s.ld, self.s.batch
            self.rm = wg.ViewShape((X.shape[1], X.shape[0], X.shape[2]), self.ld, self.batch, 8)
        else:
            dt = F16 if kind == "f16" else F32
            self.s = Stored(gpu, np.full(X.shape, np.nan) if out else X, dt, "aligned", fill=SENTINEL[dt] if out else np.nan)
            self.buf, self.cm, self.rm, self.ld, self.batch = self.s.buf, self.s.cm, self.s.rm, self.s.ld, self.s.batch

    def read(self, what=""):
        got = self.s.read(what)
        return got if self.kind == "bf16" else np.ascontiguousarray(got).view(KINDS[self.kind][1])

    def repoison(self):
        """An output parent as it was uploaded: the sentinel everywhere, the view NaN."""
        flat = self.s.base.copy()
        flat[self.s.idx] = KINDS[self.kind][3] if self.kind == "bf16" else np.nan
        self.gpu.queue().write_buffer(self.s.buf, 0, flat)

    def free(self):
        self.s.buf.destroy()


_DATA = {}


def _data(kind, M, K, N, Z):
    """(A, B, the expected bits), shared by the cases of one product."""
    key = (kind, M, K, N, Z)
    if _DATA.get("key") != key:
        seed = M * 7 + K * 5 + N * 3 + Z
        if kind == "bf16":  # the operands tests/test_gpu_bf16.py uses for its exact cases: every result a bf16 value
            A, Bm = _small_ints(np.random.default_rng(seed), M, K, N, Z)
            want = B.to_bits(np.stack([A[:, :, z] @ Bm[:, :, z] for z in range(Z)], -1))
        else:
            dt = F16 if kind == "f16" else F32
            A, Bm = _operands(seed, dt, M, K, N, Z)
            want = np.ascontiguousarray(U.special_product(A, Bm, dt)).view(KINDS[kind][1])
        _DATA.clear()
        _DATA.update(key=key, v=(A, Bm, want))
    return _DATA["v"]


def _same_bits(kind, got, want, what):
    if kind == "bf16":  # (zeros as one class: the sign of an exact zero sum is open -- tests/test_gpu_bf16.py)
        U.assert_same_class_bits(B.from_bits(got), B.from_bits(want), what)
    else:
        U.assert_bits_equal(got.view(KINDS[kind][0]), want.view(KINDS[kind][0]), what)


def _call(gpu, kind, tr, rm, out, a, b):
    wg, L = _wg(), _lib()
    dt = L.WG_BF16 if kind == "bf16" else wg.wgcore.wg_dtype(KINDS[kind][0])
    h = gpu._ctx.handle
    if rm:
        return L.check(L.lib.wg_gemm_rm(h, int(wg.GemmVariant.GemmTr), dt, out.buf._h, out.rm.to_c(), a.buf._h, a.rm.to_c(), b.buf._h, b.rm.to_c()))
    variant = int(wg.GemmVariant.GemmTr if tr else wg.GemmVariant.Gemm)
    L.check(L.lib.wg_gemm(h, variant, dt, out.buf._h, out.cm.to_c(), a.buf._h, a.cm.to_c(), b.buf._h, b.cm.to_c()))  # (check: WG_OK or an exception)


def _run_gemm(gpu, kind, tr, rm, M, K, N, Z, far, far_kw, what):
    """The product with the operand `far` ("m1" / "m2" / "out") in a Far parent laid out by far_kw, the other two dense and small. Returns (log, the three
    operands, seconds of the second call); asserts the bits, the untouched surroundings of the output, and a second call's identical bits."""
    A, Bm, want = _data(kind, M, K, N, Z)
    stored = {"m1": np.transpose(A, (1, 0, 2)) if (tr and not rm) else A, "m2": np.transpose(Bm, (1, 0, 2)) if rm else Bm,
              "out": np.zeros((N, M, Z) if rm else (M, N, Z))}  # (row-major K x M is the column-major M x K; row-major K x N and M x N are stored transposed)
    ops = {}
    try:
        for name, X in stored.items():
            if name != far:
                ops[name] = Near(gpu, kind, X, out=name == "out")
            elif name == "out":
                ops[name] = Far(gpu, kind, np.full(X.shape, KINDS[kind][3], KINDS[kind][1]), out=True, **far_kw(X.shape[0]))
            else:
                ops[name] = Far(gpu, kind, _encode(kind, X), **far_kw(X.shape[0]))
        gpu.take_path()
        _call(gpu, kind, tr, rm, ops["out"], ops["m1"], ops["m2"])
        log = gpu.take_path()
        got = ops["out"].read(what)
        got = np.transpose(got, (1, 0, 2)) if rm else got
        _same_bits(kind, got, want, f"{what} [{log}]")
        ops["out"].repoison()  # (the second call has every element of the view to write again)
        gpu.sync()
        t0 = time.perf_counter()
        _call(gpu, kind, tr, rm, ops["out"], ops["m1"], ops["m2"])
        gpu.sync()
        secs = time.perf_counter() - t0
        assert gpu.take_path() == log, what
        again = ops["out"].read(what + ", second call")
        U.assert_bits_equal(np.transpose(again, (1, 0, 2)) if rm else again, got, f"{what}: a second call")
        geom = {n: (o.ld, o.batch) for n, o in ops.items()}
        return log, geom, secs
    finally:
        for o in ops.values():
            o.free()


# --------------------------------------------------------------------------------------------------------
# B1: both sides of every guard
# --------------------------------------------------------------------------------------------------------
BF16_TOO = {("f16_tiles_m2", "m16"), ("f16_tiles_m2", "t128")}  # the 256 x 256 per-tile launch and the 128 x 128 kernel, on bfloat16 as well
GUARD_PARAMS = [pytest.param(g, c, tr, kind, side, id=f"{g.name}-{c.label}-{'tr' if tr else 'nn'}-{kind}-{'T' if side else 'T-8'}")
                for g in H.GUARDS if g.family != "gemv32" for c in g.cases for tr in c.variants if tr not in g.unreachable
                for kind in (("f32",) if g.family in ("f32", "f32big", "rm32") else ("f16", "bf16") if (g.name, c.label) in BF16_TOO else ("f16",))
                for side in (0, 1)]


@pytest.mark.parametrize("g,case,tr,kind,side", GUARD_PARAMS)
def test_guard_gemm(gpu, knobs, g, case, tr, kind, side):
    M, K, N = case.M, case.K, case.N
    ld = g.T - 8 + 8 * side
    rm = g.family in ("rm16", "rm32")
    knobs(case.knobs)
    what = f"{g.name} {case.label} {'tr' if tr else 'nn'} {kind} ld = {ld}"
    log, geom, secs = _run_gemm(gpu, kind, tr, rm, M, K, N, 1, g.operand, lambda rows: dict(ld=ld), what)
    print(f"\nTIME {what}: {log!r} {secs * 1e6:.0f} us, far operand {H.far_bytes(g, case, tr, ld) / GiB:.2f} GiB")
    if rm:  # the launcher of the N-contiguous kernels logs one tag; dma_ok is an argument of the kernel
        assert g.fast in log, f"{what}: took {log!r}"
        return
    fam = "f16" if g.family == "f16" else "f32"
    (lda, ab), (ldb, bb), (ldc, cb) = geom["m1"], geom["m2"], geom["out"]
    leaf, want_log = H.expected(fam, tr, M, K, N, case.knobs, lda, ldb, ldc, 1, (ab, bb, cb), prefix=kind, cus=int(gpu.adapter()["compute_units"]))
    assert log == want_log, f"{what}: the plan logs {want_log!r}, the launch {log!r}"
    if g.same_log:  # gemm_f32.hip:602: the same kernel on either side, told by an argument which tile body to run
        assert leaf == "big" and g.fast in log, log
    else:
        assert (leaf in g.fast) == (side == 0), f"{what}: the plan's leaf is {leaf}"


GEMV_PARAMS = [pytest.param(g, c, tr, side, id=f"{g.name}-{c.label}-{'t' if tr else 'n'}-{'T' if side else 'T-8'}")
               for g in H.GUARDS if g.family == "gemv32" for c in g.cases for tr in c.variants if tr not in g.unreachable for side in (0, 1)]


@pytest.mark.parametrize("g,case,tr,side", GEMV_PARAMS)
def test_guard_gemv_as_gemm(gpu, g, case, tr, side):
    """gemv.hip:992: 9 .. 64 right-hand sides run on the f32 few-column Gemm kernel while its 32-bit offsets suffice for the matrix and the vectors, on the plain
    Gemv kernels past that. Not a planner's decision: the tag is asserted, not a whole log."""
    R, K, nrhs = case.M, case.K, case.N
    ld = g.T - 8 + 8 * side
    A, V, want = _data("f32", R, K, nrhs, 1)
    row = GRow("far", F32, tr, *((K, R) if tr else (R, K)), nrhs, 1, "")
    far_m = g.operand == "m1"
    Xm = np.transpose(A, (1, 0, 2)) if tr else A  # (GemvTr: m = op(m)^T)
    m = v = out = None
    try:
        m = Far(gpu, "f32", _encode("f32", Xm), ld=ld) if far_m else Near(gpu, "f32", Xm)
        v = Near(gpu, "f32", V) if far_m else Far(gpu, "f32", _encode("f32", V), ld=ld)
        out = Near(gpu, "f32", np.zeros((R, nrhs, 1)), out=True)
        gpu.take_path()
        _gemv_call(gpu, row, out, m, v)
        log = gpu.take_path()
        what = f"{g.name} {case.label} {'t' if tr else 'n'} ld = {ld} [{log}]"
        assert log.startswith("gemv>") and (g.fast in log) == (side == 0), what
        got = out.read(what)
        _same_bits("f32", got, want, what)
        out.repoison()
        _gemv_call(gpu, row, out, m, v)
        assert gpu.take_path() == log
        U.assert_bits_equal(out.read(what), got, what + ": a second call")
    finally:
        for o in (m, v, out):
            if o is not None:
                o.free()


# --------------------------------------------------------------------------------------------------------
# B2: far views, one per Gemm leaf
# --------------------------------------------------------------------------------------------------------
FAR_ROWS = ("f16_skinny", "f16_skinny_split", "f16_t128", "f16_t128_split", "f16_t256x128", "f16_m16_static", "f16_m16_queues", "f16_m16_splitk", "f16_cont",
            "f16_pad_k", "f16_generic", "f16_t128_krem",
            "f32_mid_unsplit", "f32_mid_forced", "f32_mid_split_forced", "f32_fewrow", "f32_fewrow_skinnyT", "f32_skinny", "f32_skinny_split", "f32_skinny_panels",
            "f32_big", "f32_big_splitk",
            "rm_f16_nt", "rm_f16_t128nc", "rm_f16_t256x128nc", "rm_f32_nt")
ROWS = {r.name: r for r in LEAVES + EXTRA_LEAVES + RM_LEAVES}
FAR_PARAMS = [pytest.param(ROWS[n], far, id=f"{n}-{far}") for n in FAR_ROWS for far in ("m1", "m2", "out")]


def _far_layout(kind):
    """offset = stride_mat: 16-bit 2^31 + 8 (the second matrix starts past 2^32 elements and 8 GiB), f32 2^30 + 4 (past 4 GiB and 8 GiB of bytes; 2^32 elements
    of f32 would need a 16 GiB parent)."""
    at = (1 << 31) + 8 if kind != "f32" else (1 << 30) + 4
    return lambda rows: dict(ld=rows + 8, off=at, batch=at)


def _mats(row, tr, rm):
    """Two matrices wherever the row's leaf takes a batch (the planner says so for this very geometry), else the row's one matrix."""
    if rm or row.mats > 1:
        return 2
    fam = "f16" if row.dtype == F16 else "f32"
    at = (1 << 31) + 8 if fam == "f16" else (1 << 30) + 4
    M, K, N = row.M, row.K, row.N
    _, log = H.expected(fam, tr, M, K, N, row.knobs, mats=2, batches=(at, (K + 8) * N + 8, (M + 8) * N + 8))
    return 2 if Row.took(row.leaf, log) else 1


@pytest.mark.parametrize("row,far", FAR_PARAMS)
def test_far_gemm(gpu, knobs, row, far):
    rm = getattr(row, "api", "cm") == "rm"
    tr = row.variants[0]
    kind = "f16" if row.dtype == F16 else "f32"
    M, K, N = row.M, row.K, row.N
    Z = _mats(row, tr, rm)
    knobs(row.knobs)
    what = f"{row.name} {'tr' if tr else 'nn'} x {Z}, far {far}"
    log, geom, _ = _run_gemm(gpu, kind, tr, rm, M, K, N, Z, far, _far_layout(kind), what)
    assert Row.took(row.leaf, log), f"{what}: expected {row.leaf!r}, took {log!r}"
    if not rm:  # the launchers execute their plans: the whole log is the planner's for this exact query
        (lda, ab), (ldb, bb), (ldc, cb) = geom["m1"], geom["m2"], geom["out"]
        _, want_log = H.expected(kind, tr, M, K, N, row.knobs, lda, ldb, ldc, Z, (ab, bb, cb), cus=int(gpu.adapter()["compute_units"]))
        assert log == want_log, f"{what}: the plan logs {want_log!r}, the launch {log!r}"



# an output whose columns are 2^24 + 8 elements apart: from column 256 on `column * ldc` passes 2^32 ELEMENTS. A store index formed in 32 bits would wrap column
# 256 + j to 256 * ldc mod 2^32 + j * ldc = 2048 + j * ldc elements from the view's start: 2048 elements past the start of column j, which for these runs of 72 .. 264
# rows is the sentinel margin behind column j's run. Far.read checks the margins first ("wrote outside the output view"), and columns 256 .. 263 would keep their NaN,
# so the bits fail as well. 264 columns of 16-bit elements are 8.3 GiB; the same on f32 would need 16.5 GiB: out of reach.
WIDE_OUT = [("m16", H.T256, 264, 256, 264), ("t128", {"f16_tile": 128}, 264, 256, 264), ("t256x128", {"f16_tile": 256128}, 264, 256, 264),
            ("generic", {}, 72, 36, 264), ("pad_k", {}, 264, 260, 264)]


@pytest.mark.parametrize("tr", [False, True])
@pytest.mark.parametrize("label,kn,M,K,N", WIDE_OUT, ids=[w[0] for w in WIDE_OUT])
def test_far_out_columns_past_2_32_elements(gpu, knobs, label, kn, M, K, N, tr):
    knobs(kn)
    ldc = (1 << 24) + 8
    assert (N - 1) * ldc >= 1 << 32
    what = f"{label} {'tr' if tr else 'nn'} {M} x {K} x {N}, ldc = 2^24 + 8"
    log, geom, _ = _run_gemm(gpu, "f16", tr, False, M, K, N, 1, "out", lambda rows: dict(ld=ldc), what)
    (lda, ab), (ldb, bb), (_, cb) = geom["m1"], geom["m2"], geom["out"]
    leaf, want_log = H.expected("f16", tr, M, K, N, kn, lda, ldb, ldc, 1, (ab, bb, cb), cus=int(gpu.adapter()["compute_units"]))
    assert log == want_log and leaf == {"pad_k": "pad"}.get(label, label), f"{what}: the plan logs {want_log!r} ({leaf}), the launch {log!r}"

# --------------------------------------------------------------------------------------------------------
# B2: far matrices, one row per Gemv kernel
# --------------------------------------------------------------------------------------------------------
FAR_GEMV = ("n_t2", "n_t1_split", "f16_n_t4_split", "small_rl8", "f16_small_rl4", "t_t2", "t_t2_split", "f16_t_t4", "tcols_e4u4", "f16_tcols_e8u4", "f16_tcols_split",
            "tlds_nr2_c1_256", "any_n_k69", "f16_any_t")
GROWS = {r.name: r for r in GEMV_LEAVES}
# f32 Gemv on 64 columns 2^25 apart, GemvTr on 256 columns 2^23 apart: the last column starts past 4 GiB. The matrix alone is 8 GiB, so under the 13 GiB cap it
# cannot also start past 4 GiB of its parent: these two are at offset 0 (the rows above are the far views). The leaf is the row's: the Gemv heuristics read the
# leading dimension only for one right-hand side of f32 GemvTr (gemv.hip uses_t_cols), which neither of these is.
HUGE_LD = {"n_t1": 1 << 25, "t_t2_split": 1 << 23}
FAR_GEMV_PARAMS = [pytest.param(GROWS[n], None, id=n) for n in FAR_GEMV] + [pytest.param(GROWS[n], ld, id=f"{n}-ld2^{ld.bit_length() - 1}") for n, ld in HUGE_LD.items()]


@pytest.mark.parametrize("row,huge_ld", FAR_GEMV_PARAMS)
def test_far_gemv(gpu, knobs, row, huge_ld):
    kind = "f16" if row.dtype == F16 else "f32"
    ro, k = (row.C, row.R) if row.tr else (row.R, row.C)
    Z = row.mats
    knobs(row.knobs)
    A, V, want = _data(kind, ro, k, row.nrhs, Z)
    Xm = np.transpose(A, (1, 0, 2)) if row.tr else A  # (GemvTr: m = op(m)^T)
    at = (1 << 31) + 8 if kind == "f16" else (1 << 30) + 4
    if huge_ld:
        assert Z == 1 and (Xm.shape[1] - 1) * huge_ld * 4 > 1 << 32
        layout = dict(ld=huge_ld)
    elif row.name.startswith(("any_", "f16_any")):  # the any-alignment kernels are reached by an odd leading dimension and offset
        layout = dict(ld=Xm.shape[0] + (1 if Xm.shape[0] % 2 == 0 else 2), off=at + 1, batch=at + 1)
    else:
        ld = -(-(Xm.shape[0] + 8) // row.ld_mult) * row.ld_mult
        layout = dict(ld=ld, off=at, batch=max(at, ld * Xm.shape[1] + 8))
    m = v = out = None
    try:
        m = Far(gpu, kind, _encode(kind, Xm), **layout)
        v = Near(gpu, kind, V)
        out = Near(gpu, kind, np.zeros((ro, row.nrhs, Z)), out=True)
        gpu.take_path()
        _gemv_call(gpu, row, out, m, v)
        log = gpu.take_path()
        what = f"{row.name} far matrix {layout} [{log}]"
        assert log.startswith("gemv") and Row.took(row.leaf, log, row.not_), f"{what}: expected {row.leaf!r}"
        got = out.read(what)
        _same_bits(kind, got, want, what)
        out.repoison()
        _gemv_call(gpu, row, out, m, v)
        assert gpu.take_path() == log
        U.assert_bits_equal(out.read(what), got, what + ": a second call")
    finally:
        for o in (m, v, out):
            if o is not None:
                o.free()


# --------------------------------------------------------------------------------------------------------
# B2: copies, Reduce, OpAssign / Axpy at the far end of an 8 GiB parent
# --------------------------------------------------------------------------------------------------------
def _dt(kind):
    return _wg().wgcore.wg_dtype(KINDS[kind][0])


@pytest.mark.parametrize("kind", ["f16", "f32"])
@pytest.mark.parametrize("far", ["src", "dst"])
def test_far_copy_view(gpu, kind, far):
    """wg_copy_view of a 264 x 96 x 2 block: from (or into) a view whose columns are 2^24 (f32: 2^23) elements apart, whose first matrix straddles the 4 GiB byte
    mark of the parent and whose second one straddles element 2^32 (f32: 8 GiB), into (from) a small dense one: the bits, and nothing else touched."""
    L, h = _lib(), gpu._ctx.handle
    at = (1 << 31) + 8 if kind == "f16" else (1 << 30) + 4
    ut = KINDS[kind][1]
    ld = 1 << (24 if kind == "f16" else 23)
    geom = dict(ld=ld, off=at - 95 * ld // 2, batch=at)
    X = np.random.default_rng(11).integers(-2048, 2049, (264, 96, 2)).astype(np.float64)
    src = dst = None
    try:
        if far == "src":
            src = Far(gpu, kind, _encode(kind, X), **geom)
            dst = Near(gpu, kind, np.zeros(X.shape), out=True)
        else:
            src = Near(gpu, kind, X)
            dst = Far(gpu, kind, np.full(X.shape, KINDS[kind][3], ut), out=True, **geom)
        L.check(L.lib.wg_copy_view(h, _dt(kind), dst.buf._h, dst.cm.to_c(), src.buf._h, src.cm.to_c()))
        U.assert_bits_equal(dst.read("copy_view"), _encode(kind, X), f"copy_view, far {far}")
    finally:
        for o in (src, dst):
            if o is not None:
                o.free()


# path, length, columns, the kernel it must reach
FAR_REDUCE = [("single", 4097, 1, "reduce.rows4/"), ("single", 300007, 1, "reduce.long"), ("fast", 65541, 1, "reduce.fast/"), ("batched", 1000, 1, "reduce.rows4/"),
              ("batched", 1000, 3, "reduce.rows4/")]


@pytest.mark.parametrize("path,n,cols,leaf", FAR_REDUCE, ids=[f"{p}-{n}x{c}" for p, n, c, _ in FAR_REDUCE])
def test_far_reduce(gpu, oracle_c, path, n, cols, leaf):
    """f16 vectors that end at element 2^32 - 8 of an 8 GiB parent (three columns: 2^31 - 8 apart, the last one starting there): every op on integers whose result is
    the same in any order, to the bit of the C oracle -- as tests/test_gpu_operands.py test_reduce_special_values compares its finite case."""
    wg, L, h = _wg(), _lib(), gpu._ctx.handle
    from oracle import wgsl_oracle as wo
    from test_gpu_epilogue import _upload
    stride = (1 << 31) - 8
    off = (1 << 32) - 8 - n if cols == 1 else 8  # (three columns: at 8, 2^31 and 2^32 - 8 -- the last one's elements pass index 2^32)
    rng = np.random.default_rng(n + cols)
    call = {"single": L.lib.wg_reduce, "fast": L.lib.wg_reduce_fast, "batched": L.lib.wg_reduce_batched}[path]
    for op, wop, fam in ((wg.ReduceOp.Min, wo.MIN, "minmax"), (wg.ReduceOp.Max, wo.MAX, "minmax"), (wg.ReduceOp.Sum, wo.SUM, "sum"),
                         (wg.ReduceOp.SqNorm, wo.SQNORM, "sum"), (wg.ReduceOp.Prod, wo.PROD, "prod")):
        case, x = _reduce_data(rng, n, fam, F16)[0]
        assert case == "finite"
        xs = np.stack([np.roll(x, 7 * c) for c in range(cols)], 1).astype(F16)
        far = res = None
        try:
            far = Far(gpu, "f16", np.ascontiguousarray(xs).view(np.uint16)[:, :, None], ld=stride if cols > 1 else n, off=off)
            res = _upload(gpu, np.full(cols, np.nan, F16))
            gpu.take_path()
            L.check(call(h, int(op), _dt("f16"), far.buf._h, far.cm.to_c(), res._h))
            got = res.read(gpu.device())
            log = gpu.take_path()
            want_leaf = "reduce.fast/" if path == "single" and n >= 65536 and fam == "minmax" else leaf  # (as test_reduce_special_values: Min / Max of a long vector)
            assert want_leaf in log, f"{path} n={n} {op.name}: expected {want_leaf!r}, took {log!r}"
            x32 = xs.astype(np.float32)
            want = np.array([oracle_c.reduce(int(wop), np.ascontiguousarray(x32[:, c]), wo.Shape(n, 1, 1, n, n, 0)) for c in range(cols)], np.float32).astype(F16)
            assert np.isfinite(want).all()
            U.assert_same_class_bits(got, want, f"far {path} {op.name} n={n} x {cols} [{log}]")
        finally:
            for o in (far,):
                if o is not None:
                    o.free()
            if res is not None:
                res.destroy()


@pytest.mark.parametrize("kind", ["f16", "f32"])
@pytest.mark.parametrize("far", ["a", "b"])
def test_far_op_assign_and_axpy(gpu, kind, far):
    """wg_op_assign (Add, Div, Copy) and wg_axpy on 100003 elements with `a` (or `b`) ending 8 elements before the end of an 8 GiB parent -- element 2^32 - 8 (16-bit),
    2^31 - 8 (f32) -- and the other operand small: the correctly rounded f32 result rounded once, to the bit; around `a`, and where a 32-bit wrap would land, nothing
    changes."""
    wg, L, h = _wg(), _lib(), gpu._ctx.handle
    n = 100003
    off = ((1 << 32) if kind == "f16" else (1 << 31)) - 8 - n
    st = KINDS[kind][0]
    rng = np.random.default_rng(5 + (far == "a"))
    a0 = (rng.random(n, dtype=np.float32) * 4 - 2).astype(st)
    b0 = (rng.random(n, dtype=np.float32) * 3 + 0.5).astype(st)  # (no zero divisor)
    x, y = a0.astype(np.float32), b0.astype(np.float32)
    alpha = np.float32(U.AXPY_ALPHA)
    with np.errstate(all="ignore"):
        cases = [("Add", x + y), ("Div", x / y), ("Copy", y), ("axpy", U.fmaf_f32(alpha, y, x))]
    for name, r in cases:
        a = b = None
        try:
            bits = lambda v: np.ascontiguousarray(v).view(KINDS[kind][1])[:, None, None]
            a = Far(gpu, kind, bits(a0), ld=n, off=off, out=True) if far == "a" else Near(gpu, kind, a0.astype(np.float64)[:, None, None])
            b = Far(gpu, kind, bits(b0), ld=n, off=off) if far == "b" else Near(gpu, kind, b0.astype(np.float64)[:, None, None])
            if name == "axpy":
                L.check(L.lib.wg_axpy(h, float(alpha), _dt(kind), a.buf._h, a.cm.to_c(), b.buf._h, b.cm.to_c()))
            else:
                L.check(L.lib.wg_op_assign(h, int(wg.OpAssignVariant[name]), _dt(kind), a.buf._h, a.cm.to_c(), b.buf._h, b.cm.to_c()))
            got = a.read(name)[:, 0, 0]
            U.assert_bits_equal(got.view(st), r.astype(st), f"{name} {kind}, far {far}")
        finally:
            for o in (a, b):
                if o is not None:
                    o.free()


# --------------------------------------------------------------------------------------------------------
# B2: the few-row form's transposes from and into far views with huge leading dimensions; wg_gemv_mixed on a far 16-bit matrix
# --------------------------------------------------------------------------------------------------------
FEWROW = ROWS["f32_fewrow"]  # 96 x 256 x 8192: M in 65 .. 128 and N > 4096 take the form at any leading dimension
# the far operand: past 4 GiB of its parent, its columns 2^22 (m1: 96 or 256 columns) or 2^18 (m2, out: 8192 columns) elements apart -- 8 .. 12 GiB parents
FEWROW_LD = {"m1": 1 << 22, "m2": 1 << 18, "out": 1 << 18}


@pytest.mark.parametrize("tr", [False, True])
@pytest.mark.parametrize("far", ["m1", "m2", "out"])
def test_far_fewrow_transposes(gpu, knobs, far, tr):
    """Gemm: op(m1) is transposed from m1 where it lies (far m1: a far, huge-ld source) and the result is transposed into the output (far out: a far, huge-ld
    destination; its columns' margins and wrap windows stay untouched); GemmTr skips the first copy. The log is the planner's, its leaf the few-row form."""
    M, K, N = FEWROW.M, FEWROW.K, FEWROW.N
    knobs(FEWROW.knobs)
    at, ld = (1 << 30) + 4, FEWROW_LD[far]
    what = f"f32_fewrow {'tr' if tr else 'nn'}, far {far} at ld = {ld}"
    log, geom, _ = _run_gemm(gpu, "f32", tr, False, M, K, N, 1, far, lambda rows: dict(ld=ld, off=at), what)
    (lda, ab), (ldb, bb), (ldc, cb) = geom["m1"], geom["m2"], geom["out"]
    leaf, want_log = H.expected("f32", tr, M, K, N, FEWROW.knobs, lda, ldb, ldc, 1, (ab, bb, cb), cus=int(gpu.adapter()["compute_units"]))
    assert leaf == "fewrow" and log == want_log and log.endswith(" transpose") and (tr or "f32.fewrow>transpose" in log), f"{what}: plan {want_log!r}, launch {log!r}"


# name, GemvTr, stored rows, stored columns, right-hand sides, the tags (tests/test_gpu_gemv_mixed.py CASES: n_split_2mats and tcols_e8_2mats, two matrices each)
MIXED = [("n_split_2mats", False, 64, 256, 2, ["gemv.n/t=2,ns=", "gemv.combine/ns="]), ("tcols_e8_2mats", True, 1024, 512, 1, ["gemv.tcols/e=8,u=4,v=1,ns=1"])]


@pytest.mark.parametrize("kind", ["f16", "bf16"])
@pytest.mark.parametrize("name,tr,R,C,nrhs,tags", MIXED, ids=[m[0] for m in MIXED])
def test_far_gemv_mixed(gpu, name, tr, R, C, nrhs, tags, kind):
    """wg_gemv_mixed (a 16-bit matrix, f32 vectors and result; its own dispatcher): two matrices at offset = stride_mat = 2^31 + 8 of an 8 GiB parent -- the second
    starts past 2^32 elements --, the f32 vectors and the output small. Integer operands: the f32 result is exact in any order."""
    L, wg = _lib(), _wg()
    ro, k = (C, R) if tr else (R, C)
    A, V, _ = _data(kind, ro, k, nrhs, 2)
    want = np.ascontiguousarray(U.special_product(A, V, F32)).view(np.uint32)
    Xm = np.transpose(A, (1, 0, 2)) if tr else A
    at = (1 << 31) + 8
    m = v = out = None
    try:
        m = Far(gpu, kind, _encode(kind, Xm), ld=R + 8, off=at, batch=at)
        v = Near(gpu, "f32", V)
        out = Near(gpu, "f32", np.zeros((ro, nrhs, 2)), out=True)
        variant = int(wg.GemvVariant.GemvTr if tr else wg.GemvVariant.Gemv)
        dt = L.WG_BF16 if kind == "bf16" else _dt("f16")
        logs = []
        for _ in range(2):
            gpu.take_path()
            L.check(L.lib.wg_gemv_mixed(gpu._ctx.handle, variant, dt, out.buf._h, out.cm.to_c(), m.buf._h, m.cm.to_c(), v.buf._h, v.cm.to_c()))
            logs.append(gpu.take_path())
            what = f"gemv_mixed {name} {kind}, far matrix [{logs[-1]}]"
            assert logs[-1].startswith(f"gemv>{kind}w.gemv") and all(t in logs[-1] for t in tags), what
            U.assert_bits_equal(out.read(what), want, what)
            out.repoison()
        assert logs[0] == logs[1]
    finally:
        for o in (m, v, out):
            if o is not None:
                o.free()
