"""WG_BF16 on the GPU, through every operator that takes a dtype. Before the feature every call below failed with WG_ERR_INVALID_ARG ("unknown dtype 2").

The contract (include/wgebra_hip.h, wg_dtype): bf16 -> f32 exact, ONE round-to-nearest-even at the store, f32 accumulation in the f16 kernels' orders. Expected
values come from tests/_bf16.py (bit-level RNE, independent of the package's helper). Tolerances: |got - truth| <= f32_gate(K, sum|a||b|) + 2^-8 |truth| + 2^-126
(half a bf16 ulp of the result: bf16 has 8 significant bits, exactly as 2^-11 is half an f16 ulp), and 2 gate + 2^-8 |o| + 2^-126 against the f32 restatement o.

  1  Gemm / GemmTr on the F16_SHAPES of test_gpu_parity.py under each forced 16-bit tile family            test_gemm_bf16_shapes
  2  small-integer operands (every result exact in bf16), +-Inf / NaN operands, on every f16 leaf's shape    test_gemm_bf16_exact_and_special
  3  one rounding, and which one: alpha acc + beta c on bf16 ties and next to them; overflow to Inf          test_gemm_ex_rounds_once_to_nearest_even
  4  the launch log of the bf16 call = the f16 call's with "f16." -> "bf16."                                 test_same_tree_as_f16_*
  5  the continuous walk is bit-identical to the per-tile launch                                             test_continuous_walk_is_bit_identical
  6  views: odd offset / leading dimension, staged lengths, odd N, wg_gemm_rm natively and through the copy   test_gemm_bf16_views, test_gemm_rm_native_equals_copy
  7  Gemv / GemvTr, wg_gemv_rm, the any-alignment kernels, several right-hand sides                          test_gemv_bf16
  8  Reduce, batched, fast, wg_gemv_reduce                                                                   test_reduce_bf16, test_gemv_reduce_bf16
  9  OpAssign (five ops), Axpy                                                                               test_op_assign_bf16
 10  wg_copy_view, wg_cube_to_matrix move the 16 bits unchanged                                              test_copies_move_bits
 11  recorded and replayed; a CU-masked context                                                              test_recorded_and_masked
 12  Gemm and GemmTr 8192^3, sampled                                                                         test_fullsize_8192
 13  f16 results are bit for bit what they were before the 16-bit sources became a switch (fixture)           test_f16_bits_unchanged
"""
import faulthandler
import os
import sys

import numpy as np
import pytest

import _bf16 as B
import _util as U
from test_gpu_epilogue import LEAVES, Row, knobs  # noqa: F401  (knobs: the fixture)
from test_gpu_operands import EXTRA_LEAVES, GEMV_LEAVES, RM_LEAVES
from test_gpu_parity import F16_SHAPES, f16_tile  # noqa: F401  (f16_tile: the fixture that forces a 16-bit tile family)

pytestmark = pytest.mark.gpu

S_STORAGE = 128 | 4 | 8
F16 = np.float16
TINY = 2.0 ** -126


def _wg():
    import wgmath_amd as wg
    return wg


def _L():
    from wgmath_amd import _lib
    return _lib


@pytest.fixture(autouse=True)
def _time_limit():
    """No test of this file may hang the run: after 300 s a watchdog thread (faulthandler: C code, so a call blocked inside the HIP runtime does not hold it up) dumps
    the tracebacks and ENDS THE PROCESS -- the session stops there and nothing more is started on a card that may have hung."""
    faulthandler.dump_traceback_later(300, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


# ---- plumbing --------------------------------------------------------------------------------------------------------------------------------------
def up_bits(gpu, bits):
    """uint16 bf16 patterns -> a bf16 tensor."""
    wg = _wg()
    bits = np.ascontiguousarray(bits, np.uint16).ravel()
    return wg.TensorBuilder.tensor((bits.size,), S_STORAGE).build_init(gpu.device(), bits.view(wg.bfloat16), wg.bfloat16)


def up(gpu, flat):
    wg = _wg()
    flat = np.ascontiguousarray(flat).ravel()
    return wg.TensorBuilder.tensor((flat.size,), S_STORAGE).build_init(gpu.device(), flat, flat.dtype)


def rd_bits(gpu, t):
    return t.read(gpu.device()).view(np.uint16)


def run(gpu, fn):
    enc = gpu.device().create_command_encoder()
    with enc.compute_pass("bf16", None) as p:
        fn(p)
    gpu.queue().submit([enc.finish()])


class Mat:
    """A stack of matrices X[r, c, z] stored column-major in a buffer of 16-bit patterns at `off`, leading dimension rows + `pad`, `gap` elements between
    matrices; everything else holds `fill` (a quiet NaN with a payload no kernel writes)."""

    def __init__(self, gpu, bits, off=0, pad=0, gap=0, fill=0x7FC5, dt="bf16"):
        wg = _wg()
        R, C, Z = bits.shape
        self.ld, self.off = R + pad, off
        self.batch = self.ld * C + gap
        self.size = off + self.batch * Z + 9
        self.idx = off + np.arange(R)[:, None, None] + np.arange(C)[None, :, None] * self.ld + np.arange(Z)[None, None, :] * self.batch
        self.base = np.full(self.size, fill, np.uint16)
        flat = self.base.copy()
        flat[self.idx] = bits
        self.gpu, self.dt = gpu, dt
        self.buf = up_bits(gpu, flat) if dt == "bf16" else up(gpu, flat.view(F16))
        self.shape = wg.ViewShape((R, C, Z), self.ld, self.batch, off)
        self.mask = np.ones(self.size, bool)
        self.mask[self.idx.ravel()] = False

    def read(self, what=""):
        flat = self.buf.read(self.gpu.device()).view(np.uint16)
        assert np.array_equal(flat[self.mask], self.base[self.mask]), f"{what}: wrote outside the view"
        return flat[self.idx]


def gemm(gpu, tr, out, a, b, alpha=None, beta=None, rm=False, dt=None):
    wg, L = _wg(), _L()
    dt = L.WG_BF16 if dt is None else dt
    h = gpu._ctx.handle
    variant = int(wg.GemmVariant.GemmTr if tr else wg.GemmVariant.Gemm)
    if rm:
        L.check(L.lib.wg_gemm_rm(h, variant, dt, out.buf._h, out.shape.to_c(), a.buf._h, a.shape.to_c(), b.buf._h, b.shape.to_c()))
    elif alpha is None:
        L.check(L.lib.wg_gemm(h, variant, dt, out.buf._h, out.shape.to_c(), a.buf._h, a.shape.to_c(), b.buf._h, b.shape.to_c()))
    else:
        L.check(L.lib.wg_gemm_ex(h, variant, dt, float(alpha), float(beta), out.buf._h, out.shape.to_c(), a.buf._h, a.shape.to_c(), b.buf._h, b.shape.to_c()))


def rnd_bits(rng, shape):
    """U[-1, 1) rounded to bf16, as bits."""
    return B.to_bits(rng.random(shape, dtype=np.float32) * 2 - 1)


def stored_a(A_bits, tr):
    """op(A) is M x K x Z; GemmTr stores it K x M."""
    return np.transpose(A_bits, (1, 0, 2)) if tr else A_bits


def product_check(got_bits, A_bits, B_bits, K, what):
    got = B.from_bits(got_bits).astype(np.float64)
    for z in range(A_bits.shape[2]):
        a64, b64 = B.from_bits(A_bits[:, :, z]).astype(np.float64), B.from_bits(B_bits[:, :, z]).astype(np.float64)
        truth, sabs = a64 @ b64, np.abs(a64) @ np.abs(b64)
        tol = U.f32_gate(K, sabs) + 2.0 ** -8 * np.abs(truth) + TINY
        err = np.abs(got[:, :, z] - truth)
        assert not np.isnan(err).any(), f"{what}: NaN left in the output"
        print(f"{what} mat {z}: worst err/tol {(err / tol).max():.3g}")
        assert (err <= tol).all(), f"{what} mat {z}: worst err/tol = {(err / tol).max():.3g} at {np.unravel_index((err / tol).argmax(), err.shape)}"


# ---- 1 -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K,N,mats", F16_SHAPES)
@pytest.mark.parametrize("tr", [False, True])
def test_gemm_bf16_shapes(gpu, oracle_c, f16_tile, M, K, N, mats, tr):
    from oracle import wgsl_oracle as wo
    rng = np.random.default_rng(M * 31 + K * 17 + N + mats + int(tr))
    A, Bm = rnd_bits(rng, (M, K, mats)), rnd_bits(rng, (K, N, mats))
    a, b = Mat(gpu, stored_a(A, tr)), Mat(gpu, Bm)
    out = Mat(gpu, np.full((M, N, mats), 0x7FC0, np.uint16))
    gemm(gpu, tr, out, a, b)
    got = out.read("shapes")
    product_check(got, A, Bm, K, f"bf16 gemm {M}x{K}x{N} tr={tr} tile={f16_tile}")
    # the f32 restatement on the (exactly representable) bf16 operands, where it finishes in seconds: the rule of test_gemm_f16_shapes
    if (tr or f16_tile == "auto") and M * K * N * mats <= (1 << 31):
        s1 = wo.Shape(K, M, mats) if tr else wo.Shape(M, K, mats)
        s2, so = wo.Shape(K, N, mats), wo.Shape(M, N, mats)
        af = B.from_bits(stored_a(A, tr)).transpose(2, 1, 0).ravel().copy()  # column-major, matrices back to back
        bf = B.from_bits(Bm).transpose(2, 1, 0).ravel().copy()
        orc = np.zeros(M * N * mats, np.float32)
        oracle_c.gemm(wo.GEMM_TR if tr else wo.GEMM, orc, so, af, s1, bf, s2)
        O = wo.view(orc, so)
        g = B.from_bits(got).astype(np.float64)
        for t in range(mats):
            a64, b64 = B.from_bits(A[:, :, t]).astype(np.float64), B.from_bits(Bm[:, :, t]).astype(np.float64)
            o64 = O[:, :, t].astype(np.float64)
            tol = 2.0 * U.f32_gate(K, np.abs(a64) @ np.abs(b64)) + 2.0 ** -8 * np.abs(o64) + TINY
            err = np.abs(g[:, :, t] - o64)
            assert (err <= tol).all(), f"bf16 gemm {M}x{K}x{N} mat {t} tr={tr} vs the f32 restatement: worst err/tol {(err / tol).max():.3g}"


# ---- 2 -------------------------------------------------------------------------------------------------------------------------------------------
F16_ROWS = [r for r in LEAVES + EXTRA_LEAVES if r.dtype == F16]
ROW_CASES = [pytest.param(r, tr, id=f"{r.name}-{'tr' if tr else 'nn'}") for r in F16_ROWS for tr in r.variants]


def _small_ints(rng, M, K, N, Z):
    """Integer operands whose every partial sum stays below 2^8 in magnitude: at most 8 nonzeros (|a| <= 3) per row of op(A), |b| <= 3: |sum| <= 72. Any order
    and any split of K give the same exact f32 sum, and the result is a bf16 value."""
    A = np.zeros((M, K, Z))
    for z in range(Z):
        cols = rng.integers(0, K, (M, 8))
        A[np.arange(M)[:, None], cols, z] = rng.integers(-3, 4, (M, 8))
    return A, rng.integers(-3, 4, (K, N, Z)).astype(np.float64)


def _bf_dtype_leaf(tags):
    return tuple(t.replace("f16.", "bf16.") for t in ((tags,) if isinstance(tags, str) else tags))


@pytest.mark.parametrize("row,tr", ROW_CASES)
def test_gemm_bf16_exact_and_special(gpu, knobs, row, tr):
    M, K, N, Z = row.M, row.K, row.N, row.mats
    knobs(row.knobs)
    rng = np.random.default_rng(M * 7 + K * 5 + N * 3 + Z + int(tr))
    A, Bv = _small_ints(rng, M, K, N, Z)
    want = np.stack([A[:, :, z] @ Bv[:, :, z] for z in range(Z)], -1)
    assert np.abs(want).max() < 256 and np.array_equal(B.from_bits(B.to_bits(want)), want.astype(np.float32))
    a, b = Mat(gpu, stored_a(B.to_bits(A), tr)), Mat(gpu, B.to_bits(Bv))
    out = Mat(gpu, np.full((M, N, Z), 0x7FC0, np.uint16))
    gpu.take_path()
    gemm(gpu, tr, out, a, b)
    log = gpu.take_path()
    assert Row.took(_bf_dtype_leaf(row.leaf), log), f"{row.name}: expected {_bf_dtype_leaf(row.leaf)!r}, took {log!r}"
    got = B.from_bits(out.read("exact"))
    U.assert_same_class_bits(got, want.astype(np.float32), f"{row.name} exact [{log}]")  # (zeros as one class: the sign of an exact zero sum is open)
    # +-Inf and NaN operands: a few k carry them (tests/_util.special_product: the finite part exactly, the others as IEEE outer products)
    As, Bs = A.copy(), Bv.copy()
    ks = rng.choice(K, 3, replace=False)
    As[rng.integers(0, M), ks[0], :] = np.inf
    As[rng.integers(0, M), ks[1], :] = -np.inf
    Bs[ks[2], rng.integers(0, N), :] = np.nan
    Bs[ks[0], :, :] = np.where(Bs[ks[0], :, :] == 0, 1.0, Bs[ks[0], :, :])  # (no Inf * 0 on that row: keeps finite outputs beside the others)
    want_s = B.from_bits(B.to_bits(U.special_product(As, Bs, np.float64)))
    assert np.isfinite(want_s).any() and not np.isfinite(want_s).all()
    a, b = Mat(gpu, stored_a(B.to_bits(As), tr)), Mat(gpu, B.to_bits(Bs))
    out = Mat(gpu, np.full((M, N, Z), 0x7FC0, np.uint16))
    gemm(gpu, tr, out, a, b)
    U.assert_same_class_bits(B.from_bits(out.read("special")), want_s, f"{row.name} special [{gpu.take_path()}]")


# ---- 3 -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr", [False, True])
@pytest.mark.parametrize("M,K,tile", [(64, 8, 0), (256, 64, 128), (512, 256, 256)])  # the generic kernel; the 128 x 128 kernel; the 256 x 256 kernel
def test_gemm_ex_rounds_once_to_nearest_even(gpu, knobs, M, K, tile, tr):
    """acc[i, j] = x_i y_j exactly (one nonzero k; a product of two bf16 values is exact in f32). Row i's value lands on the bf16 tie 1 + (2 i + 1) 2^-8, one f32 ulp
    below it and one above, through alpha alone (beta = 0 over a NaN prefill: one tie for every element), through beta c (alpha acc = 1: a tie per row) and through both; expected bits:
    to_bf16(fmaf_f32(beta, c, fl32(alpha acc))). Truncation, round-half-up and a second rounding in between each fail some of these."""
    knobs({"f16_tile": tile})
    N = M
    A, Bv = np.zeros((M, K, 1)), np.zeros((K, N, 1))
    A[:, K // 2, 0] = 1.0
    Bv[K // 2, :, 0] = 1.0
    A[0, K // 2, 0], Bv[K // 2, 0, 0] = 2.0 ** 64 * 1.5, 2.0 ** 63  # acc[0, 0] = 1.5 2^127 (finite in f32); row 0 / column 0 otherwise 2^64 1.5 and 2^63
    a, b = Mat(gpu, stored_a(B.to_bits(A), tr)), Mat(gpu, B.to_bits(Bv))
    acc = (A[:, :, 0] @ Bv[:, :, 0]).astype(np.float32)
    i = np.arange(M) % 64
    tie = (1.0 + (2.0 * i + 1.0) * 2.0 ** -8).astype(np.float32)  # exactly halfway between two bf16 values
    c = B.to_bits(((2.0 * i + 1.0) * 2.0 ** -8).astype(np.float32))  # bf16 values (odd integers below 128, scaled): 1 + c is row i's tie
    c0 = np.repeat(c[:, None], N, 1)[:, :, None]
    for name, step in (("tie", 0), ("below", -1), ("above", +1)):
        al = tie if step == 0 else np.nextafter(tie, np.float32(0 if step < 0 else 4))  # (alpha is one scalar per call: the ties of rows 3 and 5)
        for al_s, be_s in ((1.0, 1.0), (float(al[3]), 0.0), (float(al[5]), 0.5), (-0.75, 2.0)):
            out = Mat(gpu, c0.copy() if be_s != 0.0 else np.full((M, N, 1), 0x7FC0, np.uint16))
            gemm(gpu, tr, out, a, b, al_s, be_s)
            with np.errstate(over="ignore"):
                v = (np.float32(al_s) * acc).astype(np.float32)
                want = B.to_bits(U.fmaf_f32(np.float32(be_s), B.from_bits(c0[:, :, 0]), v) if be_s != 0.0 else v)
            got = out.read(name)[:, :, 0]
            bad = got != want
            assert not bad.any(), f"{name} gemm_ex({al_s}, {be_s}) [{gpu.take_path()}]: {bad.sum()} elements differ, first {np.argwhere(bad)[0]}: got {got[bad][0]:#06x}, want {want[bad][0]:#06x}"
    # (1, 1) above put every row on its tie: RNE must have gone to the even neighbour there -- the expected bits say so themselves
    want11 = B.to_bits(U.fmaf_f32(np.float32(1), B.from_bits(c0[:, :, 0]), acc))
    k = i[1:]
    assert np.array_equal(want11[1:, 1], (0x3F80 + k + (k & 1)).astype(np.uint16))
    # an f32 value above the largest bf16, still finite in f32: Inf
    out = Mat(gpu, np.full((M, N, 1), 0x7FC0, np.uint16))
    gemm(gpu, tr, out, a, b, 1.332, 0.0)
    v00 = np.float32(1.332) * acc[0, 0]
    assert np.isfinite(v00) and B.to_bits(v00) == 0x7F80
    assert out.read("overflow")[0, 0, 0] == 0x7F80
    # (1, 0) is wg_gemm, bit for bit; beta == 0 never reads the NaN prefill
    o1, o2 = Mat(gpu, np.full((M, N, 1), 0x7FC0, np.uint16)), Mat(gpu, np.full((M, N, 1), 0xFFFF, np.uint16))
    gemm(gpu, tr, o1, a, b)
    gemm(gpu, tr, o2, a, b, 1.0, 0.0)
    assert np.array_equal(o1.read(), o2.read()) and np.array_equal(o1.read()[:, :, 0], B.to_bits(acc))


# ---- 4 -------------------------------------------------------------------------------------------------------------------------------------------
def _both_logs(gpu, call):
    """The launch logs of `call(dt_name)` for f16 and for bf16."""
    logs = {}
    for dt in ("f16", "bf16"):
        gpu.take_path()
        call(dt)
        logs[dt] = gpu.take_path()
    return logs


def _rand16(rng, shape, dt):
    x = rng.random(shape, dtype=np.float32) * 2 - 1
    return B.to_bits(x) if dt == "bf16" else x.astype(F16).view(np.uint16)


@pytest.mark.parametrize("row,tr", ROW_CASES + [pytest.param(r, True, id=r.name) for r in RM_LEAVES if r.dtype == F16])
def test_same_tree_as_f16_gemm(gpu, knobs, row, tr):
    L = _L()
    M, K, N, Z = row.M, row.K, row.N, row.mats
    knobs(row.knobs)
    rm = getattr(row, "api", "cm") == "rm"

    def call(dt, ab=None):
        rng = np.random.default_rng(1)
        if rm:  # row-major GemmTr: m1 is K x M row-major = column-major M x K; m2 K x N row-major = column-major N x K; out M x N row-major = N x M
            a, b = Mat(gpu, _rand16(rng, (M, K, Z), dt), dt=dt), Mat(gpu, _rand16(rng, (N, K, Z), dt), dt=dt)
            out = Mat(gpu, np.full((N, M, Z), 0x7E00, np.uint16), dt=dt)
            wg = _wg()
            for m_, (r_, c_) in ((a, (K, M)), (b, (K, N)), (out, (M, N))):
                m_.shape = wg.ViewShape((r_, c_, Z), m_.shape.stride, m_.shape.stride_mat, 0)
            gemm(gpu, True, out, a, b, rm=True, dt=L.WG_BF16 if dt == "bf16" else L.WG_F16)
            return
        a, b = Mat(gpu, _rand16(rng, (K, M, Z) if tr else (M, K, Z), dt), dt=dt), Mat(gpu, _rand16(rng, (K, N, Z), dt), dt=dt)
        out = Mat(gpu, _rand16(rng, (M, N, Z), dt), dt=dt)
        gemm(gpu, tr, out, a, b, *(ab or (None, None)), dt=L.WG_BF16 if dt == "bf16" else L.WG_F16)

    logs = _both_logs(gpu, call)
    assert Row.took(row.leaf, logs["f16"]), (row.name, logs)
    assert logs["bf16"] == logs["f16"].replace("f16.", "bf16."), logs
    if not rm:
        logs = _both_logs(gpu, lambda dt: call(dt, (0.5, -2.0)))
        assert logs["bf16"] == logs["f16"].replace("f16.", "bf16."), logs


F16_GROWS = [r for r in GEMV_LEAVES if r.dtype == F16]


def _gemv_c(gpu, tr, dt, out, m, v, rm=False):
    wg, L = _wg(), _L()
    fn = L.lib.wg_gemv_rm if rm else L.lib.wg_gemv
    L.check(fn(gpu._ctx.handle, int(wg.GemvVariant.GemvTr if tr else wg.GemvVariant.Gemv), L.WG_BF16 if dt == "bf16" else L.WG_F16, out.buf._h, out.shape.to_c(),
               m.buf._h, m.shape.to_c(), v.buf._h, v.shape.to_c()))


@pytest.mark.parametrize("row", F16_GROWS, ids=[r.name for r in F16_GROWS])
def test_same_tree_as_f16_gemv_leaves(gpu, knobs, row):
    knobs(row.knobs)
    ro, k = (row.C, row.R) if row.tr else (row.R, row.C)

    def call(dt):
        rng = np.random.default_rng(2)
        pad = (-row.R) % row.ld_mult
        m = Mat(gpu, _rand16(rng, (row.R, row.C, row.mats), dt), pad=pad, dt=dt)
        vo = dict(off=1, pad=1, gap=3) if row.vodd else {}
        v, out = Mat(gpu, _rand16(rng, (k, row.nrhs, row.mats), dt), dt=dt, **vo), Mat(gpu, np.full((ro, row.nrhs, row.mats), 0x7E00, np.uint16), dt=dt, **vo)
        _gemv_c(gpu, row.tr, dt, out, m, v)

    logs = _both_logs(gpu, call)
    assert Row.took(row.leaf, logs["f16"], row.not_), (row.name, logs)
    assert logs["bf16"] == logs["f16"].replace("f16.", "bf16."), logs


@pytest.mark.parametrize("tr", [False, True])
@pytest.mark.parametrize("nrhs", [1, 3, 8, 16])
@pytest.mark.parametrize("off", [0, 1])
def test_same_tree_as_f16_gemv_and_reduce(gpu, tr, nrhs, off):
    wg, L = _wg(), _L()
    R, C = 1024, 2048
    ro, k = (C, R) if tr else (R, C)

    def call(dt):
        rng = np.random.default_rng(3)
        m = Mat(gpu, _rand16(rng, (R, C, 1), dt), off=off, dt=dt)
        v, out = Mat(gpu, _rand16(rng, (k, nrhs, 1), dt), dt=dt), Mat(gpu, np.full((ro, nrhs, 1), 0x7E00, np.uint16), dt=dt)
        _gemv_c(gpu, tr, dt, out, m, v)
        res = Mat(gpu, np.full((nrhs, 1, 1), 0x7E00, np.uint16), dt=dt)
        code = L.WG_BF16 if dt == "bf16" else L.WG_F16
        for op in (wg.ReduceOp.Sum, wg.ReduceOp.Max):  # one vector, a batch, the two-pass form
            vec = wg.ViewShape((ro, 1, 1), ro, ro, 0)
            L.check(L.lib.wg_reduce(gpu._ctx.handle, int(op), code, out.buf._h, vec.to_c(), res.buf._h))
            L.check(L.lib.wg_reduce_batched(gpu._ctx.handle, int(op), code, out.buf._h, out.shape.to_c(), res.buf._h))
            L.check(L.lib.wg_reduce_fast(gpu._ctx.handle, int(op), code, m.buf._h, wg.ViewShape((R * C, 1, 1), 1, 1, off).to_c(), res.buf._h))

    logs = _both_logs(gpu, call)
    assert "reduce." in logs["f16"] and ("gemv" in logs["f16"])
    assert logs["bf16"] == logs["f16"].replace("f16.", "bf16."), logs


# ---- 5 -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr", [False, True])
@pytest.mark.parametrize("M,K,N,mats", [(8192, 256, 8192, 1), (4352 + 248, 256, 4096 + 129, 1), (2048, 512, 2048, 5)])  # whole rounds; ragged; a batch
def test_continuous_walk_is_bit_identical(gpu, knobs, M, K, N, mats, tr):
    rng = np.random.default_rng(M + K + N)
    A, Bm = rnd_bits(rng, (M, K, mats)), rnd_bits(rng, (K, N, mats))
    a, b = Mat(gpu, stored_a(A, tr)), Mat(gpu, Bm)
    res, logs = {}, {}
    for cont in (0, 1, -1):
        knobs({"f16_tile": 256})  # (the 256 x 128 pairs would take the shortest K otherwise)
        old = gpu.set_tuning("f16_cont", cont)
        try:
            out = Mat(gpu, np.full((M, N, mats), 0x7FC0, np.uint16))
            gpu.take_path()
            gemm(gpu, tr, out, a, b)
            logs[cont] = gpu.take_path()
            res[cont] = out.read(f"cont={cont}")
        finally:
            gpu.set_tuning("f16_cont", old)
    assert "bf16.cont" in logs[1] and "bf16.cont" not in logs[0] and "bf16.m16" in logs[0], logs
    assert not np.isnan(B.from_bits(res[0])).any()
    assert np.array_equal(res[1], res[0]), f"the continuous walk differs from the per-tile launch in {(res[1] != res[0]).sum()} elements"
    assert np.array_equal(res[-1], res[0])
    z = mats - 1
    rows, cols = rng.integers(0, M, 48), rng.integers(0, N, 48)
    a64, b64 = B.from_bits(A[rows, :, z]).astype(np.float64), B.from_bits(Bm[:, cols, z]).astype(np.float64)
    truth, sabs = a64 @ b64, np.abs(a64) @ np.abs(b64)
    err = np.abs(B.from_bits(res[1][np.ix_(rows, cols, [z])][:, :, 0]).astype(np.float64) - truth)
    assert (err <= U.f32_gate(K, sabs) + 2.0 ** -8 * np.abs(truth) + TINY).all()


# ---- 6 -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr", [False, True])
@pytest.mark.parametrize("M,K,N,mats", [(512, 256, 512, 1), (264, 96, 520, 2), (264, 192, 520, 2), (1028, 512, 1028, 1), (1024, 1028, 1024, 1), (61, 30, 19, 1), (516, 260, 127, 2),
                                        (512, 320, 3, 1)])
def test_gemm_bf16_views(gpu, M, K, N, mats, tr):
    """Odd offsets and leading dimensions with a gap between matrices on all three views; M % 8 != 0 and K % 8 != 0 (the padded and staged paths); N odd. The
    result is the dense call's, bit for bit, wherever the same kernels ran (the launch log says), and nothing is written outside the output view."""
    rng = np.random.default_rng(M + 3 * K + 5 * N + int(tr))
    A, Bm = rnd_bits(rng, (M, K, mats)), rnd_bits(rng, (K, N, mats))
    c0 = rnd_bits(rng, (M, N, mats))
    got = {}
    for layout, kw in (("dense", {}), ("odd", dict(off=1, pad=3, gap=7)), ("odd2", dict(off=3, pad=1, gap=1))):
        a, b = Mat(gpu, stored_a(A, tr), **kw), Mat(gpu, Bm, **kw)
        out = Mat(gpu, np.full((M, N, mats), 0x7FC0, np.uint16), **kw)
        gpu.take_path()
        gemm(gpu, tr, out, a, b)
        o2 = Mat(gpu, c0, **kw)
        gemm(gpu, tr, o2, a, b, -1.5, 0.25)
        # the kernels that did the arithmetic: the log without its wrappers (staging, padding: copies)
        leaves = [t.split(">")[-1] for t in gpu.take_path().split()]
        got[layout] = (out.read(layout), o2.read(layout + " ex"), leaves)
    product_check(got["dense"][0], A, Bm, K, f"bf16 views {M}x{K}x{N} tr={tr}")
    for layout in ("odd", "odd2"):
        if got[layout][2] == got["dense"][2]:  # the same kernels on copies or in place: the same bits
            assert np.array_equal(got[layout][0], got["dense"][0]), f"{layout}: differs from the dense call {got[layout][2]}"
            assert np.array_equal(got[layout][1], got["dense"][1]), f"{layout}: gemm_ex differs from the dense call {got[layout][2]}"
        else:  # (a small product whose odd views go to another kernel -- another summation order: the contract's bound)
            product_check(got[layout][0], A, Bm, K, f"bf16 views {M}x{K}x{N} tr={tr} {layout} {got[layout][2]}")
    # gemm_ex against f64: |alpha| gate + half an ulp of the result's magnitude bound
    g = B.from_bits(got["dense"][1]).astype(np.float64)
    for z in range(mats):
        a64, b64 = B.from_bits(A[:, :, z]).astype(np.float64), B.from_bits(Bm[:, :, z]).astype(np.float64)
        cz = B.from_bits(c0[:, :, z]).astype(np.float64)
        truth = -1.5 * (a64 @ b64) + 0.25 * cz
        tol = 1.5 * U.f32_gate(K, np.abs(a64) @ np.abs(b64)) + 2.0 ** -8 * np.abs(truth) + 2.0 ** -24 * (np.abs(1.5 * (a64 @ b64)) + np.abs(0.25 * cz)) + TINY
        assert (np.abs(g[:, :, z] - truth) <= tol).all()


@pytest.mark.parametrize("tr", [False, True])
@pytest.mark.parametrize("M,K,N,mats,tile", [(512, 256, 512, 1, 256), (384, 320, 264, 2, 128), (512, 256, 384, 1, 256128), (100, 52, 36, 1, 0)])
def test_gemm_rm_native_equals_copy(gpu, knobs, M, K, N, mats, tile, tr):
    """wg_gemm_rm, both variants: row-major views; GemmTr with WG_TUNE_RM_TR_NATIVE 0 (transpose + Gemm) and 1 (m1 where it lies) gives equal bits."""
    wg = _wg()
    rng = np.random.default_rng(M + K + N + int(tr))
    A, Bm = rnd_bits(rng, (M, K, mats)), rnd_bits(rng, (K, N, mats))
    # row-major X (R x C) is the memory of the column-major X^T (C x R)
    m1 = A if tr else np.transpose(A, (1, 0, 2))  # GemmTr: m1 is K x M row-major = cm M x K; Gemm: m1 M x K row-major = cm K x M
    a, b = Mat(gpu, m1), Mat(gpu, np.transpose(Bm, (1, 0, 2)))
    a.shape = wg.ViewShape(((K, M) if tr else (M, K)) + (mats,), a.shape.stride, a.shape.stride_mat, 0)
    b.shape = wg.ViewShape((K, N, mats), b.shape.stride, b.shape.stride_mat, 0)
    res = {}
    for native in (0, 1):
        knobs({"f16_tile": tile, "rm_tr_native": native})
        out = Mat(gpu, np.full((N, M, mats), 0x7FC0, np.uint16))
        out.shape = wg.ViewShape((M, N, mats), out.shape.stride, out.shape.stride_mat, 0)
        gpu.take_path()
        gemm(gpu, tr, out, a, b, rm=True)
        res[native] = (np.transpose(out.read(), (1, 0, 2)), gpu.take_path())
    if tr and tile:
        assert "transpose" in res[0][1] and "transpose" not in res[1][1] and "bf16." in res[1][1], (res[0][1], res[1][1])
    assert np.array_equal(res[0][0], res[1][0]), (res[0][1], res[1][1])
    product_check(res[1][0], A, Bm, K, f"bf16 gemm_rm {M}x{K}x{N} tr={tr}")


# ---- 7 -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr", [False, True])
@pytest.mark.parametrize("R,C,mats,kw", [(1024, 512, 1, {}), (4096, 4096, 1, {}), (2052, 4096, 2, {}), (64, 4096, 1, {}), (130, 69, 1, {}), (67, 130, 2, {}),
                                         (1024, 2048, 1, dict(off=1, pad=3, gap=5))])
def test_gemv_bf16(gpu, R, C, mats, kw, tr):
    """Gemv / GemvTr and the row-major forms, on aligned views (the tuned kernels), lengths that are not multiples of 4 and an odd offset / leading dimension (the
    any-alignment kernels): against f64 with f32_gate + 2^-8 |truth|, one right-hand side at a time and 3 and 8 at once (the same bits on a second run)."""
    wg = _wg()
    rng = np.random.default_rng(R + 2 * C + int(tr))
    ro, k = (C, R) if tr else (R, C)
    Mb, Vb = rnd_bits(rng, (R, C, mats)), rnd_bits(rng, (k, 8, mats))
    m = Mat(gpu, Mb, **kw)
    single = []
    for j in range(8):
        v, out = Mat(gpu, Vb[:, j:j + 1, :]), Mat(gpu, np.full((ro, 1, mats), 0x7FC0, np.uint16))
        _gemv_c(gpu, tr, "bf16", out, m, v)
        single.append(out.read("gemv")[:, 0, :])
    single = np.stack(single, 1)
    for z in range(mats):
        m64 = B.from_bits(Mb[:, :, z]).astype(np.float64)
        m64 = m64.T if tr else m64
        v64 = B.from_bits(Vb[:, :, z]).astype(np.float64)
        truth, sabs = m64 @ v64, np.abs(m64) @ np.abs(v64)
        err = np.abs(B.from_bits(single[:, :, z]).astype(np.float64) - truth)
        tol = U.f32_gate(k, sabs) + 2.0 ** -8 * np.abs(truth) + TINY
        assert (err <= tol).all(), f"bf16 gemv {R}x{C} tr={tr} mat {z}: worst err/tol {(err / tol).max():.3g}"
    for nrhs in (3, 8):
        v, out = Mat(gpu, Vb[:, :nrhs, :]), Mat(gpu, np.full((ro, nrhs, mats), 0x7FC0, np.uint16))
        gpu.take_path()
        _gemv_c(gpu, tr, "bf16", out, m, v)
        log = gpu.take_path()
        got = out.read("gemv multi")
        assert "bf16." in log or "gemv_any" in log, log
        for z in range(mats):  # (another register tile or a hand-off to the Gemm kernels: another order, the contract's bound. The f16 / f32 tests assert no bit equality between the multi-RHS and the single-RHS form either: tests/test_gpu_fullsize.py's 8-RHS case and test_gemv_f16 hold each column to the f64 bound, and test_gpu_operands.py::test_gemv_leaf_operands asserts the same bits on a second run of the same launch -- both asserted here)
            m64 = B.from_bits(Mb[:, :, z]).astype(np.float64)
            m64 = m64.T if tr else m64
            v64 = B.from_bits(Vb[:, :nrhs, z]).astype(np.float64)
            truth = m64 @ v64
            assert (np.abs(B.from_bits(got[:, :, z]).astype(np.float64) - truth) <= U.f32_gate(k, np.abs(m64) @ np.abs(v64)) + 2.0 ** -8 * np.abs(truth) + TINY).all(), log
        _gemv_c(gpu, tr, "bf16", out, m, v)  # ... and deterministic: the same bits on a second run
        assert np.array_equal(out.read("gemv multi, second run"), got)
    # row-major: out = op(m) v with m row-major = the column-major call of the other variant on the same memory
    if not kw:
        v, o_rm, o_cm = Mat(gpu, Vb[:, :1, :]), Mat(gpu, np.full((ro, 1, mats), 0x7FC0, np.uint16)), Mat(gpu, np.full((ro, 1, mats), 0x7FC0, np.uint16))
        m_rm = Mat(gpu, np.transpose(Mb, (1, 0, 2)))  # the R x C matrix stored row-major
        m_rm.shape = wg.ViewShape((R, C, mats), m_rm.shape.stride, m_rm.shape.stride_mat, 0)
        _gemv_c(gpu, tr, "bf16", o_rm, m_rm, v, rm=True)
        got = B.from_bits(o_rm.read("gemv_rm")[:, 0, :]).astype(np.float64)
        for z in range(mats):
            m64 = B.from_bits(Mb[:, :, z]).astype(np.float64)
            m64 = m64.T if tr else m64
            v64 = B.from_bits(Vb[:, 0, z]).astype(np.float64)
            truth = m64 @ v64
            assert (np.abs(got[:, z] - truth) <= U.f32_gate(k, np.abs(m64) @ np.abs(v64)) + 2.0 ** -8 * np.abs(truth) + TINY).all()


# ---- 8 -------------------------------------------------------------------------------------------------------------------------------------------
REDUCE_N = [0, 1, 127, 128, 129, 345, 65536]


@pytest.mark.parametrize("n", REDUCE_N)
@pytest.mark.parametrize("off", [0, 3])
def test_reduce_bf16(gpu, oracle_c, n, off):
    """Min, Max, Sum, Prod: the bits of the f32 restatement (reference order) on the widened operands, rounded once with the helper; SqNorm: the f16 test's rule --
    the same bits too (the restatement rounds x * x separately, as the kernel does). One vector, a batch of three, and the two-pass form (Min / Max: the same bits;
    Sum / SqNorm: within n 2^-24 sum|x| + half a bf16 ulp of the f64 value; Prod: within (n 2^-24 + 2^-8) |product|). n = 0: the op's initial value, rounded to bf16."""
    wg = _wg()
    from oracle import wgsl_oracle as wo
    dev, shapes = gpu.device(), wg.ViewShapeBuffers()
    rng = np.random.default_rng(n + off)
    cols = 3
    x = rnd_bits(rng, (max(n, 1) * cols,))
    if n:
        x[rng.integers(0, n * cols, 4)] = B.to_bits(np.array([1.5, -1.75, 1.25, -1.0], np.float32))
    flat = np.concatenate([np.full(off, 0x7FC0, np.uint16), x, np.full(5, 0x7FC0, np.uint16)])
    t = up_bits(gpu, flat)
    x32 = B.from_bits(x)
    for op, wop in ((wg.ReduceOp.Min, wo.MIN), (wg.ReduceOp.Max, wo.MAX), (wg.ReduceOp.Sum, wo.SUM), (wg.ReduceOp.Prod, wo.PROD), (wg.ReduceOp.SqNorm, wo.SQNORM)):
        xs = x32 if op != wg.ReduceOp.Prod else None
        tt = t
        if op == wg.ReduceOp.Prod:  # magnitudes near 1, so that the product of n of them stays finite and nonzero
            xp = B.to_bits(np.where(rng.random(x.size) < 0.5, -1.0, 1.0) * (1.0 + rng.integers(-2, 3, x.size) * 2.0 ** -7))
            tt, xs = up_bits(gpu, np.concatenate([np.full(off, 0x7FC0, np.uint16), xp, np.full(5, 0x7FC0, np.uint16)])), B.from_bits(xp)
        with np.errstate(over="ignore", invalid="ignore"):
            ref32 = np.array([oracle_c.reduce(int(wop), xs, wo.Shape(n, 1, 1, max(n, 1), max(n, 1), c * n)) for c in range(cols)], np.float32)
        want = B.to_bits(ref32)
        red = wg.Reduce.new(dev, op)
        res1, res3, resf = up_bits(gpu, [0x7FC0]), up_bits(gpu, [0x7FC0] * cols), up_bits(gpu, [0x7FC0])
        v1 = wg.GpuTensorView(wg.ViewShape((n, 1, 1), max(n, 1), max(n, 1), off), tt, 1)
        v3 = wg.GpuTensorView(wg.ViewShape((n, cols, 1), n, n * cols, off), tt, 2)
        run(gpu, lambda p: (red.dispatch(dev, shapes, p, v1, res1), red.dispatch_batched(dev, shapes, p, v3, res3), red.dispatch_fast(dev, shapes, p, v1, resf)))
        g1, g3, gf = rd_bits(gpu, res1), rd_bits(gpu, res3), rd_bits(gpu, resf)
        what = f"n={n} off={off} {op.name}"
        U.assert_same_class_bits(B.from_bits(g1), B.from_bits(want[:1]), what)
        U.assert_same_class_bits(B.from_bits(g3), B.from_bits(want), what + " batched")
        if op in (wg.ReduceOp.Min, wg.ReduceOp.Max) or n <= 1:
            U.assert_same_class_bits(B.from_bits(gf), B.from_bits(want[:1]), what + " fast")
        elif op == wg.ReduceOp.Prod:  # re-associated: n roundings of relative 2^-24 each, whatever the order, + half a bf16 ulp
            exact = float(np.prod(xs[:n].astype(np.float64)))
            assert np.isfinite(exact) and exact != 0.0
            assert abs(float(B.from_bits(gf)[0]) - exact) <= (1.01 * n * 2.0 ** -24 + 2.0 ** -8) * abs(exact) + TINY, what + " fast"
        else:
            sabs = float(np.abs(xs[:n].astype(np.float64) ** (2 if op == wg.ReduceOp.SqNorm else 1)).sum())
            exact = float((xs[:n].astype(np.float64) ** (2 if op == wg.ReduceOp.SqNorm else 1)).sum())
            assert abs(float(B.from_bits(gf)[0]) - exact) <= n * 2.0 ** -24 * sabs + 2.0 ** -8 * abs(exact) + TINY, what + " fast"


@pytest.mark.parametrize("R,C", [(512, 256), (8192, 1024)])
def test_gemv_reduce_bf16(gpu, R, C):
    """wg_gemv_reduce is wg_gemv followed by wg_reduce, bit for bit."""
    wg, L = _wg(), _L()
    rng = np.random.default_rng(R + C)
    m, v = Mat(gpu, rnd_bits(rng, (R, C, 1))), Mat(gpu, rnd_bits(rng, (C, 1, 1)))
    y = Mat(gpu, np.full((R, 1, 1), 0x7FC0, np.uint16))
    _gemv_c(gpu, False, "bf16", y, m, v)
    for op in (wg.ReduceOp.Min, wg.ReduceOp.Max, wg.ReduceOp.Sum, wg.ReduceOp.SqNorm):
        r1, r2 = up_bits(gpu, [0x7FC0]), up_bits(gpu, [0x7FC0])
        L.check(L.lib.wg_reduce(gpu._ctx.handle, int(op), L.WG_BF16, y.buf._h, y.shape.to_c(), r1._h))
        gpu.take_path()
        L.check(L.lib.wg_gemv_reduce(gpu._ctx.handle, int(wg.GemvVariant.Gemv), int(op), L.WG_BF16, r2._h, m.buf._h, m.shape.to_c(), v.buf._h, v.shape.to_c()))
        assert "gemv_reduce.two>" in gpu.take_path()
        a, b = rd_bits(gpu, r1), rd_bits(gpu, r2)
        assert a[0] == b[0] and not np.isnan(B.from_bits(a)[0]), (op, a, b)


# ---- 9 -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1757, (1 << 20) + 3])
@pytest.mark.parametrize("offa,offb", [(0, 0), (1, 1), (3, 6)])
def test_op_assign_bf16(gpu, n, offa, offb):
    """Add, Sub, Mul, Div, Copy and Axpy: f32 arithmetic on the widened operands, rounded once -- bit for bit; alpha = +-1 are Add / Sub; nothing around the views moves."""
    wg = _wg()
    dev, shapes = gpu.device(), wg.ViewShapeBuffers()
    rng = np.random.default_rng(n + offa)
    xa, xb = rnd_bits(rng, (n,)), B.to_bits((rng.random(n, dtype=np.float32) + 0.5) * np.where(rng.random(n) < 0.5, -1, 1).astype(np.float32))
    xa[:4], xb[:4] = [0x7F80, 0xFF80, 0x7FC0, 0x0001], [0x3F80, 0x3F80, 0x3F80, 0x0001]  # Inf, -Inf, NaN, the smallest subnormal
    fa, fb = B.from_bits(xa), B.from_bits(xb)
    pad = lambda x, off: np.concatenate([np.full(off, 0x7FC5, np.uint16), x, np.full(11, 0x7FC5, np.uint16)])
    tb = up_bits(gpu, pad(xb, offb))
    vb = wg.GpuTensorView(wg.ViewShape((n, 1, 1), n, n, offb), tb, 1)
    V = wg.OpAssignVariant
    with np.errstate(all="ignore"):
        cases = [(V.Add, fa + fb), (V.Sub, fa - fb), (V.Mul, fa * fb), (V.Div, fa / fb), (V.Copy, fb)]
        axpy = {al: U.fmaf_f32(np.float32(al), fb, fa) for al in (1.0, -1.0, 0.3, -2.5)}
    results = {}

    def one(name, fn, want32):
        ta = up_bits(gpu, pad(xa, offa))
        va = wg.GpuTensorView(wg.ViewShape((n, 1, 1), n, n, offa), ta, 1)
        run(gpu, lambda p: fn(p, va))
        got = rd_bits(gpu, ta)
        assert (got[:offa] == 0x7FC5).all() and (got[offa + n:] == 0x7FC5).all(), f"{name}: wrote outside the view"
        results[name] = got[offa:offa + n]
        U.assert_same_class_bits(B.from_bits(results[name]), B.from_bits(B.to_bits(want32.astype(np.float32))), f"{name} n={n} offsets ({offa}, {offb})")

    for var, want in cases:
        one(var.name, lambda p, va, var=var: wg.OpAssign.new(dev, var).dispatch(dev, shapes, p, va, vb), want)
    for al, want in axpy.items():
        one(f"axpy{al}", lambda p, va, al=al: wg.Axpy.from_device(dev).dispatch(dev, shapes, p, al, va, vb), want)
    assert np.array_equal(results["axpy1.0"], results["Add"]) and np.array_equal(results["axpy-1.0"], results["Sub"])
    assert np.array_equal(results["Copy"], xb)  # (a copy moves the bits: the subnormal and the NaN payload included)


# ---- 10 ------------------------------------------------------------------------------------------------------------------------------------------
def test_copies_move_bits(gpu):
    wg, L = _wg(), _L()
    rng = np.random.default_rng(10)
    R, C, Z = 67, 29, 3
    src_bits = rng.integers(0, 1 << 16, (R, C, Z)).astype(np.uint16)  # every kind of pattern: NaN payloads, subnormals, Inf
    src_bits[:3, 0, 0] = [0x7FA5, 0xFFC1, 0x0001]
    for kw_s, kw_d in ((dict(off=1, pad=3, gap=5), {}), ({}, dict(off=3, pad=1, gap=2)), (dict(off=2, pad=2, gap=2), dict(off=5, pad=4, gap=9))):
        src, dst = Mat(gpu, src_bits, **kw_s), Mat(gpu, np.full((R, C, Z), 0x7FC0, np.uint16), **kw_d)
        L.check(L.lib.wg_copy_view(gpu._ctx.handle, L.WG_BF16, dst.buf._h, dst.shape.to_c(), src.buf._h, src.shape.to_c()))
        assert np.array_equal(dst.read("copy_view"), src_bits)
    # a larger destination: zero fill past the source
    src, dst = Mat(gpu, src_bits), Mat(gpu, np.full((R + 5, C + 2, Z), 0x7FC0, np.uint16), off=1)
    L.check(L.lib.wg_copy_view(gpu._ctx.handle, L.WG_BF16, dst.buf._h, dst.shape.to_c(), src.buf._h, src.shape.to_c()))
    d = dst.read("copy_view zero fill")
    assert np.array_equal(d[:R, :C], src_bits) and not d[R:].any() and not d[:, C:].any()
    # cube [mg, np, P] -> matrix (P mg x np): out[g mg + i, j] = cube[i, j, g]
    mg, np_, P = 24, 17, 4
    cube_bits = rng.integers(0, 1 << 16, (mg, np_, P)).astype(np.uint16)
    cube, out = Mat(gpu, cube_bits), Mat(gpu, np.full((mg * P, np_, 1), 0x7FC0, np.uint16))
    L.check(L.lib.wg_cube_to_matrix(gpu._ctx.handle, L.WG_BF16, cube.buf._h, cube.shape.to_c(), out.buf._h, out.shape.to_c()))
    want = np.concatenate([cube_bits[:, :, g] for g in range(P)], 0)
    assert np.array_equal(out.read("cube_to_matrix")[:, :, 0], want)


# ---- 11 ------------------------------------------------------------------------------------------------------------------------------------------
REPLAY = [("t128", 512, 512, 512, {"f16_tile": 128}), ("t256x128", 1024, 512, 1024, {"f16_tile": 256128}), ("m16", 4096, 512, 4096, {"f16_tile": 256, "f16_cont": 0}),
          ("cont", 4096, 256, 8192, {"f16_tile": 256, "f16_cont": 1}), ("splitk", 512, 4096, 512, {"f16_tile": 128}), ("generic", 72, 36, 40, {})]


@pytest.mark.parametrize("where", ["whole", "cu248"])
def test_recorded_and_masked(gpu, where):
    """One Gemm per kernel family and one Gemv, eager, then recorded once and replayed twice into a re-poisoned output: the eager bits each time. On the whole chip and on a
    CU-masked context (248 CUs, the missing ones from one XCD), whose eager bits equal the whole chip's where the leaf is the same."""
    wg, L = _wg(), _L()
    inst = gpu if where == "whole" else wg.GpuInstance.new(0, cu_count=248, one_xcd=True)
    try:
        for name, M, K, N, kn in REPLAY:
            saved = {k: inst.set_tuning(k, v) for k, v in kn.items()}
            try:
                rng = np.random.default_rng(M + K + N)
                A, Bm = rnd_bits(rng, (M, K, 1)), rnd_bits(rng, (K, N, 1))
                a, b, out = Mat(inst, A), Mat(inst, Bm), Mat(inst, np.full((M, N, 1), 0x7FC0, np.uint16))
                inst.take_path()
                gemm(inst, False, out, a, b)
                log = inst.take_path()
                assert "bf16." in log, log
                eager = out.read(name)
                enc = inst.device().create_command_encoder(record=True)
                try:
                    gemm(inst, False, out, a, b)
                finally:
                    cb = enc.finish()
                assert inst.take_path() == log
                for rep in range(2):
                    inst.queue().write_buffer(out.buf, 0, out.base.view(wg.bfloat16))
                    inst.queue().submit([cb])
                    assert np.array_equal(out.read(f"{name} replay {rep}"), eager), f"{name} [{log}] replay {rep} on {where}"
                del cb
                if name in ("t128", "generic"):
                    product_check(eager, A, Bm, K, f"{name} on {where}")
            finally:
                for k, v in saved.items():
                    inst.set_tuning(k, v)
        rng = np.random.default_rng(11)
        R, C = 2048, 1024
        Mb, Vb = rnd_bits(rng, (R, C, 1)), rnd_bits(rng, (C, 1, 1))
        m, v, out = Mat(inst, Mb), Mat(inst, Vb), Mat(inst, np.full((R, 1, 1), 0x7FC0, np.uint16))
        _gemv_c(inst, False, "bf16", out, m, v)
        eager = out.read("gemv")
        enc = inst.device().create_command_encoder(record=True)
        try:
            _gemv_c(inst, False, "bf16", out, m, v)
        finally:
            cb = enc.finish()
        for rep in range(2):
            inst.queue().write_buffer(out.buf, 0, out.base.view(wg.bfloat16))
            inst.queue().submit([cb])
            assert np.array_equal(out.read("gemv replay"), eager)
        del cb
        m64, v64 = B.from_bits(Mb[:, :, 0]).astype(np.float64), B.from_bits(Vb[:, 0, 0]).astype(np.float64)
        truth = m64 @ v64
        assert (np.abs(B.from_bits(eager[:, 0, 0]).astype(np.float64) - truth) <= U.f32_gate(C, np.abs(m64) @ np.abs(v64)) + 2.0 ** -8 * np.abs(truth) + TINY).all()
    finally:
        if inst is not gpu:
            inst.sync()
            inst.close()


# ---- 12 ------------------------------------------------------------------------------------------------------------------------------------------
def test_fullsize_8192(gpu):
    n = 8192
    rng = np.random.default_rng(12)
    a_bits, b_bits = rnd_bits(rng, (n * n,)), rnd_bits(rng, (n * n,))
    ta, tb, tc = up_bits(gpu, a_bits), up_bits(gpu, b_bits), up_bits(gpu, np.full(n * n, 0x7FC0, np.uint16))
    wg, L = _wg(), _L()
    sh = wg.ViewShape((n, n, 1), n, n * n, 0)
    A0, Bf = B.from_bits(a_bits).reshape(n, n, order="F"), B.from_bits(b_bits).reshape(n, n, order="F")
    for tr in (False, True):
        gpu.take_path()
        L.check(L.lib.wg_gemm(gpu._ctx.handle, int(wg.GemmVariant.GemmTr if tr else wg.GemmVariant.Gemm), L.WG_BF16, tc._h, sh.to_c(), ta._h, sh.to_c(), tb._h, sh.to_c()))
        log = gpu.take_path()
        assert log.startswith("bf16."), log
        C = B.from_bits(rd_bits(gpu, tc)).reshape(n, n, order="F")
        assert np.isfinite(C).all()
        A = A0.T if tr else A0
        r = np.random.default_rng(6)
        rows, cols = np.unique(r.integers(0, n, 40)), np.unique(r.integers(0, n, 512))
        a64, b64 = A[rows].astype(np.float64), Bf[:, cols].astype(np.float64)
        truth, sabs = a64 @ b64, np.abs(a64) @ np.abs(b64)
        tol = U.f32_gate(n, sabs) + 2.0 ** -8 * np.abs(truth) + TINY
        err = np.abs(C[np.ix_(rows, cols)].astype(np.float64) - truth)
        assert (err <= tol).all(), f"bf16 gemm 8192^3 tr={tr} [{log}]: worst err/tol {(err / tol).max():.3g}"


# ---- 13 ------------------------------------------------------------------------------------------------------------------------------------------
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import record_f16_bits as F16FIX  # noqa: E402  (tools/record_f16_bits.py: the cases and the recorder of the fixture)


@pytest.mark.parametrize("name", [c[0] for c in F16FIX.CASES])
@pytest.mark.parametrize("tr", [False, True])
def test_f16_bits_unchanged(gpu, name, tr):
    """The f16 Gemm on four leaves (continuous walk, m16 + cut-up tail, 128 x 128 with split-K, generic) gives the bits recorded on the commit before the 16-bit
    sources became an element-type switch (tests/golden/f16_bits_before_bf16.npz: sha256 of each output, 4096 sampled elements, the launch log)."""
    fix = U.golden("f16_bits_before_bf16")
    key = f"{name}_{'tr' if tr else 'nn'}"
    bits, log = F16FIX.compute(gpu, name, tr)
    assert log == str(fix[key + "_log"]), (log, str(fix[key + "_log"]))
    assert np.array_equal(bits[F16FIX.sample_index(name, tr, bits.size)], fix[key + "_sample"])
    assert F16FIX.digest(bits) == str(fix[key + "_sha256"])
