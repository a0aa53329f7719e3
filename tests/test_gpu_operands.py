"""Every leaf of the Gemm and Gemv launchers on operands whose correct result is known to the bit: integer operands, poisoned neighbours, and +-Inf / NaN
inside the views.

Integer operands in [-8, 8] (zeros included) make every product and partial sum an integer below 2^24: the f32 accumulation is exact in any order and
any split of K, so the header's contract ("f32 accumulation, result rounded once (RNE)") fixes every output bit -- the f64 product rounded once to f32
or f16 (tests/_util.py special_product; checked on the CPU by tests/test_special_model.py). f16 operands add four rows of A built to land on the f16
edges (odd sums above 2048 that must round, sums in [65504, 65520) that round to 65504, sums from 65520 on that round to +-Inf); the test asserts each
case occurs. Per row of LEAVES (tests/test_gpu_epilogue.py), RM_LEAVES (row-major GemmTr) and GEMV_LEAVES, and per variant:
  exact    dense operands: bit-equal to the model; gemm_ex (alpha, beta) in {(1, 0), (2, 0), (0.5, 0.25), (-1, 1)} on an integer C0, bit-equal to the
           model of alpha * truth + beta * C0 (exact in f32: one rounding to f16) on whichever leaf the call takes; Gemv with several right-hand sides
           twice, bit-identical;
  aligned  the same data in parent buffers of quiet NaN everywhere outside the views (before the offset, in the leading-dimension gap, between matrices,
           after the end) at 16-byte-aligned offsets and gaps: the same leaf, the same bits -- a kernel that multiplies a value it read outside the view
           by zero instead of dropping it turns that output into NaN;
  odd      the same at offset 1 and an odd leading dimension: the leaf in the row's `odd` tag, the same bits;
  special  +Inf, -Inf and NaN at k = 0, k = K - 1, a k inside the K % 64 remainder, the last row and column (the ragged tiles), the last matrix, and
           an Inf opposite a zero of the other operand (Inf * 0 = NaN): NaN as a class, Inf with its sign, finite values to the bit.
Every call asserts the leaf it reaches from the launch log (wg_debug_take_path). Then the Reduce kernels and the fused Gemv + Reduce with +-Inf, NaN
and overflow against the C oracle (NaN as a class; Min / Max without NaN inputs, which WGSL leaves unspecified)."""
import numpy as np
import pytest

import _util as U
from test_gpu_epilogue import F16, F32, LEAVES, SENTINEL, Row, _lib, _upload, _wg, knobs  # noqa: F401  (knobs: the fixture)

pytestmark = pytest.mark.gpu

# offset, extra leading dimension, gap between matrices, elements after the end (None: the odd leading dimension)
LAYOUTS = {"dense": (0, 0, 0, 0), "aligned": (8, 8, 8, 8), "odd": (1, None, 3, 5)}
AB_EXACT = ((1.0, 0.0), (2.0, 0.0), (0.5, 0.25), (-1.0, 1.0))
CASES = ("exact", "aligned", "odd", "special")


class Stored:
    """A logical matrix X (r x c x mats, float64) stored column-major as X, or as X^T (`tr`), inside a parent buffer whose other elements are `fill`.
    `ld_mult`: the leading dimension rounded up to a multiple of it (a heuristic reads it)."""

    def __init__(self, gpu, X, dtype, layout, tr=False, fill=np.nan, ld_mult=1):
        S = np.transpose(X, (1, 0, 2)) if tr else X
        rs, cs, z = S.shape
        off, pad, gap, tail = LAYOUTS[layout]
        if pad is None:
            pad = 1 if rs % 2 == 0 else 2
        ld = max(rs + pad, 1)
        ld = -(-ld // ld_mult) * ld_mult
        self.ld, self.off, self.batch = ld, off, ld * cs + gap
        size = off + self.batch * z + tail
        self.idx = off + np.arange(rs)[:, None, None] + np.arange(cs)[None, :, None] * ld + np.arange(z)[None, None, :] * self.batch
        self.base = np.full(size, fill, dtype) if not isinstance(fill, np.unsignedinteger) else np.full(size, fill).view(dtype)
        flat = self.base.copy()
        with np.errstate(over="ignore", invalid="ignore"):
            flat[self.idx] = S.astype(dtype)
        self.mask = np.ones(size, bool)
        self.mask[self.idx.ravel()] = False
        self.tr, self.gpu = tr, gpu
        self.buf = _upload(gpu, flat)
        wg = _wg()
        self.cm = wg.ViewShape((rs, cs, z), ld, self.batch, off)  # the column-major view of the stored matrix
        self.rm = wg.ViewShape((cs, rs, z), ld, self.batch, off)  # the same memory as a row-major view (of X when tr, of X^T otherwise)

    def read(self, what):
        flat = self.buf.read(self.gpu.device())
        assert flat[self.mask].tobytes() == self.base[self.mask].tobytes(), f"{what}: wrote outside the output view"
        S = flat[self.idx]
        return np.transpose(S, (1, 0, 2)) if self.tr else S


def _ints(rng, shape):
    x = rng.integers(-8, 9, shape).astype(np.float64)
    x[rng.random(shape) < 0.15] = 0.0
    return x


F16_EDGE_ROWS = ((2047, 1), (2047, 3), (-2047, -3), (96, 1))  # with B[0, :] = 32 and B[1, :] in [0, 8]: 65504 + b, 65504 + 3 b, its negative, 3072 + b


def _operands(seed, dtype, M, K, N, Z):
    """Integer A (M x K x Z) and B (K x N x Z); for f16, rows of A on the f16 edges (F16_EDGE_ROWS)."""
    rng = np.random.default_rng(seed)
    A, B = _ints(rng, (M, K, Z)), _ints(rng, (K, N, Z))
    if dtype == F16:
        assert M >= 8 and K >= 2, (M, K)
        B[0], B[1] = 32.0, rng.integers(0, 9, (N, Z))
        B[1, 0] = 7.0  # (one right-hand side: 65511, 65525 -> Inf, -Inf, 3079)
        for r, (p, q) in zip((1, M // 3, M // 2, 2 * M // 3), F16_EDGE_ROWS):
            A[r] = 0.0
            A[r, 0], A[r, 1] = p, q
        if N >= 2:  # a column of 63s: partial sums over a part of K are odd and above 2048 -- a split that stores f16 partials rounds them
            B[2:, N // 2] = 63.0
    sabs = np.stack([np.abs(A[:, :, z]) @ np.abs(B[:, :, z]) for z in range(Z)], -1)
    assert sabs.max() < 2.0 ** 24, "the operands must multiply exactly in f32"
    return A, B


def _specials(A, B):
    A, B = A.copy(), B.copy()
    M, K, Z = A.shape
    N, zl = B.shape[1], Z - 1
    krem = (K // 64) * 64 + (K % 64) // 2 if K % 64 else K // 2  # inside the K % 64 remainder (the middle of K when there is none)
    A[0, 0, 0] = np.inf                      # k = 0
    if N == 1 and Z == 1:                    # (one vector: a special value in it would reach every output)
        A[M - 2, K - 1, 0] = -np.inf         # k = K - 1
    else:
        B[K - 1, N - 1, zl] = -np.inf        # k = K - 1, the last column, the last matrix
    A[M - 1, krem, zl] = np.nan              # the last row, the remainder of K
    k0 = max(1, K // 3) if K > 2 else 0
    B[k0, 0, 0] = 0.0                        # Inf * 0
    A[M // 4, k0, 0] = -np.inf
    A[(M // 2 + 3) % M, K - 1, 0] = np.inf   # k = K - 1 again, in the first matrix
    return A, B


def _check_f16_edges(truth):
    t = np.abs(truth[np.isfinite(truth)])
    assert ((t > 2048) & (t % 2 == 1)).any(), "no f16 output needs rounding"
    assert ((t >= 65504) & (t < 65520)).any(), "no f16 output in [65504, 65520)"
    assert (t >= 65520).any(), "no f16 output rounds to Inf"


_CACHE = {}


def _data(key, seed, dtype, M, K, N, Z):
    """Operands, the exact model, the special operands and their model, for one (row, variant): shared by its four cases."""
    if _CACHE.get("key") != key:
        A, B = _operands(seed, dtype, M, K, N, Z)
        As, Bs = _specials(A, B)
        _CACHE.clear()
        _CACHE.update(key=key, A=A, B=B, As=As, Bs=Bs, truth=U.special_product(A, B, np.float64), want=U.special_product(A, B, dtype),
                      want_s=U.special_product(As, Bs, dtype))
        fin = np.isfinite(_CACHE["want_s"])
        assert fin.mean() > 0.25 and not fin.all(), "the special case must keep finite outputs beside the non-finite ones"
    return _CACHE


# --------------------------------------------------------------------------------------------------------
# Gemm leaves
# --------------------------------------------------------------------------------------------------------
def _rm(row):
    row.api = "rm"
    return row


# row-major GemmTr (wg_gemm_rm): m1 where it lies, m2 contiguous along N -- gemm_f16_nt.hip, gemm_f16_t128.hip's and gemm_f32.hip's B_NC instances
RM_LEAVES = [
    _rm(Row("rm_f16_nt", F16, 512, 256, 512, 1, "f16.nt", {"rm_tr_native": 1, "f16_tile": 256}, variants=(True,))),
    _rm(Row("rm_f16_t128nc", F16, 384, 320, 264, 2, "f16.t128nc/tm=128", {"rm_tr_native": 1, "f16_tile": 128}, variants=(True,))),
    _rm(Row("rm_f16_t256x128nc", F16, 512, 256, 384, 1, "f16.t128nc/tm=256", {"rm_tr_native": 1, "f16_tile": 256128}, variants=(True,))),
    _rm(Row("rm_f32_nt", F32, 260, 132, 384, 2, "f32.nt", {"rm_tr_native": 1}, variants=(True,))),
]
# leaves whose K-remainder code the rows of LEAVES do not reach
EXTRA_LEAVES = [
    Row("f16_skinny_ktail", F16, 32768, 296, 8, 1, "f16.skinny/ns=1", variants=(True,)),  # K % 64 = 40: the zeroed tail chunks of the last stage
    Row("f16_t128_krem", F16, 512, 552, 512, 1, "f16.t128/ns=1", {"f16_tile": 128}),     # K % 64 = 40: the zero-padded remainder stage
    Row("f32_mid_krem", F32, 1000, 300, 1000, 1, "f32.mid", {"f32_mid": 128064}),
]
# the leaf the odd layout (offset 1, odd leading dimensions) takes where it is not the dense one
ODD_LEAF = {("f16_skinny", True): "f16.pad>f16.t128/ns=1", ("f16_skinny_ktail", True): "f16.pad>f16.t128/ns=1",
            ("f16_skinny_split", True): "f16.pad>f16.t128/ns=2 splitk.reduce/ns=2",
            ("f16_as_gemv", False): "f16.generic", ("f16_as_gemv", True): "f16.generic",
            ("f32_as_gemv", False): "f32.skinny/ns=2 splitk.reduce/ns=2", ("f32_as_gemv", True): "f32.skinny/ns=2 splitk.reduce/ns=2"}
GEMM_PARAMS = [pytest.param(r, tr, c, id=f"{r.name}-{'tr' if tr else 'nn'}-{c}") for r in LEAVES + EXTRA_LEAVES + RM_LEAVES for tr in r.variants for c in CASES]


def _gemm_call(gpu, row, tr, out, a, b, alpha=None, beta=None):
    wg, L = _wg(), _lib()
    dt = wg.wgcore.wg_dtype(row.dtype)
    h = gpu._ctx.handle
    if getattr(row, "api", "cm") == "rm":
        L.check(L.lib.wg_gemm_rm(h, int(wg.GemmVariant.GemmTr), dt, out.buf._h, out.rm.to_c(), a.buf._h, a.rm.to_c(), b.buf._h, b.rm.to_c()))
        return
    variant = int(wg.GemmVariant.GemmTr if tr else wg.GemmVariant.Gemm)
    if alpha is None:
        L.check(L.lib.wg_gemm(h, variant, dt, out.buf._h, out.cm.to_c(), a.buf._h, a.cm.to_c(), b.buf._h, b.cm.to_c()))
    else:
        L.check(L.lib.wg_gemm_ex(h, variant, dt, float(alpha), float(beta), out.buf._h, out.cm.to_c(), a.buf._h, a.cm.to_c(), b.buf._h, b.cm.to_c()))


def _gemm_operands(gpu, row, tr, A, B, layout, c0=None):
    """m1, m2 and the output (NaN, or c0) stored as the row's API reads them: column-major op(A) and B, or row-major A^T (K x M) and B (K x N)."""
    rm = getattr(row, "api", "cm") == "rm"
    a = Stored(gpu, A, row.dtype, layout, tr=tr and not rm)  # (row-major K x M is the column-major M x K)
    b = Stored(gpu, B, row.dtype, layout, tr=rm)
    init = np.full((A.shape[0], B.shape[1], A.shape[2]), np.nan) if c0 is None else c0
    out = Stored(gpu, init, row.dtype, "odd" if layout == "odd" else layout, tr=rm, fill=SENTINEL[row.dtype])
    return a, b, out


@pytest.mark.parametrize("row,tr,case", GEMM_PARAMS)
def test_gemm_leaf_operands(gpu, knobs, row, tr, case):
    dtype, M, K, N, Z = row.dtype, row.M, row.K, row.N, row.mats
    knobs(row.knobs)
    gpu.take_path()
    d = _data((row.name, tr), M * 7 + K * 5 + N * 3 + Z + int(tr), dtype, M, K, N, Z)
    if case == "special":
        for layout in ("dense", "odd"):
            a, b, out = _gemm_operands(gpu, row, tr, d["As"], d["Bs"], layout)
            _gemm_call(gpu, row, tr, out, a, b)
            log = gpu.take_path()
            leaf = ODD_LEAF.get((row.name, tr), row.leaf) if layout == "odd" else row.leaf
            assert Row.took(leaf, log), f"{row.name} special {layout}: expected {leaf!r}, took {log!r}"
            U.assert_same_class_bits(out.read("special"), d["want_s"], f"{row.name} special {layout} [{log}]")
        return
    if dtype == F16:
        _check_f16_edges(d["truth"])
    a, b, out = _gemm_operands(gpu, row, tr, d["A"], d["B"], "dense" if case == "exact" else case)
    _gemm_call(gpu, row, tr, out, a, b)
    log = gpu.take_path()
    leaf = ODD_LEAF.get((row.name, tr), row.leaf) if case == "odd" else row.leaf
    assert Row.took(leaf, log), f"{row.name} {case}: expected {leaf!r}, took {log!r}"
    U.assert_bits_equal(out.read(case), d["want"], f"{row.name} {case} [{log}]")
    if case != "exact" or getattr(row, "api", "cm") == "rm":
        return
    rng = np.random.default_rng(M + N)
    c0 = _ints(rng, (M, N, Z))
    for alpha, beta in AB_EXACT:
        a, b, out = _gemm_operands(gpu, row, tr, d["A"], d["B"], "dense", c0=c0)
        _gemm_call(gpu, row, tr, out, a, b, alpha, beta)
        log = gpu.take_path()
        assert Row.took(row.leaf, log) or Row.took(row.ab, log, row.not_ab), f"{row.name} ({alpha}, {beta}): took {log!r}"
        with np.errstate(over="ignore"):
            want = (alpha * d["truth"] + beta * c0 + 0.0).astype(dtype)
        U.assert_bits_equal(out.read(f"gemm_ex({alpha}, {beta})"), want, f"{row.name} gemm_ex({alpha}, {beta}) [{log}]")


# --------------------------------------------------------------------------------------------------------
# Gemv leaves (gemv.hip wgk_gemv and what it hands off to)
# --------------------------------------------------------------------------------------------------------
class GRow:
    """One Gemv leaf: dtype, variant (tr), the matrix R x C, right-hand sides, matrices, the tag(s) the call must log (`not_`: a tag it must not),
    the tag of the odd layout, knobs, a multiple the matrix's leading dimension keeps (a heuristic reads it), and whether the vectors and the output
    take the odd layout in every case (`vodd`)."""

    def __init__(self, name, dtype, tr, R, C, nrhs, mats, leaf, not_=None, odd=None, knobs=None, ld_mult=1, vodd=False):
        self.name, self.dtype, self.tr, self.R, self.C, self.nrhs, self.mats = name, dtype, tr, R, C, nrhs, mats
        self.leaf, self.not_, self.knobs, self.ld_mult, self.vodd = leaf, not_, knobs or {}, ld_mult, vodd
        self.odd = odd or f"gemv_any/{'t' if tr else 'n'},ns="


GEMV_LEAVES = [
    # N, launch-bound: one kernel, no partials (rows per workgroup by the output length)
    GRow("small_rl8", F32, False, 4096, 1024, 1, 1, "gemv.small/rl=8"),
    GRow("small_rl4", F32, False, 2048, 512, 2, 1, "gemv.small/rl=4"),
    GRow("small_rl2", F32, False, 512, 512, 1, 2, "gemv.small/rl=2"),
    GRow("f16_small_rl4", F16, False, 2048, 512, 1, 1, "gemv.small/rl=4"),
    # N, unsplit (K <= 64) and split + combine; the register tile = 1, 2, 4, 8 right-hand sides
    GRow("n_t1", F32, False, 1024, 64, 1, 1, "gemv.n/t=1,ns=1"),
    GRow("n_t2", F32, False, 1024, 64, 2, 3, "gemv.n/t=2,ns=1"),
    GRow("n_t4", F32, False, 1024, 64, 3, 1, "gemv.n/t=4,ns=1"),
    GRow("n_t8", F32, False, 1024, 64, 6, 1, "gemv.n/t=8,ns=1"),
    GRow("n_t1_split", F32, False, 64, 4096, 1, 1, "gemv.n/t=1,ns=64 gemv.combine/ns=64"),
    GRow("n_t8_split", F32, False, 64, 4096, 8, 2, "gemv.n/t=8,ns=64 gemv.combine/ns=64"),
    GRow("f16_n_t4_split", F16, False, 64, 4096, 3, 1, "gemv.n/t=4,ns=64 gemv.combine/ns=64"),
    GRow("f16_n_t2", F16, False, 1024, 64, 2, 2, "gemv.n/t=2,ns=1"),
    # T on the 4-columns-per-wave kernel: f32 columns 64 KiB apart (one right-hand side), 2 .. 8 right-hand sides on few outputs
    GRow("t_t1_split", F32, True, 16384, 32, 1, 1, "gemv.t/t=1,ns=8 gemv.combine/ns=8", ld_mult=16384),
    GRow("t_t2", F32, True, 1024, 512, 2, 1, "gemv.t/t=2,ns=1"),
    GRow("t_t4", F32, True, 1024, 512, 4, 2, "gemv.t/t=4,ns=1"),
    GRow("t_t8", F32, True, 1024, 512, 7, 1, "gemv.t/t=8,ns=1"),
    GRow("t_t2_split", F32, True, 8192, 256, 2, 1, "gemv.t/t=2,ns=4 gemv.combine/ns=4"),
    GRow("f16_t_t4", F16, True, 1024, 512, 4, 1, "gemv.t/t=4,ns=1"),
    # T, one right-hand side: a half-wave per column (f16 16-byte loads where every column stays aligned, 4 or 8 loads in flight), two: the 2-vector form
    GRow("tcols_e4u4", F32, True, 1024, 1024, 1, 1, "gemv.tcols/e=4,u=4,v=1,ns=1"),
    GRow("tcols_e4u8", F32, True, 2048, 1024, 1, 2, "gemv.tcols/e=4,u=8,v=1,ns=1"),
    GRow("tcols_v2", F32, True, 2052, 4096, 2, 1, "gemv.tcols/e=4,u=4,v=2,ns=1"),
    GRow("f16_tcols_e8u4", F16, True, 1024, 1024, 1, 1, "gemv.tcols/e=8,u=4,v=1,ns=1"),
    GRow("f16_tcols_e8u8", F16, True, 4096, 4096, 1, 1, "gemv.tcols/e=8,u=8,v=1,ns=1"),
    GRow("f16_tcols_e4u4", F16, True, 1020, 1024, 1, 1, "gemv.tcols/e=4,u=4,v=1,ns=1"),
    GRow("f16_tcols_e4u8", F16, True, 2052, 4096, 1, 1, "gemv.tcols/e=4,u=8,v=1,ns=1"),
    GRow("f16_tcols_split", F16, True, 4096, 1024, 1, 1, "gemv.tcols/e=8,u=4,v=1,ns=2 gemv.combine/ns=2"),
    GRow("f16_tcols_v2_e8", F16, True, 1024, 2048, 2, 1, "gemv.tcols/e=8,u=4,v=2,ns=1"),
    GRow("f16_tcols_v2_e4", F16, True, 1020, 2048, 2, 1, "gemv.tcols/e=4,u=4,v=2,ns=1"),
    # f32 T, 2 .. 8 right-hand sides with the vectors in the LDS: the five workgroup shapes and the three tiles
    GRow("tlds_nr2_c1_256", F32, True, 1024, 2048, 2, 1, "gemv.tlds/nr=2,c=1,th=256"),
    GRow("tlds_nr2_c1_512", F32, True, 128, 4096, 2, 1, "gemv.tlds/nr=2,c=1,th=512", knobs={"gemvt_lds": 1}),
    GRow("tlds_nr8_c1_1024", F32, True, 128, 8192, 8, 1, "gemv.tlds/nr=8,c=1,th=1024", knobs={"gemvt_lds": 1}),
    GRow("tlds_nr8_c2", F32, True, 1024, 16384, 5, 1, "gemv.tlds/nr=8,c=2,th=1024", knobs={"gemvt_lds": 1}),
    GRow("tlds_nr4_c4", F32, True, 128, 32768, 4, 1, "gemv.tlds/nr=4,c=4,th=1024"),
    GRow("tlds_nr4_batch", F32, True, 128, 256, 3, 3, "gemv.tlds/nr=4,c=1,th=256", knobs={"gemvt_lds": 1}),
    # hand-offs to the Gemm kernels: more than 8 right-hand sides, and 3 .. 8 on matrices past a size (few_rhs_as_gemm)
    GRow("f32_9rhs_gemm", F32, False, 512, 256, 9, 1, "gemv>f32.skinny/ns=2 splitk.reduce/ns=2", odd="gemv_any/n,ns=1"),
    GRow("f32_5rhs_gemm", F32, False, 8192, 1536, 5, 1, "gemv>f32.skinny/ns=4 splitk.reduce/ns=4"),
    GRow("f32_tr_8rhs_gemm", F32, True, 1024, 4096, 8, 1, "gemv>f32.skinny/ns=8 splitk.reduce/ns=8", odd="gemv_any/t,ns=1"),
    GRow("f16_9rhs_gemm", F16, True, 512, 256, 9, 1, "gemv>f16.t128/ns=1", odd="gemv_any/t,ns=1"),
    GRow("f16_8rhs_gemm", F16, False, 4096, 2048, 8, 1, "gemv>f16.t128/ns=2 splitk.reduce/ns=2", odd="gemv_any/n,ns=8"),
    # a matrix the vec4 kernels cannot take as it lies (a length that is not a multiple of 4): the any-alignment kernels, ragged wave ranges
    GRow("any_n_k69", F32, False, 130, 69, 2, 1, "gemv_any/n,ns=1"),  # (the last wave range, 54 .. 68, ends in a partial group of 8 columns)
    GRow("f16_any_t", F16, True, 67, 130, 1, 1, "gemv_any/t,ns=1"),
    # an aligned matrix with the vectors and the output at odd offsets: copies of those (`stage>`), the matrix where it lies
    GRow("f32_stage_v", F32, False, 128, 64, 2, 1, ("stage>gemv>", "gemv.n/"), vodd=True),
    GRow("f16_stage_v", F16, True, 64, 128, 1, 1, ("stage>gemv>", "f16.gemv"), vodd=True),
]
GEMV_PARAMS = [pytest.param(r, c, id=f"{r.name}-{c}") for r in GEMV_LEAVES for c in CASES]


def _gemv_call(gpu, row, out, m, v):
    wg, L = _wg(), _lib()
    variant = int(wg.GemvVariant.GemvTr if row.tr else wg.GemvVariant.Gemv)
    L.check(L.lib.wg_gemv(gpu._ctx.handle, variant, wg.wgcore.wg_dtype(row.dtype), out.buf._h, out.cm.to_c(), m.buf._h, m.cm.to_c(), v.buf._h, v.cm.to_c()))


def _gemv_run(gpu, row, A, V, layout):
    m = Stored(gpu, A, row.dtype, layout, tr=row.tr, ld_mult=row.ld_mult if layout != "odd" else 1)  # (GemvTr: m = op(m)^T)
    vl = "odd" if row.vodd else layout
    v = Stored(gpu, V, row.dtype, vl)
    out = Stored(gpu, np.full((A.shape[0], V.shape[1], A.shape[2]), np.nan), row.dtype, vl, fill=SENTINEL[row.dtype])
    _gemv_call(gpu, row, out, m, v)
    log = gpu.take_path()
    return out, log, (m, v)


@pytest.mark.parametrize("row,case", GEMV_PARAMS)
def test_gemv_leaf_operands(gpu, knobs, row, case):
    dtype, Z = row.dtype, row.mats
    ro, k = (row.C, row.R) if row.tr else (row.R, row.C)
    knobs(row.knobs)
    gpu.take_path()
    d = _data(("gemv", row.name), ro * 7 + k * 5 + row.nrhs * 3 + Z + int(row.tr), dtype, ro, k, row.nrhs, Z)
    if case == "special":
        for layout in ("dense", "odd"):
            out, log, _ = _gemv_run(gpu, row, d["As"], d["Bs"], layout)
            leaf, not_ = (row.odd, None) if layout == "odd" else (row.leaf, row.not_)
            assert Row.took(leaf, log, not_), f"{row.name} special {layout}: expected {leaf!r}, took {log!r}"
            U.assert_same_class_bits(out.read("special"), d["want_s"], f"{row.name} special {layout} [{log}]")
        return
    if dtype == F16:
        _check_f16_edges(d["truth"])
    out, log, (m, v) = _gemv_run(gpu, row, d["A"], d["B"], "dense" if case == "exact" else case)
    leaf, not_ = (row.odd, None) if case == "odd" else (row.leaf, row.not_)
    assert Row.took(leaf, log, not_), f"{row.name} {case}: expected {leaf!r}, took {log!r}"
    got = out.read(case)
    U.assert_bits_equal(got, d["want"], f"{row.name} {case} [{log}]")
    if case == "exact" and row.nrhs > 1:  # several right-hand sides: the same bits on a second run (the header's determinism)
        _gemv_call(gpu, row, out, m, v)
        assert gpu.take_path() == log
        U.assert_bits_equal(out.read("second run"), got, f"{row.name}: a second run")


# --------------------------------------------------------------------------------------------------------
# Reduce and the fused Gemv + Reduce with +-Inf, NaN and overflow
# --------------------------------------------------------------------------------------------------------
def _run(gpu, fn):
    enc = gpu.device().create_command_encoder()
    with enc.compute_pass("ops", None) as p:
        fn(p)
    gpu.queue().submit([enc.finish()])


def _reduce_data(rng, n, ops, dtype):
    """(case, x) pairs of integers in [-8, 8] whose result is the same in every order: a finite case, then per op family +-Inf and NaN for Sum / Prod /
    SqNorm and values large enough that the sum, the product or the squares overflow; +-Inf only for Min / Max."""
    x = rng.integers(-8, 9, n).astype(np.float64)
    pos = rng.choice(n, 12, replace=False)
    big = 60000.0 if dtype == F16 else 3.0e38
    if ops == "minmax":
        y = x.copy()
        y[pos[:2]] = (np.inf, -np.inf)
        return [("finite", x), ("inf", y)]
    if ops == "prod":  # |x| >= 1 everywhere: every partial product grows, so the overflow does not depend on the order
        f = np.where(rng.random(n) < 0.5, -1.0, 1.0)
        f[pos[:10]] = 2.0  # (a finite, exact product: +-1024)
        x[x == 0] = 1.0
        y = x.copy()
        y[pos[:3]] = (2.0 ** 60, -(2.0 ** 60), 2.0 ** 20) if dtype == F32 else (256.0, -256.0, 64.0)
        z = x.copy()
        z[pos[0]] = np.inf
        w = z.copy()
        w[pos[1]] = np.nan
        return [("finite", f), ("overflow", y), ("inf", z), ("nan", w)]
    y = x.copy()  # the sum of two large values of one sign overflows whatever comes between them
    y[pos[:2]] = big
    z = x.copy()
    z[pos[:2]] = (np.inf, -np.inf)  # Inf + -Inf = NaN
    w = x.copy()
    w[pos[0]] = np.nan
    v = x.copy()
    v[pos[0]] = -np.inf
    f = x if dtype == F32 else np.where(rng.random(n) < 400.0 / n, x, 0.0)  # (f16: few nonzeros, so that the sum of squares stays below 65504)
    return [("finite", f), ("overflow", y), ("inf_pair", z), ("nan", w), ("inf", v)]


# path, length, offset, the kernel it must reach (offset 4: the vec4 instance of reduce_rows4, 3: the element-aligned one)
REDUCE_PATHS = [("single", 4097, 3, "reduce.rows4/al=0"), ("single", 4097, 4, "reduce.rows4/al=1"), ("single", 300007, 3, "reduce.long"),
                ("batched", 1000, 3, "reduce.rows4/al=0"), ("batched", 1000, 4, "reduce.rows4/al=1"), ("batched", 300007, 4, "reduce.long"),
                ("fast", 65541, 3, "reduce.fast/")]


@pytest.mark.parametrize("dtype", [F32, F16])
@pytest.mark.parametrize("path,n,off,leaf", REDUCE_PATHS)
def test_reduce_special_values(gpu, oracle_c, path, n, off, leaf, dtype):
    wg = _wg()
    from oracle import wgsl_oracle as wo
    rng = np.random.default_rng(n + off + (dtype == F16))
    dev, shapes = gpu.device(), wg.ViewShapeBuffers()
    for op, wop, fam in ((wg.ReduceOp.Min, wo.MIN, "minmax"), (wg.ReduceOp.Max, wo.MAX, "minmax"), (wg.ReduceOp.Sum, wo.SUM, "sum"),
                         (wg.ReduceOp.SqNorm, wo.SQNORM, "sum"), (wg.ReduceOp.Prod, wo.PROD, "prod")):
        red = wg.Reduce.new(dev, op)
        for case, x in _reduce_data(rng, n, fam, dtype):
            cols = 3 if path == "batched" else 1
            xs = np.concatenate([np.roll(x, 7 * c) for c in range(cols)]).astype(dtype)  # (a few vectors: the same values in other places)
            flat = np.concatenate([np.full(off, np.nan, dtype), xs, np.full(5, np.nan, dtype)])  # NaN before and after the view
            t = _upload(gpu, flat)
            res = _upload(gpu, np.full(cols, np.nan, dtype))
            view = wg.GpuTensorView(wg.ViewShape((n, cols, 1), n, n * cols, off), t, 2 if cols > 1 else 1)
            gpu.take_path()
            if path == "batched":
                _run(gpu, lambda p: red.dispatch_batched(dev, shapes, p, view, res))
            elif path == "fast":
                _run(gpu, lambda p: red.dispatch_fast(dev, shapes, p, view, res))
            else:
                _run(gpu, lambda p: red.dispatch(dev, shapes, p, view, res))
            got = res.read(dev)
            log = gpu.take_path()
            # (Min / Max of one long vector: order-free, the two-pass kernels -- wgk_reduce)
            want_leaf = "reduce.fast/" if path == "single" and n >= 65536 and fam == "minmax" else leaf
            assert want_leaf in log, f"{path} n={n} offset {off} {op.name}: expected {want_leaf!r}, took {log!r}"
            x32 = xs.astype(np.float32)
            with np.errstate(over="ignore", invalid="ignore"):
                want = np.array([oracle_c.reduce(int(wop), x32, wo.Shape(n, 1, 1, n, n, c * n)) for c in range(cols)], np.float32).astype(dtype)
            assert np.isfinite(want).all() == (case == "finite"), (case, op.name, want)  # (each case is what it claims to be)
            U.assert_same_class_bits(got, want, f"{path} {case} {op.name} {np.dtype(dtype).name} [{log}]")


# y = m v per case (k0: a column of A opposite 3, k1: opposite 2^127, k2: opposite 2^17 -- all ones makes every y positive: 2^17 + |sum| <= 2^17 + 64 C)
# and the class each op's result must have ("fin": finite; Min / Max are skipped where y holds a NaN)
GEMV_REDUCE_CASES = {
    "finite": {"Min": "fin", "Max": "fin", "Sum": "fin", "SqNorm": "fin"},
    "overflow": {"Min": "fin", "Max": "fin", "Sum": "+inf", "SqNorm": "+inf", "Prod": "+inf"},  # y[33] = y[34] = 2^127
    "inf_pair": {"Min": "-inf", "Max": "+inf", "Sum": "nan", "SqNorm": "+inf", "Prod": "-inf"},  # y[17] = +Inf, y[R - 1] = -Inf
    "one_inf": {"Min": "-inf", "Max": "fin", "Sum": "-inf", "SqNorm": "+inf", "Prod": "-inf"},  # y[R - 1] = -Inf
    "nan": {"Sum": "nan", "SqNorm": "nan", "Prod": "nan"},  # y[R / 2] = NaN
}


def _gemv_reduce_operands(rng, R, C, case):
    k0, k1, k2 = 5, 9, 11
    A, V = _ints(rng, (R, C, 1)), _ints(rng, (C, 1, 1))
    V[k0, 0, 0], V[k1, 0, 0], V[k2, 0, 0] = 3.0, 2.0 ** 127, 2.0 ** 17
    A[:, k1, 0] = 0.0
    if case != "finite":
        A[:, k2, 0] = 1.0
    if case == "overflow":
        A[33, k1, 0] = A[34, k1, 0] = 1.0  # (2^127 + an integer is 2^127 in any order)
    if case == "inf_pair":
        A[17, k0, 0] = np.inf
    if case in ("inf_pair", "one_inf"):
        A[R - 1, k0, 0] = -np.inf
    if case == "nan":
        A[R // 2, 2, 0] = np.nan
    return A, V


def _klass(x):
    return "nan" if np.isnan(x) else "+inf" if x == np.inf else "-inf" if x == -np.inf else "fin"


@pytest.mark.parametrize("R,C,leaf", [(512, 256, "gemv.small_reduce/rl=2"), (2048, 512, "gemv.small_reduce/rl=4"), (4096, 1024, "gemv.small_reduce/rl=8"),
                                      (8192, 1024, "gemv_reduce.two>gemv>")])
@pytest.mark.parametrize("case", list(GEMV_REDUCE_CASES))
def test_gemv_reduce_special_values(gpu, oracle_c, R, C, leaf, case):
    """result = reduce(op, m v) on integer operands, one kind of value per case: all finite, overflow (the sum, the squares and the product of 2^127),
    +Inf and -Inf, one -Inf, one NaN. The bits of the oracle's Reduce on the exact y (NaN as a class), on the fused kernel and on the two-launch form;
    the class of each expected result is asserted first, so no case can pass on a result that ignores y."""
    wg = _wg()
    from oracle import wgsl_oracle as wo
    dev = gpu.device()
    rng = np.random.default_rng(R + C)
    A, V = _gemv_reduce_operands(rng, R, C, case)
    y = U.special_product(A, V, F32)[:, 0, 0]
    m = Stored(gpu, A, F32, "aligned")
    v = _upload(gpu, V.ravel().astype(F32))
    mv = wg.GpuTensorView(m.cm, m.buf, 2)
    for name, klass in GEMV_REDUCE_CASES[case].items():
        op, wop = wg.ReduceOp[name], getattr(wo, name.upper())
        with np.errstate(over="ignore", invalid="ignore"):
            want = np.array([oracle_c.reduce(int(wop), y, wo.Shape(R, 1, 1, R, R, 0))], np.float32)
        assert _klass(want[0]) == klass, (case, name, want)
        res = _upload(gpu, np.full(1, np.nan, F32))
        gpu.take_path()
        _run(gpu, lambda p: wg.gemv_reduce(p, op, res, mv, v, wg.GemvVariant.Gemv))
        log = gpu.take_path()
        assert leaf in log, f"{R} x {C} {op.name}: expected {leaf!r}, took {log!r}"
        U.assert_same_class_bits(res.read(dev), want, f"gemv_reduce {R} x {C} {case} {op.name} [{log}]")
