"""The leading-dimension guards of the LDS-DMA kernels, on the host: no GPU, no context.

The tuned Gemm kernels keep ONE 32-bit byte offset per lane and DMA piece; a dozen host-side guards promise that `rows of a tile * ld * sizeof(T)` stays in
range. This file holds the table of those guards (GUARDS) and proves it against the pure planners, so that tests/test_gpu_far_views.py -- which runs both sides
of every guard on a device -- cannot drift from the code:

  * per guard the threshold T (the smallest refused leading dimension, in elements, of the named operand) is FOUND by bisection over `ld` with everything else
    fixed, asking wg_debug_gemm16_plan / wg_debug_gemm32_plan with the case's real query; no constant is copied from the planners. T - 8 is admitted, T and
    T + 8 are refused, and a sample of leading dimensions on either side shows the predicate monotone (planner rows: "f16", "f32");
  * the guards that sit in a launcher and not in a planner (gemm_f32.hip's dma_ok, gemm_f16_nt.hip, gemv.hip) cannot be asked: they are explicit rows whose
    predicate RESTATES the source line, constant included. For these rows the bisection proves the table against itself, not against the code; what the host file
    adds for them is the range of the protected expressions at the restated threshold. Which test then sees a changed constant in the source: gemv.hip:992 -- the
    GPU cases, whose log changes across the guard; gemm_f32.hip:602 / :647 (dma_ok, a kernel argument: the same log on both sides) and gemm_f16_nt.hip:231 (no GPU
    case fits the memory cap) -- NO test. A change there has to bring its row along by hand;
  * per guard, `exprs` restates the kernel expressions the guard protects -- (rows * ld + elements) * sizeof(T) + bias, at the lane where each is largest, bias
    terms included -- and the test asserts their value at ld = T - 8 below 2^32, or below 2^31 where the kernel or its descriptor says so (gemm_f16.hip:103).
    A guard constant that is too lax by a factor of two fails here, before anything runs on a GPU;
  * for every admitted (T - 8) and refused (T) query of a GPU case, `expected(...)` gives the plan's leaf and tag string: the GPU file asserts exactly these.

Run with -s to see, per guard: T, the protected expressions and their maxima at T - 8.
"""
import ctypes

import pytest

from wgmath_amd import _lib
from test_gemm16_plan_host import plan as plan16, query as query16
from test_gpu_epilogue import F32_KNOBS, F32_KNOB_SETS

GiB = 1 << 30
CAP_BYTES = 13 * GiB  # device memory one GPU case may hold
CUS = 256


class Expr:
    """One protected kernel expression, (rows * ld + add) * es + bias bytes, at the lane / piece where it is largest; `bits`: the range it must stay in."""

    def __init__(self, where, rows, add, es, bias=0, bits=31, only_tr=None):
        self.where, self.rows, self.add, self.es, self.bias, self.bits, self.only_tr = where, rows, add, es, bias, bits, only_tr

    def value(self, ld):
        return (self.rows * ld + self.add) * self.es + self.bias


class Case:
    """One product of a guard's GPU cases: knobs, (M, K, N) and the variants it runs."""

    def __init__(self, label, knobs, M, K, N, variants):
        self.label, self.knobs, self.M, self.K, self.N, self.variants = label, knobs, M, K, N, variants


class Guard:
    """family: "f16" (gemm16_plan.hip), "f32" (gemm32_plan.hip), or an explicit one ("f32big", "rm16", "rm32", "gemv32": `pred` restates the source line);
    explicit rows are the table's own statement: a changed constant in gemm_f32.hip:602 / :647 or gemm_f16_nt.hip:231 is seen by no test (module docstring).
    operand: "m1" / "m2"; fast: the plan leaves (planner rows) or the tag (explicit rows) on the admitted side; same_log: the launch log cannot differ across
    the guard (a kernel ARGUMENT decides)."""

    def __init__(self, name, family, operand, T, fast, exprs, cases, pred=None, same_log=False, unreachable=()):
        self.name, self.family, self.operand, self.T, self.fast, self.exprs, self.cases = name, family, operand, T, fast, exprs, cases
        self.pred, self.same_log, self.unreachable = pred, same_log, unreachable  # unreachable: variants whose far operand does not fit CAP_BYTES


M16, T128, SK = "gemm_f16.hip", "gemm_f16_t128.hip", "gemm_f32_skinny.hip"
T256 = {"f16_tile": 256, "f16_cont": 0}
BIG = {"f32_mid": 0, "f32_panels": 0}
NN, TR = (False,), (True,)
BOTH = (False, True)

GUARDS = [
    # ---- 16-bit tiles: gemm16_plan.hip `off_ok` (256 x 256, 256 x 128 and 128 x 128 kernels) -----------------------------------------------------------------
    # GemmTr m1 (K x M, k-contiguous rows): a_voff = (ra * lda + 8 chunk) * 2 + (BIAS - 1024 (q & 3)), ra <= 255, chunk <= 7, BIAS = 3072
    Guard("f16_tiles_tr_m1", "f16", "m1", 1 << 22, ("m16", "t128", "t256x128"),
          [Expr(f"{M16}:248", 255, 56, 2, 3072), Expr(f"{T128}:129 (TM = 256)", 255, 24, 2, 3072)],
          [Case("m16", T256, 256, 256, 256, TR), Case("m16_ragged", T256, 264, 256, 264, TR), Case("t128", {"f16_tile": 128}, 256, 256, 256, TR),
           Case("t256x128", {"f16_tile": 256128}, 256, 256, 256, TR)]),
    # Gemm m1 (M x K, column-major): a_voff = ((4 (P >> 1) + (lane >> 2 & 3)) * lda + mpiece) * 2 + BIAS: k row <= 31, mpiece <= 248; and the cursor step of a
    # half-stage, 32 k rows = 64 * lda bytes, an SGPR increment that must fit 32 bits (a_step_fits; its own test below)
    Guard("f16_tiles_nn_m1", "f16", "m1", 1 << 25, ("m16", "t128", "t256x128"),
          [Expr(f"{M16}:256", 31, 248, 2, 3072), Expr(f"{T128}:136", 31, 248, 2, 3072), Expr(f"{M16}:274 (a half-stage's step)", 32, 0, 2, 0, bits=32)],
          [Case("m16", T256, 256, 192, 256, NN), Case("t128", {"f16_tile": 128}, 256, 64, 256, NN), Case("t128_ragged", {"f16_tile": 128}, 136, 64, 136, NN),
           Case("t256x128", {"f16_tile": 256128}, 256, 64, 256, NN)]),
    # m2 (K x N, k-contiguous columns): b_voff = (rb * ldb + 8 chunk) * 2 + (BIAS - 1024 (q & 3)), rb <= 255 (128 x 128 and 256 x 128 kernels: <= 127)
    Guard("f16_tiles_m2", "f16", "m2", 1 << 22, ("m16", "t128", "t256x128"),
          [Expr(f"{M16}:266", 255, 56, 2, 3072), Expr(f"{T128}:149", 127, 24, 2, 3072)],
          [Case("m16", T256, 256, 256, 256, BOTH), Case("m16_ragged", T256, 264, 256, 264, BOTH), Case("t128", {"f16_tile": 128}, 256, 256, 256, BOTH),
           Case("t256x128", {"f16_tile": 256128}, 256, 256, 256, BOTH)]),
    # ---- 16-bit few-column kernel (GemmTr only): gemm16_plan.hip:146 -------------------------------------------------------------------------------------------
    # m1: rel = (row - r0) * lda * 2, row - r0 <= 31, + 16 chunk (<= 112) + TR_BIAS; its far operand has M >= 512 columns of 2^25 elements: 32 GiB, out of reach
    Guard("f16_skinny_m1", "f16", "m1", 1 << 25, ("skinny",), [Expr(f"{SK}:139-140", 31, 56, 2, 3072)], [Case("skinny", {}, 512, 16384, 8, TR)], unreachable=TR),
    # m2: b_voff = col * ldb * 2 + 16 chunk + TR_BIAS, col <= N - 1 <= 15 (the guard allows 31)
    Guard("f16_skinny_m2", "f16", "m2", 1 << 25, ("skinny",), [Expr(f"{SK}:166", 31, 56, 2, 3072)],
          [Case("skinny_n8", {}, 512, 16384, 8, TR), Case("skinny_n16", {}, 520, 16384, 16, TR)]),
    # ---- f32 256 x 128 kernel: gemm_f32.hip:602, `dma_ok`, a kernel argument read at :518 (the log cannot differ) --------------------------------------------------
    # m1: GemmTr a_voff = (row * lda + 4 chunk) * 4, row <= 255; Gemm a_voff = ((4 wave + q) * lda + 4 lane) * 4: k row <= 15, m <= 252
    Guard("f32_big_m1", "f32big", "m1", 1 << 21, "f32.big", [Expr("gemm_f32.hip:326", 255, 12, 4, only_tr=True), Expr("gemm_f32.hip:323", 15, 252, 4, only_tr=False)],
          [Case("big", BIG, 256, 64, 256, BOTH), Case("big_ragged", BIG, 264, 64, 136, BOTH)],
          pred=lambda ld: ld * 256 * 4 < (1 << 31), same_log=True),  # g.dma_ok = ((uint64_t)m1.ld * 256u * 4u < (1ull << 31)) && ...
    # m2: b_voff = (row * ldb + 4 chunk) * 4, row <= 127
    Guard("f32_big_m2", "f32big", "m2", 1 << 22, "f32.big", [Expr("gemm_f32.hip:336", 127, 12, 4)],
          [Case("big", BIG, 256, 64, 256, BOTH), Case("big_ragged", BIG, 264, 64, 136, BOTH)],
          pred=lambda ld: ld * 128 * 4 < (1 << 31), same_log=True),  # ... && ((uint64_t)m2.ld * 128u * 4u < (1ull << 31))
    # ---- f32 mid family: gemm32_plan.hip:44 mid_ok -------------------------------------------------------------------------------------------------------------------
    # m1: GemmTr voff = (row * lda + 4 chunk) * 4, row <= BM - 1 <= 127; Gemm voff = (krow * lda + m) * 4, krow <= 15 (2 x 2-wave tiles) / 31 (k-split tiles), m <= 124
    Guard("f32_mid_m1", "f32", "m1", 1 << 22, ("mid",),
          [Expr("gemm_f32_mid.hip:121", 127, 12, 4, only_tr=True), Expr("gemm_f32_mid.hip:348", 127, 28, 4, only_tr=True),
           Expr("gemm_f32_mid.hip:118", 15, 124, 4, only_tr=False), Expr("gemm_f32_mid.hip:345", 31, 92, 4, only_tr=False)],
          [Case("mid128x128", {"f32_mid": 128128}, 256, 64, 256, BOTH), Case("mid128x128_ragged", {"f32_mid": 128128}, 136, 64, 136, BOTH),
           Case("mid64x64_split", {"f32_mid": 64064, "f32_mid_split": 4}, 128, 128, 128, BOTH)]),
    # m2: voff = (row * ldb + 4 chunk) * 4, row <= BN - 1 <= 127
    Guard("f32_mid_m2", "f32", "m2", 1 << 22, ("mid",), [Expr("gemm_f32_mid.hip:125", 127, 12, 4), Expr("gemm_f32_mid.hip:352", 127, 28, 4)],
          [Case("mid128x128", {"f32_mid": 128128}, 256, 64, 256, BOTH), Case("mid128x128_ragged", {"f32_mid": 128128}, 136, 64, 136, BOTH),
           Case("mid64x64_split", {"f32_mid": 64064, "f32_mid_split": 4}, 128, 128, 128, BOTH)]),
    # ---- f32 few-column kernel: gemm32_plan.hip:163 --------------------------------------------------------------------------------------------------------------------
    # m1: GemmTr rel + 16 chunk + TR_BIAS with rel = (row - r0) * lda * 4, row - r0 <= 31; Gemm a_voff = (kr * lda + m) * 4 + TR_BIAS, kr <= 31, m <= 28.
    # GemmTr's far m1 has M >= 512 columns of 2^24 elements: 32 GiB, out of reach
    Guard("f32_skinny_m1", "f32", "m1", 1 << 24, ("skinny",), [Expr(f"{SK}:139-140", 31, 28, 4, 3072, only_tr=True), Expr(f"{SK}:150", 31, 28, 4, 3072, only_tr=False)],
          [Case("skinny_n8", {}, 512, 128, 8, BOTH), Case("skinny_n64", {}, 520, 128, 64, BOTH)], unreachable=TR),
    # m2: b_voff = col * ldb * 4 + 16 chunk + TR_BIAS, col <= 63
    Guard("f32_skinny_m2", "f32", "m2", 1 << 23, ("skinny",), [Expr(f"{SK}:166", 63, 28, 4, 3072)],
          [Case("skinny_n8", {}, 512, 128, 8, BOTH), Case("skinny_n64", {}, 520, 128, 64, BOTH)]),
    # ---- f32 transposed few-column form (M <= 64 rows, N >= 512): gemm32_plan.hip:155; past it the few-row form on transposed copies ---------------------------------
    # the kernel runs the transposed product: m1' = m2 (TRANS_A: row - r0 <= 31), m2' = m1 -- GemmTr: col * ldb * 4, col <= 63; Gemm (k-major): (kr * ldb + col) * 4,
    # kr <= 31, col <= 60. The far m2 has N >= 512 columns of 2^24 elements: 32 GiB, out of reach in both variants
    Guard("f32_skinnyT_m2", "f32", "m2", 1 << 24, ("skinny_t",), [Expr(f"{SK}:139-140 (m1' = m2)", 31, 28, 4, 3072)], [Case("skinnyT", {}, 16, 128, 512, BOTH)],
          unreachable=BOTH),
    Guard("f32_skinnyT_m1", "f32", "m1", 1 << 23, ("skinny_t",),
          [Expr(f"{SK}:166 (m2' = m1)", 63, 28, 4, 3072, only_tr=True), Expr(f"{SK}:159 (m2' = m1, k-major)", 31, 60, 4, 3072, only_tr=False)],
          [Case("skinnyT_m16", {}, 16, 128, 512, BOTH), Case("skinnyT_m64", {}, 64, 128, 520, BOTH)]),
    # ---- N-contiguous kernels (the native row-major GemmTr) ---------------------------------------------------------------------------------------------------------
    # f16, gemm_f16_nt.hip:231: a_voff / b_voff = (krow * ld + x) * 2 + NT_BIAS, krow <= 31, x <= 248; the cursor step 32 * ld * 2 is a uint32. Both operands
    # have K >= 256 columns (the kernel's minimum) of 2^25 elements: 16 GiB, out of reach
    Guard("rm16_nt", "rm16", "m1", 1 << 25, "f16.nt", [Expr("gemm_f16_nt.hip:71-72", 31, 248, 2, 3072), Expr("gemm_f16_nt.hip:77 (a half-stage's step)", 32, 0, 2, 0)],
          [Case("nt", {"rm_tr_native": 1, "f16_tile": 256}, 256, 256, 256, TR)],
          pred=lambda ld: not ld * 64 >= (1 << 31), unreachable=TR),  # if ((uint64_t)lda * 64u >= (1ull << 31) || (uint64_t)ldb * 64u >= (1ull << 31)) return WG_ERR_UNSUPPORTED;
    # f32, gemm_f32.hip:647 (dma_ok again: a kernel argument): a_voff = ((4 wave + q) * lda + 4 lane) * 4, k row <= 15, m <= 252; b_voff the same with n <= 124
    Guard("rm32_nt_m1", "rm32", "m1", 1 << 25, "f32.nt", [Expr("gemm_f32.hip:323", 15, 252, 4)],
          [Case("nt", {"rm_tr_native": 1}, 256, 64, 256, TR), Case("nt_ragged", {"rm_tr_native": 1}, 264, 64, 136, TR)],
          pred=lambda ld: ld * 16 * 4 < (1 << 31), same_log=True),  # g.dma_ok = ((uint64_t)a_mcontig.ld * 16u * 4u < (1ull << 31)) && ...
    Guard("rm32_nt_m2", "rm32", "m2", 1 << 25, "f32.nt", [Expr("gemm_f32.hip:332", 15, 124, 4)],
          [Case("nt", {"rm_tr_native": 1}, 256, 64, 256, TR), Case("nt_ragged", {"rm_tr_native": 1}, 264, 64, 136, TR)],
          pred=lambda ld: ld * 16 * 4 < (1 << 31), same_log=True),  # ... && ((uint64_t)b_ncontig.ld * 16u * 4u < (1ull << 31))
    # ---- Gemv with 9 .. 64 right-hand sides as an f32 Gemm with few columns: gemv.hip:992 (the few-column kernel's expressions) -------------------------------------
    Guard("gemv32_m", "gemv32", "m1", 1 << 24, "f32.skinny", [Expr(f"{SK}:139-140", 31, 28, 4, 3072, only_tr=True), Expr(f"{SK}:150", 31, 28, 4, 3072, only_tr=False)],
          [Case("rhs9", {}, 512, 128, 9, BOTH)],
          pred=lambda ld: ld * 32 * 4 < (1 << 31), unreachable=TR),  # (uint64_t)m.ld * 32u * 4u < (1ull << 31) && ...
    Guard("gemv32_v", "gemv32", "m2", 1 << 23, "f32.skinny", [Expr(f"{SK}:166", 63, 28, 4, 3072)], [Case("rhs9", {}, 512, 128, 9, BOTH), Case("rhs64", {}, 520, 128, 64, BOTH)],
          pred=lambda ld: ld * 64 * 4 < (1 << 31)),  # ... && (uint64_t)v.ld * 64u * 4u < (1ull << 31)
]
BY_NAME = {g.name: g for g in GUARDS}
PLANNED = [g for g in GUARDS if g.family in ("f16", "f32")]


def far_geometry(g, case, tr):
    """(rows, columns) of the stored far operand of a case, as the column-major API stores it (the row-major API: m1 is M x K m-contiguous, m2 is N x K)."""
    M, K, N = case.M, case.K, case.N
    if g.family in ("rm16", "rm32"):
        return (M, K) if g.operand == "m1" else (N, K)
    if g.operand == "m1":
        return (K, M) if tr else (M, K)
    return K, N


def far_bytes(g, case, tr, ld):
    rows, cols = far_geometry(g, case, tr)
    return ((cols - 1) * ld + rows) * (2 if g.family in ("f16", "rm16") else 4)


def plan32(q):
    p, buf = _lib.Gemm32PlanC(), ctypes.create_string_buffer(256)
    _lib.check(_lib.lib.wg_debug_gemm32_plan(ctypes.byref(q), ctypes.byref(p), buf, len(buf), None))
    return p, buf.value.decode()


def query32(tr, M, K, N, mats, knobs, cus=CUS):
    q = _lib.Gemm32QueryC()
    q.trans, q.M, q.N, q.K, q.nmats = int(tr), M, N, K, mats
    q.lda, q.ldb, q.ldc = (K if tr else M), K, M
    q.a_batch, q.b_batch, q.c_batch = M * K, K * N, M * N
    q.alpha, q.beta, q.cus = 1.0, 0.0, cus
    for k, v in zip(F32_KNOBS, F32_KNOB_SETS[0]):  # the context's defaults
        setattr(q, k[4:], knobs.get(k, v))
    return q


def expected(family, tr, M, K, N, knobs, lda=None, ldb=None, ldc=None, mats=1, batches=None, prefix="f16", cus=CUS):
    """(leaf name, tag string) of the planner for the product on views with these leading dimensions (None: dense) and matrix strides."""
    q = query16(tr, M, K, N, mats, knobs, cus=cus) if family == "f16" else query32(tr, M, K, N, mats, knobs, cus=cus)
    for name, v in (("lda", lda), ("ldb", ldb), ("ldc", ldc)):
        if v is not None:
            setattr(q, name, v)
    q.a_batch, q.b_batch, q.c_batch = batches or (q.lda * (M if tr else K), q.ldb * N, q.ldc * N)
    if family == "f16":
        p, log, _ = plan16(q, prefix)
        return _lib.GEMM16_LEAVES[p.leaf], log
    p, log = plan32(q)
    return _lib.GEMM32_LEAVES[p.leaf], log


def guard_expected(g, case, tr, ld, prefix="f16"):
    kw = {"lda" if g.operand == "m1" else "ldb": ld}
    return expected(g.family, tr, case.M, case.K, case.N, case.knobs, prefix=prefix, **kw)


def admitted(g, case, tr, ld):
    if g.pred is not None:
        return bool(g.pred(ld))
    return guard_expected(g, case, tr, ld)[0] in g.fast


def bisect_threshold(g, case, tr):
    """The smallest refused leading dimension (a multiple of 8) of the guard's operand, everything else fixed."""
    rows, _ = far_geometry(g, case, tr)
    lo, hi = -(-rows // 8), (1 << 29) // 8  # in units of 8 elements: admitted at the dense leading dimension, refused at 2^29
    assert admitted(g, case, tr, 8 * lo), f"{g.name} {case.label}: refused on a dense operand"
    assert not admitted(g, case, tr, 8 * hi), f"{g.name} {case.label}: admitted at ld = 2^29"
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if admitted(g, case, tr, 8 * mid) else (lo, mid)
    return 8 * hi


GUARD_CASES = [pytest.param(g, c, tr, id=f"{g.name}-{c.label}-{'tr' if tr else 'nn'}") for g in GUARDS for c in g.cases for tr in c.variants]


@pytest.mark.parametrize("g,case,tr", GUARD_CASES)
def test_threshold_found_by_bisection(g, case, tr):
    """T is where the table says, and the predicate is monotone around it."""
    T = bisect_threshold(g, case, tr)
    assert T == g.T, f"{g.name} {case.label}: the smallest refused leading dimension is {T} = 2^{T.bit_length() - 1}, the table says {g.T}"
    assert admitted(g, case, tr, T - 8) and not admitted(g, case, tr, T) and not admitted(g, case, tr, T + 8)
    rows, _ = far_geometry(g, case, tr)
    dense = -(-rows // 8) * 8
    below = sorted({dense, dense + 8, T // 2, T // 2 + 8, T - 4096, T - 16, T - 8} - set(range(dense)))
    above = [T, T + 8, T + 4096, 2 * T - 8, 2 * T, 4 * T, (1 << 32) - 8]
    assert all(admitted(g, case, tr, ld) for ld in below if ld >= dense), f"{g.name}: not monotone below T"
    assert not any(admitted(g, case, tr, ld) for ld in above), f"{g.name}: not monotone above T"
    if g.pred is None:  # what the plan says on either side: the GPU file asserts these logs
        (leaf0, log0), (leaf1, log1) = guard_expected(g, case, tr, T - 8), guard_expected(g, case, tr, T)
        assert leaf0 in g.fast and leaf1 not in g.fast and leaf1 != "unsupported" and log0 != log1, (leaf0, log0, leaf1, log1)
        print(f"\n{g.name} {case.label} {'tr' if tr else 'nn'}: T = 2^{T.bit_length() - 1}; T - 8 -> {log0!r}; T -> {log1!r}; "
              f"far operand {far_bytes(g, case, tr, T) / GiB:.2f} GiB")


@pytest.mark.parametrize("g", GUARDS, ids=[g.name for g in GUARDS])
def test_protected_expressions_stay_in_range(g):
    """At ld = T - 8 -- the largest leading dimension the guard admits -- every 32-bit byte offset the kernels form stays in its range; at T (what a constant
    too lax by two would admit: 2 T - 8) the largest one of them leaves the 2^31 range the guards promise."""
    worst = 0
    T = max(bisect_threshold(g, c, tr) for c in g.cases for tr in c.variants)  # what the code admits, not what the table says
    for e in g.exprs:
        v = e.value(T - 8)
        print(f"\n{g.name}: T = 2^{T.bit_length() - 1}; {e.where}: ({e.rows} * ld + {e.add}) * {e.es} + {e.bias} = {v} = 2^{e.bits} - {(1 << e.bits) - v} at T - 8")
        assert 0 <= v < (1 << e.bits), f"{g.name}: {e.where} reaches {v} at ld = T - 8 = {T - 8}, past 2^{e.bits}"
        worst = max(worst, e.value(2 * T - 8) >> e.bits)
    # the guards are not all tight (gemm_f32.hip's Gemm m1 has 16-fold headroom); a doubled threshold must still leave 2^32, the hardware's range, intact or
    # be caught above: recorded, the assertion is the one per expression
    print(f"{g.name}: at twice the threshold the largest expression is {'past' if worst else 'within'} its range")


def test_a_doubled_threshold_is_caught():
    """The mutation the table exists for: were off_ok's 256 rows 128 (T doubled), the expressions' maxima at the then-admitted 2 T - 8 leave the range."""
    for name in ("f16_tiles_tr_m1", "f16_tiles_m2", "f16_tiles_nn_m1", "f32_mid_m2", "f32_skinny_m2", "f32_big_m2"):
        g = BY_NAME[name]
        assert any(e.value(2 * g.T - 8) >= (1 << e.bits) for e in g.exprs), name


def test_a_step_fits_never_decides():
    """gemm16_plan.hip:165 `a_step_fits` (Gemm: 64 * lda < 2^32) is implied by off_ok (Gemm: 64 * lda < 2^31): from the off_ok threshold on every leading dimension
    is refused, and below it the half-stage step is below 2^31 -- so no query exists in which a_step_fits alone flips `fast`."""
    g = BY_NAME["f16_tiles_nn_m1"]
    for case in g.cases:
        T = bisect_threshold(g, case, False)
        assert 64 * (T - 8) < (1 << 31) < (1 << 32), "every admitted Gemm m1 steps less than 2^31 bytes per half-stage"
        for ld in (T, (1 << 26) - 8, 1 << 26, (1 << 26) + 8, 1 << 27, (1 << 32) - 8):  # around a_step_fits' own threshold, 2^26, and beyond
            assert not admitted(g, case, False, ld), ld
    # ... and GemmTr's a_step_fits is `true` by definition


def test_cases_fit_the_memory_cap():
    """Every GPU case's far operand fits 13 GiB at T, except the variants the table marks unreachable -- which do not."""
    for g in GUARDS:
        for c in g.cases:
            for tr in c.variants:
                need = far_bytes(g, c, tr, g.T)
                assert (need > CAP_BYTES) == (tr in g.unreachable), f"{g.name} {c.label} {'tr' if tr else 'nn'}: {need / GiB:.2f} GiB"
