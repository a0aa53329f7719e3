"""The `out = alpha * acc + beta * out` epilogue (wg_gemm_ex) on every leaf of the f16 and f32 Gemm launchers' dispatch trees, and Gemv on views that are
not vec4-aligned with many right-hand sides.

Each leaf has its own copy of the epilogue (the kernel's store, the split-K reduce, the tail reduce, the balance units, the padded output seeded from C).
Every row of LEAVES names the leaf it must reach, asserted from the context's launch log (wg_debug_take_path) so that a heuristic change cannot quietly
move a row to another leaf. Per row, variant and output view (dense; odd offset, odd leading dimension and a gap between matrices):
  1. Gemm into a NaN prefill: within the f64 bound (U.f32_gate; f16 + half an f16 ulp), no NaN left;
  2. gemm_ex(1, 0) into NaN / +-Inf: bit-identical to 1, same log;
  3. gemm_ex(alpha, 0): f32 bit-equal to fl32(alpha * R); f16 (alpha = 2) bit-equal to 2 * R16 where both are normal f16;
  4. gemm_ex(alpha, beta) on a random C0: on the same leaf, f32 is bit-equal to fmaf(beta, C0, fl32(alpha * R)) (tests/_util.py fmaf_f32); f16 and
     rerouted calls within |alpha| gate + an ulp of |alpha truth| + |beta C0| of the f64 value; the log shows the leaf (or reroute) the row expects;
  5. everything around and between the output's columns and matrices is bit-unchanged (a sentinel NaN pattern).
"""
import ctypes
import itertools

import numpy as np
import pytest

import _util as U

pytestmark = pytest.mark.gpu

S_STORAGE = 128 | 4 | 8  # STORAGE | COPY_SRC | COPY_DST
AB = ((-1.5, 0.25), (1.0, 1.0), (0.5, -2.0))
SENTINEL = {np.float32: np.uint32(0x7FC5A5A5), np.float16: np.uint16(0x7E5A)}  # quiet NaNs with a payload no kernel writes


def _wg():
    import wgmath_amd as wg
    return wg


def _lib():
    from wgmath_amd import _lib
    return _lib


class Row:
    """One leaf: dtype, (M, K, N, mats), the knobs it sets, the tag(s) its (1, 0) log must contain and the tag(s) its (alpha, beta) logs must contain (`ab`;
    None: the same as `leaf`), a tag those logs must NOT contain (`not_ab`: a leaf that requires beta == 0), the variants it takes, and whether the leaf needs an aligned
    output (then asserted on the dense view only)."""

    def __init__(self, name, dtype, M, K, N, mats, leaf, knobs=None, ab=None, not_ab=None, variants=(False, True), dense_only=False):
        self.name, self.dtype, self.M, self.K, self.N, self.mats = name, dtype, M, K, N, mats
        self.leaf, self.knobs, self.ab, self.not_ab, self.variants, self.dense_only = leaf, knobs or {}, ab or leaf, not_ab, variants, dense_only

    @staticmethod
    def took(tags, log, without=None):
        return all(t in log for t in ((tags,) if isinstance(tags, str) else tags)) and (without is None or without not in log)


F16, F32 = np.float16, np.float32
LEAVES = [
    # ---- f16 (gemm_f16.hip and what it hands off to) ----
    Row("f16_skinny", F16, 32768, 256, 8, 1, "f16.skinny/ns=1", variants=(True,), dense_only=True),      # the kernel's own store (one split)
    Row("f16_skinny_split", F16, 4096, 2048, 8, 1, "f16.skinny/ns=8 splitk.reduce/ns=8", variants=(True,), dense_only=True),
    Row("f16_t128", F16, 512, 512, 512, 1, "f16.t128/ns=1", {"f16_tile": 128}),
    Row("f16_t128_split", F16, 512, 4096, 512, 1, "f16.t128/ns=4 splitk.reduce/ns=4", {"f16_tile": 128}),
    Row("f16_t256x128", F16, 1024, 512, 1024, 1, "f16.t256x128", {"f16_tile": 256128}),
    Row("f16_m16_static", F16, 4096, 512, 4096, 1, "f16.m16/ns=1", {"f16_tile": 256, "f16_sched": 0}),
    Row("f16_m16_queues", F16, 4096, 512, 4096, 1, "f16.m16q/ns=1", {"f16_tile": 256, "f16_sched": 1}),
    Row("f16_m16_balance", F16, 4096, 1024, 4096, 1, "f16.m16bal/ns=1", {"f16_tile": 256, "f16_balance": 1}),
    Row("f16_m16_splitk", F16, 1024, 4096, 1024, 1, "f16.m16/ns=16 splitk.reduce/ns=16", {"f16_tile": 256, "f16_cont": 0}),
    Row("f16_m16_tail", F16, 4352, 1024, 4096, 1, "f16.m16/ns=1 f16.m16tail/ns=4 f16.tail_reduce", {"f16_tile": 256, "f16_cont": 0}),
    # the continuous walk requires beta == 0: (alpha, beta) calls take the per-tile launch
    Row("f16_cont", F16, 4096, 256, 8192, 1, "f16.cont", {"f16_tile": 256, "f16_cont": 1}, ab="f16.m16/ns=1", not_ab="f16.cont"),
    # M = 4 (mod 8): the output is padded, and seeded from C when beta != 0; K = 4 (mod 8): only the operands are
    Row("f16_pad_c", F16, 1028, 512, 1028, 1, "f16.pad/c>", ab="f16.pad/c=seed>"),
    Row("f16_pad_k", F16, 1024, 1028, 1024, 1, "f16.pad>"),
    Row("f16_generic", F16, 72, 36, 40, 3, "f16.generic"),
    Row("f16_staged", F16, 61, 30, 19, 1, "stage/c>", ab="stage/c=seed>"),
    # aligned views, N % 4 != 0, N < 8: a Gemv with N right-hand sides -- for (1, 0) only
    Row("f16_as_gemv", F16, 512, 256, 3, 1, "gemv>", ab="f16.", not_ab="gemv>", dense_only=True),
    # ---- f32 (gemm_f32.hip, gemm_f32_mid.hip, gemm_f32_skinny.hip) ----
    Row("f32_mid_unsplit", F32, 64, 512, 16384, 1, "f32.mid64x64/ns=1"),
    Row("f32_mid_split", F32, 64, 4096, 4096, 1, ("f32.mid64x64/ns=", "splitk.reduce/ns=")),
    Row("f32_mid_forced", F32, 1024, 256, 1024, 1, "f32.mid128x64/ns=1", {"f32_mid": 128064}),
    Row("f32_mid_split_forced", F32, 256, 4096, 256, 1, "f32.mid64x64/ns=4 splitk.reduce/ns=4", {"f32_mid": 64064, "f32_mid_split": 4}),
    # few rows, many columns: the transposed product -- beta != 0 needs the old output inside the product, so those calls go elsewhere
    Row("f32_fewrow", F32, 96, 256, 8192, 1, "f32.fewrow>", ab="f32.", not_ab="fewrow"),
    Row("f32_fewrow_skinnyT", F32, 32, 512, 4096, 1, "f32.skinnyT/", ab="f32.", not_ab="skinnyT"),
    Row("f32_skinny", F32, 16384, 128, 16, 1, "f32.skinny/ns=1"),
    Row("f32_skinny_split", F32, 4096, 1024, 16, 1, "f32.skinny/ns=8 splitk.reduce/ns=8"),
    Row("f32_skinny_panels", F32, 512, 512, 512, 1, "f32.skinny/p=8,", {"f32_panels": 1}),
    Row("f32_big", F32, 4096, 256, 4096, 1, "f32.big/ns=1", {"f32_mid": 0, "f32_panels": 0}),
    Row("f32_big_splitk", F32, 512, 4096, 512, 1, "f32.big/ns=16 splitk.reduce/ns=16", {"f32_mid": 0, "f32_panels": 0}),
    Row("f32_big_tail", F32, 4352, 1024, 2048, 1, "f32.big/ns=1 f32.bigtail/ns=8 f32.tail_reduce", {"f32_mid": 0, "f32_panels": 0}),
    Row("f32_staged", F32, 61, 30, 19, 1, "stage/c>", ab="stage/c=seed>"),
    Row("f32_as_gemv", F32, 512, 256, 3, 1, "gemv>", ab="f32.", not_ab="gemv>", dense_only=True),
]
CASES = [pytest.param(r, tr, id=f"{r.name}-{'tr' if tr else 'nn'}") for r in LEAVES for tr in r.variants]


@pytest.fixture
def knobs(gpu):
    """Sets a row's knobs (wg_ctx_set_tuning) and restores them afterwards, as tests/test_gpu_parity.py's f16_tile does."""
    saved = {}

    def set_(d, inst=None):
        for k, v in d.items():
            if inst is None or inst is gpu:
                saved.setdefault(k, gpu.set_tuning(k, v))
            else:  # (a context of the test's own: restored, or closed, by the test)
                inst.set_tuning(k, v)

    yield set_
    for k, v in saved.items():
        gpu.set_tuning(k, v)


def _upload(gpu, flat):
    wg = _wg()
    return wg.TensorBuilder.tensor((flat.size,), S_STORAGE).build_init(gpu.device(), flat, flat.dtype.type)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32 if x.dtype.itemsize == 4 else np.uint16)


class OutView:
    """An output view inside a buffer filled with SENTINEL: `dense` (offset 0, ld = M, matrices back to back) or odd (offset 1, ld = M + 3 (f16) / M + 5 (f32),
    7 elements between matrices); 37 sentinel elements after the last one."""

    def __init__(self, gpu, dtype, M, N, mats, dense):
        self.ld = M if dense else M + (3 if dtype == F16 else 5)
        self.off = 0 if dense else 1
        self.batch = self.ld * N + (0 if dense else 7)
        self.size = self.off + self.batch * mats + 37
        self.idx = (self.off + np.arange(M)[:, None, None] + np.arange(N)[None, :, None] * self.ld + np.arange(mats)[None, None, :] * self.batch)
        self.mask = np.ones(self.size, bool)
        self.mask[self.idx.ravel()] = False
        self.base = np.full(self.size, SENTINEL[dtype]).view(dtype)
        self.gpu, self.dtype = gpu, dtype
        self.buf = _upload(gpu, self.base.copy())
        wg = _wg()
        self.shape = wg.ViewShape((M, N, mats), self.ld, self.batch, self.off)

    def fill(self, vals):
        """The view's elements = vals (M x N x mats), the rest the sentinel."""
        flat = self.base.copy()
        flat[self.idx] = vals
        self.gpu.queue().write_buffer(self.buf, 0, flat)

    def read(self, what):
        flat = self.buf.read(self.gpu.device())
        assert np.array_equal(_bits(flat[self.mask]), _bits(self.base[self.mask])), f"{what}: wrote outside the output view"
        return flat[self.idx]


def _gemm(gpu, tr, dtype, out, a, ash, b, bsh, alpha=None, beta=None):
    wg, L = _wg(), _lib()
    variant = int(wg.GemmVariant.GemmTr if tr else wg.GemmVariant.Gemm)
    dt = wg.wgcore.wg_dtype(dtype)
    if alpha is None:
        L.check(L.lib.wg_gemm(gpu._ctx.handle, variant, dt, out.buf._h, out.shape.to_c(), a._h, ash.to_c(), b._h, bsh.to_c()))
    else:
        L.check(L.lib.wg_gemm_ex(gpu._ctx.handle, variant, dt, float(alpha), float(beta), out.buf._h, out.shape.to_c(), a._h, ash.to_c(), b._h, bsh.to_c()))


def _f16_normal(x):
    # (from 2^-13 on: an accumulator just below 2^-14 rounds UP to that normal f16 on the subnormals' grid, while twice it rounds on the normals' finer one)
    return np.abs(x.astype(np.float32)) >= np.float32(2.0 ** -13)


@pytest.mark.parametrize("row,tr", CASES)
def test_epilogue_leaf(gpu, knobs, row, tr, record_property):
    wg = _wg()
    dtype, M, K, N, mats = row.dtype, row.M, row.K, row.N, row.mats
    knobs(row.knobs)
    gpu.take_path()  # (whatever earlier tests left)
    rng = np.random.default_rng(M * 7 + K * 5 + N * 3 + mats + int(tr))
    a = (rng.random((mats, M * K), dtype=np.float32) * 2 - 1).astype(dtype)  # op(A) stored K x M (GemmTr) or M x K, column-major, matrices back to back
    b = (rng.random((mats, K * N), dtype=np.float32) * 2 - 1).astype(dtype)
    ta, tb = _upload(gpu, a.ravel()), _upload(gpu, b.ravel())
    ash = wg.ViewShape(((K, M) if tr else (M, K)) + (mats,), K if tr else M, M * K, 0)
    bsh = wg.ViewShape((K, N, mats), K, K * N, 0)
    A = np.stack([a[z].reshape(((M, K) if tr else (K, M))).T.astype(np.float64) for z in range(mats)], -1)  # column-major -> [row, col, mat]
    A = np.transpose(A, (1, 0, 2)) if tr else A
    B = np.stack([b[z].reshape((N, K)).T.astype(np.float64) for z in range(mats)], -1)
    truth = np.stack([A[:, :, z] @ B[:, :, z] for z in range(mats)], -1)
    sabs = np.stack([np.abs(A[:, :, z]) @ np.abs(B[:, :, z]) for z in range(mats)], -1)
    gate = U.f32_gate(K, sabs) + (2.0 ** -11 * np.abs(truth) + 2.0 ** -25 if dtype == F16 else 0.0)
    c0 = (rng.random((M, N, mats), dtype=np.float32) * 2 - 1).astype(dtype)
    nan_inf = np.resize(np.array([np.nan, np.inf, -np.inf], dtype), (M, N, mats))
    eps = 2.0 ** -10 if dtype == F16 else 2.0 ** -23
    logs = []
    for dense in (True, False):
        view = "dense" if dense else "odd"
        check_leaf = dense or not row.dense_only
        out = OutView(gpu, dtype, M, N, mats, dense)
        # 1. Gemm into NaN
        out.fill(np.full((M, N, mats), np.nan, dtype))
        _gemm(gpu, tr, dtype, out, ta, ash, tb, bsh)
        log1 = gpu.take_path()
        R = out.read(f"gemm {view}")
        logs.append(f"{view}: {log1}")
        if check_leaf:
            assert Row.took(row.leaf, log1), f"{row.name} {view}: expected the leaf {row.leaf!r}, the call took {log1!r}"
        assert not np.isnan(R).any(), f"{view}: {np.isnan(R).sum()} NaN left in the output"
        err = np.abs(R.astype(np.float64) - truth)
        assert (err <= gate).all(), f"gemm {view} [{log1}]: worst err/tol {(err / gate).max():.3g}"
        # 2. gemm_ex(1, 0) into NaN / +-Inf: the same bits, the same kernels
        out.fill(nan_inf)
        _gemm(gpu, tr, dtype, out, ta, ash, tb, bsh, 1.0, 0.0)
        log2 = gpu.take_path()
        U.assert_bits_equal(out.read(f"gemm_ex(1, 0) {view}"), R, f"gemm_ex(1, 0) {view} vs gemm [{log2}]")
        assert log2 == log1, f"gemm_ex(1, 0) {view} took {log2!r}, gemm {log1!r}"
        # 3. gemm_ex(alpha, 0) into NaN: beta = 0 reads nothing, alpha scales the accumulator once
        alpha3 = -1.5 if dtype == F32 else 2.0
        out.fill(np.full((M, N, mats), np.nan, dtype))
        _gemm(gpu, tr, dtype, out, ta, ash, tb, bsh, alpha3, 0.0)
        log3 = gpu.take_path()
        got = out.read(f"gemm_ex({alpha3}, 0) {view}")
        logs.append(f"{view} ({alpha3}, 0): {log3}")
        if log3 == log1:
            if dtype == F32:
                U.assert_bits_equal(got, (np.float32(alpha3) * R).astype(F32), f"gemm_ex({alpha3}, 0) {view} vs fl32(alpha R) [{log3}]")
            else:
                ok = _f16_normal(R) & _f16_normal(got)
                U.assert_bits_equal(got[ok], (F16(alpha3) * R)[ok], f"gemm_ex({alpha3}, 0) {view} vs alpha R16 [{log3}]")
        elif check_leaf:
            assert Row.took(row.ab, log3, row.not_ab), f"{row.name} {view} ({alpha3}, 0): took {log3!r}"
        tol = abs(alpha3) * gate + eps * np.abs(alpha3 * truth)
        err = np.abs(got.astype(np.float64) - alpha3 * truth)
        assert (err <= tol).all(), f"gemm_ex({alpha3}, 0) {view} [{log3}]: worst err/tol {(err / tol).max():.3g}"
        # 4. gemm_ex(alpha, beta) on C0
        for alpha, beta in AB:
            out.fill(c0)
            _gemm(gpu, tr, dtype, out, ta, ash, tb, bsh, alpha, beta)
            log4 = gpu.take_path()
            got = out.read(f"gemm_ex({alpha}, {beta}) {view}")
            logs.append(f"{view} ({alpha}, {beta}): {log4}")
            if check_leaf:
                assert Row.took(row.ab, log4, row.not_ab), \
                    f"{row.name} {view} ({alpha}, {beta}): expected {row.ab!r}{'' if row.not_ab is None else ' without ' + repr(row.not_ab)}, took {log4!r}"
            if log4 == log1 and dtype == F32:
                want = U.fmaf_f32(np.float32(beta), c0, (np.float32(alpha) * R).astype(F32))
                U.assert_bits_equal(got, want, f"gemm_ex({alpha}, {beta}) {view} vs fmaf(beta, C0, fl32(alpha R)) [{log4}]")
            c64 = c0.astype(np.float64)
            want64 = alpha * truth + beta * c64
            tol = abs(alpha) * gate + eps * (np.abs(alpha * truth) + np.abs(beta * c64))
            err = np.abs(got.astype(np.float64) - want64)
            assert (err <= tol).all(), f"gemm_ex({alpha}, {beta}) {view} [{log4}]: worst err/tol {(err / tol).max():.3g}"
    record_property("leaf_logs", " | ".join(logs))
    print(f"\n{row.name} {'tr' if tr else 'nn'}: " + " | ".join(logs))


# --------------------------------------------------------------------------------------------------------
# The f32 launcher executes its plan (gemm32_plan.hip): the real launch log is the planner's, leaf by leaf
# --------------------------------------------------------------------------------------------------------
def _plan32(tr, M, K, N, mats, cus, knobs):
    """(plan, tags) of wg_debug_gemm32_plan for the product on dense views."""
    L = _lib()
    q, p, buf = L.Gemm32QueryC(), L.Gemm32PlanC(), ctypes.create_string_buffer(256)
    q.trans, q.M, q.N, q.K, q.nmats = int(tr), M, N, K, mats
    q.lda, q.ldb, q.ldc = (K if tr else M), K, M
    q.a_batch, q.b_batch, q.c_batch = M * K, K * N, M * N
    q.alpha, q.beta, q.cus = 1.0, 0.0, cus
    q.mid, q.mid_split, q.skinny, q.panels = knobs
    L.check(L.lib.wg_debug_gemm32_plan(ctypes.byref(q), ctypes.byref(p), buf, len(buf), None))
    return p, buf.value.decode()


F32_KNOBS = ("f32_mid", "f32_mid_split", "f32_skinny", "f32_panels")
# the context's defaults first; then, as the rows of LEAVES do, the mid family and the panels off (the 256 x 128 tiles on products of a test's size) and the panels forced
F32_KNOB_SETS = ((-1, 0, -1, -1), (0, 0, -1, 0), (-1, 0, -1, 1))


def _smallest_query_per_leaf(cus):
    """kind of plan -> (knobs, variant, M, K, N, matrices, tags): for every leaf of the f32 launcher -- and, within a leaf, with and without a K cut, a cut-up tail, a
    copy of op(m1) -- the smallest product (by M N K matrices, below 2^33 flop) of a grid of sizes that the planner sends there on `cus` compute units."""
    L, best = _lib(), {}
    sizes = (4, 16, 32, 48, 64, 96, 128, 256, 512, 1024, 2048, 4096, 4352, 8192)
    for knobs, tr, mats, M, N, K in itertools.product(F32_KNOB_SETS, (False, True), (1, 4), sizes, sizes, (32, 128, 256, 512, 1024, 4096)):
        if 2 * M * N * K * mats >= 2 ** 33:
            continue
        p, log = _plan32(tr, M, K, N, mats, cus, knobs)
        leaf = L.GEMM32_LEAVES[p.leaf]
        if leaf in ("nothing", "unsupported"):
            continue
        kind, size = (leaf, p.nsplit > 1, p.tail_r > 0, bool(p.copy_a)), M * N * K * mats
        if kind not in best or size < best[kind][0]:
            best[kind] = (size, knobs, tr, M, K, N, mats, log)
    return {k: v[1:] for k, v in best.items()}


def test_f32_executor_logs_its_plan(gpu, knobs):
    """The smallest product the planner sends to each leaf, on the whole chip and on 8 CUs: the launch log is exactly wg_debug_gemm32_plan's tags (with
    tests/test_gemm32_plan_host.py, which holds the planner to the launcher it replaced, this pins the executor to the plan), and the result is the f64 product
    within the file's f32 bound."""
    wg = _wg()
    small = wg.GpuInstance.new(0, cu_count=8)
    try:
        for cus, inst in ((int(gpu.adapter()["compute_units"]), gpu), (8, small)):
            found = _smallest_query_per_leaf(cus)
            assert {k[0] for k in found} == {"mid", "skinny", "skinny_panels", "skinny_t", "fewrow", "big"}, sorted(found)
            assert len(found) >= 10, sorted(found)
            inst.take_path()
            for kind, (kn, tr, M, K, N, mats, want) in sorted(found.items()):
                knobs(dict(zip(F32_KNOBS, kn)), inst)
                rng = np.random.default_rng(M * 7 + K * 5 + N * 3 + mats + int(tr))
                a = rng.random((mats, M * K), dtype=np.float32) * 2 - 1
                b = rng.random((mats, K * N), dtype=np.float32) * 2 - 1
                ta, tb = _upload(inst, a.ravel()), _upload(inst, b.ravel())
                ash = wg.ViewShape(((K, M) if tr else (M, K)) + (mats,), K if tr else M, M * K, 0)
                bsh = wg.ViewShape((K, N, mats), K, K * N, 0)
                out = OutView(inst, F32, M, N, mats, dense=True)
                out.fill(np.full((M, N, mats), np.nan, F32))
                _gemm(inst, tr, F32, out, ta, ash, tb, bsh)
                log = inst.take_path()
                what = f"{kind} {'tr' if tr else 'nn'} {M} x {K} x {N} x {mats} on {cus} CUs"
                assert log == want, f"{what}: the plan logs {want!r}, the launch {log!r}"
                R = out.read(what).astype(np.float64)
                for z in range(mats):
                    A = a[z].astype(np.float64).reshape((M, K) if tr else (K, M))
                    A = A if tr else A.T  # (column-major K x M read row-major is op(A); column-major M x K read row-major is its transpose)
                    B = b[z].astype(np.float64).reshape((N, K)).T
                    err, gate = np.abs(R[:, :, z] - A @ B), U.f32_gate(K, np.abs(A) @ np.abs(B))
                    assert (err <= gate).all(), f"{what} [{log}]: worst err/tol {(err / gate).max():.3g}"
    finally:
        for k, v in zip(F32_KNOBS, F32_KNOB_SETS[0]):
            small.set_tuning(k, v)
        small.sync()
        small.close()


# --------------------------------------------------------------------------------------------------------
# Gemv on matrix views that are not vec4-aligned (gemv_any.hip), many right-hand sides
# --------------------------------------------------------------------------------------------------------
def _gemv_case(gpu, dtype, tr, R, C, ld, om, nrhs, mats, seed, aligned_twin=True):
    wg = _wg()
    rng = np.random.default_rng(seed)
    vlen, olen = (R, C) if tr else (C, R)
    mb = ld * C + 3  # a gap between matrices
    pm = (rng.random(om + mb * mats + 5, dtype=np.float32) - 0.5).astype(dtype)
    for z in range(mats):  # the parent's element past every column's end must not leak in
        for c in range(C):
            if ld > R:
                pm[om + z * mb + c * ld + R] = np.inf
    vld, vb = vlen + 1, (vlen + 1) * nrhs + 2
    pv = (rng.random(3 + vb * mats, dtype=np.float32) - 0.5).astype(dtype)
    m_idx = om + np.arange(R)[:, None, None] + np.arange(C)[None, :, None] * ld + np.arange(mats)[None, None, :] * mb
    v_idx = 3 + np.arange(vlen)[:, None, None] + np.arange(nrhs)[None, :, None] * vld + np.arange(mats)[None, None, :] * vb
    A = pm[m_idx].astype(np.float64)
    A = np.transpose(A, (1, 0, 2)) if tr else A
    X = pv[v_idx].astype(np.float64)
    truth = np.einsum("rkz,knz->rnz", A, X, optimize=True)
    sabs = np.einsum("rkz,knz->rnz", np.abs(A), np.abs(X), optimize=True)
    tol = U.f32_gate(vlen, sabs) + (2.0 ** -11 * np.abs(truth) + 2.0 ** -25 if dtype == F16 else 0.0)
    tm, tv = _upload(gpu, pm), _upload(gpu, pv)
    m_view = wg.GpuTensorView(wg.ViewShape((R, C, mats), ld, mb, om), tm, 2)
    v_view = wg.GpuTensorView(wg.ViewShape((vlen, nrhs, mats), vld, vb, 3), tv, 2)
    out = OutView(gpu, dtype, olen, nrhs, mats, dense=False)
    out.fill(np.full((olen, nrhs, mats), np.nan, dtype))
    o_view = wg.GpuTensorView(out.shape, out.buf, 2)
    variant = wg.GemvVariant.GemvTr if tr else wg.GemvVariant.Gemv
    gemv, shapes = wg.Gemv.from_device(gpu.device()), wg.ViewShapeBuffers()
    gpu.take_path()
    enc = gpu.device().create_command_encoder()
    with enc.compute_pass("gemv", None) as p:
        gemv.dispatch_generic(gpu.device(), shapes, p, o_view, m_view, v_view, variant)
    gpu.queue().submit([enc.finish()])
    got = out.read("gemv on an unaligned matrix view").astype(np.float64)
    log = gpu.take_path()
    assert "gemv_any/" in log, f"expected the any-alignment Gemv, the call took {log!r}"
    err = np.abs(got - truth)
    assert np.isfinite(got).all() and (err <= tol).all(), f"gemv [{log}]: worst err/tol {(err / tol).max():.3g}"
    if aligned_twin:  # the same numbers in an aligned matrix (ld % 4 == 0, offset 0): its kernels, within the bound of the same truth, and close to each other
        ld2 = (R + 3) // 4 * 4
        pm2 = np.zeros(ld2 * C * mats, dtype)
        pm2[(np.arange(R)[:, None, None] + np.arange(C)[None, :, None] * ld2 + np.arange(mats)[None, None, :] * ld2 * C).ravel()] = pm[m_idx].ravel()
        tm2 = _upload(gpu, pm2)
        m2_view = wg.GpuTensorView(wg.ViewShape((R, C, mats), ld2, ld2 * C, 0), tm2, 2)
        out2 = OutView(gpu, dtype, olen, nrhs, mats, dense=True)
        enc = gpu.device().create_command_encoder()
        with enc.compute_pass("gemv", None) as p:
            gemv.dispatch_generic(gpu.device(), shapes, p, wg.GpuTensorView(out2.shape, out2.buf, 2), m2_view, v_view, variant)
        gpu.queue().submit([enc.finish()])
        got2 = out2.read("gemv on the aligned twin").astype(np.float64)
        gpu.take_path()
        assert (np.abs(got2 - truth) <= tol).all() and (np.abs(got2 - got) <= 2 * tol).all()
    return log


@pytest.mark.parametrize("dtype", [F32, F16])
@pytest.mark.parametrize("tr", [False, True])
@pytest.mark.parametrize("mats", [1, 3])
@pytest.mark.parametrize("nrhs", [4, 8, 9, 16, 64, 257])
def test_gemv_any_many_rhs(gpu, dtype, tr, mats, nrhs):
    """1 .. 257 right-hand sides on a matrix view at an odd offset with an odd leading dimension: against f64 and against the same data in an aligned
    matrix (whose Gemv from 9 right-hand sides on runs on the Gemm kernels)."""
    _gemv_case(gpu, dtype, tr, 301, 203, 305, 1, nrhs, mats, seed=nrhs * 10 + mats + int(tr))


@pytest.mark.parametrize("tr", [False, True])
def test_gemv_any_more_than_65535_rhs(gpu, tr):
    """70001 right-hand sides (the launch grid's z limit is 65535): the pairs (matrix, right-hand side) go in chunks."""
    log = _gemv_case(gpu, F32, tr, 37, 29, 37, 1, 70001, 1, seed=70001 + int(tr), aligned_twin=False)
    assert "chunks=2" in log, log


@pytest.mark.parametrize("tr", [False, True])
def test_gemv_any_more_than_65535_matrices_x_rhs(gpu, tr):
    """30000 matrices x 3 right-hand sides."""
    log = _gemv_case(gpu, F32, tr, 12, 9, 13, 1, 3, 30000, seed=30000 + int(tr), aligned_twin=False)
    assert "chunks=2" in log, log
