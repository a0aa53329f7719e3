"""Every leaf at the ends of the exponent range: subnormal operands, subnormal results and their ties, and the epilogue's second rounding. No tolerance
appears in this file: every expected value is fixed to the bit by construction (tests/_util.py; the models are checked on the CPU by
tests/test_special_model.py, which also asserts every share and witness count below for every row).

Operands are scaled integers, A = I_A 2^ea and B = I_B 2^eb with I_A, I_B in [-8, 8] (tests/test_gpu_operands.py's distribution): every product and partial
sum is an integer below 2^24 times 2^(ea + eb), so with ea + eb >= -149 the f32 accumulation is exact in any order and any split of K, and the contract
("f32 accumulation, one rounding") fixes every output bit. Per row of LEAVES, EXTRA_LEAVES, RM_LEAVES and GEMV_LEAVES, per variant and element type (the
f16 rows as f16 and as bf16), on the dense and on the row's odd layout in NaN-filled parents:
  sub_in    every element of A a subnormal of its type (2^-24, 2^-133, 2^-149), B scaled up so that the results are normal; then the roles swapped. A leaf
            that drops subnormal inputs returns zeros.
  sub_out   normal operands, ea + eb = s chosen per row ON THE MODEL (U.plan_straddle) so that the results straddle the smallest normal: every second row
            of A carries an anchor a[i, 0] b[0, j] = +-2^t with 2^t 2^s the smallest normal, the other rows stay small. At least 1/4 of the outputs are
            nonzero subnormals, 1/10 normal and (16 bits: s lies below the subnormal quantum) 1/20 exact ties on the subnormal grid. An f32 output cannot
            tie (the accumulation is exact only on the 2^-149 grid): its ties come from gemm_ex(0.5, .) below.
  gemm_ex   both cases with the pairs AB_EXACT on a C0 of scaled integers (subnormal where the output is), against the contract's model
            narrow(fmaf_f32(beta, c, fl32(alpha acc))) (U.epilogue_model).
  second    16-bit rows: an alpha, then a beta, that are generic f32 values (alpha acc needs more than 24 bits), once with outputs in the normal range and
            once at the sub_out scale. The scalars come from a deterministic search over a fixed list (U.plan_witnesses) for WITNESSES: outputs where the
            contract's value differs from the single rounding of the exact alpha acc + beta c, which is what a fused multiply-add-narrow gives. At least
            one per row, at least 8 from 2^16 outputs on, for (alpha, 0) and (alpha, beta) separately. wg_gemm_rm has no alpha / beta: its rows take
            the first three cases only.
Mixed Gemv (a 16-bit matrix, f32 vectors and result) takes sub_in on the matrix and on the vector and sub_out in f32, on the rows of
tests/test_gpu_gemv_mixed.py. Then Reduce over REDUCE_PATHS, OpAssign and Axpy on subnormals, the smallest normals, gradual and complete underflow and
subnormal quotients. Every call asserts the leaf it reaches from the launch log.
A row with 2^23 outputs or more keeps its shape and takes fewer cases (the odd layout and gemm_ex, with two pairs of AB_EXACT, on sub_out alone; the
swapped roles on its first variant; the (alpha, beta) call alone in the normal range of `second`): the module then costs the GPU suite no more than tests/test_gpu_operands.py does."""
import numpy as np
import pytest

import _util as U
from test_gpu_epilogue import F16, F32, LEAVES, Row, _lib, _wg, knobs  # noqa: F401  (knobs: the fixture)
from test_gpu_gemv_mixed import CASES as MIXED_CASES
from test_gpu_operands import AB_EXACT, EXTRA_LEAVES, GEMV_LEAVES, LAYOUTS, ODD_LEAF, REDUCE_PATHS, RM_LEAVES, _ints

pytestmark = pytest.mark.gpu

S_STORAGE = 128 | 4 | 8
NAN = {"f32": 0x7FC00000, "f16": 0x7E00, "bf16": 0x7FC0}
SENTINEL = {"f32": 0x7FC5A5A5, "f16": 0x7E5A, "bf16": 0x7FC5}  # quiet NaNs with a payload no kernel writes
# sub_in: (exponent of the subnormal operand, exponent of the other one): [-8, 8] 2^12 are f16 values, and every result is normal
SUB_IN = {"f16": (-24, 12), "bf16": (-133, 100), "f32": (-149, 100)}


def kinds_of(dtype):
    return ("f32",) if dtype == F32 else ("f16", "bf16")


def code_of(kind):
    L = _lib()
    return {"f32": L.WG_F32, "f16": L.WG_F16, "bf16": L.WG_BF16}[kind]


def tags_of(tags, kind):
    """A row's tags for `kind`: the bf16 log is the f16 one with the element prefix replaced (include/wgebra_hip.h)."""
    if tags is None or kind != "bf16":
        return tags
    return tags.replace("f16.", "bf16.") if isinstance(tags, str) else tuple(t.replace("f16.", "bf16.") for t in tags)


def upload_bits(gpu, kind, bits):
    wg = _wg()
    bits = np.ascontiguousarray(bits, U.BITS_T[kind]).ravel()
    dt = {"f32": np.float32, "f16": np.float16}.get(kind) or wg.bfloat16
    return wg.TensorBuilder.tensor((bits.size,), S_STORAGE).build_init(gpu.device(), bits.view(dt), dt)


class Held:
    """A logical matrix X (r x c x mats, float64 values of `kind`; None: NaN) stored column-major as X, or as X^T (`tr`), as bit patterns inside a parent
    buffer that is NaN everywhere else (`sentinel`: the payload no kernel writes). `layout`: a name of LAYOUTS or (offset, extra leading dimension, gap
    between matrices, elements after the end)."""

    def __init__(self, gpu, X, kind, layout, shape=None, tr=False, sentinel=False, ld_mult=1, bits=None):
        rs, cs, z = ((X if bits is None else bits).shape if shape is None else shape)
        if tr:
            rs, cs = cs, rs
        off, pad, gap, tail = LAYOUTS[layout] if isinstance(layout, str) else layout
        if pad is None:
            pad = 1 if rs % 2 == 0 else 2
        ld = -(-max(rs + pad, 1) // ld_mult) * ld_mult
        self.dims, self.ld, self.off, self.batch = (rs, cs, z), ld, off, ld * cs + gap
        self.fill = U.BITS_T[kind]((SENTINEL if sentinel else NAN)[kind])
        flat = np.full(off + self.batch * z + tail, self.fill)
        if X is not None:
            bits = U.narrow_bits(kind, X)
            assert np.array_equal(U.widen_bits(kind, bits), X), "an operand is not a value of its type"
        if bits is not None:  # (given as bits: checked where they were made)
            self._view(flat)[...] = np.transpose(bits, (2, 0, 1) if tr else (2, 1, 0))
        self.tr, self.gpu, self.kind = tr, gpu, kind
        self.buf = upload_bits(gpu, kind, flat)
        wg = _wg()
        self.cm = wg.ViewShape((rs, cs, z), ld, self.batch, off)  # the column-major view of the stored matrix
        self.rm = wg.ViewShape((cs, rs, z), ld, self.batch, off)  # the same memory as a row-major view

    def _view(self, flat):
        """The stored matrix inside the flat parent, as [matrix, column, row] (strides: no index array of the parent's size)."""
        (rs, cs, z), it = self.dims, flat.itemsize
        return np.lib.stride_tricks.as_strided(flat[self.off:], (z, cs, rs), (self.batch * it, self.ld * it, it))

    def read(self, what):
        flat = np.asarray(self.buf.read(self.gpu.device())).view(U.BITS_T[self.kind])
        (rs, cs, z), end = self.dims, self.off + self.batch * self.dims[2]
        v = self._view(flat)
        if self.ld == rs and self.batch == rs * cs:  # nothing between the columns: the parent's head and tail
            S = np.transpose(v, (1, 2, 0) if self.tr else (2, 1, 0))
            clean = (flat[:self.off] == self.fill).all() and (flat[end:] == self.fill).all()
        else:
            flat = flat.copy()
            v = self._view(flat)
            S = np.transpose(v, (1, 2, 0) if self.tr else (2, 1, 0)).copy()
            v[...] = self.fill
            clean = (flat == self.fill).all()
        assert clean, f"{what}: wrote outside the output view"
        return S


def assert_bits(got, want, zero, what):
    """Bit equality; where the expected f32 value is an exact zero (`zero`: the mask, or the exact values), a zero of either sign (the sign of an exact
    zero sum is open)."""
    if np.array_equal(got, want):
        return
    zero = zero if zero.dtype == bool else zero == 0
    sign = np.array(1 << (8 * got.dtype.itemsize - 1), got.dtype)
    ok = (got == want) | (zero & ((got & ~sign) == 0))
    if not ok.all():
        i = np.argwhere(~ok)
        raise AssertionError(f"{what}: {len(i)} of {got.size} elements differ bitwise; first at {tuple(i[0])}: got {got[tuple(i[0])]:#x}, expected {want[tuple(i[0])]:#x}")


# --------------------------------------------------------------------------------------------------------
# operands and plans: shared with tests/test_special_model.py, which asserts them for every row on the CPU
# --------------------------------------------------------------------------------------------------------
_PLAN = {}


def base_operands(key, M, K, N, Z):
    """(IA, IB, P0, anchored, IC) per row, cached for the row in hand: the integers of tests/test_gpu_operands.py with column 0 of IA zero (the anchor's
    place in sub_out), their exact product P0, +-1 on every second row (where sub_out puts its anchor), and the integers of C0."""
    if _PLAN.get("key") != key:
        rng = np.random.default_rng(sum(map(ord, key)) + M * 7 + K * 5 + N * 3 + Z)
        IA, IB, IC = _ints(rng, (M, K, Z)), _ints(rng, (K, N, Z)), _ints(rng, (M, N, Z))
        IA[:, 0, :] = 0.0
        anchored = np.zeros((M, 1, 1))
        anchored[1::4], anchored[3::4] = 1.0, -1.0
        _PLAN.clear()
        _PLAN.update(key=key, IA=IA, IB=IB, IC=IC, IC8=(IC + 8).astype(np.int32), P0=U.int_product(IA, IB), anchored=anchored)
    return _PLAN


def sub_out_operands(d, kind):
    """(IA, IB, P, s) of sub_out for `kind`: the anchor 2^t = 2^ceil(t / 2) (column 0 of every second row of IA, signs alternating) times 2^floor(t / 2)
    (row 0 of IB), t and s from U.plan_straddle; cached beside the row's operands."""
    if ("out", kind) not in d:
        j, t, s, shares = U.plan_straddle(kind, d["P0"], d["anchored"])
        IA, IB = d["IA"].copy(), d["IB"].copy()
        IA[:, 0:1, :] = d["anchored"] * 2.0 ** -(-t // 2)
        IB[0, :, :] = 2.0 ** (t // 2)
        d["out", kind] = (IA, IB, d["P0"] + d["anchored"] * 2.0 ** t, s)
    return d["out", kind]


def cases_of(d, kind):
    """(name, IA, ea, IB, eb, P, exponent of C0) per case."""
    lo, hi = SUB_IN[kind]
    IA, IB, P, s = sub_out_operands(d, kind)
    return [("sub_in", d["IA"], lo, d["IB"], hi, d["P0"], lo + hi), ("sub_in_swapped", d["IA"], hi, d["IB"], lo, d["P0"], lo + hi),
            ("sub_out", IA, s // 2, IB, s - s // 2, P, U.QUANTUM[kind])]


def second_plan(d, kind, rng_name):
    """(P, s, exponent of C0, alpha, beta, witnesses of (alpha, 0), witnesses of (alpha, beta)) for the second-rounding test in the normal range (acc = P0)
    or at the sub_out scale."""
    if ("second", kind, rng_name) not in d:
        P, s, ce = (d["P0"], 0, 0) if rng_name == "normal" else (sub_out_operands(d, kind)[2], sub_out_operands(d, kind)[3], U.QUANTUM[kind])
        need = 8 if P.size >= 2 ** 16 else 1
        alpha, w0 = U.plan_witnesses(kind, P, s, need)
        beta, w1 = U.plan_witnesses(kind, P, s, need, alpha=alpha, c_int=d["IC"], c_exp=ce)
        d["second", kind, rng_name] = (P, s, ce, alpha, beta, w0, w1)
    return d["second", kind, rng_name]


GEMM_ROWS = LEAVES + EXTRA_LEAVES + RM_LEAVES
GEMM_PARAMS = [pytest.param(r, tr, k, id=f"{r.name}-{'tr' if tr else 'nn'}-{k}") for r in GEMM_ROWS for tr in r.variants for k in kinds_of(r.dtype)]
SECOND_PARAMS = [pytest.param(r, tr, k, id=f"{r.name}-{'tr' if tr else 'nn'}-{k}") for r in LEAVES + EXTRA_LEAVES if r.dtype == F16 for tr in r.variants
                 for k in kinds_of(r.dtype)]
GEMV_PARAMS = [pytest.param(r, k, id=f"{r.name}-{k}") for r in GEMV_LEAVES for k in kinds_of(r.dtype)]
MIXED_PARAMS = [pytest.param(c, k, id=f"{c[0]}-{k}") for c in MIXED_CASES for k in ("f16", "bf16")]


# --------------------------------------------------------------------------------------------------------
# Gemm leaves
# --------------------------------------------------------------------------------------------------------
def _gemm_call(gpu, row, tr, kind, out, a, b, alpha=None, beta=None):
    wg, L = _wg(), _lib()
    h, dt = gpu._ctx.handle, code_of(kind)
    if getattr(row, "api", "cm") == "rm":
        L.check(L.lib.wg_gemm_rm(h, int(wg.GemmVariant.GemmTr), dt, out.buf._h, out.rm.to_c(), a.buf._h, a.rm.to_c(), b.buf._h, b.rm.to_c()))
        return
    variant = int(wg.GemmVariant.GemmTr if tr else wg.GemmVariant.Gemm)
    if alpha is None:
        L.check(L.lib.wg_gemm(h, variant, dt, out.buf._h, out.cm.to_c(), a.buf._h, a.cm.to_c(), b.buf._h, b.cm.to_c()))
    else:
        L.check(L.lib.wg_gemm_ex(h, variant, dt, float(alpha), float(beta), out.buf._h, out.cm.to_c(), a.buf._h, a.cm.to_c(), b.buf._h, b.cm.to_c()))


def _gemm_inputs(gpu, row, tr, kind, A, B, layout):
    rm = getattr(row, "api", "cm") == "rm"
    return Held(gpu, A, kind, layout, tr=tr and not rm), Held(gpu, B, kind, layout, tr=rm)  # (row-major K x M is the column-major M x K)


def _gemm_out(gpu, row, kind, shape, layout, c0=None):
    return Held(gpu, None, kind, layout, shape=shape, tr=getattr(row, "api", "cm") == "rm", sentinel=True, bits=c0)


def _c0_bits(d, kind, ce):
    """C0 = IC 2^ce as bits of `kind`, cached beside the row's operands."""
    if ("c0", kind, ce) not in d:
        c0 = np.ldexp(d["IC"], ce)
        d["c0", kind, ce] = U.narrow_bits(kind, c0)
        assert np.array_equal(U.widen_bits(kind, d["c0", kind, ce]), c0)
    return d["c0", kind, ce]


def _took_ab(row, kind, log, beta):
    """An (alpha, beta) call reached the row's leaf: its `ab` tags without `not_ab`, or -- beta == 0 alone -- the leaf of the plain call."""
    return Row.took(tags_of(row.ab, kind), log, tags_of(row.not_ab, kind)) or (beta == 0.0 and Row.took(tags_of(row.leaf, kind), log))


@pytest.mark.parametrize("row,tr,kind", GEMM_PARAMS)
def test_gemm_leaf_exponent_range(gpu, knobs, row, tr, kind):
    M, K, N, Z = row.M, row.K, row.N, row.mats
    knobs(row.knobs)
    gpu.take_path()
    d = base_operands(row.name, M, K, N, Z)
    heavy = M * N * Z >= 1 << 23  # (such a row takes fewer cases, never a smaller shape: see the header)
    for name, IA, ea, IB, eb, P, ce in cases_of(d, kind):
        if heavy and name == "sub_in_swapped" and tr != row.variants[0]:
            continue
        A, B = np.ldexp(IA, ea), np.ldexp(IB, eb)
        x, want = U.scaled_product(IA, IB, ea, eb, kind, P=P)
        if name != "sub_out":
            assert (np.abs(A) < 2.0 ** U.EMIN[kind]).all() if name == "sub_in" else (np.abs(B) < 2.0 ** U.EMIN[kind]).all()
            assert (np.abs(x[x != 0]) >= 2.0 ** U.EMIN[kind]).all() and (x != 0).mean() > 0.9, "sub_in: the results must be normal"
        for layout in ("odd", "dense")[heavy and name != "sub_out":]:
            a, b = _gemm_inputs(gpu, row, tr, kind, A, B, layout)
            out = _gemm_out(gpu, row, kind, (M, N, Z), layout)
            _gemm_call(gpu, row, tr, kind, out, a, b)
            log = gpu.take_path()
            leaf = tags_of(ODD_LEAF.get((row.name, tr), row.leaf) if layout == "odd" else row.leaf, kind)
            assert Row.took(leaf, log), f"{row.name} {name} {layout}: expected {leaf!r}, took {log!r}"
            assert_bits(out.read(name), want, x, f"{row.name} {kind} {name} {layout} [{log}]")
        if name == "sub_in_swapped" or getattr(row, "api", "cm") == "rm":
            continue
        c0 = _c0_bits(d, kind, ce)
        for alpha, beta in (AB_EXACT[:0] if name == "sub_in" else AB_EXACT[1::2]) if heavy else AB_EXACT:  # (a, b: the dense operands, the last of the loop above)
            out = _gemm_out(gpu, row, kind, (M, N, Z), "dense", c0=c0 if beta != 0.0 else None)
            _gemm_call(gpu, row, tr, kind, out, a, b, alpha, beta)
            log = gpu.take_path()
            assert _took_ab(row, kind, log, beta), f"{row.name} {name} ({alpha}, {beta}): took {log!r}"
            wbits, zero = U.epilogue_bits(kind, alpha, P, ea + eb, beta, d["IC"], ce, d["IC8"])
            assert_bits(out.read(name), wbits, zero, f"{row.name} {kind} {name} gemm_ex({alpha}, {beta}) [{log}]")


@pytest.mark.parametrize("row,tr,kind", SECOND_PARAMS)
def test_gemm_leaf_second_rounding(gpu, knobs, row, tr, kind):
    """narrow(fmaf_f32(beta, c, fl32(alpha acc))) with generic alpha and beta, on the leaf the (alpha, beta) call takes; the plan guarantees outputs that a
    single rounding of the exact alpha acc + beta c gets wrong (asserted on the model here too, from the bits the plan's scalars give)."""
    M, K, N, Z = row.M, row.K, row.N, row.mats
    knobs(row.knobs)
    gpu.take_path()
    d = base_operands(row.name, M, K, N, Z)
    for rng_name in ("normal", "sub_out"):
        P, s, ce, alpha, beta, w0, w1 = second_plan(d, kind, rng_name)
        IA, IB = (d["IA"], d["IB"]) if rng_name == "normal" else sub_out_operands(d, kind)[:2]
        a, b = _gemm_inputs(gpu, row, tr, kind, np.ldexp(IA, s // 2), np.ldexp(IB, s - s // 2), "dense")
        c0 = _c0_bits(d, kind, ce)
        heavy = M * N * Z >= 1 << 23  # (fewer cases, never a smaller shape: in the normal range the (alpha, beta) call alone, whose v is the (alpha, 0) call's)
        for al, be in ((alpha, 0.0), (alpha, beta))[heavy and rng_name == "normal":]:
            want, zero = U.epilogue_bits(kind, al, P, s, be, d["IC"], ce, d["IC8"])  # (its witnesses: second_plan, asserted there on the distinct values)
            out = _gemm_out(gpu, row, kind, (M, N, Z), "dense", c0=c0 if be != 0.0 else None)
            _gemm_call(gpu, row, tr, kind, out, a, b, al, be)
            log = gpu.take_path()
            assert _took_ab(row, kind, log, be), f"{row.name} {rng_name} ({al}, {be}): took {log!r}"
            if row.name == "f16_cont" and be == 0.0:  # (the continuous walk has an alpha epilogue of its own: beta == 0 must stay on it)
                assert "f16.cont" in log, log
            got = out.read(rng_name)
            assert_bits(got, want, zero, f"{row.name} {kind} {rng_name} gemm_ex({al}, {be}) [{log}], {w1 if be else w0} witnesses")


# --------------------------------------------------------------------------------------------------------
# Gemv leaves, and the mixed Gemv
# --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row,kind", GEMV_PARAMS)
def test_gemv_leaf_exponent_range(gpu, knobs, row, kind):
    wg, L = _wg(), _lib()
    Z = row.mats
    ro, k = (row.C, row.R) if row.tr else (row.R, row.C)
    knobs(row.knobs)
    gpu.take_path()
    d = base_operands("gemv" + row.name, ro, k, row.nrhs, Z)
    variant = int(wg.GemvVariant.GemvTr if row.tr else wg.GemvVariant.Gemv)
    for name, IA, ea, IB, eb, P, _ in cases_of(d, kind):
        x, want = U.scaled_product(IA, IB, ea, eb, kind, P=P)
        for layout in ("dense", "odd"):
            m = Held(gpu, np.ldexp(IA, ea), kind, layout, tr=row.tr, ld_mult=row.ld_mult if layout != "odd" else 1)  # (GemvTr: m = op(m)^T)
            vl = "odd" if row.vodd else layout
            v, out = Held(gpu, np.ldexp(IB, eb), kind, vl), Held(gpu, None, kind, vl, shape=(ro, row.nrhs, Z), sentinel=True)
            L.check(L.lib.wg_gemv(gpu._ctx.handle, variant, code_of(kind), out.buf._h, out.cm.to_c(), m.buf._h, m.cm.to_c(), v.buf._h, v.cm.to_c()))
            log = gpu.take_path()
            leaf, not_ = (row.odd, None) if layout == "odd" else (row.leaf, row.not_)
            assert Row.took(tags_of(leaf, kind), log, tags_of(not_, kind)), f"{row.name} {name} {layout}: expected {leaf!r}, took {log!r}"
            assert_bits(out.read(name), want, x, f"{row.name} {kind} {name} {layout} [{log}]")


def mixed_cases(d, kind):
    """(name, IA, ea, IB, eb, P): the matrix subnormal in its 16-bit type; the f32 vector subnormal (under an f16 matrix, whose largest power of two is 2^15,
    the results are then subnormal f32 values too); f32 results that straddle 2^-126 -- from normal operands under bf16, from a subnormal vector under
    f16, whose smallest normal is 2^-14."""
    lo, hi = SUB_IN[kind]
    IA, IB, P, s = sub_out_operands(d, "f32")
    ea = -14 if kind == "f16" else s // 2
    return [("sub_in_matrix", d["IA"], lo, d["IB"], hi, d["P0"]), ("sub_in_vector", d["IA"], hi, d["IB"], -149, d["P0"]), ("sub_out", IA, ea, IB, s - ea, P)]


@pytest.mark.parametrize("case,kind", MIXED_PARAMS)
def test_gemv_mixed_exponent_range(gpu, case, kind):
    wg, L = _wg(), _lib()
    name, tr, R, C, nrhs, Z, (moff, mpad), voff, tags = case
    k, ro = (R, C) if tr else (C, R)
    d = base_operands("mixed" + name, ro, k, nrhs, Z)
    variant = int(wg.GemvVariant.GemvTr if tr else wg.GemvVariant.Gemv)
    gpu.take_path()
    for cname, IA, ea, IB, eb, P in mixed_cases(d, kind):
        x, want = U.scaled_product(IA, IB, ea, eb, "f32", P=P)
        if cname != "sub_out":
            assert (np.abs(np.ldexp(IA, ea)) < 2.0 ** U.EMIN[kind]).all() if cname == "sub_in_matrix" else (np.abs(np.ldexp(IB, eb)) < 2.0 ** -126).all()
        m = Held(gpu, np.ldexp(IA, ea), kind, (moff, mpad, mpad, 8), tr=tr)
        v = Held(gpu, np.ldexp(IB, eb), "f32", (voff, voff, 0, 8))
        out = Held(gpu, None, "f32", (voff, voff, 0, 8), shape=(ro, nrhs, Z), sentinel=True)
        L.check(L.lib.wg_gemv_mixed(gpu._ctx.handle, variant, code_of(kind), out.buf._h, out.cm.to_c(), m.buf._h, m.cm.to_c(), v.buf._h, v.cm.to_c()))
        log = gpu.take_path()
        pos = 0
        for tag in tags:
            assert tag in log[pos:], f"{name}: expected {tags} in order, the call took {log!r}"
            pos = log.index(tag, pos)
        assert_bits(out.read(cname), want, x, f"mixed {name} {kind} {cname} [{log}]")


# --------------------------------------------------------------------------------------------------------
# Reduce
# --------------------------------------------------------------------------------------------------------
def reduce_cases(kind, n, rng):
    """(op name, case, x as exact float64 values of `kind`, expected exact float64 value before the one rounding, order-free) per case."""
    q, lo = U.QUANTUM[kind], 2.0 ** U.EMIN[kind]
    pos = rng.choice(n, 8, replace=False)
    out = []
    # Sum: integers on the subnormal grid, exact in any order (every partial sum stays below 2^24 quanta); one half of the vector is the other's negative in
    # another order, so that the total (3, and 5 more for an odd n) is a subnormal too
    I = _ints(rng, n)
    I[n // 2:2 * (n // 2)] = -I[:n // 2][rng.permutation(n // 2)]
    I[2 * (n // 2):] = 5.0
    I[pos[3]] += 3.0
    out.append(("Sum", "grid", np.ldexp(I, q), np.ldexp(I.sum(), q)))
    # Min / Max: the extreme is a subnormal (positive, negative), all-subnormal vectors, the smallest subnormal beside +-0
    big = np.where(rng.random(n) < 0.5, 1.0, 3.0)
    for sgn, op in ((1.0, "Min"), (-1.0, "Max")):  # the extreme of +-(1, 3, one subnormal) is that subnormal
        x = sgn * big
        x[pos[0]] = sgn * 5 * 2.0 ** q
        out.append((op, "positive extreme" if sgn > 0 else "negative extreme", x, x[pos[0]]))
        x = -sgn * big * 2.0 ** q * 2  # (op of values that are all subnormal, the extreme the odd one)
        x[pos[1]] = -sgn * 7 * 2.0 ** q
        out.append((op, "all subnormal", x, x[pos[1]]))
    z = np.where(rng.random(n) < 0.5, 0.0, -0.0)
    for op, v in (("Max", 2.0 ** q), ("Min", -(2.0 ** q))):  # the smallest subnormal beside +-0 is the extreme: canonicalised to zero, it would be lost
        x = z.copy()
        x[pos[2]] = v
        out.append((op, "beside zeros", x, v))
    # Prod: powers of two no greater than 1 whose product is an exact subnormal: every partial product is at least the final one, exact in any order
    e = np.zeros(n)
    e[pos[:6]] = (-q - 2) // 7
    e[pos[6]] = (-q - 2) - e.sum()
    assert (e >= 0).all() and e.sum() == -q - 2 and 2.0 ** -e.max() >= lo
    sg = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    out.append(("Prod", "subnormal product", sg * 2.0 ** -e, np.prod(sg) * 2.0 ** (q + 2)))
    if kind != "f32":  # Prod, the second rounding: four factors at the head of a vector of ones (elements 0 and 2, 1 and 3 meet first in the reference's order,
        # and their pairs at its last multiplication), whose f32 product narrows to another value than the exact product does (U.prod_witness)
        f, v = U.prod_witness(kind)
        x = np.ones(n)
        x[:4] = f
        out.append(("Prod", "second rounding", x, v))
    if kind == "f32":  # SqNorm: every square rounded on its own onto the 2^-149 grid, ties included (3 2^-75 squares to 4.5 quanta: 4); the sum of those is exact
        x = np.ldexp(_ints(rng, n), -75)
        sq = (x * x).astype(np.float32).astype(np.float64)
        assert ((np.ldexp(x * x, 149) % 1.0) == 0.5).mean() > 0.1 and np.ldexp(sq.sum(), 149) < 2.0 ** 24
        out.append(("SqNorm", "squares on the grid", x, sq.sum()))
    return out


@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("path,n,off,leaf", REDUCE_PATHS)
def test_reduce_exponent_range(gpu, oracle_c, path, n, off, leaf, kind):
    wg, L = _wg(), _lib()
    from oracle import wgsl_oracle as wo
    rng = np.random.default_rng(n + off + len(kind))
    cols = 3 if path == "batched" else 1
    fn = {"single": L.lib.wg_reduce, "batched": L.lib.wg_reduce_batched, "fast": L.lib.wg_reduce_fast}[path]
    for opn, case, x, exact in reduce_cases(kind, n, rng):
        if case == "second rounding" and path == "fast":  # (its order is its own: four factors in one lane's chain are not the exact pairs)
            continue
        op = wg.ReduceOp[opn]
        xs = np.concatenate([np.roll(x, 7 * c) for c in range(cols)])  # (a few vectors: the same values in other places)
        t = Held(gpu, xs.reshape(n, cols, 1, order="F"), kind, (off, 0, 0, 5))  # NaN before and after the view
        res = upload_bits(gpu, kind, np.full(cols, NAN[kind], U.BITS_T[kind]))
        gpu.take_path()
        shape = wg.ViewShape((n, cols, 1), n, n * cols, off) if path == "batched" else wg.ViewShape((n, 1, 1), n, n, off)
        L.check(fn(gpu._ctx.handle, int(op), code_of(kind), t.buf._h, shape.to_c(), res._h))
        got = np.ascontiguousarray(res.read(gpu.device())).view(U.BITS_T[kind])
        log = gpu.take_path()
        want_leaf = "reduce.fast/" if path == "single" and n >= 65536 and opn in ("Min", "Max") else leaf
        assert want_leaf in log, f"{path} n={n} offset {off} {opn}: expected {want_leaf!r}, took {log!r}"
        want = U.narrow_bits(kind, U.rne_grid(kind, np.full(cols, exact)))
        assert exact != 0 and (abs(exact) < 2.0 ** U.EMIN[kind] or case == "second rounding") and (U.widen_bits(kind, want) != 0).all(), (opn, case, exact)  # (a nonzero subnormal)
        what = f"{path} {opn} {case} {kind} [{log}]"
        assert np.array_equal(got, want), f"{what}: got {got}, expected {want}"
        if path != "fast":  # the reference's order: the C oracle on the widened vector, rounded once
            with np.errstate(under="ignore"):
                ref = np.array([oracle_c.reduce(int(getattr(wo, opn.upper())), xs.astype(np.float32), wo.Shape(n, 1, 1, n, n, c * n)) for c in range(cols)], np.float32)
            assert np.array_equal(got, U.narrow_bits(kind, ref)), f"{what}: differs from the oracle, {got} vs {U.narrow_bits(kind, ref)}"


# --------------------------------------------------------------------------------------------------------
# OpAssign and Axpy
# --------------------------------------------------------------------------------------------------------
def op_assign_operands(kind, n, rng):
    """(a, b) as float64 values of `kind`, n elements in a cycle of nine families: subnormals; the smallest normals; pairs whose sum, then whose
    difference, is subnormal; pairs whose product underflows gradually, then entirely (to zero or to one quantum); pairs whose quotient is subnormal
    (halves, quarters and eighths of a quantum: ties and exact ones; and thirds); a subnormal with a normal; and U.axpy_witness_pairs, on which a fused
    Axpy differs."""
    q, em, p = U.QUANTUM[kind], U.EMIN[kind], U.PREC[kind]
    full = 2.0 ** (p - 1)  # (the integers below it, times the quantum, are the subnormals)
    sg = lambda: np.where(rng.random(n) < 0.5, -1.0, 1.0)
    k = lambda hi: rng.integers(1, int(hi), n).astype(np.float64)
    mant = lambda: (full + k(full)) / full  # (1, 2) in p bits
    sub_a, sub_b = sg() * k(full) * 2.0 ** q, sg() * k(full) * 2.0 ** q
    nrm_a, nrm_b = sg() * (full + k(8) - 1) * 2.0 ** q, sg() * (full + k(8) - 1) * 2.0 ** q  # the smallest normals: 2^(p - 1) + 0 .. 6 quanta
    near = nrm_a - np.sign(nrm_a) * k(full) * 2.0 ** q  # nrm_a less a subnormal, toward zero: a multiple of the quantum below nrm_a, a value of the type
    e1 = rng.integers(em // 2 - 2, em // 2 + 3, n)
    grad_a, grad_b = sg() * mant() * 2.0 ** e1, sg() * mant() * 2.0 ** (em - 3 - e1)  # products in 2^(EMIN - 3) [1, 4): most of them inexact subnormals
    gone_a, gone_b = sg() * mant() * 2.0 ** (-p - 1), sg() * mant() * 2.0 ** em  # products in 2^(q - 2) [1, 4): below, at and above half a quantum
    quo_a = sg() * k(2 * full) * 2.0 ** (q + 3)
    quo_b = np.where(np.arange(n) % 16 >= 8, 3.0, 2.0 ** rng.integers(4, 7, n)) * sg()
    wa, wb = U.axpy_witness_pairs(kind)
    fams = ((sub_a, sub_b), (nrm_a, nrm_b), (nrm_a, -near), (nrm_a, near), (grad_a, grad_b), (gone_a, gone_b), (quo_a, quo_b), (sub_a, nrm_b),
            (np.resize(wa, n), np.resize(wb, n)))
    a, b = np.empty(n), np.empty(n)
    fam = np.arange(n) % len(fams)
    for f, (x, y) in enumerate(fams):
        a[fam == f], b[fam == f] = x[fam == f], y[fam == f]
    return a, b


def op_assign_model(kind, a64, b64, alpha=U.AXPY_ALPHA):
    """(name -> expected bits, the bits of a fused Axpy): numpy f32 arithmetic on the widened operands, narrowed once; Axpy: narrow(fmaf_f32(alpha, b, a))."""
    a32, b32 = a64.astype(np.float32), b64.astype(np.float32)
    assert np.array_equal(U.widen_bits(kind, U.narrow_bits(kind, a32)), a64) and np.array_equal(U.widen_bits(kind, U.narrow_bits(kind, b32)), b64)
    with np.errstate(all="ignore"):
        r = {"Add": a32 + b32, "Sub": a32 - b32, "Mul": a32 * b32, "Div": a32 / b32, "Copy": b32, "Axpy": U.fmaf_f32(np.float32(alpha), b32, a32)}
    return {name: U.narrow_bits(kind, v) for name, v in r.items()}, U.narrow_bits(kind, U.rne_grid(kind, U.fma_round_odd(np.float32(alpha), b32, a64)))


OP_SIZES = [(1, 0, 0), (3, 1, 1), (1757, 0, 0), (1757, 3, 3), (1757, 1, 2), (100003, 5, 9), (1 << 20, 0, 4)]  # tests/test_gpu_parity.py test_op_assign_offsets


@pytest.mark.parametrize("n,off_a,off_b", OP_SIZES)
@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
def test_op_assign_and_axpy_exponent_range(gpu, n, off_a, off_b, kind):
    wg, L = _wg(), _lib()
    a64, b64 = op_assign_operands(kind, n, np.random.default_rng(n + off_a * 17 + off_b))
    wants, fused = op_assign_model(kind, a64, b64)
    if n >= 1757 and kind != "f32":  # (a vector long enough to hold them; an f32 Axpy is one fmaf: nothing to fuse)
        assert (fused != wants["Axpy"]).sum() >= 8
    tb = Held(gpu, b64.reshape(n, 1, 1), kind, (off_b, 0, 0, 16 - off_b))
    for name, want in wants.items():
        ta = Held(gpu, a64.reshape(n, 1, 1), kind, (off_a, 0, 0, 16 - off_a), sentinel=True)
        if name == "Axpy":
            L.check(L.lib.wg_axpy(gpu._ctx.handle, float(U.AXPY_ALPHA), code_of(kind), ta.buf._h, ta.cm.to_c(), tb.buf._h, tb.cm.to_c()))
        else:
            L.check(L.lib.wg_op_assign(gpu._ctx.handle, int(wg.OpAssignVariant[name]), code_of(kind), ta.buf._h, ta.cm.to_c(), tb.buf._h, tb.cm.to_c()))
        got = ta.read(name)[:, 0, 0]
        assert not np.isnan(U.widen_bits(kind, want)).any()  # (no family holds 0 / 0 or Inf - Inf)
        bad = got != want
        assert not bad.any(), (f"{name} {kind} n={n} offsets ({off_a}, {off_b}): {bad.sum()} elements differ; first at {np.flatnonzero(bad)[0]}: "
                               f"a = {a64[bad][0]!r}, b = {b64[bad][0]!r}, got {got[bad][0]:#x}, expected {want[bad][0]:#x}")
