"""wg_gemv_q4 on the GPU, through the C ABI: a matrix of packed 4-bit weights with one f32 scale per group of logical rows, f32 vectors, f32 result. Before the feature
the symbol did not exist.

The contract (include/wgebra_hip.h): byte j of a column holds logical row 2 j in its low and row 2 j + 1 in its high nibble, q = n - 8; W[r, c] = scales[r // G, c] *
q[r, c]; out = W^T v; q formed exactly, nothing narrowed, f32 FMAs and multiplies, the accumulator stored as it is; deterministic. Cases, inputs, truth and gate are
tests/_q4.py's (tests/test_gemv_q4_model.py checks them on the CPU).

  1  every leaf ran (wg_debug_take_path): the streaming kernel at the smallest lengths at which it can go wrong, the element-by-element one on views that are off
  2  |got - f64 sum s q v| <= f32_gate(2 k, sum |s q v|)                                              test_leaves_truth_and_determinism (1, 2, 6)
  3  exact operands to the bit, -8 and 7 planted; scale 2^-140: exact subnormals                     test_exact_operands, test_subnormal_scale
  4  nibble order and lane map: a unit vector at every row of a chunk and at both ends of a tail     test_nibble_order_and_lane_map
  5  against wg_gemv_q8 on the unpacked int8: to the bit on exact operands, within twice the gate    test_against_wg_gemv_q8
  6  NaN in out overwritten; NaN / Inf in v or in a scale reach exactly their outputs; 0 * Inf = NaN  test_special_values
  7  the same call twice is bit-identical, the cut contraction included                               (in 1)
     every cut case (1 and 3 right-hand sides, 1 and 2 matrices, either tile) runs on a workspace that a NaN-scaled call of another shape has just filled, in 1, 3
     and 10: an unwritten partial is a NaN in the result                                              dirty_workspace
  8  status codes and messages, out = W v among them                                                  test_status_codes, test_workspace_inside_a_recording
  9  aliasing, on addresses                                                                          test_aliasing
 10  recorded and replayed; a CU-masked context                                                      test_recorded_and_masked
 11  a matrix whose third column starts past 4 GiB of its parent                                     test_far_view
 12  the Python operators with quantize_q4                                                           test_python_operators
No test asserts a time.
"""
import ctypes
import faulthandler

import numpy as np
import pytest

import _q4
import _util as U

pytestmark = pytest.mark.gpu

S_STORAGE = 128 | 4 | 8
NAN32 = np.float32(np.nan)
SENTINEL8 = np.uint8(0x5A)
GiB = 1 << 30


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
class Op:
    """X[r, c, z] stored column-major at element `off` with leading dimension r + pad and `gap` elements between matrices, in a poisoned parent: NaN for float32,
    the sentinel byte 0x5A for packed bytes and int8."""

    def __init__(self, gpu, vals, dtype=np.float32, off=0, pad=0, gap=0):
        wg = _wg()
        vals = np.asarray(vals, dtype)
        R, C, Z = vals.shape
        self.gpu, self.dtype = gpu, np.dtype(dtype)
        self.ld = R + pad
        self.batch = self.ld * C + gap
        self.size = off + self.batch * Z + 16
        self.idx = off + np.arange(R)[:, None, None] + np.arange(C)[None, :, None] * self.ld + np.arange(Z)[None, None, :] * self.batch
        self.init = np.full(self.size, NAN32 if self.dtype == np.float32 else SENTINEL8.astype(dtype), dtype)
        self.init[self.idx] = vals
        self.buf = wg.TensorBuilder.tensor((self.size,), S_STORAGE).build_init(gpu.device(), self.init, self.init.dtype)
        self.shape = wg.ViewShape((R, C, Z), self.ld, self.batch, off)
        self.outside = np.ones(self.size, bool)
        self.outside[self.idx.ravel()] = False

    def poison(self):
        self.gpu.queue().write_buffer(self.buf, 0, self.init)

    def read(self, what=""):
        flat = self.buf.read(self.gpu.device())
        assert np.isnan(flat[self.outside]).all(), f"{what}: wrote outside the view"
        return np.ascontiguousarray(flat[self.idx])


class View:
    """A view of somebody else's buffer."""

    def __init__(self, buf, shape):
        self.buf, self.shape = buf, shape


def call(inst, G, out, m, s, v, variant=None, fn="wg_gemv_q4"):
    """(status, message) of wg_gemv_q4 (or of wg_gemv_q8, whose signature it shares)."""
    wg, L = _wg(), _L()
    variant = int(wg.GemvVariant.GemvTr) if variant is None else int(variant)
    rc = getattr(L.lib, fn)(inst._ctx.handle, variant, int(G), out.buf._h, out.shape.to_c(), m.buf._h, m.shape.to_c(), s.buf._h, s.shape.to_c(), v.buf._h, v.shape.to_c())
    return rc, L.lib.wg_last_error_string().decode()


def run(inst, G, out, m, s, v, fn="wg_gemv_q4"):
    rc, msg = call(inst, G, out, m, s, v, fn=fn)
    assert rc == 0, msg


def build_case(gpu, case, q, s, v):
    """The operands of a case on the device: the packed matrix at its byte offset / padding / gap, the scales in a view of their own that no kernel may assume dense
    (offset 3, leading dimension + 1, gap 2), v and out at the case's offset (leading dimensions padded by 4 when it is not zero)."""
    name, k, C, nrhs, Z, G, (moff, mpad, gap), voff, tag = case
    vp = 4 if voff else 0
    m = Op(gpu, _q4.pack(q), np.uint8, off=moff, pad=mpad, gap=gap)
    sc = Op(gpu, s, off=3, pad=1, gap=2)
    vv = Op(gpu, v, off=voff, pad=vp)
    out = Op(gpu, np.full((C, nrhs, Z), NAN32), off=voff, pad=vp)
    return m, sc, vv, out


_DIRTY = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_dirty():
    yield
    _DIRTY.clear()


def planned(inst, case, m, sc, vv, out):
    """wg_debug_gemv_q4_plan's plan for the query a call on these views fills, on the context's CU count (a CU-masked context's own)."""
    L = _L()
    name, k, C, nrhs, Z, G = case[:6]
    info = inst.adapter()
    q, p = L.GemvQ4QueryC(), L.GemvQ4PlanC()
    kw = dict(trans=1, rows=k // 2, cols=C, nrhs=nrhs, mats=Z, group_rows=G, ldm=m.ld, lds=sc.ld, ldv=vv.ld, ldo=out.ld, m_batch=m.batch, s_batch=sc.batch, v_batch=vv.batch,
              o_batch=out.batch, cus=info.get("stream_compute_units", info["compute_units"]))
    for key, op, es in (("m_addr16", m, 1), ("v_addr16", vv, 4)):
        kw[key] = (L.lib.wg_buf_device_ptr(op.buf._h) + es * op.shape.offset) % 16
    for key, v in kw.items():
        setattr(q, key, v)
    tags = ctypes.create_string_buffer(128)
    assert L.lib.wg_debug_gemv_q4_plan(ctypes.byref(q), ctypes.byref(p), tags, 128) == 0
    return p


def dirty_workspace(inst, case, ops):
    """Before a cut case (`ops`: its operands) runs: one call on _q4.DIRTY, a larger cut problem of another shape whose scales are all NaN, so that every f32 partial
    in the context's workspace the case should write holds NaN -- a partial it fails to write shows in its result. Through the planner: the dirtying call is cut and
    its workspace covers the case's; its outputs x right-hand sides is another one, so stale values cannot line up. Nothing happens for a case that is not cut."""
    plan = planned(inst, case, *ops)
    if plan.nsplit == 1:
        return
    d = _q4.DIRTY
    first = id(inst) not in _DIRTY
    if first:
        q, s, v = _q4.random_inputs(d, salt=9)
        _DIRTY[id(inst)] = (inst,) + build_case(inst, d, q, np.full_like(s, NAN32), v)
    dops = _DIRTY[id(inst)][1:]
    dplan = planned(inst, d, *dops)
    assert dplan.nsplit > 1 and dplan.workspace_bytes >= plan.workspace_bytes > 0, (dplan.nsplit, dplan.workspace_bytes, plan.workspace_bytes)
    assert d[2] * d[3] != case[2] * case[3]
    m, sc, vv, out = dops
    run(inst, d[5], out, m, sc, vv)
    if first:
        assert np.isnan(out.read("dirty")).all(), "NaN scales did not reach every partial of the dirtying call"
    inst.take_path()


def _raw(gpu, arr):
    """A buffer of exactly arr.nbytes bytes."""
    wg = _wg()
    arr = np.ascontiguousarray(arr)
    return wg.TensorBuilder.tensor((arr.size,), S_STORAGE).build_init(gpu.device(), arr, arr.dtype)


# ---- 1, 2, 7 -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", _q4.CASES, ids=_q4.CASE_IDS)
def test_leaves_truth_and_determinism(gpu, case):
    name, k, C, nrhs, Z, G = case[:6]
    q, s, v = _q4.random_inputs(case)
    assert q.min() == -8 and q.max() == 7
    m, sc, vv, out = build_case(gpu, case, q, s, v)
    dirty_workspace(gpu, case, (m, sc, vv, out))  # (a cut case: NaN in every partial it should write)
    gpu.take_path()
    run(gpu, G, out, m, sc, vv)
    path = gpu.take_path()
    print(name, "->", path)
    got = out.read(name)  # (out was NaN everywhere: overwritten inside the view, untouched outside)
    # 1: the leaf (the plan on the whole chip: tests/test_gemv_q4_plan_host.py pins the same tags on 256 CUs)
    tags = path.split(" ")
    assert all(t.startswith("gemv_q4/") for t in tags), path
    if gpu.adapter()["compute_units"] == 256:
        assert tags[0] == case[8], f"{name}: expected {case[8]}, the call took '{path}'"
    elif not name.startswith("t4_"):  # (a part with fewer CUs cuts the *_split cases differently and takes the wide form sooner: the kernel is the same)
        assert tags[0].split(",ns=")[0] == case[8].split(",ns=")[0], f"{name}: expected {case[8]} up to the cut, the call took '{path}'"
    ns = int(tags[0].split("ns=")[1]) if "ns=" in tags[0] else 1
    assert tags[1:] == ([f"gemv_q4/combine,ns={ns}"] if ns > 1 else []), path
    if name.endswith("_split"):
        assert ns > 1, f"{name}: the contraction was not cut ({path})"
    # 2: the truth
    truth, sabs = _q4.truth64(q, s, v, G)
    _q4.assert_within_gate(got, truth, k, sabs, name)
    # 7: the same bits again
    dirty_workspace(gpu, case, (m, sc, vv, out))
    out.poison()
    run(gpu, G, out, m, sc, vv)
    U.assert_bits_equal(out.read(name), got, f"{name}: second call")


# ---- 3 -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", _q4.EXACT_CASES, ids=[c[0] for c in _q4.EXACT_CASES])
def test_exact_operands(gpu, case):
    """q over all 16 values with -8 and 7 planted, integer v in [-4, 4], power-of-two scales (2^-2 .. 2^2; 2^0 .. 2^1 at k = 65536), on every case, the two
    cut ones included (partials in the workspace, the combine pass): (max scale / min scale) * sum |q||v| < 2^24 (asserted), so every partial sum in any order and with the scale entering anywhere is exact: the result is fixed by construction."""
    name, k, C, nrhs, Z, G = case[:6]
    q, s, v = _q4.exact_inputs(case)
    assert (q == -8).any() and (q == 7).any() and _q4.exactness_condition(q, s, v) < 2.0 ** 24
    m, sc, vv, out = build_case(gpu, case, q, s, v)
    dirty_workspace(gpu, case, (m, sc, vv, out))
    gpu.take_path()
    run(gpu, G, out, m, sc, vv)
    assert (" gemv_q4/combine,ns=" in gpu.take_path()) == name.endswith("_split"), name
    truth, _ = _q4.truth64(q, s, v, G)
    want = truth.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), truth)
    U.assert_same_class_bits(out.read(name), want, name)  # (zeros as one class: the sign of an exact zero sum is open)


@pytest.mark.parametrize("case", [c for c in _q4.CASES if c[0] in ("t_piece", "t_chunk_plus", "t_8rhs", "t_split", "t4_chunk_plus", "t4_3rhs", "t4_split", "any_t")],
                         ids=lambda c: c[0])
def test_subnormal_scale(gpu, case):
    """Every scale 2^-140: the results are 2^-140 times an integer -- exact f32 values, most of them subnormal. Nothing is flushed on the way."""
    name, k, C, nrhs, Z, G = case[:6]
    q, s, v = _q4.exact_inputs(case, scale_exp=(-140, -140), salt=2)
    assert _q4.exactness_condition(q, s, v) < 2.0 ** 24
    m, sc, vv, out = build_case(gpu, case, q, s, v)
    gpu.take_path()
    run(gpu, G, out, m, sc, vv)
    assert (" gemv_q4/combine,ns=" in gpu.take_path()) == name.endswith("_split"), name
    truth, _ = _q4.truth64(q, s, v, G)
    want = truth.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), truth)
    sub = (want != 0) & (np.abs(want) < np.float32(2.0 ** -126))
    assert sub.mean() > 0.25, f"{name}: only {sub.mean():.2f} of the results are subnormal (the case shows nothing)"
    U.assert_same_class_bits(out.read(name), want, name)


# ---- 4 -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,tag", [(_q4.T_COLS + 1, "gemv_q4/t,nr=8,u=4,c=1,ns=1"), (_q4.WIDE + 1, "gemv_q4/t,nr=8,u=1,c=4,ns=1")], ids=["cols1", "cols4"])
def test_nibble_order_and_lane_map(gpu, C, tag):
    """The right-hand sides are unit vectors: one at every logical row of the first chunk and at the first and the last row of the guarded tail behind it (k = a
    chunk + two loads). out[c, j] must then be fl32(s[r_j // G, c] * q[r_j, c]) exactly -- d = q * 1 + zeros is exact, fmaf(s, d, 0) rounds once, and the fold adds
    zeros. Neighbouring rows, nibbles, lanes and columns carry different q, and every group and column its own scale with a full mantissa: a swapped nibble, a wrong
    lane, a wrong group or a wrong column of a pair shows here and nowhere else."""
    k, G = _q4.CHUNK + 2 * _q4.LOAD, 32
    rows = np.r_[np.arange(_q4.CHUNK), _q4.CHUNK, k - 1]
    r, c = np.arange(k)[:, None], np.arange(C)[None, :]
    q = ((r * 7 + r // 16 * 5 + r // 512 * 3 + c * 3 + c // 4) % 16 - 8).astype(np.int8)[:, :, None]
    assert all((np.diff(q[:, j, 0].astype(int)) != 0).all() for j in (0, 1, C - 1)) and (q[:, 0, 0] != q[:, 1, 0]).all() and set(np.unique(q)) == set(range(-8, 8))
    rng = np.random.default_rng(C)
    s = (1 + rng.random((k // G, C, 1), dtype=np.float32)).astype(np.float32)
    v = np.zeros((k, rows.size, 1), np.float32)
    v[rows, np.arange(rows.size), 0] = 1
    m, sc, vv, out = Op(gpu, _q4.pack(q), np.uint8), Op(gpu, s), Op(gpu, v), Op(gpu, np.full((C, rows.size, 1), NAN32))
    gpu.take_path()
    run(gpu, G, out, m, sc, vv)
    path = gpu.take_path()
    if gpu.adapter()["compute_units"] == 256:
        assert path == tag, path
    want = (s[rows // G, :, 0] * q[rows, :, 0].astype(np.float32)).astype(np.float32).T  # [C, rows]
    got = out.read("unit vectors")[:, :, 0]
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} of {got.size} wrong; first: column {bad[0][0]}, row {rows[bad[0][1]]}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"


# ---- 5 -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,C,nrhs,G", [(1056, 24, 2, 32), (10336, 9, 1, 128), (1056, 8200, 3, 96), (65536, 8, 2, 128), (16384, 4096, 1, 96),
                                        (208, 9, 2, 32)], ids=["t", "t_trips", "t_4cols", "t_cut", "t_4cols_cut", "any_t"])
def test_against_wg_gemv_q8(gpu, k, C, nrhs, G):
    """The same values through wg_gemv_q8 (GemvTr) on the unpacked int8 matrix: to the bit on exact operands, within twice the gate of each other on random ones."""
    case = (f"vs_q8_{k}_{C}", k, C, nrhs, 1, G)
    for kind in ("exact", "random"):
        q, s, v = _q4.exact_inputs(case) if kind == "exact" else _q4.random_inputs(case)
        m4, m8, sc, vv = Op(gpu, _q4.pack(q), np.uint8), Op(gpu, q, np.int8), Op(gpu, s), Op(gpu, v)
        o4, o8 = Op(gpu, np.full((C, nrhs, 1), NAN32)), Op(gpu, np.full((C, nrhs, 1), NAN32))
        gpu.take_path()
        run(gpu, G, o4, m4, sc, vv)
        p4 = gpu.take_path()
        run(gpu, G, o8, m8, sc, vv, fn="wg_gemv_q8")
        p8 = gpu.take_path()
        assert p4.startswith("gemv_q4/") and p8.startswith("gemv_q8/"), (p4, p8)
        if k >= 16384:  # the two cut shapes: partials in the workspace and the combine pass, to the bit below
            assert " gemv_q4/combine,ns=" in p4, p4
        got4, got8 = o4.read("q4"), o8.read("q8")
        truth, sabs = _q4.truth64(q, s, v, G)
        if kind == "exact":
            assert _q4.exactness_condition(q, s, v) < 2.0 ** 24
            U.assert_same_class_bits(got4, got8, f"{kind}: q4 against q8")
            U.assert_same_class_bits(got4, truth.astype(np.float32), f"{kind}: q4 against the truth")
        else:
            _q4.assert_within_gate(got4, truth, k, sabs, "q4")
            err = np.abs(got4.astype(np.float64) - got8.astype(np.float64))
            both = 2 * _q4.gate(k, sabs)
            print(f"worst |q4 - q8| / (2 gate) = {(err / both).max():.3g}")
            assert (err <= both).all(), f"worst |q4 - q8| / (2 gate) = {(err / both).max():.3g}"


# ---- 6 -------------------------------------------------------------------------------------------------------------------------------------------------
SPECIAL = [c for c in _q4.CASES if c[0] in ("t_chunk_plus", "t_2mats", "t_8rhs", "t4_trips", "t4_3rhs", "any_t")]


@pytest.mark.parametrize("what", ["v_nan", "v_inf", "scale_nan", "scale_inf", "zero_scale_inf_v"])
@pytest.mark.parametrize("case", SPECIAL, ids=lambda c: c[0])
def test_special_values(gpu, case, what):
    """`out` starts as NaN and is overwritten. ONE special entry -- in v (right-hand side 1 of matrix 0) or in the scales (one group of one column of matrix 0) --
    reaches exactly the outputs whose sums contain it. Weights are nonzero and v is nonzero, so an Inf term is an Inf, never 0 * Inf, except where the case asks."""
    name, k, C, nrhs, Z, G = case[:6]
    rng = _q4.rng_of(name, 5)
    q = (rng.integers(1, 4, (k, C, Z)) * rng.choice([-1, 1], (k, C, Z))).astype(np.int8)
    ng = _q4.n_groups(k, G)
    s = np.ldexp(np.float32(1), rng.integers(-1, 2, (ng, C, Z))).astype(np.float32)
    v = (rng.integers(1, 4, (k, nrhs, Z)) * rng.choice([-1, 1], (k, nrhs, Z))).astype(np.float32)
    g0, c0, y0, k0 = ng - 1, C // 2, min(1, nrhs - 1), k - 1  # the last group (a partial one where the case has it), a middle column, the last contracted entry
    hit = np.zeros((C, nrhs, Z), bool)       # outputs that must be non-finite
    nan_only = np.zeros((C, nrhs, Z), bool)  # ... of which those that must be NaN
    r0 = int(np.flatnonzero(np.arange(k) // G == g0)[0])
    if what in ("v_nan", "v_inf"):
        v[k0, y0, 0] = np.nan if what == "v_nan" else np.inf
        hit[:, y0, 0] = True
        nan_only[:, y0, 0] = what == "v_nan"
    elif what in ("scale_nan", "scale_inf"):
        s[g0, c0, 0] = np.nan if what == "scale_nan" else np.inf
        hit[c0, :, 0] = True  # the column's dot product contains the group
        nan_only[hit] = what == "scale_nan"
    else:  # a zero scale against an Inf in v: 0 * Inf = NaN where the two meet, +-Inf wherever another (nonzero) scale meets the Inf
        s[g0, c0, 0], v[r0, y0, 0] = 0, np.inf
        hit[:, y0, 0] = True
        nan_only[c0, y0, 0] = True
    m, sc, vv, out = build_case(gpu, case, q, s, v)
    run(gpu, G, out, m, sc, vv)
    got = out.read(f"{name} {what}")
    assert np.isfinite(got[~hit]).all(), f"{name} {what}: {np.count_nonzero(~np.isfinite(got[~hit]))} outputs outside the special entry's reach are not finite"
    assert not np.isfinite(got[hit]).any(), f"{name} {what}: {np.count_nonzero(np.isfinite(got[hit]))} outputs the special entry reaches are finite"
    assert np.isnan(got[nan_only]).all(), f"{name} {what}: an output that must be NaN is {got[nan_only][~np.isnan(got[nan_only])][:1]}"
    if what in ("v_inf", "zero_scale_inf_v"):
        inf = hit & ~nan_only
        kk = k0 if what == "v_inf" else r0
        want_sign = np.sign(s[kk // G, :, 0].astype(np.float64) * q[kk, :, 0])  # one Inf term per output: its sign is the weight's
        assert np.array_equal(np.sign(got[:, y0, 0][inf[:, y0, 0]]), want_sign[inf[:, y0, 0]]) and inf.any(), f"{name} {what}: the sign of an Inf"
    # the finite outputs are the exact product (small integers times powers of two)
    truth, _ = _q4.truth64(q, np.where(np.isfinite(s), s, 1), np.where(np.isfinite(v), v, 1), G)
    assert np.array_equal(got[~hit].astype(np.float64), truth[~hit])


# ---- 8 -------------------------------------------------------------------------------------------------------------------------------------------------
def test_status_codes(gpu):
    wg, L = _wg(), _L()
    V = wg.GemvVariant
    RB, C, G = 32, 32, 32
    k, ng = 2 * RB, 2 * RB // G
    mb, sb, vb, ob = _raw(gpu, np.full(RB * C, 0x99, np.uint8)), _raw(gpu, np.ones(ng * C, np.float32)), _raw(gpu, np.ones(k, np.float32)), _raw(gpu, np.zeros(C, np.float32))
    sh = wg.ViewShape
    m, s, v, out = View(mb, sh((RB, C, 1), RB, RB * C, 0)), View(sb, sh((ng, C, 1), ng, ng * C, 0)), View(vb, sh((k, 1, 1), k, k, 0)), View(ob, sh((C, 1, 1), C, C, 0))
    gpu.take_path()
    # an m buffer sized in bytes is fine: every nibble is 9, q = 1, so every output is k
    rc, msg = call(gpu, G, out, m, s, v)
    assert rc == 0, msg
    assert np.array_equal(ob.read(gpu.device()), np.full(C, k, np.float32)) and gpu.take_path() == "gemv_q4/t,nr=1,u=8,c=1,ns=1"
    done = ob.read(gpu.device()).copy()

    def refused(rc_msg, status, message=None, contains=None):
        rc, msg = rc_msg
        assert rc == status and (message is None or msg == message) and (contains is None or contains in msg), (rc, msg)
        assert gpu.take_path() == "" and ob.read(gpu.device()).tobytes() == done.tobytes(), "a refused call launched or wrote"

    # out = W v is not this call's product: UNSUPPORTED, and the message says where it lives (before any dimension is looked at)
    for variant in (V.Gemv, V.GemvFast):
        refused(call(gpu, G, out, m, s, v, variant), L.WG_ERR_UNSUPPORTED,
                "Gemv: wg_gemv_q4 computes out = W^T v only (WG_GEMV_TR); wg_gemv_q8 computes out = W v, on int8 weights")
        # ... a mismatched, a badly grouped or an empty call with these variants included (the header says so)
        refused(call(gpu, G, out, m, s, View(vb, sh((RB, 1, 1), RB, RB, 0)), variant), L.WG_ERR_UNSUPPORTED, contains="wg_gemv_q8 computes out = W v")
        refused(call(gpu, 7, out, m, s, v, variant), L.WG_ERR_UNSUPPORTED, contains="wg_gemv_q8 computes out = W v")
        refused(call(gpu, G, View(ob, sh((C, 0, 1), C, C, 0)), m, s, v, variant), L.WG_ERR_UNSUPPORTED, contains="wg_gemv_q8 computes out = W v")
    refused(call(gpu, G, out, m, s, v, 7), L.WG_ERR_INVALID_ARG, "Gemv: unknown variant 7")
    # a NULL buffer on a live context, each of the four in turn (before the variant is looked at: asked with both a legal and an unknown one)
    for which in range(4):
        hs = [None if i == which else b.buf._h for i, b in enumerate((out, m, s, v))]
        for variant in (int(V.GemvTr), 7):
            rc = L.lib.wg_gemv_q4(gpu._ctx.handle, variant, G, hs[0], out.shape.to_c(), hs[1], m.shape.to_c(), hs[2], s.shape.to_c(), hs[3], v.shape.to_c())
            refused((rc, L.lib.wg_last_error_string().decode()), L.WG_ERR_INVALID_ARG, f"Gemv: buffer argument {which} is NULL")
    ob2 = _raw(gpu, np.zeros(C, np.float32))
    rc, msg = call(gpu, G, View(ob2, out.shape), m, s, v, V.GemvTrFast)  # GemvTrFast is GemvTr
    assert rc == 0 and np.array_equal(ob2.read(gpu.device()), np.full(C, k, np.float32)) and gpu.take_path() == "gemv_q4/t,nr=1,u=8,c=1,ns=1", (rc, msg)
    # group_rows
    for bad in (0, 16, 48, 63):
        refused(call(gpu, bad, out, m, s, v), L.WG_ERR_INVALID_ARG, f"Gemv: group_rows {bad} is neither a positive multiple of 32 nor at least the {k} logical rows of m")
    # the scales' shape: one row of scales short, a column short, the scales of groups of 32 under groups of 64; one row for a per-column call is right
    refused(call(gpu, G, out, m, View(sb, sh((ng - 1, C, 1), ng, ng * C, 0)), v), L.WG_ERR_DIM_MISMATCH,
            f"Gemv: dimension mismatch. (m [{RB},{C},1] packed: k {k}, group_rows {G}, scales [{ng - 1},{C},1], expected [{ng},{C},1])")
    refused(call(gpu, G, out, m, View(sb, sh((ng, C - 1, 1), ng, ng * C, 0)), v), L.WG_ERR_DIM_MISMATCH, contains=f"scales [{ng},{C - 1},1], expected [{ng},{C},1]")
    refused(call(gpu, 64, out, m, s, v), L.WG_ERR_DIM_MISMATCH, contains=f"expected [1,{C},1]")
    for per_column in (k, 1000, 77):
        assert call(gpu, per_column, out, m, View(sb, sh((1, C, 1), 1, C, 0)), v)[0] == 0
        assert gpu.take_path() != "" and np.array_equal(ob.read(gpu.device()), np.full(C, k, np.float32))
    # the dimension check comes first: v with m.rows entries (the bytes, not the weights), out with another length than m.cols
    refused(call(gpu, G, out, m, s, View(vb, sh((RB, 1, 1), RB, RB, 0))), L.WG_ERR_DIM_MISMATCH,
            f"Gemv: dimension mismatch. (out [{C},1,1], m [{RB},{C},1]^T packed: k {k}, v [{RB},1,1])")
    refused(call(gpu, G, View(ob, sh((C - 1, 1, 1), C, C, 0)), m, s, v), L.WG_ERR_DIM_MISMATCH, contains=f"(out [{C - 1},1,1], m [")
    refused(call(gpu, 8, out, m, s, View(vb, sh((RB, 1, 1), RB, RB, 0))), L.WG_ERR_DIM_MISMATCH, contains="]^T packed: k 64, v [")  # (before the group_rows check)
    # each operand out of bounds at its own element size
    refused(call(gpu, G, out, View(_raw(gpu, np.zeros(RB * C - 1, np.uint8)), m.shape), s, v), L.WG_ERR_OUT_OF_BOUNDS,
            f"Gemv: view `m` addresses {RB * C} elements but its buffer holds {RB * C - 1}")
    refused(call(gpu, G, out, m, View(_raw(gpu, np.ones(ng * C - 1, np.float32)), s.shape), v), L.WG_ERR_OUT_OF_BOUNDS,
            f"Gemv: view `scales` addresses {ng * C} elements but its buffer holds {ng * C - 1}")
    refused(call(gpu, G, out, m, s, View(_raw(gpu, np.ones(k - 1, np.float32)), v.shape)), L.WG_ERR_OUT_OF_BOUNDS, f"Gemv: view `v` addresses {k} elements but its buffer holds {k - 1}")
    refused(call(gpu, G, View(_raw(gpu, np.zeros(C, np.uint8)), out.shape), m, s, v), L.WG_ERR_OUT_OF_BOUNDS,  # an `out` sized as if it held bytes
            f"Gemv: view `out` addresses {C} elements but its buffer holds {C // 4}")
    # empty operands: WG_OK, nothing launched, nothing written
    assert call(gpu, G, View(ob, sh((C, 0, 1), C, C, 0)), m, s, v)[0] == 0
    h0 = ctypes.c_void_p()
    L.check(L.lib.wg_buf_create(gpu._ctx.handle, 0, S_STORAGE, ctypes.byref(h0)))
    try:
        for which in range(4):
            hs = [h0 if i == which else b.buf._h for i, b in enumerate((out, m, s, v))]
            rc = L.lib.wg_gemv_q4(gpu._ctx.handle, int(V.GemvTr), G, hs[0], out.shape.to_c(), hs[1], m.shape.to_c(), hs[2], s.shape.to_c(), hs[3], v.shape.to_c())
            assert rc == 0, (which, L.lib.wg_last_error_string().decode())
    finally:
        L.check(L.lib.wg_buf_destroy(h0))
    assert gpu.take_path() == "" and ob.read(gpu.device()).tobytes() == done.tobytes()
    # nmats * ceil(nrhs / 8) > 65535: wg_gemv_q8's limit and message
    many = View(_raw(gpu, np.zeros(4 * 65536, np.float32)), sh((4, 1, 65536), 4, 4, 0))
    m4, s4, v4 = View(mb, sh((16, 4, 1), 16, 0, 0)), View(sb, sh((1, 4, 1), 1, 0, 0)), View(vb, sh((32, 1, 1), 32, 0, 0))
    refused(call(gpu, 32, many, m4, s4, v4), L.WG_ERR_UNSUPPORTED, "Gemv: nmats * ceil(nrhs/8) = 65536 exceeds 65535")


def test_workspace_inside_a_recording():
    """The partials of a cut contraction live in the context's workspace: on a fresh context it cannot grow inside a recording (WG_ERR_WORKSPACE, as wg_gemv_q8); after
    one eager call the same call records, and the replay has the eager bits."""
    wg, L = _wg(), _L()
    inst = wg.GpuInstance.new(0)
    try:
        case = [c for c in _q4.CASES if c[0] == "t_split"][0]
        k, G = case[1], case[5]
        q, s, v = _q4.random_inputs(case, salt=7)
        m, sc, vv, out = build_case(inst, case, q, s, v)
        enc = inst.device().create_command_encoder(record=True)
        try:
            rc, msg = call(inst, G, out, m, sc, vv)
        finally:
            cb = enc.finish()
        assert rc == L.WG_ERR_WORKSPACE, (rc, msg)
        del cb
        inst.take_path()
        run(inst, G, out, m, sc, vv)
        assert " gemv_q4/combine,ns=" in inst.take_path()
        want = out.read()
        truth, sabs = _q4.truth64(q, s, v, G)
        _q4.assert_within_gate(want, truth, k, sabs, "eager")
        out.poison()
        enc = inst.device().create_command_encoder(record=True)
        try:
            rc, msg = call(inst, G, out, m, sc, vv)
        finally:
            cb = enc.finish()
        assert rc == 0, msg
        inst.queue().submit([cb])
        U.assert_bits_equal(out.read(), want, "cut contraction, replayed")
        del cb
    finally:
        inst.sync()


# ---- 9 -------------------------------------------------------------------------------------------------------------------------------------------------
def test_aliasing(gpu):
    """Decided on addresses, `out` (f32) against `m` (1 byte) in 1-byte units; nothing is launched, logged or written by a refused call."""
    wg, L = _wg(), _L()
    sh = wg.ViewShape
    rng = np.random.default_rng(31)
    RB, C, G = 32, 256, 32
    k = 2 * RB
    case = ("alias", k, C, 1, 1, G)
    q, s, v = _q4.exact_inputs(case)
    truth = _q4.truth64(q, s, v, G)[0]
    sc, vv = Op(gpu, s), Op(gpu, v)
    # one buffer: C floats of `out` at byte 0, then the packed matrix from byte 4 C on
    raw = np.zeros(4 * C + RB * C + 16, np.uint8)
    raw[: 4 * C] = np.full(C, NAN32).view(np.uint8)
    raw[4 * C: 4 * C + RB * C] = _q4.pack(q)[:, :, 0].ravel(order="F")
    buf = _raw(gpu, raw)
    o, mm = View(buf, sh((C, 1, 1), C, C, 0)), View(buf, sh((RB, C, 1), RB, RB * C, 4 * C))  # the matrix begins exactly where out ends
    gpu.take_path()
    rc, msg = call(gpu, G, o, mm, sc, vv)
    assert rc == 0 and gpu.take_path().startswith("gemv_q4/t,"), msg
    after = buf.read(gpu.device())
    assert np.array_equal(after[: 4 * C].view(np.float32).astype(np.float64), truth.ravel()), "touching views: wrong result"
    assert np.array_equal(after[4 * C:], raw[4 * C:]), "touching views: the matrix changed"
    # the matrix one byte earlier: the last byte of out is shared -> refused, nothing written, nothing logged
    gpu.queue().write_buffer(buf, 0, raw)
    rc, msg = call(gpu, G, o, View(buf, sh((RB, C, 1), RB, RB * C, 4 * C - 1)), sc, vv)
    assert rc == L.WG_ERR_ALIASED and msg == "Gemv: `out` overlaps `m` (the written view shares memory with a view the call reads)", (rc, msg)
    assert gpu.take_path() == "" and buf.read(gpu.device()).tobytes() == raw.tobytes()
    # ... and through a second handle over the same allocation that starts at the last byte of out
    base = L.lib.wg_buf_device_ptr(buf._h)
    h = ctypes.c_void_p()
    L.check(L.lib.wg_buf_wrap(gpu._ctx.handle, ctypes.c_void_p(base + 4 * C - 1), RB * C, ctypes.byref(h)))
    try:
        rc = L.lib.wg_gemv_q4(gpu._ctx.handle, int(wg.GemvVariant.GemvTr), G, buf._h, o.shape.to_c(), h, sh((RB, C, 1), RB, RB * C, 0).to_c(), sc.buf._h, sc.shape.to_c(),
                              vv.buf._h, vv.shape.to_c())
        assert rc == L.WG_ERR_ALIASED and "`out` overlaps `m`" in L.lib.wg_last_error_string().decode()
    finally:
        L.check(L.lib.wg_buf_destroy(h))
    assert gpu.take_path() == ""

    # out interleaved between the columns of a strided matrix: m is 16 bytes x 8 with leading dimension 48; the 32 bytes of padding behind column j are 8 floats =
    # out[:, j] for j < 3 (f32 offset 4 + 12 j)
    R2, C2, ld, nrhs = 16, 8, 48, 3
    q2, s2, v2 = _q4.exact_inputs(("alias2", 2 * R2, C2, nrhs, 1, 32))
    raw2 = np.zeros(ld * C2 + 16, np.uint8)
    midx = np.arange(R2)[:, None] + np.arange(C2)[None, :] * ld
    raw2[midx] = _q4.pack(q2)[:, :, 0]
    buf2 = _raw(gpu, raw2)
    sc2, vv2 = Op(gpu, s2), Op(gpu, v2)
    o2, m2 = View(buf2, sh((C2, nrhs, 1), ld // 4, 0, R2 // 4)), View(buf2, sh((R2, C2, 1), ld, 0, 0))
    rc, msg = call(gpu, 32, o2, m2, sc2, vv2)
    assert rc == 0, msg
    after2 = buf2.read(gpu.device())
    oidx = R2 // 4 + np.arange(C2)[:, None] + np.arange(nrhs)[None, :] * (ld // 4)
    assert np.array_equal(after2.view(np.float32)[oidx].astype(np.float64), _q4.truth64(q2, s2, v2, 32)[0][:, :, 0]), "interleaved views: wrong result"
    assert np.array_equal(after2[midx], raw2[midx]), "interleaved views: the matrix changed"
    o2.shape = sh((C2, nrhs, 1), ld // 4, 0, R2 // 4 - 1)  # one float earlier: the last four bytes of every column of m
    rc, msg = call(gpu, 32, o2, m2, sc2, vv2)
    assert rc == L.WG_ERR_ALIASED and "`out` overlaps `m`" in msg

    # out inside scales; out inside v
    R3, C3 = 32, 64  # k = 64: two groups of 32
    m3 = Op(gpu, rng.integers(0, 256, (R3, C3, 1)).astype(np.uint8), np.uint8)
    s3, v3 = Op(gpu, np.ones((2, C3, 1), np.float32)), Op(gpu, np.ones((2 * R3, 3, 1), np.float32))
    before_s, before_v = s3.buf.read(gpu.device()).copy(), v3.buf.read(gpu.device()).copy()
    gpu.take_path()
    rc, msg = call(gpu, 32, View(s3.buf, sh((C3, 1, 1), C3, C3, 8)), m3, s3, View(v3.buf, sh((2 * R3, 1, 1), 2 * R3, 2 * R3, 0)))
    assert rc == L.WG_ERR_ALIASED and msg == "Gemv: `out` overlaps `scales` (the written view shares memory with a view the call reads)", (rc, msg)
    rc, msg = call(gpu, 32, View(v3.buf, sh((C3, 2, 1), 2 * R3, 4 * R3, 2 * R3)), m3, s3, View(v3.buf, sh((2 * R3, 2, 1), 2 * R3, 4 * R3, 0)))  # out in columns 1 .. 2 of v
    assert rc == L.WG_ERR_ALIASED and msg == "Gemv: `out` overlaps `v` (the written view shares memory with a view the call reads)", (rc, msg)
    assert gpu.take_path() == "" and s3.buf.read(gpu.device()).tobytes() == before_s.tobytes() and v3.buf.read(gpu.device()).tobytes() == before_v.tobytes()

    # the read operands may overlap each other: the scales ARE the first bytes of the matrix (2^e as bytes: 0, 0, 0x80 or 0, 0x3e .. 0x40)
    R4, C4, G4 = 64, 16, 32
    ng4 = 2 * R4 // G4
    sc4 = np.ldexp(np.float32(1), rng.integers(-2, 3, ng4 * C4)).astype(np.float32)
    raw4 = rng.integers(0, 256, R4 * C4).astype(np.uint8)
    raw4[: sc4.nbytes] = sc4.view(np.uint8)
    buf4 = _raw(gpu, raw4)
    q4, s4 = _q4.unpack(raw4.reshape(R4, C4, 1, order="F")), sc4.reshape(ng4, C4, 1, order="F")
    v4 = rng.integers(-4, 5, (2 * R4, 1, 1)).astype(np.float32)
    o4, vv4 = Op(gpu, np.full((C4, 1, 1), NAN32)), Op(gpu, v4)
    rc, msg = call(gpu, G4, o4, View(buf4, sh((R4, C4, 1), R4, R4 * C4, 0)), View(buf4, sh((ng4, C4, 1), ng4, ng4 * C4, 0)), vv4)
    assert rc == 0, msg
    assert _q4.exactness_condition(q4, s4, v4) < 2.0 ** 24
    assert np.array_equal(o4.read("m over scales").astype(np.float64), _q4.truth64(q4, s4, v4, G4)[0])


# ---- 10 ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def masked():
    wg = _wg()
    inst = wg.GpuInstance.new(0, cu_count=248, one_xcd=True)
    yield inst
    inst.sync()


REPLAY = [c for c in _q4.CASES if c[0] in ("t_trips", "t_8rhs", "t_split", "t4_8rhs", "t4_trips", "any_t", "t_3rhs_split", "t_2mats_split", "t4_3rhs_split", "t4_2mats_split")]


@pytest.mark.parametrize("where", ["whole", "masked"])
def test_recorded_and_masked(gpu, masked, where):
    """Eager, then recorded once and replayed twice into a re-poisoned output (a cut case: on a workspace dirtied before the eager call and before each replay): the
    eager bits each time. On the whole chip and on a CU-masked context (248 CUs: the
    plan reads the context's CU count), where the truth gate and determinism hold."""
    inst = gpu if where == "whole" else masked
    for case in REPLAY:
        name, k, C, nrhs, Z, G = case[:6]
        q, s, v = _q4.random_inputs(case, salt=3)
        m, sc, vv, out = build_case(inst, case, q, s, v)
        dirty_workspace(inst, case, (m, sc, vv, out))
        inst.take_path()
        run(inst, G, out, m, sc, vv)
        log = inst.take_path()
        assert log.startswith("gemv_q4/") and (" gemv_q4/combine,ns=" in log) == name.endswith("_split"), (name, log)
        eager = out.read(name)
        truth, sabs = _q4.truth64(q, s, v, G)
        _q4.assert_within_gate(eager, truth, k, sabs, f"{name} {where}")
        out.poison()
        enc = inst.device().create_command_encoder(record=True)
        try:
            run(inst, G, out, m, sc, vv)
        finally:
            cb = enc.finish()
        assert inst.take_path() == log
        for rep in range(2):
            dirty_workspace(inst, case, (m, sc, vv, out))
            out.poison()
            inst.queue().submit([cb])
            U.assert_bits_equal(out.read(name), eager, f"{name} {where}: replay {rep}")
        del cb


# ---- 11 ------------------------------------------------------------------------------------------------------------------------------------------------
def test_far_view(gpu):
    """A packed matrix of 512 bytes (1024 logical rows) x 3 columns with leading dimension 2^31 + 16: the third column starts past 4 GiB of its parent. Only the
    columns are written (the parent is uninitialised). Exact operands, to the bit: a column offset formed in 32 bits reads the wrong bytes."""
    wg, L = _wg(), _L()
    RB, C, G, ld = 512, 3, 128, 2 ** 31 + 16
    k = 2 * RB
    nbytes = -(-(2 * ld + RB + 4096) // 65536) * 65536
    free, _ = gpu.mem_info()
    if free < nbytes + 2 * GiB:
        pytest.skip(f"{free / GiB:.1f} GiB of device memory free, the case needs {nbytes / GiB:.1f} + 2")
    q, s, v = _q4.exact_inputs(("far", k, C, 2, 1, G))
    assert _q4.exactness_condition(q, s, v) < 2.0 ** 24
    packed = _q4.pack(q)
    big = wg.TensorBuilder.tensor((65536, nbytes // 65536), S_STORAGE).build(gpu.device(), np.uint8)
    try:
        for c in range(C):
            col = np.ascontiguousarray(packed[:, c, 0])
            L.check(L.lib.wg_buf_write(gpu._ctx.handle, big._h, c * ld, col.ctypes.data_as(ctypes.c_void_p), col.nbytes))
        m = View(big, wg.ViewShape((RB, C, 1), ld, 2 ** 32 - 16, 0))
        sc, vv, out = Op(gpu, s), Op(gpu, v), Op(gpu, np.full((C, 2, 1), NAN32))
        gpu.take_path()
        run(gpu, G, out, m, sc, vv)
        assert gpu.take_path().startswith("gemv_q4/t,")
        truth, _ = _q4.truth64(q, s, v, G)
        U.assert_same_class_bits(out.read("far"), truth.astype(np.float32), "far view")
    finally:
        gpu.sync()
        big.destroy()


# ---- 12 ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [32, 128, 4096])
def test_python_operators(gpu, G):
    """Gemv.dispatch_q4_tr / dispatch_q4_generic on tensors, through a compute pass: a random f32 matrix quantised with quantize_q4, against the f64 truth of the
    DEQUANTISED matrix within the gate of item 2; uint8 tensors build, upload and read back."""
    wg = _wg()
    dev, shapes = gpu.device(), wg.ViewShapeBuffers()
    rng = np.random.default_rng(41 + G)
    k, C = 1056, 72
    w = rng.standard_normal((k, C)).astype(np.float32)
    packed, s = wg.quantize_q4(w, G)
    q = _q4.unpack(packed)
    assert np.array_equal(wg.dequantize_q4(packed, s, G), (s[np.arange(k) // G] * q.astype(np.float32)).astype(np.float32))  # fl32(s q): one rounding
    tm = wg.TensorBuilder.matrix(k // 2, C, S_STORAGE).build_init(dev, packed)
    ts = wg.TensorBuilder.matrix(s.shape[0], C, S_STORAGE).build_init(dev, s)
    assert tm.dtype == np.uint8 and np.array_equal(tm.read(dev), packed.ravel(order="F"))
    op = wg.Gemv.from_device(dev)
    for method, extra in (("dispatch_q4_tr", ()), ("dispatch_q4_generic", (wg.GemvVariant.GemvTr,)), ("dispatch_q4_generic", ())):
        v = (rng.random((k, 1, 1), dtype=np.float32) * 2 - 1).astype(np.float32)
        tv = wg.TensorBuilder.vector(k, S_STORAGE).build_init(dev, v.ravel())
        to = wg.TensorBuilder.vector(C, S_STORAGE).build_init(dev, np.full(C, NAN32))
        gpu.take_path()
        enc = dev.create_command_encoder()
        p = enc.compute_pass("q4", None)
        getattr(op, method)(dev, shapes, p, to, tm, ts, tv, G, *extra)
        p.end()
        gpu.queue().submit([enc.finish()])
        got = to.read(dev)
        assert gpu.take_path().startswith("gemv_q4/t,"), method
        truth, sabs = _q4.truth64(q[:, :, None], s[:, :, None], v, G)
        _q4.assert_within_gate(got, truth, k, sabs, f"{method} G = {G}")
        # ... and the quantisation error itself is what it should be: each weight within s / 2, so the product within sum (s / 2) |v|
        half = s.astype(np.float64)[np.arange(k) // G] * (0.5 + 2.0 ** -16)
        bound = half.T @ np.abs(v[:, 0, 0].astype(np.float64))
        assert (np.abs(truth[:, 0, 0] - w.T.astype(np.float64) @ v[:, 0, 0].astype(np.float64)) <= bound + 1e-30).all()
    with pytest.raises(wg.WgError):  # out = W v is the library's refusal, surfaced
        enc = dev.create_command_encoder()
        p = enc.compute_pass("q4", None)
        try:
            op.dispatch_q4_generic(dev, shapes, p, to, tm, ts, tv, G, wg.GemvVariant.Gemv)
        finally:
            p.end()
            gpu.queue().submit([enc.finish()])
