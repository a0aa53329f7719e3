"""Shared by the wg_gemm_q8 tests (tests/test_gpu_gemm_q8.py on the device, tests/test_gemm_q8_model.py and tests/test_gemm_q8_plan_host.py on the CPU): the cases,
their inputs, the float64 truth, and a NumPy float32 model of the kernel's sum. Inputs, truth, gate and exactness condition are tests/_q8.py's with x in the place of v.

The contract (include/wgebra_hip.h): out = W^T x, W[r, c, z] = scales[r // G, c, z] * q[r, c, z]; int8 -> f16 / bf16 exactly, x read as the 16-bit value it is, every
product exact in f32; per group d = the MFMA chain from zero, acc = fmaf(s, d, acc). Each of the k terms takes at most two f32 roundings (its addition into d, and
its share of the group's fmaf): the gate is _q8.gate = f32_gate(2 k, sum |s q x|). Nothing is narrowed: there is no half-ulp term.
"""
import numpy as np

import _bf16
import _q8
import _util as U

STEP = 32        # rows of one MFMA step; the unit of group_rows and of every cut on the MFMA leaf (wgmath_amd/csrc/gemm_q8_plan.hpp)
WAVE_OUT = 32    # outputs per wave
BLOCK_OUT = 128  # outputs per workgroup (4 waves)
DTYPES = ("f16", "bf16")

DENSE = dict(m=(0, 0, 0), x=(0, 0), o=(0, 0))


def _case(name, k, outputs, n, G, Z=1, tag="gemm_q8/mfma,{dt},nt=2,ns=1", m=(0, 0, 0), x=(0, 0), o=(0, 0)):
    """m: (byte offset, leading-dimension padding, gap between matrices); x: (element offset, leading-dimension padding); o: the same in floats. tag: the first tag the
    call logs on 256 CUs."""
    return dict(name=name, k=k, outputs=outputs, n=n, G=G, Z=Z, tag=tag, m=m, x=x, o=o)


CASES = (
    [_case("one_step", 32, 16, 16, 32),
     _case("outputs_minus", 32, 15, 16, 32),  # the output mask
     _case("outputs_plus", 32, 17, 16, 32)]
    # column edges: half a tile, the 4-row blocks of D, the second 32-column tile, the second pass, a last pass of 2 columns
    + [_case(f"cols_{n}", 64, 16, n, 32, tag="gemm_q8/mfma,{dt},nt=%d,ns=1" % (2 if n <= 32 else 4)) for n in (1, 8, 15, 17, 64, 65, 130)]
    # groups: 96 is no power of two and 512 = 5.33 groups (a partial last group); 33 outputs: a second wave with one live output
    + [_case(f"groups_{G}", 512, 33, 20, G) for G in (32, 64, 96, 128)]
    + [_case("per_column", 512, 33, 20, 6000),                                         # no multiple of 16: one scale per output
       _case("lane_map", 64, 32, 32, 32),                                              # structured data, exact compare
       _case("blocks", 160, 130, 33, 32, tag="gemm_q8/mfma,{dt},nt=4,ns=1"),             # a second workgroup; a trip (128 rows) and a guarded step; a second tile of 1 column
       _case("two_mats", 544, 17, 9, 32, Z=2, m=(32, 16, 48), x=(8, 8), o=(1, 3)),      # `out` needs only 4-byte alignment
       _case("cut", 65536, 16, 16, 128, tag="gemm_q8/mfma,{dt},nt=2,ns=128"),            # 1 MiB of weights on one workgroup: the plan must cut k
       # the element-by-element kernel
       _case("any_m", 37, 7, 5, 16, tag="gemm_q8/any", m=(1, 3, 5)),
       _case("any_g16", 64, 9, 3, 16, tag="gemm_q8/any"),                               # everything aligned, but G % 32 != 0
       _case("any_x", 64, 9, 3, 32, tag="gemm_q8/any", x=(1, 0)),
       _case("any_k48", 48, 5, 2, 6000, tag="gemm_q8/any")])                            # k % 16 == 0 only: not taken by the MFMA leaf (no zero-filled half step)
CASE_IDS = [c["name"] for c in CASES]
EXACT_CASES = [c for c in CASES if c["k"] <= 2048]  # the exact operands need k <= 2048

WHOLE = 1 << 30  # a group size >= every k here: one scale per output


def _cut(name, k, outputs, n, G, Z=1, nt=2, ns=2, **views):
    return _case(name, k, outputs, n, G, Z, tag="gemm_q8/mfma,{dt},nt=%d,ns=%d" % (nt, ns), **views)


# The cut contraction (k over grid.y, f32 partials [z][split][n][outputs] in the workspace, a combine pass): the smallest shapes that reach each line. The floor is 512
# rows per split, so k >= 1024; 4 x 256 CUs against one or a few workgroups always want more splits than k / 512 allows: ns = k // 512 and the rows per split are
# ceil(k / ns) rounded up to the group (to 32 where the group is the whole column). tests/test_gemm_q8_plan_host.py pins ns and the rows per split of every row.
CUT_CASES = [
    _cut("cut_odd_steps", 1088, 16, 16, 32),                     # 2 x 544: 17 steps per split, the second split starts on an odd step
    _cut("cut_short_last", 1600, 33, 20, 32, ns=3),              # 544, 544, 512: a shorter last split; a second wave with one live output
    _cut("cut_g96_partial", 1120, 33, 20, 96),                   # 576, 544: 6 groups per split (no power of two); the last split ends inside a group of 64 rows
    _cut("cut_g64_views", 1152, 17, 9, 64, Z=2, m=(32, 16, 48), x=(8, 8), o=(1, 3, 5)),  # two_mats' strides and a gap between the matrices of `out`: z > 0
    _cut("cut_per_column", 1088, 33, 20, WHOLE),                 # one scale per output under a cut (groups_per_split 0)
    _cut("cut_passes", 1088, 130, 65, 32, nt=4),                 # T = 2 under a cut; a pass of one column; a second workgroup; the combine's third block has 2 live outputs
    _cut("cut_passes_mats", 2048, 65, 130, 128, Z=3, nt=4, ns=4),  # blockIdx.z = z * passes + pass with both above 1
    _cut("cut_ns5", 2560, 16, 16, 32, ns=5),                     # the combine: wave 0 adds two splits, waves 1 .. 3 one each
    _cut("cut_ns29", 14848, 33, 20, WHOLE, ns=29),               # wave 0 on the 8-wide loop, waves 1 .. 3 on the tail alone
    _cut("cut_ns32", 16384, 70, 3, 128, ns=32),                  # every wave exactly one wide trip, no tail; the combine's second block
    _cut("cut_ns33", 16896, 16, 16, 32, ns=33),                  # one tail element behind a wide trip, on wave 0 only
    _cut("cut_ns36", 18432, 16, 16, 32, ns=36),                  # one tail element on every wave
    _cut("cut_masked", 4096, 130, 130, 32, Z=2, nt=4, ns=8),     # 12 workgroups: ns 8 on 256 CUs, 6 on 16, 3 on 8
]
CUT_IDS = [c["name"] for c in CUT_CASES]
CUT_LANE_MAP = _cut("cut_lane_map", 1088, 32, 32, 32)
DIRTY = _case("dirty", 4096, 256, 192, 32, tag="gemm_q8/mfma,{dt},nt=4,ns=8")  # the call that fills the workspace with NaN partials before a cut case runs


def by_name(name):
    return [c for c in CASES + CUT_CASES if c["name"] == name][0]


def out_view(c):
    """(element offset, leading-dimension padding, gap between matrices) of `out`: a case's o is (offset, padding) or all three."""
    return tuple(c["o"]) + (0,) * (3 - len(c["o"]))


def cut_exact_inputs(c, dt, salt=1):
    """Exact operands for a cut case of any length: exact_inputs up to k = 2048; beyond, its narrower variant -- q over the full range with -128 and 127 planted, x in
    {-1, 0, 1}, scales 2^0 or 2^1: 2 * 128 k < 2^24 up to k = 65535. The tests assert _q8.exactness_condition on what they draw."""
    if c["k"] <= 2048:
        return exact_inputs(c, dt, salt=salt)
    q, s, _ = _q8.exact_inputs(q8case(c, dt), (0, 1), salt)
    x = _q8.rng_of(c["name"] + dt, salt + 50).integers(-1, 2, (c["k"], c["n"], c["Z"])).astype(np.float32)
    return q, s, x


def q8case(c, suffix=""):
    """The case in tests/_q8.py's form: (name, GemvTr, rows, cols, right-hand sides, matrices, group_rows)."""
    return (c["name"] + suffix, True, c["k"], c["outputs"], c["n"], c["Z"], c["G"])


def round16(dt, x32):
    """float32 values after ONE rounding to `dt`, as float32 (exactly representable)."""
    x32 = np.asarray(x32, np.float32)
    if dt == "f16":
        return x32.astype(np.float16).astype(np.float32)
    return _bf16.from_bits(_bf16.to_bits(x32)).astype(np.float32).reshape(x32.shape)


def bits16(dt, x32):
    """The 16-bit patterns of values that are representable in `dt`."""
    x32 = np.asarray(x32, np.float32)
    b = x32.astype(np.float16).view(np.uint16) if dt == "f16" else np.asarray(_bf16.to_bits(x32), np.uint16).reshape(x32.shape)
    return np.ascontiguousarray(b)


def random_inputs(c, dt, salt=0):
    """_q8.random_inputs with x rounded to the 16-bit type: (q int8 [k, outputs, Z], scales f32 [groups, outputs, Z], x f32 [k, n, Z] representable in dt)."""
    q, s, v = _q8.random_inputs(q8case(c, dt), salt)
    return q, s, round16(dt, v)


def exact_inputs(c, dt, scale_exp=(-2, 2), salt=1):
    """_q8.exact_inputs: q over the full range with -128 and 127 planted, integer x in [-4, 4] (f16 and bf16 values), power-of-two scales."""
    return _q8.exact_inputs(q8case(c, dt), scale_exp, salt)


def lane_map_inputs(c):
    """Structured operands for the lane-map check: every (row, output) and (row, column) pair has a value that depends asymmetrically on both indices, so a swapped
    row / column or a k permutation applied to one operand only changes the result. Exact: sum |q||x| <= 64 * 127 * 4, scales 1, 2, 4."""
    k, outs, n, Z = c["k"], c["outputs"], c["n"], c["Z"]
    r, o, col = np.arange(k)[:, None], np.arange(outs)[None, :], np.arange(n)[None, :]
    q = (((r * 7 + o * 13) % 255) - 127).astype(np.int8)[:, :, None].repeat(Z, 2)
    x = (((r * 3 + col * 5 + (r * col) % 7) % 9) - 4).astype(np.float32)[:, :, None].repeat(Z, 2)
    s = np.ldexp(np.float32(1), (np.arange(outs) % 3))[None, :, None].repeat(_q8.n_groups(k, c["G"]), 0).repeat(Z, 2).astype(np.float32)
    return q, s, x


def truth64(q, s, x, G):
    """(W^T x, sum |s q x|) in float64: [outputs, n, Z]."""
    return _q8.truth64(q, s, x, G, True)


def query_kw(c, dt, cus=256):
    """The wg_gemm_q8_query a call on the case's views fills (buffers are 256-byte aligned: a view's address modulo 16 is its offset's)."""
    k, outs, n, Z, G = c["k"], c["outputs"], c["n"], c["Z"], c["G"]
    (moff, mpad, gap), (xoff, xpad), (ooff, opad, ogap) = c["m"], c["x"], out_view(c)
    ldm, ldx, ldo, lds = k + mpad, k + xpad, outs + opad, _q8.n_groups(k, G) + 1
    return dict(k=k, outputs=outs, n=n, mats=Z, group_rows=G, x_bf16=int(dt == "bf16"), ldm=ldm, lds=lds, ldx=ldx, ldo=ldo, m_batch=ldm * outs + gap, s_batch=lds * outs + 2,
                x_batch=ldx * n, o_batch=ldo * n + ogap, m_addr16=moff % 16, x_addr16=2 * xoff % 16, o_addr16=4 * ooff % 16, cus=cus)


# ---- the float32 model -------------------------------------------------------------------------------------------------------------------------------
def _chain(P, order):
    """Sum of the float32 terms P[i] (axis 0) in float32: one accumulator ascending, or halves recursively (floor 8 terms)."""
    if order == "sequential" or P.shape[0] <= 8:
        d = np.zeros(P.shape[1:], np.float32)
        for i in range(P.shape[0]):
            d = (d + P[i]).astype(np.float32)
        return d
    h = P.shape[0] // 2
    return (_chain(P[:h], order) + _chain(P[h:], order)).astype(np.float32)


def model32(q, s, x, G, order="sequential"):
    """The kernel's sum in float32: every product q x exact (8 x 11 bits), per group d = the chain of its products from zero in `order`, then acc = fmaf(s, d, acc)
    with the groups ascending ("sequential") or, for "pairwise", the groups' scaled sums s * d added over halves -- a cut contraction's partial sums."""
    k, outs, Z = q.shape
    n = x.shape[1]
    out = np.zeros((outs, n, Z), np.float32)
    ob = max(1, min(outs, (1 << 23) // max(k * n, 1)))  # outputs per block (they do not interact): the products of a block stay near 8 M elements
    for z, o0 in ((z, o0) for z in range(Z) for o0 in range(0, outs, ob)):
        qb, sb = q[:, o0:o0 + ob, None, z], s[:, o0:o0 + ob, z]
        P = qb.astype(np.float32) * x[:, None, :, z].astype(np.float32)  # [k, block, n], exact
        assert np.array_equal(P.astype(np.float64), qb.astype(np.float64) * x[:, None, :, z].astype(np.float64))
        parts = []
        acc = np.zeros(P.shape[1:], np.float32)
        for g in range(_q8.n_groups(k, G)):
            d = _chain(P[g * G:(g + 1) * G], order)
            if order == "sequential":
                acc = U.fmaf_f32(sb[g][:, None], d, acc)
            else:
                parts.append(U.fmaf_f32(sb[g][:, None], d, np.float32(0)))
        out[o0:o0 + ob, :, z] = acc if order == "sequential" else _chain(np.stack(parts), order)
    return out
