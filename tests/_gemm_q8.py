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
    (moff, mpad, gap), (xoff, xpad), (ooff, opad) = c["m"], c["x"], c["o"]
    ldm, ldx, ldo, lds = k + mpad, k + xpad, outs + opad, _q8.n_groups(k, G) + 1
    return dict(k=k, outputs=outs, n=n, mats=Z, group_rows=G, x_bf16=int(dt == "bf16"), ldm=ldm, lds=lds, ldx=ldx, ldo=ldo, m_batch=ldm * outs + gap, s_batch=lds * outs + 2,
                x_batch=ldx * n, o_batch=ldo * n, m_addr16=moff % 16, x_addr16=2 * xoff % 16, o_addr16=4 * ooff % 16, cus=cus)


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
    for z in range(Z):
        P = q[:, :, None, z].astype(np.float32) * x[:, None, :, z].astype(np.float32)  # [k, outs, n], exact
        assert np.array_equal(P.astype(np.float64), q[:, :, None, z].astype(np.float64) * x[:, None, :, z].astype(np.float64))
        parts = []
        acc = np.zeros((outs, n), np.float32)
        for g in range(_q8.n_groups(k, G)):
            d = _chain(P[g * G:(g + 1) * G], order)
            if order == "sequential":
                acc = U.fmaf_f32(s[g, :, z][:, None], d, acc)
            else:
                parts.append(U.fmaf_f32(s[g, :, z][:, None], d, np.float32(0)))
        out[:, :, z] = acc if order == "sequential" else _chain(np.stack(parts), order)
    return out
