"""Shared by the wg_gemm_q4 tests (tests/test_gpu_gemm_q4.py on the device, tests/test_gemm_q4_model.py and tests/test_gemm_q4_plan_host.py on the CPU): the cases,
their inputs and the float64 truth. The packed layout, the gate and the exactness condition are tests/_q4.py's with x in the place of v; the 16-bit helpers and the
float32 model of "chain per group, then fmaf" are tests/_gemm_q8.py's, on _q4.unpack of the packed bytes.

The contract (include/wgebra_hip.h): out = W^T x, W[r, c, z] = scales[r // G, c, z] * q[r, c, z], q = n - 8 formed exactly in the 16-bit type; x read as the 16-bit
value it is, every product exact in f32; per group d = the MFMA chain from zero, acc = fmaf(s, d, acc). Each of the k terms takes at most two f32 roundings: the gate is
_q4.gate = f32_gate(2 k, sum |s q x|). Nothing is narrowed: there is no half-ulp term.
"""
import numpy as np

import _gemm_q8 as G8
import _q4

STEP = 32        # logical rows of one MFMA step: k % STEP == 0 on the streaming kernel (wgmath_amd/csrc/gemm_q4_plan.hpp; the plan's `step`)
TRIP = 256       # rows per trip: 4 16-byte loads per lane, a double step of 64 rows each
WAVE_OUT = 32    # outputs per wave
BLOCK_OUT = 128  # outputs per workgroup (4 waves)
DTYPES = G8.DTYPES
round16, bits16 = G8.round16, G8.bits16


def _case(name, k, outputs, n, G, Z=1, tag="gemm_q4/mfma,{dt},nt=2,ns=1", m=(0, 0, 0), x=(0, 0), o=(0, 0)):
    """k: logical rows (the matrix has k / 2 rows of bytes). m: (byte offset, leading-dimension padding, gap between matrices; bytes); x: (element offset,
    leading-dimension padding); o: the same in floats. tag: the first tag the call logs on 256 CUs."""
    return dict(name=name, k=k, outputs=outputs, n=n, G=G, Z=Z, tag=tag, m=m, x=x, o=o)


CASES = (
    [_case("one_step", STEP, 16, 16, 32),       # half a double step: the upper half of the wave loads nothing
     _case("outputs_minus", STEP, 15, 16, 32),  # the output mask
     _case("outputs_plus", STEP, 17, 16, 32)]
    # column edges: half a tile, the 4-row blocks of D, the second 32-column tile, the second pass, a last pass of 2 columns
    + [_case(f"cols_{n}", 64, 16, n, 32, tag="gemm_q4/mfma,{dt},nt=%d,ns=1" % (2 if n <= 32 else 4)) for n in (1, 8, 15, 17, 64, 65, 130)]
    # groups: 32 puts two groups into every 16-byte load; 96 is no power of two and leaves a partial last group; 33 outputs: a second wave with one live output
    + [_case(f"groups_{G}", 512, 33, 20, G) for G in (32, 64, 96, 128)]
    + [_case("per_column", 512, 33, 20, 6000),                                         # no multiple of 32: one scale per output
       _case("blocks", TRIP + STEP, 130, 33, 32, tag="gemm_q4/mfma,{dt},nt=4,ns=1"),     # a second workgroup; one trip and one guarded step; a second tile of 1 column
       _case("two_mats", 544, 17, 9, 32, Z=2, m=(32, 16, 48), x=(8, 8), o=(1, 3)),      # `out` needs only 4-byte alignment
       _case("cut", 65536, 16, 16, 128, tag="gemm_q4/mfma,{dt},nt=2,ns=128"),            # 512 KiB of weights on one workgroup: the plan must cut k
       # the element-by-element kernel
       _case("any_m", 74, 7, 5, 32, Z=2, tag="gemm_q4/any", m=(1, 3, 5)),
       _case("any_rows", 208, 9, 3, 32, tag="gemm_q4/any"),                             # 104 bytes of k: everything aligned, but k % 32 == 16
       _case("any_x", 64, 9, 3, 32, tag="gemm_q4/any", x=(1, 0))])
CASE_IDS = [c["name"] for c in CASES]
EXACT_CASES = CASES  # every case: _q4.exact_scale_exp(k) gives 2^-2 .. 2^2 up to k = 16384 and 2^0 .. 2^1 for the cut one
WHOLE = 1 << 30  # a group size >= every k here: one scale per output


def _cut(name, k, outputs, n, G, Z=1, nt=2, ns=2, **views):
    return _case(name, k, outputs, n, G, Z, tag="gemm_q4/mfma,{dt},nt=%d,ns=%d" % (nt, ns), **views)


# The cut contraction (k over grid.y, f32 partials [z][split][n][outputs] in the workspace, a combine pass): tests/_gemm_q8.py's rows on the packed matrix. A lane's
# 16-byte load covers half a double step of 64 rows: a split of 17 steps (544 rows) ENDS on half a double step in the middle of k, and the next one begins at byte
# offset 16 mod 32. tests/test_gemm_q4_plan_host.py pins ns and the rows per split of every row, and that some split starts on an odd step.
CUT_CASES = [
    _cut("cut_odd_steps", 1088, 16, 16, 32),                     # 2 x 544: 17 steps per split; half a double step mid-k; the second split starts on an odd step
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
DIRTY = _case("dirty", 4096, 256, 192, 32, tag="gemm_q4/mfma,{dt},nt=4,ns=8")  # the call that fills the workspace with NaN partials before a cut case runs
out_view = G8.out_view


def by_name(name):
    return [c for c in CASES + CUT_CASES if c["name"] == name][0]


LANE_MAP = _case("lane_map", 64, 32, 32, 32)
IDENTITY = _case("identity", 2 * STEP, 32, 2 * STEP, 32, tag="gemm_q4/mfma,{dt},nt=4,ns=1")  # N = k, x the identity: out[o, r] = s q[r, o]


def q4case(c, suffix=""):
    """The case in tests/_q4.py's form: (name, k, columns, right-hand sides, matrices, group_rows)."""
    return (c["name"] + suffix, c["k"], c["outputs"], c["n"], c["Z"], c["G"])


def random_inputs(c, dt, salt=0):
    """_q4.random_inputs with x rounded to the 16-bit type: (q int8 in -8 .. 7 [k, outputs, Z], scales f32 [groups, outputs, Z], x f32 [k, n, Z] representable in dt)."""
    q, s, v = _q4.random_inputs(q4case(c, dt), salt)
    return q, s, round16(dt, v)


def exact_inputs(c, dt, scale_exp=None, salt=1):
    """_q4.exact_inputs: q over all 16 values with -8 and 7 planted in even and in odd rows, integer x in [-4, 4] (f16 and bf16 values), power-of-two scales."""
    return _q4.exact_inputs(q4case(c, dt), scale_exp, salt)


def lane_map_inputs(c):
    """_gemm_q8.lane_map_inputs with the weights reduced into -8 .. 7: still asymmetric in (row, output) and (row, column)."""
    q, s, x = G8.lane_map_inputs(c)
    r, o = np.arange(c["k"])[:, None], np.arange(c["outputs"])[None, :]
    q = (((r * 7 + o * 13 + (r * o) % 5) % 16) - 8).astype(np.int8)[:, :, None].repeat(c["Z"], 2)
    return q, s, x


def truth64(q, s, x, G):
    """(W^T x, sum |s q x|) in float64: [outputs, n, Z]."""
    return _q4.truth64(q, s, x, G)


def model32(q, s, x, G, order="sequential"):
    """The kernel's sum in float32 (_gemm_q8.model32: chain per group, then fmaf) on the unpacked nibbles -- through pack and unpack, as the kernel sees them."""
    return G8.model32(_q4.unpack(_q4.pack(q)), s, x, G, order)


def query_kw(c, dt, cus=256):
    """The wg_gemm_q4_query a call on the case's views fills (buffers are 256-byte aligned: a view's address modulo 16 is its offset's)."""
    k, outs, n, Z, G = c["k"], c["outputs"], c["n"], c["Z"], c["G"]
    (moff, mpad, gap), (xoff, xpad), (ooff, opad, ogap) = c["m"], c["x"], out_view(c)
    ldm, ldx, ldo, lds = k // 2 + mpad, k + xpad, outs + opad, _q4.n_groups(k, G) + 1
    return dict(k=k, outputs=outs, n=n, mats=Z, group_rows=G, x_bf16=int(dt == "bf16"), ldm=ldm, lds=lds, ldx=ldx, ldo=ldo, m_batch=ldm * outs + gap, s_batch=lds * outs + 2,
                x_batch=ldx * n, o_batch=ldo * n + ogap, m_addr16=moff % 16, x_addr16=2 * xoff % 16, o_addr16=4 * ooff % 16, cus=cus)
