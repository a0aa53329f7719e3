"""Shared by the wg_gemv_q4 tests (tests/test_gpu_gemv_q4.py on the device, tests/test_gemv_q4_model.py on the CPU): the cases, their inputs, the float64 truth, the
gate, and the float32 model of the scaled sum (tests/_q8.py's, on the unpacked nibbles).

The contract (include/wgebra_hip.h): byte j of a column holds logical row 2 j in its low and row 2 j + 1 in its high nibble; a nibble n stands for q = n - 8;
W[r, c, z] = scales[r // G, c, z] * q[r, c, z]; out = W^T v; f32 FMAs and multiplies only. n - 8 is exact, so each of the k terms of a sum takes at most two f32
roundings -- the FMA's, and at most one for the scale wherever it enters (per element into the weight, or per 16-weight piece into the piece's sum) -- and nothing
more: the gate is wg_gemv_q8's, the project's f32 gate at twice the count, f32_gate(2 k, sum |s q v|). It is derived, not measured. Nothing is narrowed: there is no
half-ulp term.
"""
import numpy as np

import _q8
import _util as U

# The kernel's constants (wgmath_amd/csrc/gemv_q4_plan.hpp), in LOGICAL rows (weights):
LOAD = 32        # weights per 16-byte load: k % 32 == 0 on the streaming kernel
PIECE = 16       # weights per piece (half a load): the unit of the scale in the streaming kernel
CHUNK = 1024     # rows a half-wave covers per load (32 lanes x 32)
T_COLS = 8       # columns (half-waves) per workgroup, times the plan's 1 or 4 columns per half-wave
TRIP8 = 8 * CHUNK  # 1 column per half-wave, 1 or 2 right-hand sides: 8 loads in flight per lane -- 8192 rows per trip (3 .. 8 right-hand sides: 4 loads, 4096 rows)
TRIP2 = 2 * CHUNK  # 4 columns per half-wave, 1 or 2 right-hand sides: 2 loads in flight per lane and column (3 .. 8: 1 load, 1024 rows)
WIDE = 8192      # outputs from which 4 columns per half-wave still give each of 256 CUs a workgroup of 32 columns

# name, k (logical rows: the matrix has k / 2 rows of bytes), columns, right-hand sides, matrices, group_rows, (matrix byte offset, leading-dimension padding, gap between
# matrices; bytes), offset of v and out (floats; their leading dimensions are padded by 4 when it is not zero), the first tag the call must log
CASES = [
    # contraction lengths: one load; one chunk - / = / + one load; a whole trip + a partial trip of 2 chunks + a tail of 3 loads (10336 = 8192 + 2048 + 96)
    # outputs: one less than, equal to and one more than a workgroup's 8 columns
    ("t_piece", LOAD, T_COLS, 1, 1, 32, (0, 0, 0), 0, "gemv_q4/t,nr=1,u=8,c=1,ns=1"),
    ("t_chunk_minus", CHUNK - LOAD, T_COLS - 1, 1, 1, 32, (0, 0, 0), 0, "gemv_q4/t,nr=1,u=8,c=1,ns=1"),
    ("t_chunk", CHUNK, T_COLS, 1, 1, 128, (16, 16, 32), 4, "gemv_q4/t,nr=1,u=8,c=1,ns=1"),
    ("t_chunk_plus", CHUNK + LOAD, T_COLS + 1, 2, 1, 32, (0, 0, 0), 0, "gemv_q4/t,nr=2,u=8,c=1,ns=1"),
    ("t_trips", TRIP8 + 2 * CHUNK + 3 * LOAD, T_COLS + 1, 1, 1, 128, (0, 0, 0), 0, "gemv_q4/t,nr=1,u=8,c=1,ns=1"),   # 10336 rows in groups of 128: a partial last group
    ("t_trips_3rhs", TRIP8 // 2 + 2 * CHUNK + 3 * LOAD, T_COLS, 3, 1, 7001, (0, 0, 0), 0, "gemv_q4/t,nr=4,u=4,c=1,ns=1"),  # group_rows >= k and no multiple of 32: per column
    ("t_8rhs", 2 * CHUNK + LOAD, T_COLS + 1, 8, 1, 32, (0, 0, 0), 0, "gemv_q4/t,nr=8,u=4,c=1,ns=1"),
    ("t_11rhs", CHUNK + LOAD, T_COLS, 11, 1, 32, (0, 0, 0), 0, "gemv_q4/t,nr=8,u=4,c=1,ns=1"),                   # two groups of right-hand sides on grid.z: 8 + 3
    ("t_2mats", CHUNK + LOAD, T_COLS + 1, 2, 2, 96, (32, 16, 48), 4, "gemv_q4/t,nr=2,u=8,c=1,ns=1"),             # 1056 rows in groups of 96 (no power of two): 11 groups
    ("t_split", 65536, T_COLS, 1, 1, 128, (0, 0, 0), 0, "gemv_q4/t,nr=1,u=8,c=1,ns=8"),                         # 8 outputs cannot fill the chip: 8 splits of 8192 rows
    # 4 adjacent columns per half-wave (planned where 32 columns per workgroup still give every CU one): outputs one less than, equal to and one more than a multiple of
    # a workgroup's 32 columns
    ("t4_chunk_plus", CHUNK + LOAD, WIDE + 1, 1, 1, 32, (0, 0, 0), 0, "gemv_q4/t,nr=1,u=2,c=4,ns=1"),           # one guarded trip; the last half-wave has ONE live column
    ("t4_trips", TRIP2 + CHUNK + 3 * LOAD, WIDE - 1, 2, 1, 128, (16, 16, 32), 4, "gemv_q4/t,nr=2,u=2,c=4,ns=1"),  # 3168 = a trip + a chunk + 3 loads; a partial last group
    ("t4_3rhs", CHUNK + LOAD, WIDE, 3, 1, 96, (0, 0, 0), 0, "gemv_q4/t,nr=4,u=1,c=4,ns=1"),
    ("t4_8rhs", 2 * CHUNK + LOAD, WIDE, 8, 1, 4001, (0, 0, 0), 0, "gemv_q4/t,nr=8,u=1,c=4,ns=1"),
    ("t4_split", 16384, 4096, 1, 1, 96, (0, 0, 0), 0, "gemv_q4/t,nr=1,u=2,c=4,ns=2"),                           # 128 workgroups: cut in two (the floor: 8192 rows per split)
    # the cut with more than one right-hand side, and with two matrices on t_2mats' strided views: the smallest shapes either tile is cut at on 256 CUs (two splits of
    # the floor's 8192 rows; 4 columns per half-wave need 128 workgroups of 32 columns for every CU to have one)
    ("t_3rhs_split", 2 * TRIP8, T_COLS + 1, 3, 1, 128, (0, 0, 0), 0, "gemv_q4/t,nr=4,u=4,c=1,ns=2"),
    ("t_2mats_split", 2 * TRIP8, T_COLS + 1, 2, 2, 96, (32, 16, 48), 4, "gemv_q4/t,nr=2,u=8,c=1,ns=2"),      # 8192 is no multiple of 96: a group straddles the cut
    ("t4_3rhs_split", 2 * TRIP8, 4096, 3, 1, 96, (0, 0, 0), 0, "gemv_q4/t,nr=4,u=1,c=4,ns=2"),
    ("t4_2mats_split", 2 * TRIP8, 2048, 2, 2, 128, (32, 16, 48), 4, "gemv_q4/t,nr=2,u=2,c=4,ns=2"),
    # the element-by-element kernel: byte offset 1 with leading dimension + 3, 37 rows of bytes, vectors at float offset 1; everything aligned but m.rows % 16;
    # everything aligned but the vectors' offset
    ("any_t", 74, 5, 2, 2, 32, (1, 3, 5), 1, "gemv_q4/any_t"),
    ("any_t_rows", 208, 9, 11, 1, 32, (0, 0, 0), 0, "gemv_q4/any_t"),                                          # 104 bytes: 104 % 16 != 0
    ("any_t_vector", 128, 6, 1, 1, 64, (0, 0, 0), 1, "gemv_q4/any_t"),
]
CASE_IDS = [c[0] for c in CASES]
# the call that fills the workspace with NaN partials (its scales are NaN) before a cut case runs: 4 splits of 8192 rows, 8 x 1024 outputs each -- more than any
# cut case writes, and another outputs x right-hand sides than any of them has
DIRTY = ("dirty", 4 * TRIP8, 1024, 8, 1, 128, (0, 0, 0), 0, "gemv_q4/t,nr=8,u=4,c=1,ns=4")
EXACT_CASES = CASES  # every case, the two cut ones included: exact_scale_exp(k) keeps (max scale / min scale) * 32 k below 2^24


def exact_scale_exp(k):
    """The exponents of the power-of-two scales of the exact operands: |q| <= 8 and |v| <= 4 bound sum |q||v| by 32 k, so 2^-2 .. 2^2 (a ratio of 16) serve up to
    k = 16384 (16 * 32 * 16384 = 2^23) and 2^0 .. 2^1 (a ratio of 2) up to k = 131072. The tests assert the condition itself on the operands they draw."""
    assert 2 * 32 * k < 2 ** 24
    return (-2, 2) if 16 * 32 * k < 2 ** 24 else (0, 1)


def n_groups(k, G):
    return -(-k // G)


def rng_of(name, salt=0):
    return np.random.default_rng(sum(map(ord, name)) * 11 + salt)


def pack(q):
    """int8 in -8 .. 7 [k, C, Z] -> bytes [k / 2, C, Z]: row 2 j in the LOW nibble of byte j, row 2 j + 1 in the HIGH one (restated here, not imported: the GPU tests
    must not inherit a mistake of wgmath_amd.pack_q4)."""
    n = (q.astype(np.int16) + 8).astype(np.uint8)
    return (n[0::2] + 16 * n[1::2]).astype(np.uint8)


def unpack(m):
    q = np.empty((2 * m.shape[0],) + m.shape[1:], np.int8)
    q[0::2] = (m % 16).astype(np.int8) - 8
    q[1::2] = (m // 16).astype(np.int8) - 8
    return q


def random_inputs(case, salt=0):
    """(q int8 [k, C, Z], scales f32 [groups, C, Z], v f32 [k, nrhs, Z]): nibbles over all 16 values, scales in [2^-8, 2^-6), v in [-1, 1)."""
    name, k, C, nrhs, Z, G = case[:6]
    rng = rng_of(name, salt)
    q = rng.integers(-8, 8, (k, C, Z), dtype=np.int8)
    s = ((1 + 3 * rng.random((n_groups(k, G), C, Z), dtype=np.float32)) * np.float32(2.0 ** -8)).astype(np.float32)
    v = (rng.random((k, nrhs, Z), dtype=np.float32) * 2 - 1).astype(np.float32)
    return q, s, v


def exact_inputs(case, scale_exp=None, salt=1):
    """Operands whose product is exact in f32 whatever the order and wherever the scale enters: q over all 16 values with both ends planted, integer v in [-4, 4],
    scales 2^e with e in scale_exp (inclusive; by default exact_scale_exp(k))."""
    name, k, C, nrhs, Z, G = case[:6]
    scale_exp = exact_scale_exp(k) if scale_exp is None else scale_exp
    rng = rng_of(name, salt)
    q = rng.integers(-8, 8, (k, C, Z), dtype=np.int8)
    flat = q.reshape(-1)
    step = max(flat.size // 64, 2)
    flat[::step][:8] = -8  # (both ends of the range for sure, in even and odd rows: low and high nibbles)
    flat[1::step][:8] = 7
    s = np.ldexp(np.float32(1), rng.integers(scale_exp[0], scale_exp[1] + 1, (n_groups(k, G), C, Z))).astype(np.float32)
    v = rng.integers(-4, 5, (k, nrhs, Z)).astype(np.float32)
    return q, s, v


def truth64(q, s, v, G):
    """(W^T v, sum |s q v|) per matrix in float64: [outputs, nrhs, Z], on the unpacked nibbles. s q is exact in float64 (24 x 4 bits). Column blocks keep the
    float64 copy of the largest case small."""
    k, C, Z = q.shape
    gi = np.arange(k) // G
    out, sabs = np.zeros((C, v.shape[1], Z)), np.zeros((C, v.shape[1], Z))
    for z in range(Z):
        V = v[:, :, z].astype(np.float64)
        for c0 in range(0, C, 512):
            W = s[:, c0:c0 + 512, z].astype(np.float64)[gi] * q[:, c0:c0 + 512, z]
            out[c0:c0 + 512, :, z] = W.T @ V
            sabs[c0:c0 + 512, :, z] = np.abs(W).T @ np.abs(V)
    return out, sabs


def gate(k, sabs):
    """The tolerance of the contract: the project's f32 gate at twice the count (two roundings per term)."""
    return U.f32_gate(2 * k, sabs)


def assert_within_gate(got, truth, k, sabs, what=""):
    got, truth = np.asarray(got, np.float64).ravel(), np.asarray(truth, np.float64).ravel()
    tol = gate(k, np.asarray(sabs).ravel())
    err = np.abs(got - truth)
    bad = err > tol
    worst = float((err / tol).max())
    print(f"{what}: worst err / gate = {worst:.3g}")
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} elements exceed f32_gate(2 * {k}, sum|s q v|); worst err / gate = {worst:.3g}"
    return worst


def exactness_condition(q, s, v):
    """(max scale / min scale) * max over outputs of sum |q||v| -- below 2^24 every partial sum, in any order and with the scale entering anywhere, is an integer
    multiple of the smallest scale below 2^24 of them: exact in f32 as long as that scale is at least 2^-149."""
    assert 32 * q.shape[0] < 2 ** 24  # (integers: the float32 sums below are exact, and a quarter of the float64 copy of the largest case)
    sabs = max((np.abs(q[:, :, z]).astype(np.float32).T @ np.abs(v[:, :, z])).max() for z in range(q.shape[2]))
    return float(s.max() / s.min()) * float(sabs)


def model32(q, s, v, G, scale="piece", order="sequential"):
    """The scaled sum in float32 for one placement of the scale ("piece": per 16 weights, the streaming kernel; "element": the element-by-element kernel) and one
    summation order: tests/_q8.py's model of GemvTr on the unpacked nibbles -- its pieces are 16 rows, as here."""
    return _q8.model32(q, s, v, G, True, scale, order)
