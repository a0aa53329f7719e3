"""Shared by the wg_gemv_q8 tests (tests/test_gpu_gemv_q8.py on the device, tests/test_gemv_q8_model.py on the CPU): the cases, their inputs, the float64 truth, the
gate, and a NumPy float32 model of the scaled sum. The model test runs the yardsticks of the GPU tests on the same inputs without a device.

The contract (include/wgebra_hip.h): W[r, c, z] = scales[r // G, c, z] * q[r, c, z]; out = W v (Gemv) or W^T v (GemvTr); int8 widened exactly, f32 FMAs and multiplies
only. Each of the k terms of a sum takes at most two f32 roundings -- the FMA's, and at most one for the scale wherever it enters (per element into the weight, per
16-weight piece into the piece's sum, or into the vector entry) -- so the gate is the project's f32 gate at twice the count: f32_gate(2 k, sum |s q v|). Nothing is
narrowed: there is no half-ulp term.
"""
import numpy as np

import _util as U

# The kernels' constants (wgmath_amd/csrc/gemv_q8_plan.hpp):
PIECE = 16       # weights per 16-byte load; the unit of the scale in the streaming kernels
CHUNK = 512      # T: rows a half-wave covers per load (32 lanes x 16)
T_COLS = 8       # T: columns (half-waves) per workgroup
TRIP8 = 8 * CHUNK  # T, 1 or 2 right-hand sides: 8 loads in flight per lane -- 4096 rows per trip (3 .. 8 right-hand sides: 4 loads, 2048 rows)
N_ROWS = 1024    # N: rows per workgroup (64 lanes x 16); its 4 waves take a quarter of the columns each, 8 columns in flight per lane

# name, GemvTr, stored rows, stored columns, right-hand sides, matrices, group_rows, (matrix byte offset, leading-dimension padding, gap between matrices),
# offset of v and out (floats; their leading dimensions are padded by 4), the first tag the call must log
CASES = [
    # T, contraction lengths: one piece; one chunk - / = / + one piece; a whole trip + a partial trip of 2 chunks + a tail of 3 pieces (5168 = 4096 + 1024 + 48)
    # outputs: one less than, equal to and one more than a workgroup's 8 columns
    ("t_piece", True, PIECE, T_COLS, 1, 1, 16, (0, 0, 0), 0, "gemv_q8/t,nr=1,u=8,c=1,ns=1"),
    ("t_chunk_minus", True, CHUNK - PIECE, T_COLS - 1, 1, 1, 32, (0, 0, 0), 0, "gemv_q8/t,nr=1,u=8,c=1,ns=1"),   # 496 rows in groups of 32: a partial last group
    ("t_chunk", True, CHUNK, T_COLS, 1, 1, 128, (16, 16, 32), 4, "gemv_q8/t,nr=1,u=8,c=1,ns=1"),
    ("t_chunk_plus", True, CHUNK + PIECE, T_COLS + 1, 2, 1, 16, (0, 0, 0), 0, "gemv_q8/t,nr=2,u=8,c=1,ns=1"),
    ("t_trips", True, TRIP8 + 2 * CHUNK + 3 * PIECE, T_COLS + 1, 1, 1, 128, (0, 0, 0), 0, "gemv_q8/t,nr=1,u=8,c=1,ns=1"),   # 5168 rows in groups of 128: a partial last group
    ("t_trips_3rhs", True, TRIP8 + 2 * CHUNK + 3 * PIECE, T_COLS, 3, 1, 6000, (0, 0, 0), 0, "gemv_q8/t,nr=4,u=4,c=1,ns=1"),  # group_rows >= rows (and no multiple of 16): per column
    ("t_8rhs", True, 2 * CHUNK + PIECE, T_COLS + 1, 8, 1, 32, (0, 0, 0), 0, "gemv_q8/t,nr=8,u=4,c=1,ns=1"),
    ("t_11rhs", True, CHUNK + PIECE, T_COLS, 11, 1, 16, (0, 0, 0), 0, "gemv_q8/t,nr=8,u=4,c=1,ns=1"),            # two groups of right-hand sides on grid.z: 8 + 3
    ("t_2048", True, 2048, T_COLS, 2, 1, 128, (0, 0, 0), 0, "gemv_q8/t,nr=2,u=8,c=1,ns=1"),
    ("t_2mats", True, CHUNK + PIECE, T_COLS + 1, 2, 2, 48, (32, 16, 48), 4, "gemv_q8/t,nr=2,u=8,c=1,ns=1"),       # 528 rows in groups of 48 (no power of two): 11 groups
    ("t_split", True, 65536, T_COLS, 1, 1, 128, (0, 0, 0), 0, "gemv_q8/t,nr=1,u=8,c=1,ns=16"),                   # 8 outputs cannot fill the chip: 16 splits of 4096 rows
    # T with 4 adjacent columns per half-wave (planned where 32 columns per workgroup still give every CU one): 2 loads in flight per column (a trip: 1024 rows),
    # 1 from 3 right-hand sides on (512); outputs one less than, equal to and one more than a multiple of a workgroup's 32 columns
    ("t4_chunk_plus", True, CHUNK + PIECE, 8192 + 1, 1, 1, 32, (0, 0, 0), 0, "gemv_q8/t,nr=1,u=2,c=4,ns=1"),   # one guarded trip; the last half-wave has ONE live column
    ("t4_trips", True, 2 * CHUNK + CHUNK + 3 * PIECE, 8192 - 1, 2, 1, 128, (16, 16, 32), 4, "gemv_q8/t,nr=2,u=2,c=4,ns=1"),  # 1584 = a trip + a chunk + 3 pieces
    ("t4_8rhs", True, 2 * CHUNK + PIECE, 8192, 8, 1, 2000, (0, 0, 0), 0, "gemv_q8/t,nr=8,u=1,c=4,ns=1"),
    ("t4_split", True, 8192, 4096, 1, 1, 48, (0, 0, 0), 0, "gemv_q8/t,nr=1,u=2,c=4,ns=2"),                   # 128 workgroups: cut in two (the floor: 4096 rows per split)
    # N, outputs: one piece; one less than, equal to and one more than a workgroup's 1024 rows (in pieces); columns: fewer than the 4 waves, no multiple of 4
    ("n_piece", False, PIECE, 16, 1, 1, 16, (0, 0, 0), 0, "gemv_q8/n,nr=1,u=8,ns=1"),
    ("n_rows_minus", False, N_ROWS - PIECE, 37, 1, 1, 16, (0, 0, 0), 0, "gemv_q8/n,nr=1,u=8,ns=1"),
    ("n_rows", False, N_ROWS, 64, 1, 1, 128, (16, 16, 32), 4, "gemv_q8/n,nr=1,u=8,ns=1"),
    ("n_rows_plus", False, N_ROWS + PIECE, 5, 2, 1, 32, (0, 0, 0), 0, "gemv_q8/n,nr=2,u=8,ns=1"),            # 1040 rows in groups of 32: a partial last group; wave 3 has no column
    ("n_3rhs", False, N_ROWS + PIECE, 70, 3, 1, 2000, (0, 0, 0), 0, "gemv_q8/n,nr=4,u=8,ns=1"),              # group_rows >= rows: per column
    ("n_8rhs", False, CHUNK + PIECE, 33, 8, 1, 160, (0, 0, 0), 0, "gemv_q8/n,nr=8,u=8,ns=1"),                # 528 rows in groups of 160: divides by no power of two, partial last group
    ("n_11rhs", False, CHUNK, 20, 11, 1, 16, (0, 0, 0), 0, "gemv_q8/n,nr=8,u=8,ns=1"),
    ("n_2mats", False, N_ROWS + PIECE, 37, 2, 2, 128, (32, 16, 48), 4, "gemv_q8/n,nr=2,u=8,ns=1"),
    ("n_split", False, PIECE, 65536, 1, 1, 16, (0, 0, 0), 0, "gemv_q8/n,nr=1,u=8,ns=1024"),                   # one workgroup of rows: 1024 splits of 64 columns
    # the cut with more than one right-hand side, and with two matrices on t_2mats' strided views: the smallest shapes each cut leaf is cut at on 256 CUs (T: two
    # splits of the floor's 4096 rows; T with 4 columns per half-wave needs 128 workgroups of 32 columns for every CU to have one; N: splits of 64 columns)
    ("t_3rhs_split", True, 2 * TRIP8, T_COLS + 1, 3, 1, 128, (0, 0, 0), 0, "gemv_q8/t,nr=4,u=4,c=1,ns=2"),
    ("t_2mats_split", True, 2 * TRIP8, T_COLS + 1, 2, 2, 48, (32, 16, 48), 4, "gemv_q8/t,nr=2,u=8,c=1,ns=2"),      # 4096 is no multiple of 48: a group straddles the cut
    ("t4_3rhs_split", True, 2 * TRIP8, 4096, 3, 1, 48, (0, 0, 0), 0, "gemv_q8/t,nr=4,u=1,c=4,ns=2"),
    ("t4_2mats_split", True, 2 * TRIP8, 2048, 2, 2, 128, (32, 16, 48), 4, "gemv_q8/t,nr=2,u=2,c=4,ns=2"),
    ("n_3rhs_split", False, 3 * PIECE, 320, 3, 1, 32, (0, 0, 0), 0, "gemv_q8/n,nr=4,u=8,ns=5"),                     # 5 splits of 64 columns; 48 rows in groups of 32
    ("n_2mats_split", False, N_ROWS + PIECE, 192, 2, 2, 128, (32, 16, 48), 4, "gemv_q8/n,nr=2,u=8,ns=3"),           # a second workgroup of 16 rows
    # the element-by-element kernels: matrix offset 1, leading dimension rows + 3, rows 37, vectors at offset 1
    ("any_t", True, 37, 5, 2, 1, 16, (1, 3, 5), 1, "gemv_q8/any_t"),
    ("any_n", False, 37, 70, 3, 2, 16, (1, 3, 5), 1, "gemv_q8/any_n"),
    ("any_t_rows", True, 100, 9, 11, 1, 32, (0, 0, 0), 0, "gemv_q8/any_t"),                                  # everything aligned but the rows: 100 % 16 != 0
    ("any_n_vector", False, 64, 48, 1, 1, 64, (0, 0, 0), 1, "gemv_q8/any_n"),                                # everything aligned but the vectors' offset
]
CASE_IDS = [c[0] for c in CASES]
# the call that fills the workspace with NaN partials (its scales are NaN) before a cut case runs: N, 16 splits of 64 columns, 3072 x 16 partials -- more than any
# cut case writes, and another outputs x right-hand sides than any of them has
DIRTY = ("dirty", False, 3 * N_ROWS, 1024, 1, 1, 128, (0, 0, 0), 0, "gemv_q8/n,nr=1,u=8,ns=16")
EXACT_CASES = [c for c in CASES if (c[2] if c[1] else c[3]) <= 2048]  # the exact operands need k <= 2048


def n_groups(rows, G):
    return -(-rows // G)


def group_index(rows, G):
    return np.arange(rows) // G


def rng_of(name, salt=0):
    return np.random.default_rng(sum(map(ord, name)) * 7 + salt)


def random_inputs(case, salt=0):
    """(q int8 [R, C, Z], scales f32 [groups, C, Z], v f32 [k, nrhs, Z]): int8 over the full range, scales in [2^-8, 2^-6), v in [-1, 1)."""
    name, tr, R, C, nrhs, Z, G = case[:7]
    rng = rng_of(name, salt)
    q = rng.integers(-128, 128, (R, C, Z)).astype(np.int8)
    s = ((1 + rng.random((n_groups(R, G), C, Z), dtype=np.float32)) * np.float32(2.0 ** -8)).astype(np.float32)
    v = (rng.random((R if tr else C, nrhs, Z), dtype=np.float32) * 2 - 1).astype(np.float32)
    return q, s, v


def exact_inputs(case, scale_exp=(-2, 2), salt=1):
    """Operands whose product is exact in f32 whatever the order and wherever the scale enters: q over the full int8 range (every value of a 256-cycle, -128 included),
    integer v in [-4, 4], scales 2^e with e in scale_exp (inclusive)."""
    name, tr, R, C, nrhs, Z, G = case[:7]
    rng = rng_of(name, salt)
    q = rng.integers(-128, 128, (R, C, Z)).astype(np.int8)
    flat = q.reshape(-1)
    step = max(flat.size // 64, 2)
    flat[::step][:8] = -128  # (both ends of the range for sure, and a few more of the one value sign-magnitude thinking forgets)
    flat[1::step][:8] = 127
    s = np.ldexp(np.float32(1), rng.integers(scale_exp[0], scale_exp[1] + 1, (n_groups(R, G), C, Z))).astype(np.float32)
    v = rng.integers(-4, 5, (R if tr else C, nrhs, Z)).astype(np.float32)
    return q, s, v


def dequantized64(q, s, G):
    """W in float64, exactly (24 x 8 bits)."""
    return s.astype(np.float64)[group_index(q.shape[0], G)] * q.astype(np.float64)


def truth64(q, s, v, G, tr):
    """(op(W) v, sum |s q v|) per matrix in float64: [outputs, nrhs, Z]."""
    W = dequantized64(q, s, G)
    A = np.transpose(W, (1, 0, 2)) if tr else W
    V = v.astype(np.float64)
    return np.einsum("rkz,kyz->ryz", A, V), np.einsum("rkz,kyz->ryz", np.abs(A), np.abs(V))


def gate(k, sabs):
    """The tolerance of the contract: the project's f32 gate at twice the count (two roundings per term)."""
    return U.f32_gate(2 * k, sabs)


def assert_within_gate(got, truth, k, sabs, what=""):
    got, truth = np.asarray(got, np.float64).ravel(), np.asarray(truth, np.float64).ravel()
    tol = gate(k, np.asarray(sabs).ravel())
    err = np.abs(got - truth)
    bad = err > tol
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} elements exceed f32_gate(2 * {k}, sum|s q v|); worst err / gate = {(err / tol).max():.3g}"
    return float((err / tol).max())


def exactness_condition(q, s, v, tr):
    """(max scale / min scale) * max over outputs of sum |q||v| -- below 2^24 every partial sum, in any order and with the scale entering anywhere, is an integer
    multiple of (min scale x 1) below 2^24 of them: exact in f32 as long as min scale * 2^0 >= 2^-149."""
    A = np.abs(q.astype(np.float64))
    A = np.transpose(A, (1, 0, 2)) if tr else A
    sabs = np.einsum("rkz,kyz->ryz", A, np.abs(v.astype(np.float64))).max()
    return float(s.max() / s.min()) * float(sabs)


# ---- the float32 model -------------------------------------------------------------------------------------------------------------------------------
def _fma32(a, b, c):
    return U.fmaf_f32(a, b, c)


def model32(q, s, v, G, tr, scale="piece", order="sequential"):
    """The scaled sum in float32, for one placement of the scale and one summation order: [outputs, nrhs, Z] float32.
    scale = "element": w = fl(s q), terms fma(w, v, acc);  "piece": d = the 16 products of a piece summed by FMAs from zero, then fma(s, d, acc) -- along the
    matrix's rows, so for Gemv (whose sum runs over columns) a piece is one term and this is fl(s v) entering the vector entry: t = fl(s v), fma(q, t, acc).
    order = "sequential": one accumulator over the terms in ascending order;  "pairwise": the terms' partial sums over halves, recursively (floor 8 terms)."""
    R, C, Z = q.shape
    k, outs, nrhs = (R, C, v.shape[1]) if tr else (C, R, v.shape[1])
    gi = group_index(R, G)
    qf = q.astype(np.float32)
    out = np.zeros((outs, nrhs, Z), np.float32)
    for z in range(Z):
        for y in range(nrhs):
            if tr:  # out[c] = sum_r s[g(r), c] q[r, c] v[r]
                S = s[gi, :, z]  # [R, C]
                if scale == "element":
                    Wt = (S * qf[:, :, z]).astype(np.float32)
                    terms = [(Wt[r], np.float32(v[r, y, z])) for r in range(R)]  # fma(w, v, acc)
                    out[:, y, z] = _sum_fma(terms, outs, order)
                else:
                    pieces = []
                    for r0 in range(0, R, 16):
                        d = np.zeros(C, np.float32)
                        for r in range(r0, min(r0 + 16, R)):
                            d = _fma32(qf[r, :, z], np.float32(v[r, y, z]), d)
                        pieces.append((S[r0], d))  # fma(s, d, acc)
                    out[:, y, z] = _sum_fma(pieces, outs, order)
            else:  # out[r] = sum_c s[g(r), c] q[r, c] v[c]
                S = s[gi, :, z]  # [R, C]
                if scale == "element":
                    Wt = (S * qf[:, :, z]).astype(np.float32)
                    terms = [(Wt[:, c], np.float32(v[c, y, z])) for c in range(C)]
                else:
                    terms = [(qf[:, c, z], (S[:, c] * np.float32(v[c, y, z])).astype(np.float32)) for c in range(C)]
                out[:, y, z] = _sum_fma(terms, outs, order)
    return out


def _sum_fma(terms, n, order):
    if order == "sequential" or len(terms) <= 8:
        acc = np.zeros(n, np.float32)
        for a, b in terms:
            acc = _fma32(a, b, acc)
        return acc
    h = len(terms) // 2
    return (_sum_fma(terms[:h], n, order) + _sum_fma(terms[h:], n, order)).astype(np.float32)
