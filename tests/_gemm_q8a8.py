"""Shared by the wg_gemm_q8a8 tests (tests/test_gpu_gemm_q8a8.py on the device, tests/test_gemm_q8a8_model.py and tests/test_gemm_q8a8_plan_host.py on the CPU): the
cases, their inputs, the float64 truth, and a NumPy float32 model of the arithmetic.

The contract (include/wgebra_hip.h): out = W^T X, W[r, c, z] = scales[r // G, c, z] * m[r, c, z], X[r, j, z] = x_scales[r // Gx, j, z] * x[r, j, z]. The contraction is
divided into CHAINS: a chain ends at every boundary of a weight group and of an activation group and, inside the finer of the two groups, every 1024 rows counted from
that group's start. d = the chain's sum of m * x in int32 (exact: |d| <= 2^24), u = x_scale * (float)d (one f32 multiply), acc = fmaf(w_scale, u, acc), chains
ascending. A cut contraction: every split sums its own chains from zero, and the partials are added in the combine pass's order -- wave w adds splits w, w + 4, ...
ascending from zero, then ((w0 + w1) + w2) + w3.

The gate (derived, not measured): the chains are exact, each takes one multiply rounding and one FMA rounding, so an output of C chains is 2 C rounded terms:
f32_gate(2 C, sum over chains |w_scale * x_scale * d|)."""
import numpy as np

import _q8
import _util as U

STEP = 32        # rows of one MFMA step; the unit of both group sizes and of every cut on the MFMA leaf (wgmath_amd/csrc/gemm_q8a8_plan.hpp)
CHAIN = 1024     # rows of a chain at most
WAVE_OUT = 32    # outputs per wave
BLOCK_OUT = 128  # outputs per workgroup (4 waves)
WHOLE = 1 << 30  # a group size >= every k here: one scale per output / per column

MFMA2, MFMA4, ANY = "gemm_q8a8/mfma,nt=2,ns=1", "gemm_q8a8/mfma,nt=4,ns=1", "gemm_q8a8/any"


def _case(name, k, outputs, n, G, Gx=None, Z=1, tag=MFMA2, m=(0, 0, 0), x=(0, 0), o=(0, 0)):
    """m: (byte offset, leading-dimension padding, gap between matrices); x: (byte offset, leading-dimension padding); o: the same in floats. tag: the first tag the
    call logs on 256 CUs."""
    return dict(name=name, k=k, outputs=outputs, n=n, G=G, Gx=G if Gx is None else Gx, Z=Z, tag=tag, m=m, x=x, o=o)


CASES = (
    [_case("one_step", 32, 16, 16, 32),
     _case("outputs_minus", 32, 15, 16, 32),  # the output mask
     _case("outputs_plus", 32, 17, 16, 32)]
    # column edges: half a tile, the 4-row blocks of D, the second 32-column tile, the second pass, a last pass of 2 columns
    + [_case(f"cols_{n}", 64, 16, n, 32, tag=MFMA2 if n <= 32 else MFMA4) for n in (1, 8, 15, 17, 64, 65, 130)]
    # groups: 96 is no power of two and 512 = 5.33 groups (a partial last group); 33 outputs: a second wave with one live output
    + [_case(f"groups_{G}", 512, 33, 20, G) for G in (32, 64, 96, 128)]
    + [_case("groups_128_whole", 512, 33, 20, 128, WHOLE),
       _case("groups_whole_32", 512, 33, 20, WHOLE, 32),
       _case("groups_64_128", 512, 33, 20, 64, 128),
       _case("groups_whole_whole", 512, 33, 20, 6000, 7000),                              # no multiples of 16: one scale per output and per column
       _case("blocks", 160, 130, 33, 32, tag=MFMA4),                                     # a second workgroup; a trip (128 rows) and a guarded step; a second tile of 1 column
       _case("two_mats", 544, 17, 9, 32, Z=2, m=(32, 16, 48), x=(16, 16), o=(1, 3)),      # `out` needs only 4-byte alignment
       _case("lane_map", 64, 32, 32, 32),                                                # structured data, exact compare
       _case("chain_cap", 2080, 16, 16, WHOLE, WHOLE, tag="gemm_q8a8/mfma,nt=2,ns=3"),    # chains of 1024, 1024 and 32 rows; all -128: a full chain is exactly 2^24
       _case("cut", 131104, 16, 16, WHOLE, WHOLE, tag="gemm_q8a8/mfma,nt=2,ns=129"),      # past 2^17 rows an uncapped int32 chain of -128 * -128 overflows
       # the element-by-element kernel
       _case("any_m", 37, 7, 5, 16, tag=ANY, m=(1, 3, 5)),
       _case("any_x", 64, 9, 3, 32, tag=ANY, x=(1, 0)),
       _case("any_g16", 64, 9, 3, 16, tag=ANY),                                          # everything aligned, but G % 32 != 0
       _case("any_g16_48", 96, 5, 3, 16, 48, tag=ANY),                                   # a coarser side whose groups hold three of the finer
       _case("any_k48", 48, 5, 2, 6000, 6000, tag=ANY)])                                 # k % 16 == 0 only: not taken by the MFMA leaf
CASE_IDS = [c["name"] for c in CASES]
ALL_MIN = ("chain_cap", "cut")  # the cases whose operands are all -128


def _cut(name, k, outputs, n, G, Gx=None, Z=1, nt=2, ns=2, **views):
    return _case(name, k, outputs, n, G, Gx, Z, tag="gemm_q8a8/mfma,nt=%d,ns=%d" % (nt, ns), **views)


# The cut contraction (k over grid.y, f32 partials [z][split][n][outputs] in the workspace, a combine pass): tests/_gemm_q8.py's rows with Gx = G, and four rows on the
# chains under a cut. The cut unit is the coarser group, or 1024 rows where neither side has groups (k = 1024 ns there). tests/test_gemm_q8a8_plan_host.py pins ns and
# the rows per split of every row.
CUT_CASES = [
    _cut("cut_odd_steps", 1088, 16, 16, 32),                     # 2 x 544: 17 steps per split, the second split starts on an odd step
    _cut("cut_short_last", 1600, 33, 20, 32, ns=3),              # 544, 544, 512: a shorter last split; a second wave with one live output
    _cut("cut_g96_partial", 1120, 33, 20, 96),                   # 576, 544: 6 groups per split (no power of two); the last split ends inside a group of 64 rows
    _cut("cut_g64_views", 1152, 17, 9, 64, Z=2, m=(32, 16, 48), x=(16, 16), o=(1, 3, 5)),  # two_mats' strides and a gap between the matrices of `out`: z > 0
    _cut("cut_per_column", 2048, 33, 20, WHOLE, WHOLE),          # one scale per output and per column under a cut: 2 x 1024
    _cut("cut_passes", 1088, 130, 65, 32, nt=4),                 # T = 2 under a cut; a pass of one column; a second workgroup; the combine's third block has 2 live outputs
    _cut("cut_passes_mats", 2048, 65, 130, 128, Z=3, nt=4, ns=4),  # blockIdx.z = z * passes + pass with both above 1
    _cut("cut_ns5", 2560, 16, 16, 32, ns=5),                     # the combine: wave 0 adds two splits, waves 1 .. 3 one each
    _cut("cut_ns29", 29696, 33, 20, WHOLE, WHOLE, ns=29),        # wave 0 on the 8-wide loop, waves 1 .. 3 on the tail alone
    _cut("cut_ns32", 16384, 70, 3, 128, ns=32),                  # every wave exactly one wide trip, no tail; the combine's second block
    _cut("cut_ns33", 16896, 16, 16, 32, ns=33),                  # one tail element behind a wide trip, on wave 0 only
    _cut("cut_ns36", 18432, 16, 16, 32, ns=36),                  # one tail element on every wave
    _cut("cut_masked", 4096, 130, 130, 32, Z=2, nt=4, ns=8),     # 12 workgroups: ns 8 on 256 CUs, 6 on 16, 3 on 8
    _cut("cut_w1536", 3072, 33, 20, 1536, WHOLE),                # 2 x 1536: chains of 1024 + 512 inside each split
    _cut("cut_g64_128", 1152, 33, 20, 64, 128),                  # the unit is the coarser group: 640 + 512; G != Gx under a cut
    _cut("cut_x2048", 4096, 16, 65, WHOLE, 2048, nt=4),          # only the activation side grouped: the chain cap restarts at the split (2 x (1024 + 1024)); 2 passes
    _cut("cut_g32_whole", 1088, 17, 9, 32, WHOLE, Z=2),          # weights grouped, activations per column
]
CUT_IDS = [c["name"] for c in CUT_CASES]
CUT_LANE_MAP = _cut("cut_lane_map", 1088, 32, 32, 32)
DIRTY = _case("dirty", 4096, 256, 192, 32, tag="gemm_q8a8/mfma,nt=4,ns=8")  # the call that fills the workspace with NaN partials before a cut case runs


def out_view(c):
    """(element offset, leading-dimension padding, gap between matrices) of `out`: a case's o is (offset, padding) or all three."""
    return tuple(c["o"]) + (0,) * (3 - len(c["o"]))


def by_name(name):
    return [c for c in CASES + CUT_CASES if c["name"] == name][0]


def n_groups(k, G):
    return _q8.n_groups(k, min(G, max(k, 1)))


def random_inputs(c, salt=0):
    """(q int8 [k, outputs, Z], s f32 [groups, outputs, Z], x int8 [k, n, Z], xs f32 [x groups, n, Z]): both int8 over the full range (all -128 for the cases that
    test the chain cap), scales in [2^-8, 2^-6)."""
    k, outs, n, Z, G, Gx = c["k"], c["outputs"], c["n"], c["Z"], c["G"], c["Gx"]
    rng = _q8.rng_of(c["name"], salt)
    if c["name"] in ALL_MIN:
        q, x = np.full((k, outs, Z), -128, np.int8), np.full((k, n, Z), -128, np.int8)
    else:
        q, x = rng.integers(-128, 128, (k, outs, Z)).astype(np.int8), rng.integers(-128, 128, (k, n, Z)).astype(np.int8)
    s = ((1 + rng.random((n_groups(k, G), outs, Z), dtype=np.float32)) * np.float32(2.0 ** -8)).astype(np.float32)
    xs = ((1 + rng.random((n_groups(k, Gx), n, Z), dtype=np.float32)) * np.float32(2.0 ** -8)).astype(np.float32)
    return q, s, x, xs


def pow2_inputs(c, w_exps=(-2, 2), x_exps=(-2, 2), salt=1):
    """Operands whose product is exact in f32 whatever the order: q over the full int8 range with -128 and 127 planted, integer x in [-4, 4], every scale a power
    of two 2^e with e drawn from w_exps / x_exps. exactness_condition below states when."""
    k, outs, n, Z = c["k"], c["outputs"], c["n"], c["Z"]
    rng = _q8.rng_of(c["name"], salt + 100)
    q = rng.integers(-128, 128, (k, outs, Z)).astype(np.int8)
    q.reshape(-1)[:2] = (-128, 127)
    x = rng.integers(-4, 5, (k, n, Z)).astype(np.int8)
    s = np.ldexp(np.float32(1), rng.choice(w_exps, (n_groups(k, c["G"]), outs, Z))).astype(np.float32)
    xs = np.ldexp(np.float32(1), rng.choice(x_exps, (n_groups(k, c["Gx"]), n, Z))).astype(np.float32)
    return q, s, x, xs


def cut_pow2_inputs(c, salt=1):
    """pow2_inputs' narrower variant for the long cut cases: q over the full range with -128 and 127 planted, x in {-1, 0, 1}, every scale 2^0 or 2^1 -- 4 * 128 k stays
    below 2^24 up to k = 32767. The tests assert exactness_condition on what they draw."""
    q, s, _, xs = pow2_inputs(c, (0, 1), (0, 1), salt)
    x = _q8.rng_of(c["name"], salt + 150).integers(-1, 2, (c["k"], c["n"], c["Z"])).astype(np.int8)
    return q, s, x, xs


def exactness_condition(q, s, x, xs):
    """(largest / smallest product of two scales) * max over outputs of sum |q||x|: below 2^24 every partial sum, in any order, is an integer multiple of the
    smallest scale product below 2^24 of them -- exact in f32 (as long as that product is a multiple of 2^-149)."""
    sabs = np.einsum("rkz,kyz->ryz", np.transpose(np.abs(q.astype(np.float64)), (1, 0, 2)), np.abs(x.astype(np.float64))).max()
    s64, xs64 = s.astype(np.float64), xs.astype(np.float64)
    return (s64.max() * xs64.max()) / (s64.min() * xs64.min()) * float(sabs)


def lane_map_inputs(c, identity):
    """Structured operands for the lane-map check (tests/_gemm_q8.py: lane_map_inputs): q depends asymmetrically on (row, output); x is the identity (out = the
    weights themselves: a swapped row / column or a k permutation applied to one operand only changes the result) or an asymmetric matrix. Scales 1, 2, 4."""
    k, outs, n, Z = c["k"], c["outputs"], c["n"], c["Z"]
    r, o, col = np.arange(k)[:, None], np.arange(outs)[None, :], np.arange(n)[None, :]
    q = (((r * 7 + o * 13) % 255) - 127).astype(np.int8)[:, :, None].repeat(Z, 2)
    if identity:
        x = (r == col).astype(np.int8)[:, :, None].repeat(Z, 2)
    else:
        x = (((r * 3 + col * 5 + (r * col) % 7) % 251) - 125).astype(np.int8)[:, :, None].repeat(Z, 2)
    s = np.ldexp(np.float32(1), (np.arange(outs) % 3))[None, :, None].repeat(n_groups(k, c["G"]), 0).repeat(Z, 2).astype(np.float32)
    xs = np.ldexp(np.float32(1), (np.arange(n) % 2))[None, :, None].repeat(n_groups(k, c["Gx"]), 0).repeat(Z, 2).astype(np.float32)
    return q, s, x, xs


def cut_lane_map_inputs(c):
    """lane_map_inputs' asymmetric operands with x narrowed to [-4, 4] (tests/_gemm_q8.py's pattern): at k = 1088 the full-range x would pass the sum bound; with it
    (largest / smallest scale product = 8) * 1088 * 127 * 4 stays below 2^24."""
    q, s, _, xs = lane_map_inputs(c, False)
    r, col = np.arange(c["k"])[:, None], np.arange(c["n"])[None, :]
    x = (((r * 3 + col * 5 + (r * col) % 7) % 9) - 4).astype(np.int8)[:, :, None].repeat(c["Z"], 2)
    return q, s, x, xs


# ---- chains ------------------------------------------------------------------------------------------------------------------------------------------
def chains(k, G, Gx, begin=0, end=None):
    """[(r0, r1)] of rows [begin, end): a chain ends with the finer group, or 1024 rows further from that group's start (begin must be a chain boundary)."""
    end = k if end is None else min(end, k)
    fine = min(min(G, k), min(Gx, k))
    out, r0 = [], begin
    while r0 < end:
        fstart = r0 - r0 % fine
        r1 = min(fstart + fine, r0 + CHAIN - (r0 - fstart) % CHAIN, end)
        out.append((r0, r1))
        r0 = r1
    return out


def boundaries(k, G, Gx):
    return {0, k} | {r1 for _, r1 in chains(k, G, Gx)}


def _gi(r0, G, k):
    return r0 // G if G < k else 0


def truth64(q, s, x, xs, G, Gx):
    """(W^T X, sum over chains |w_scale x_scale d|, chains per output) in float64: [outputs, n, Z]."""
    k, outs, Z = q.shape
    n = x.shape[1]
    truth, sabs = np.zeros((outs, n, Z)), np.zeros((outs, n, Z))
    ch = chains(k, G, Gx)
    for z in range(Z):
        for r0, r1 in ch:
            d = q[r0:r1, :, z].astype(np.int64).T @ x[r0:r1, :, z].astype(np.int64)
            t = s[_gi(r0, G, k), :, z].astype(np.float64)[:, None] * xs[_gi(r0, Gx, k), :, z].astype(np.float64)[None, :] * d
            truth[:, :, z] += t
            sabs[:, :, z] += np.abs(t)
    return truth, sabs, len(ch)


def gate(nchains, sabs):
    return U.f32_gate(2 * max(nchains, 1), sabs)


# ---- the float32 model -------------------------------------------------------------------------------------------------------------------------------
def _partial(q, s, x, xs, G, Gx, z, begin, end):
    k, outs = q.shape[:2]
    acc = np.zeros((outs, x.shape[1]), np.float32)
    for r0, r1 in chains(k, G, Gx, begin, end):
        d = q[r0:r1, :, z].astype(np.int64).T @ x[r0:r1, :, z].astype(np.int64)
        assert np.abs(d).max(initial=0) <= 2 ** 24  # exact in int32 and as a float
        with np.errstate(invalid="ignore", over="ignore"):
            u = (xs[_gi(r0, Gx, k), :, z][None, :] * d.astype(np.float32)).astype(np.float32)  # ONE f32 multiply
        with np.errstate(invalid="ignore", over="ignore"):  # (non-finite scales: 0 * Inf)
            acc = U.fmaf_f32(s[_gi(r0, G, k), :, z][:, None], u, acc)
    return acc


def model32(q, s, x, xs, G, Gx, k_per_split=None):
    """The call's bits: [outputs, n, Z] float32. k_per_split: the plan's cut (None or >= k: uncut)."""
    k, outs, Z = q.shape
    out = np.zeros((outs, x.shape[1], Z), np.float32)
    for z in range(Z):
        if not k_per_split or k_per_split >= k:
            out[:, :, z] = _partial(q, s, x, xs, G, Gx, z, 0, k)
            continue
        assert set(range(0, k, k_per_split)) <= boundaries(k, G, Gx), "a cut boundary that is no chain boundary"
        parts = [_partial(q, s, x, xs, G, Gx, z, b, b + k_per_split) for b in range(0, k, k_per_split)]
        waves = []
        for w in range(4):  # wave w adds splits w, w + 4, ... ascending from zero
            t = np.zeros_like(parts[0])
            for p in parts[w::4]:
                t = (t + p).astype(np.float32)
            waves.append(t)
        out[:, :, z] = (((waves[0] + waves[1]).astype(np.float32) + waves[2]).astype(np.float32) + waves[3]).astype(np.float32)
    return out


def query_kw(c, cus=256):
    """The wg_gemm_q8a8_query a call on the case's views fills (buffers are 256-byte aligned: a view's address modulo 16 is its offset's)."""
    k, outs, n, Z, G, Gx = c["k"], c["outputs"], c["n"], c["Z"], c["G"], c["Gx"]
    (moff, mpad, gap), (xoff, xpad), (ooff, opad, ogap) = c["m"], c["x"], out_view(c)
    ldm, ldx, ldo, lds, ldxs = k + mpad, k + xpad, outs + opad, n_groups(k, G) + 1, n_groups(k, Gx) + 2
    return dict(k=k, outputs=outs, n=n, mats=Z, group_rows=G, x_group_rows=Gx, ldm=ldm, lds=lds, ldx=ldx, ldxs=ldxs, ldo=ldo, m_batch=ldm * outs + gap, s_batch=lds * outs + 2,
                x_batch=ldx * n, xs_batch=ldxs * n + 3, o_batch=ldo * n + ogap, m_addr16=moff % 16, x_addr16=xoff % 16, o_addr16=4 * ooff % 16, cus=cus)
