// wg_gemm_q4: out = W^T x with W[r, c] = scales[r / G, c] * (float)q[r, c] -- wg_gemv_q4's packed matrix (k / 2 bytes x outputs, byte j of a column = logical rows 2 j
// (low nibble) and 2 j + 1 (high nibble), q = n - 8) with one f32 scale per group of G consecutive logical rows of a column, against N columns of f16 / bf16
// activations (k x N, k contiguous), f32 result (include/wgebra_hip.h). The shape is gemm_q8.hip's: a weight is unpacked ONCE per wave whatever N is, the products run
// on v_mfma_f32_32x32x16_{f16,bf16} with the weights on the B side (D's column is the lane's output: all 16 results of a lane belong to ONE output, a group's scale is
// one load), one or two 32 x 32 accumulator tiles per wave, k cut over grid.y, column passes on grid.z, the four waves of a workgroup on adjacent 32-output blocks.
// Per group: d = the MFMA chain over the group's steps from zero, then acc = fmaf(s, d, acc). Three things differ from int8:
//
//  1. A 16-byte load is 32 rows, not 16. Lane l (c = l & 31, h = l >> 5) keeps its 16-byte load: bytes 16 h .. 16 h + 15 of the 32 bytes output c has in a DOUBLE step
//     of 64 rows, i.e. rows 32 h .. 32 h + 31 -- a wave-load covers 32 outputs x 64 consecutive rows. An MFMA sums over both halves of the wave, so the halves
//     exchange dword pairs before anything is multiplied: two v_permlane32_swap_b32 (dword 0 against dword 2, dword 1 against dword 3: lanes 32 - 63 of the first
//     operand swap with lanes 0 - 31 of the second) leave half h with rows 16 h .. 16 h + 15 of the first 32-row step in dwords 0, 1 and rows 16 h .. 16 h + 15 of the
//     second step in dwords 2, 3. From there a step is gemm_q8.hip's step: 32 consecutive rows, so Q4_0's groups of 32 never share a chain, and no weight is zeroed to
//     separate groups. Cost: 2 swaps per 64 rows and lane (1 / 16 instruction per weight; the compiler pads each pair with one s_nop). The step stays 32 rows and
//     k % 32 == 0 the condition: in a last double step of 32 rows the upper half loads nothing (its registers only travel to dwords 2, 3 of the lower half, which
//     the skipped second step would have read).
//  2. The unpack and the row order. Masking nibbles in place ((b & 0x000f000f) | 0x64006400 ...) costs 9 instructions per dword of 8 weights but yields halfword
//     pairs of rows (r, r + 4); putting them back into x's order is 4 v_perm_b32 per 8 weights on the weights (per wave and step) or 4 per 8 rows and TILE on x:
//     13 per 8 weights at best. Instead each BYTE is expanded on its own: v_perm_b32 builds {b, 0x64, b, 0x64} (both halfwords 0x6400 | byte), one v_and_b32 with
//     0x64f0640f leaves (1024 + n_lo, 1024 + 16 n_hi), and one v_pk_fma_f16 with the per-half constants {1, 1/16} and {-1032, -72} gives (q[2 j], q[2 j + 1]) --
//     exactly (1024 + 16 n <= 1264 is an f16 value; both results are integers in -8 .. 7), and in ROW ORDER: 3 instructions per 2 weights, 12 per 8, and NEITHER
//     operand is permuted; x fragments are read as gemm_q8.hip reads them. bf16 has no packed arithmetic here: the nibbles are spread to bytes (and, shift, and
//     per dword), each byte goes through v_cvt_f32_ubyteN, 8 is subtracted in f32 (packed, v_pk_add_f32) and the high halves of two floats are packed -- exact,
//     |q| <= 8 has 4 significant bits.
//  3. The budget (the disassembly of the four instances; per step of 32 rows x 32 outputs = 16 weights per lane; T = 32-column tiles per wave):
//       f16,  T = 1: 8 v_perm_b32 + 8 v_and_b32 + 8 v_pk_fma_f16 + 1 v_permlane32_swap_b32 = 25 vector instructions, 1.56 per weight; 2 MFMAs; 104 registers
//                    (88 VGPRs + 16 AGPRs); no scratch
//       f16,  T = 2: the same 25, 1.56 per weight; 4 MFMAs; 184 registers (136 + 48); no scratch
//       bf16, T = 1: 16 v_cvt_f32_ubyteN + 8 v_perm_b32 + 4 v_and_b32 + 2 v_lshrrev_b32 + 6.2 v_pk_add_f32 + 3.6 v_add_f32 (the compiler pairs three of four
//                    subtractions) + 1 swap = 41, 2.6 per weight; 2 MFMAs; 104 registers (88 + 16); no scratch
//       bf16, T = 2: 16 + 8 + 4 + 2 + 4.5 v_pk_add_f32 + 7 v_add_f32 + 1 = 42.5, 2.7 per weight; 4 MFMAs; 164 registers (132 + 32); no scratch
//     (gemm_q8.hip: 1.25 / 1.5 per weight.) On top, per step: 0.5 global_load_dwordx4 of weights and 2 T of x, about 2 to 3.5 s_nop (the swap's and the MFMA's
//     hazards), and whenever a group ends, per tile, 22 v_accvgpr_read + 8 v_pk_fma_f32 + 23 v_accvgpr_write behind the chain's last MFMA -- at G = 32 that is every
//     step, and it is what separates the G = 32, G = 128 and per-column rows of profiles/gemm_q4.txt. None of the seven kernels of this unit uses scratch memory.
//     Tried and not in: a second launch bound (4 waves per SIMD with one tile, 3 with two). The compiler then keeps d in VGPRs (92 / 132 registers, no AGPR
//     moves, 16 v_mov per tile at a group's end) and most rows gain 1 - 5 %, 4096 x 11008 at 64 f16 columns 13 - 15 % (60 -> 52 us); but the cut aims at 4
//     workgroups per CU, and where it lands just above what then fits (1032 workgroups on 768 places at 128 columns) the second round costs 14 - 20 % (91 -> 110 us).
//     It wants the cut to know the residency first. What was measured is in DESIGN.md ("Gemm on packed 4-bit weights") and README.md.
//
//  any: one element-by-element kernel for every view the streaming kernel cannot address (gemm_q4_plan.hip: streams()): a wave per output walking the columns, a
//     lane takes a byte -- two weights -- per step: w = s * q, acc = fmaf(w, (float)x, acc), even row first. Correct, not fast; everything is read where it lies.
//
// A cut writes f32 partials [z][split][n][outputs] into the context's workspace; the quantized families' one combine pass (quant_combine.hip: wgk_q_combine) adds them
// in a fixed order (no atomics: same bits every call). Outputs past the last one re-read the last one, columns past N the last column; neither is stored.
#include "wg_internal.hpp"
#include "gemm_q4_plan.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kLoads = 4;                          // 16-byte loads of weights in flight per lane
constexpr uint32_t kDouble = 2u * kGQStep;         // rows a wave-load covers: a double step
constexpr uint32_t kTrip = kDouble * kLoads;       // 256 rows

struct GQ4Args {
    const uint8_t *m; uint32_t ldm; uint64_t m_batch; // bytes
    const float *s; uint32_t lds; uint64_t s_batch;
    const uint16_t *x; uint32_t ldx; uint64_t x_batch;
    float *dst;          // the result, or the f32 partials of a cut
    uint32_t ld_dst;     // elements between columns of the destination
    uint64_t dst_batch;
    uint64_t dst_split;  // elements between splits (partials only)
    uint32_t outputs, k, n, passes, k_per_split; // k, k_per_split: logical rows
    uint32_t group_rows;       // G
    uint32_t g_eff;            // mfma: the rows of a group as the step counter sees them (G, or 2^32 - 32 for one group per output)
    uint32_t groups_per_split; // mfma: k_per_split / G where G < k (a split begins at a group's first row), else 0
    uint32_t g_shift;          // any: r / G as r >> g_shift (G a power of two); 32: one group (G >= k); 255: divide
};

typedef uint32_t wg_u4 __attribute__((ext_vector_type(4)));
typedef float wg_f2 __attribute__((ext_vector_type(2)));
typedef float wg_f16v __attribute__((ext_vector_type(16)));
typedef _Float16 wg_h2 __attribute__((ext_vector_type(2)));
typedef _Float16 wg_h8 __attribute__((ext_vector_type(8)));
typedef __bf16 wg_b8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ wg_u4 ld_piece(const uint8_t *p) { return __builtin_nontemporal_load(reinterpret_cast<const wg_u4 *>(p)); }

// 4 packed bytes (a dword: byte j = rows 2 j, 2 j + 1) as 8 f16 in 4 dwords, in row order, exactly. Per byte: {b, 0x64, b, 0x64} & 0x64f0640f is the f16 pair
// (1024 + n_lo, 1024 + 16 n_hi); fma with (1, 1/16) and (-1032, -72) leaves (n_lo - 8, n_hi - 8).
__device__ __forceinline__ void unpack8_f16(uint32_t d, uint32_t *w) {
    const wg_h2 mul = { (_Float16)1.f, (_Float16)0.0625f }, add = { (_Float16)-1032.f, (_Float16)-72.f };
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t both = __builtin_amdgcn_perm(0x64646464u, d, 0x04000400u | j | (j << 16)) & 0x64f0640fu;
        w[j] = __builtin_bit_cast(uint32_t, __builtin_elementwise_fma(__builtin_bit_cast(wg_h2, both), mul, add));
    }
}
// byte J of x as an f32 integer: v_cvt_f32_ubyteJ, named (written as (float)((x >> 8 J) & 0xff) - 8.f the compiler folds the exact -8 back into the integer side and
// converts with shift + add + v_cvt_f32_i32: 4.5 instructions per weight instead of 2.4)
template <int J>
__device__ __forceinline__ float ubyte(uint32_t x) {
    float f;
    if constexpr (J == 0) asm("v_cvt_f32_ubyte0 %0, %1" : "=v"(f) : "v"(x));
    else if constexpr (J == 1) asm("v_cvt_f32_ubyte1 %0, %1" : "=v"(f) : "v"(x));
    else if constexpr (J == 2) asm("v_cvt_f32_ubyte2 %0, %1" : "=v"(f) : "v"(x));
    else asm("v_cvt_f32_ubyte3 %0, %1" : "=v"(f) : "v"(x));
    return f;
}
// the high halves of two floats as a bf16 pair (the low halves are zero here: nothing is cut off)
__device__ __forceinline__ uint32_t hi_halves(wg_f2 f) { return __builtin_amdgcn_perm(__float_as_uint(f[1]), __float_as_uint(f[0]), 0x07060302u); }
// ... as 8 bf16: the nibbles spread to bytes (lo: rows 0, 2, 4, 6; hi: rows 1, 3, 5, 7), each byte to f32, minus 8 in f32, the high halves of the floats
// (|q| <= 8 has 4 significant bits)
__device__ __forceinline__ void unpack8_bf16(uint32_t d, uint32_t *w) {
    const uint32_t lo = d & 0x0f0f0f0fu, hi = (d >> 4) & 0x0f0f0f0fu;
    const wg_f2 eight = { 8.f, 8.f };
    w[0] = hi_halves(wg_f2{ ubyte<0>(lo), ubyte<0>(hi) } - eight);
    w[1] = hi_halves(wg_f2{ ubyte<1>(lo), ubyte<1>(hi) } - eight);
    w[2] = hi_halves(wg_f2{ ubyte<2>(lo), ubyte<2>(hi) } - eight);
    w[3] = hi_halves(wg_f2{ ubyte<3>(lo), ubyte<3>(hi) } - eight);
}

template <bool BF> struct Elem;
template <> struct Elem<false> {
    typedef wg_h8 v8;
    static __device__ __forceinline__ void unpack8(uint32_t d, uint32_t *w) { unpack8_f16(d, w); }
    static __device__ __forceinline__ wg_f16v mfma(v8 a, v8 b, wg_f16v c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ float widen(uint16_t x) { return (float)__builtin_bit_cast(_Float16, x); }
};
template <> struct Elem<true> {
    typedef wg_b8 v8;
    static __device__ __forceinline__ void unpack8(uint32_t d, uint32_t *w) { unpack8_bf16(d, w); }
    static __device__ __forceinline__ wg_f16v mfma(v8 a, v8 b, wg_f16v c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ float widen(uint16_t x) { return __uint_as_float((uint32_t)x << 16); }
};

// the halves of the wave exchange dword pairs: before, half h holds rows 32 h .. 32 h + 31 of a double step (8 rows per dword); after, dwords 0, 1 hold rows
// 16 h .. 16 h + 15 of its first step and dwords 2, 3 rows 16 h .. 16 h + 15 of its second. All 64 lanes are active here.
__device__ __forceinline__ wg_u4 exchange(wg_u4 q) {
    const auto a = __builtin_amdgcn_permlane32_swap(q[0], q[2], false, false);
    const auto b = __builtin_amdgcn_permlane32_swap(q[1], q[3], false, false);
    return (wg_u4){ a[0], b[0], a[1], b[1] };
}

// ------------------------------------------------------------------------------------------------------
// mfma: dst[o, n] = sum_g s[g, o] * (sum_{r in g} q[r, o] x[r, n]), a wave per 32 outputs and T 32-column tiles, rows of this split
// grid = (blocks of 128 outputs, splits, mats * column passes)
// ------------------------------------------------------------------------------------------------------
template <bool BF, int T>
__global__ __launch_bounds__(kThreads) void gemm_q4_mfma_kernel(GQ4Args a) {
    typedef Elem<BF> E;
    typedef typename E::v8 v8;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t c = lane & 31u, h = lane >> 5;
    const uint64_t o0 = ((uint64_t)blockIdx.x * kGQWaves + wave) * kGQWaveOut;
    if (o0 >= a.outputs) return; // whole waves leave; there is no barrier below
    const uint32_t z = blockIdx.z / a.passes, n0 = (blockIdx.z % a.passes) * (32u * T);
    const uint32_t r_begin = blockIdx.y * a.k_per_split;
    const uint32_t r_end = (uint32_t)min((uint64_t)a.k, (uint64_t)r_begin + a.k_per_split);
    const uint32_t o = (uint32_t)min(o0 + c, (uint64_t)a.outputs - 1u); // an output past the last one re-reads the last one and is not stored
    const uint8_t *mp = a.m + z * a.m_batch + (uint64_t)o * a.ldm + 16u * h; // + r / 2: the lane's 16 bytes of the double step at row r
    const float *sp = a.s + z * a.s_batch + (uint64_t)o * a.lds;
    const uint16_t *xp[T];
#pragma unroll
    for (int t = 0; t < T; ++t) { // likewise a column past the last one
        const uint32_t col = min(n0 + 32u * t + c, a.n - 1u);
        xp[t] = a.x + z * a.x_batch + (uint64_t)col * a.ldx + 16u * h;
    }

    wg_f16v acc[T], d[T];
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) { acc[t][i] = 0.f; d[t][i] = 0.f; }

    // the load cursor's group: index into the scales and rows left in it (uniform; a split begins at a group's first row)
    uint32_t g = blockIdx.y * a.groups_per_split, gleft = a.g_eff;

    // one step: rows r .. r + 31 of every output and column of the wave (r uniform); q0, q1: the lane's 8 bytes, rows r + 16 h .. r + 16 h + 15;
    // `last`: the step ends its group or the split
    auto step = [&](uint32_t r, uint32_t q0, uint32_t q1, float s, bool last) {
        uint32_t w[8];
        E::unpack8(q0, w);
        E::unpack8(q1, w + 4);
        const v8 w_lo = __builtin_bit_cast(v8, (wg_u4){ w[0], w[1], w[2], w[3] }), w_hi = __builtin_bit_cast(v8, (wg_u4){ w[4], w[5], w[6], w[7] });
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const wg_u4 *x = reinterpret_cast<const wg_u4 *>(xp[t] + r);
            const v8 x_lo = __builtin_bit_cast(v8, x[0]), x_hi = __builtin_bit_cast(v8, x[1]);
            d[t] = E::mfma(x_lo, w_lo, d[t]);
            d[t] = E::mfma(x_hi, w_hi, d[t]);
        }
        if (last) { // (uniform)
#pragma unroll
            for (int t = 0; t < T; ++t)
#pragma unroll
                for (int i = 0; i < 16; ++i) { acc[t][i] = fmaf(s, d[t][i], acc[t][i]); d[t][i] = 0.f; }
        }
    };
    // the scale of the step the load cursor stands on, and whether that step ends its group; moves the cursor on
    auto next_group = [&](float &s, bool &ends) {
        s = sp[g];
        gleft -= kGQStep;
        ends = gleft == 0u;
        if (ends) { gleft = a.g_eff; ++g; }
    };

    uint32_t r0 = r_begin;
    for (; (uint64_t)r0 + kTrip <= r_end; r0 += kTrip) { // whole trips: kLoads 16-byte loads in flight per lane, 2 kLoads steps
        wg_u4 q[kLoads];
        float s[2 * kLoads];
        bool ends[2 * kLoads];
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
            q[u] = ld_piece(mp + (r0 + kDouble * u) / 2u);
            next_group(s[2 * u], ends[2 * u]);
            next_group(s[2 * u + 1], ends[2 * u + 1]);
        }
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
            const wg_u4 e = exchange(q[u]);
            const uint32_t r = r0 + kDouble * u;
            step(r, e[0], e[1], s[2 * u], ends[2 * u]);
            step(r + kGQStep, e[2], e[3], s[2 * u + 1], ends[2 * u + 1] || (uint64_t)r + kDouble >= r_end);
        }
    }
    if (r0 < r_end) { // what is left (< one trip): one guarded trip. k % 32 == 0: a step is all in or all out; a double step may have its first step only, and then
                      // the upper half's 16 bytes lie past the end: they are not loaded (what the lower half gets for them in dwords 2, 3 is never read)
        wg_u4 q[kLoads];
        float s[2 * kLoads];
        bool ends[2 * kLoads];
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
            const uint64_t r = (uint64_t)r0 + kDouble * u; // (64 bits: a tail next to 2^32 rows must not wrap into range)
            q[u] = (wg_u4){ 0u, 0u, 0u, 0u };
            if (r < r_end) {
                if (r + kGQStep * h < r_end) q[u] = ld_piece(mp + r / 2u);
                next_group(s[2 * u], ends[2 * u]);
                if (r + kGQStep < r_end) next_group(s[2 * u + 1], ends[2 * u + 1]);
            }
        }
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
            const uint64_t r = (uint64_t)r0 + kDouble * u;
            if (r < r_end) { // (uniform)
                const wg_u4 e = exchange(q[u]);
                step((uint32_t)r, e[0], e[1], s[2 * u], ends[2 * u] || r + kGQStep >= r_end);
                if (r + kGQStep < r_end) step((uint32_t)r + kGQStep, e[2], e[3], s[2 * u + 1], ends[2 * u + 1] || r + kDouble >= r_end);
            }
        }
    }

    // C/D of 32x32x16: column = lane & 31 (the output), row = (i & 3) + 8 (i >> 2) + 4 (lane >> 5) (the column of x): 128 contiguous bytes per wave-instruction
    if (o0 + c < a.outputs) {
        float *dp = a.dst + z * a.dst_batch + blockIdx.y * a.dst_split + o0 + c;
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const uint32_t col = n0 + 32u * t + (i & 3) + 8u * (i >> 2) + 4u * h;
                if (col < a.n) dp[(uint64_t)col * a.ld_dst] = acc[t][i];
            }
    }
}

// ------------------------------------------------------------------------------------------------------
// Any view, element by element: a wave per output, the columns one after the other, a byte (rows 2 j, 2 j + 1) per lane and step. grid = (outputs, 1, mats), 64 threads
// ------------------------------------------------------------------------------------------------------
template <bool BF>
__global__ __launch_bounds__(64) void gemm_q4_any_kernel(GQ4Args a) {
    const uint32_t o = blockIdx.x, lane = threadIdx.x, z = blockIdx.z;
    const uint8_t *mp = a.m + z * a.m_batch + (uint64_t)o * a.ldm;
    const float *sp = a.s + z * a.s_batch + (uint64_t)o * a.lds;
    const uint32_t bytes = a.k / 2u; // (k is even: k = 2 * m.rows)
    for (uint32_t col = 0; col < a.n; ++col) {
        const uint16_t *xp = a.x + z * a.x_batch + (uint64_t)col * a.ldx;
        float acc = 0.f;
        for (uint32_t j = lane; j < bytes; j += 64u) {
            const uint32_t r = 2u * j; // both rows of a byte lie in one group: G is even or >= k
            const uint32_t g = a.g_shift < 32u ? r >> a.g_shift : a.g_shift == 32u ? 0u : r / a.group_rows;
            const float s = sp[g];
            const uint32_t b = mp[j];
            const float w0 = s * ((float)(b & 15u) - 8.f), w1 = s * ((float)(b >> 4) - 8.f);
            acc = fmaf(w0, Elem<BF>::widen(xp[r]), acc);
            acc = fmaf(w1, Elem<BF>::widen(xp[(uint64_t)r + 1u]), acc);
        }
#pragma unroll
        for (int sh = 32; sh >= 1; sh >>= 1) acc += __shfl_xor(acc, sh, 64);
        if (lane == 0) a.dst[z * a.dst_batch + (uint64_t)col * a.ld_dst + o] = acc;
    }
}

} // namespace

// Launch only: kernel, column tile, cut, grid and workspace are the plan's (gemm_q4_plan.hip); the tags logged are gemm_q4_tags(p, bf16).
int wgk_gemm_q4(wg_ctx *ctx, const wg_gemm_q4_plan &p, bool bf16, uint32_t group_rows, uint32_t k, uint32_t outputs, uint32_t n, uint32_t nmats, float *out, uint32_t out_ld,
                uint64_t out_batch, wgk_mat m, wgk_mat s, wgk_mat x) {
    if (p.leaf == WG_GEMM_Q4_NOTHING) return WG_OK;
    if (p.leaf == WG_GEMM_Q4_UNSUPPORTED) return wg_set_error(p.status, "%s", p.message);
    GQ4Args a;
    a.m = (const uint8_t *)m.ptr; a.ldm = m.ld; a.m_batch = m.batch;
    a.s = (const float *)s.ptr; a.lds = s.ld; a.s_batch = s.batch;
    a.x = (const uint16_t *)x.ptr; a.ldx = x.ld; a.x_batch = x.batch;
    a.outputs = outputs; a.k = k; a.n = n; a.passes = p.col_passes; a.k_per_split = p.k_per_split;
    a.group_rows = group_rows;
    const wgk_q_groups g = wgk_q_group_args(group_rows, k, p.k_per_split, kGQStep);
    a.g_eff = g.g_eff; a.groups_per_split = g.groups_per_split; a.g_shift = g.g_shift;
    wgk_q_dst d;
    if (int rc = wgk_q_destination(ctx, p.nsplit, p.workspace_bytes, outputs, n, out, out_ld, out_batch, &d)) return rc;
    a.dst = d.dst; a.ld_dst = d.ld_dst; a.dst_batch = d.dst_batch; a.dst_split = d.dst_split;
    const wgq::Tags tags = gemm_q4_tags(p, bf16);
    const dim3 grid(p.grid[0], p.grid[1], p.grid[2]), block(p.block);
    wg_path(ctx, "%s", tags.tag[0]);
    if (p.leaf == WG_GEMM_Q4_MFMA) {
        if (p.col_tiles == 2) {
            if (bf16) hipLaunchKernelGGL((gemm_q4_mfma_kernel<true, 1>), grid, block, 0, ctx->stream, a);
            else hipLaunchKernelGGL((gemm_q4_mfma_kernel<false, 1>), grid, block, 0, ctx->stream, a);
        } else {
            if (bf16) hipLaunchKernelGGL((gemm_q4_mfma_kernel<true, 2>), grid, block, 0, ctx->stream, a);
            else hipLaunchKernelGGL((gemm_q4_mfma_kernel<false, 2>), grid, block, 0, ctx->stream, a);
        }
    } else {
        if (bf16) hipLaunchKernelGGL((gemm_q4_any_kernel<true>), grid, block, 0, ctx->stream, a);
        else hipLaunchKernelGGL((gemm_q4_any_kernel<false>), grid, block, 0, ctx->stream, a);
    }
    WG_HIP_TRY(hipGetLastError());
    if (p.nsplit > 1) {
        wg_path(ctx, "%s", tags.tag[1]);
        if (int rc = wgk_q_combine(ctx, true, a.dst, p.nsplit, outputs, n, nmats, out, out_ld, out_batch)) return rc;
    }
    return WG_OK;
}
