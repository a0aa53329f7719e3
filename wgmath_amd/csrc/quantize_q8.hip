// wg_quantize_q8: the device-side quantiser of the q8 family (include/wgebra_hip.h) -- q int8 and f32 group scales from an f32 / f16 / bf16 source, the rule of the
// Python helper quantize_q8 on the source widened exactly to f32: per group of G consecutive rows of a column s = fl32(max|x| / 127),
// q = clip(rint(fl32(x / s)), -127, 127); s == 0 gives q = 0; a group that holds a NaN or an Inf gives s = NaN, q = 0.
// The division is the correctly rounded one (the Makefile states it), per element: x * (1 / s) differs from x / s at ties. rintf rounds ties to even
// (v_rndne_f32); the clamp comes before the integer conversion. The max instructions drop NaNs, so non-finite elements are looked for explicitly.
//
//  vec: a lane per 16 consecutive rows -- 16-byte loads of the source (four for f32, two for 16 bits) and ONE 16-byte store of q. A group of G = 32 .. 1024 rows (a
//     power of two) is G / 16 = 2 .. 64 adjacent lanes of one wave: its max and its non-finite flag travel by __shfl_xor over those lanes. Lanes past the last row
//     hold zeros and store nothing (a partial last group; rows % 16 == 0, so a lane is all in or all out). grid = (workgroups per column x columns, 1, mats).
//  any: a wave (groups up to 1024 rows) or a workgroup of 256 per (group, column, matrix), two sweeps over the group's rows where they lie: the max, then the
//     quotients. Any view, any group size, one scale per column included. grid = (groups per column x columns, 1, mats).
// quantize_q8_plan below is the launcher's choice, a pure function of the query (wg_debug_quantize_q8_plan; tests/test_quantize_q8_host.py).
#include "wg_internal.hpp"

#include <cstdarg>
#include <cstdio>

namespace {

struct QArgs {
    int8_t *q; uint32_t ldq; uint64_t q_batch;
    float *s; uint32_t lds; uint64_t s_batch;
    const void *src; uint32_t ldsrc; uint64_t src_batch;
    uint32_t rows, cols, group_rows, blocks_per_col, group_lanes;
};

typedef float wg_f4 __attribute__((ext_vector_type(4)));
typedef uint32_t wg_u4 __attribute__((ext_vector_type(4)));

// DT: 0 f32, 1 f16, 2 bf16 -- the source element widened exactly
template <int DT> struct Src;
template <> struct Src<0> {
    typedef float elem;
    static __device__ __forceinline__ float widen(float x) { return x; }
};
template <> struct Src<1> {
    typedef uint16_t elem;
    static __device__ __forceinline__ float widen(uint16_t x) { return (float)__builtin_bit_cast(_Float16, x); }
};
template <> struct Src<2> {
    typedef uint16_t elem;
    static __device__ __forceinline__ float widen(uint16_t x) { return __uint_as_float((uint32_t)x << 16); }
};

// the scale of a group from its max |x| and whether it holds a non-finite element
__device__ __forceinline__ float scale_of(float mx, bool bad) { return bad ? __uint_as_float(0x7fc00000u) : mx / 127.f; }
// one quantised element; `zero`: the group's scale is 0 or NaN
__device__ __forceinline__ int quant(float x, float s, bool zero) {
    if (zero) return 0;
    const float r = rintf(x / s);
    return (int)fminf(fmaxf(r, -127.f), 127.f);
}

template <int DT>
__global__ __launch_bounds__(256) void quantize_q8_vec_kernel(QArgs a) {
    typedef typename Src<DT>::elem E;
    const uint32_t col = blockIdx.x / a.blocks_per_col, pb = blockIdx.x % a.blocks_per_col, z = blockIdx.z;
    const uint64_t row0 = ((uint64_t)pb * 256u + threadIdx.x) * 16u;
    const bool active = row0 < a.rows; // (rows % 16 == 0: all 16 rows or none)
    float v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = 0.f;
    if (active) {
        const E *sp = (const E *)a.src + z * a.src_batch + (uint64_t)col * a.ldsrc + row0;
        if (DT == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const wg_f4 t = reinterpret_cast<const wg_f4 *>(sp)[j];
#pragma unroll
                for (int i = 0; i < 4; ++i) v[4 * j + i] = t[i];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const wg_u4 t = reinterpret_cast<const wg_u4 *>(sp)[j];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    v[8 * j + 2 * i] = Src<DT>::widen((E)(t[i] & 0xffffu));
                    v[8 * j + 2 * i + 1] = Src<DT>::widen((E)(t[i] >> 16));
                }
            }
        }
    }
    float mx = 0.f;
    int bad = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float av = fabsf(v[i]);
        bad |= !(av < __uint_as_float(0x7f800000u)); // (a NaN or an Inf: fmaxf would drop the NaN)
        mx = fmaxf(mx, av);
    }
    for (uint32_t sh = 1; sh < a.group_lanes; sh <<= 1) { // (uniform; every lane of the wave takes part, the ones past the last row with zeros)
        mx = fmaxf(mx, __shfl_xor(mx, (int)sh, 64));
        bad |= __shfl_xor(bad, (int)sh, 64);
    }
    if (!active) return;
    const float s = scale_of(mx, bad != 0);
    const bool zero = bad || s == 0.f;
    wg_u4 out;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        uint32_t w = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) w |= ((uint32_t)quant(v[4 * j + i], s, zero) & 0xffu) << (8 * i);
        out[j] = w;
    }
    *reinterpret_cast<wg_u4 *>(a.q + z * a.q_batch + (uint64_t)col * a.ldq + row0) = out;
    if (threadIdx.x % a.group_lanes == 0) a.s[z * a.s_batch + (uint64_t)col * a.lds + row0 / a.group_rows] = s;
}

template <int DT>
__global__ __launch_bounds__(256) void quantize_q8_any_kernel(QArgs a) {
    typedef typename Src<DT>::elem E;
    __shared__ float red_mx[4];
    __shared__ int red_bad[4];
    const uint32_t col = blockIdx.x / a.blocks_per_col, g = blockIdx.x % a.blocks_per_col, z = blockIdx.z;
    const uint64_t r0 = (uint64_t)g * a.group_rows;
    const uint64_t r1 = min((uint64_t)a.rows, r0 + a.group_rows);
    const E *sp = (const E *)a.src + z * a.src_batch + (uint64_t)col * a.ldsrc;
    float mx = 0.f;
    int bad = 0;
    for (uint64_t r = r0 + threadIdx.x; r < r1; r += blockDim.x) {
        const float av = fabsf(Src<DT>::widen(sp[r]));
        bad |= !(av < __uint_as_float(0x7f800000u));
        mx = fmaxf(mx, av);
    }
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) {
        mx = fmaxf(mx, __shfl_xor(mx, sh, 64));
        bad |= __shfl_xor(bad, sh, 64);
    }
    if (blockDim.x > 64u) { // (uniform: a workgroup of 4 waves)
        const uint32_t wave = threadIdx.x >> 6;
        if ((threadIdx.x & 63u) == 0) { red_mx[wave] = mx; red_bad[wave] = bad; }
        __syncthreads();
        mx = fmaxf(fmaxf(red_mx[0], red_mx[1]), fmaxf(red_mx[2], red_mx[3]));
        bad = red_bad[0] | red_bad[1] | red_bad[2] | red_bad[3];
    }
    const float s = scale_of(mx, bad != 0);
    const bool zero = bad || s == 0.f;
    int8_t *qp = a.q + z * a.q_batch + (uint64_t)col * a.ldq;
    for (uint64_t r = r0 + threadIdx.x; r < r1; r += blockDim.x) qp[r] = (int8_t)quant(Src<DT>::widen(sp[r]), s, zero);
    if (threadIdx.x == 0) a.s[z * a.s_batch + (uint64_t)col * a.lds + g] = s;
}

wg_quantize_q8_plan no_launch(wg_quantize_q8_plan p, int status, const char *fmt, ...) {
    p.leaf = WG_QUANTIZE_Q8_UNSUPPORTED;
    p.status = status;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(p.message, sizeof p.message, fmt, ap);
    va_end(ap);
    return p;
}

const char *dtype_name(wg_dtype dt) { return dt == WG_F32 ? "f32" : dt == WG_F16 ? "f16" : "bf16"; }

} // namespace

// The launcher's choice: vec where a group is 2 .. 64 whole lanes of 16 rows and every 16-byte access is aligned, else any.
wg_quantize_q8_plan quantize_q8_plan(const wg_quantize_q8_query &q) {
    wg_quantize_q8_plan p = {};
    if (q.rows == 0 || q.cols == 0 || q.mats == 0) { p.leaf = WG_QUANTIZE_Q8_NOTHING; return p; }
    if (q.mats > 65535u) return no_launch(p, WG_ERR_UNSUPPORTED, "Quantize: nmats = %u exceeds 65535", q.mats);
    const uint32_t G = q.group_rows, es = q.src_elem;
    const bool g_ok = G >= 32u && G <= 1024u && (G & (G - 1u)) == 0u;
    const bool q_ok = q.q_addr16 % 16 == 0 && (q.cols <= 1 || q.ldq % 16 == 0) && (q.mats <= 1 || q.q_batch % 16 == 0);
    const bool s_ok = q.src_addr16 % 16 == 0 && (q.cols <= 1 || ((uint64_t)q.ldsrc * es) % 16 == 0) && (q.mats <= 1 || (q.src_batch * es) % 16 == 0);
    uint64_t per_col;
    if (g_ok && q.rows % 16u == 0 && q_ok && s_ok) {
        p.leaf = WG_QUANTIZE_Q8_VEC;
        p.group_lanes = G / 16u;
        p.block = 256;
        per_col = ((uint64_t)q.rows / 16u + 255u) / 256u;
    } else {
        p.leaf = WG_QUANTIZE_Q8_ANY;
        const uint32_t glen = G < q.rows ? G : q.rows;
        p.block = glen <= 1024u ? 64u : 256u;
        per_col = G >= q.rows ? 1u : (uint64_t)q.rows / G + (q.rows % G != 0);
    }
    const uint64_t gx = per_col * q.cols;
    if (gx > 0x7fffffffull) return no_launch(p, WG_ERR_UNSUPPORTED, "Quantize: %llu workgroups exceed 2^31 - 1", (unsigned long long)gx);
    p.blocks_per_col = (uint32_t)per_col;
    p.grid[0] = (uint32_t)gx; p.grid[1] = 1; p.grid[2] = q.mats;
    return p;
}

extern "C" int wg_debug_quantize_q8_plan(const wg_quantize_q8_query *query, wg_quantize_q8_plan *plan) {
    if (!query || !plan) return wg_set_error(WG_ERR_INVALID_ARG, "wg_debug_quantize_q8_plan: NULL argument");
    *plan = quantize_q8_plan(*query);
    return WG_OK;
}

int wgk_quantize_q8(wg_ctx *ctx, const wg_quantize_q8_plan &p, wg_dtype src_dtype, uint32_t group_rows, uint32_t rows, uint32_t cols, uint32_t nmats, int8_t *q, uint32_t q_ld,
                    uint64_t q_batch, float *s, uint32_t s_ld, uint64_t s_batch, wgk_mat src) {
    if (p.leaf == WG_QUANTIZE_Q8_NOTHING) return WG_OK;
    if (p.leaf == WG_QUANTIZE_Q8_UNSUPPORTED) return wg_set_error(p.status, "%s", p.message);
    QArgs a;
    a.q = q; a.ldq = q_ld; a.q_batch = q_batch;
    a.s = s; a.lds = s_ld; a.s_batch = s_batch;
    a.src = src.ptr; a.ldsrc = src.ld; a.src_batch = src.batch;
    a.rows = rows; a.cols = cols; a.group_rows = group_rows; a.blocks_per_col = p.blocks_per_col; a.group_lanes = p.group_lanes;
    const dim3 grid(p.grid[0], p.grid[1], p.grid[2]), block(p.block);
    const bool vec = p.leaf == WG_QUANTIZE_Q8_VEC;
    wg_path(ctx, "quantize_q8/%s,%s", vec ? "vec" : "any", dtype_name(src_dtype));
    if (vec) {
        if (src_dtype == WG_F32) hipLaunchKernelGGL(quantize_q8_vec_kernel<0>, grid, block, 0, ctx->stream, a);
        else if (src_dtype == WG_F16) hipLaunchKernelGGL(quantize_q8_vec_kernel<1>, grid, block, 0, ctx->stream, a);
        else hipLaunchKernelGGL(quantize_q8_vec_kernel<2>, grid, block, 0, ctx->stream, a);
    } else {
        if (src_dtype == WG_F32) hipLaunchKernelGGL(quantize_q8_any_kernel<0>, grid, block, 0, ctx->stream, a);
        else if (src_dtype == WG_F16) hipLaunchKernelGGL(quantize_q8_any_kernel<1>, grid, block, 0, ctx->stream, a);
        else hipLaunchKernelGGL(quantize_q8_any_kernel<2>, grid, block, 0, ctx->stream, a);
    }
    WG_HIP_TRY(hipGetLastError());
    return WG_OK;
}
