// Operator front-end of the C ABI: the host-side half of Gemm/Gemv/Reduce/OpAssign::dispatch.
// Mirrors, check for check, wgebra gemm.rs:75-126, gemv.rs:74-136, reduce.rs:100-113, op_assign.rs:79-94 and the
// silent-skip rules of wgcore kernel.rs:111-123,144; adds the bounds/alignment checks the reference leaves to UB, and the check wgpu makes before the reference's
// kernels ever run: a view that is written must not share memory with a view the same call reads (check_alias; the rule: include/wgebra_hip.h).
#include "wg_internal.hpp"
#include "views_overlap.hpp"
#include "gemv_q8_plan.hpp"
#include "gemv_q4_plan.hpp"
#include "gemm_q8_plan.hpp"
#include "gemm_q4_plan.hpp"
#include "gemm_q8a8_plan.hpp"
#include "gemv_plan.hpp"

namespace {

struct View {
    uint32_t rows, cols, mats, stride, stride_mat, offset;
};
inline View mk(const wg_view_shape &s) { return { s.size[0], s.size[1], s.size[2], s.stride, s.stride_mat, s.offset }; }

// Largest element index the view touches + 1 (0 for an empty view).
inline uint64_t extent(const View &v) {
    if (v.rows == 0 || v.cols == 0 || v.mats == 0) return 0;
    return (uint64_t)(v.mats - 1) * v.stride_mat + v.offset + (uint64_t)(v.rows - 1) + (uint64_t)(v.cols - 1) * v.stride + 1;
}

// (es: bytes per element -- wg_dtype_size(dt) below; wg_gemv_q8 passes the 1 of its int8 matrix, which no wg_dtype names)
int check_bounds_es(const char *op, const char *name, const View &v, const wg_buf *b, size_t es) {
    const uint64_t need = extent(v), have = b->bytes / es;
    if (need > have)
        return wg_set_error(WG_ERR_OUT_OF_BOUNDS, "%s: view `%s` addresses %llu elements but its buffer holds %llu", op, name,
                            (unsigned long long)need, (unsigned long long)have);
    return WG_OK;
}
int check_bounds(const char *op, const char *name, const View &v, const wg_buf *b, wg_dtype dt) { return check_bounds_es(op, name, v, b, wg_dtype_size(dt)); }

// The aliasing rule (include/wgebra_hip.h): the written view `w` of a call must not share a byte with a view `r` it reads. Asked after the bounds checks and before
// anything is launched or logged, on the views the call really addresses (the ones check_bounds gets) and on addresses -- base_*: element 0 of each view's buffer --,
// not on wg_buf identity. The predicate is views_overlap.hip: disjoint byte intervals cost a few comparisons.
inline wg_view_shape shape_of(const View &v) {
    wg_view_shape s;
    s.size[0] = v.rows; s.size[1] = v.cols; s.size[2] = v.mats; s.stride = v.stride; s.stride_mat = v.stride_mat; s.offset = v.offset;
    return s;
}
// (the one place that words WG_ERR_ALIASED: every operator and both element-size forms below report through it)
int aliased(const char *op, const char *wname, const char *rname, int exact) {
    if (exact) return wg_set_error(WG_ERR_ALIASED, "%s: `%s` overlaps `%s` (the written view shares memory with a view the call reads)", op, wname, rname);
    return wg_set_error(WG_ERR_ALIASED, "%s: `%s` may overlap `%s` (their byte ranges intersect and they have more than %d column runs between them: not decided exactly)", op,
                        wname, rname, WG_VIEWS_OVERLAP_MAX_RUNS);
}
int check_alias(const char *op, wg_dtype dt, const char *wname, const View &w, const void *base_w, const char *rname, const View &r, const void *base_r) {
    int exact = 1;
    if (!wg_views_overlap(shape_of(w), (uint64_t)(uintptr_t)base_w, shape_of(r), (uint64_t)(uintptr_t)base_r, (uint32_t)wg_dtype_size(dt), &exact)) return WG_OK;
    return aliased(op, wname, rname, exact);
}
// ... for a written f32 view against a read view of 16-bit elements (wg_gemv_mixed: `out` and `m` may live in one buffer): in 2-byte units (views_overlap.hpp)
int check_alias_f32_u16(const char *op, const char *wname, const View &w, const void *base_w, const char *rname, const View &r, const void *base_r) {
    int exact = 1;
    if (!wg_views_overlap_f32_u16(shape_of(w), (uint64_t)(uintptr_t)base_w, shape_of(r), (uint64_t)(uintptr_t)base_r, &exact)) return WG_OK;
    return aliased(op, wname, rname, exact);
}
// ... and against a read view of 1-byte elements (wg_gemv_q8: `out` and the int8 matrix): in 1-byte units
int check_alias_f32_u8(const char *op, const char *wname, const View &w, const void *base_w, const char *rname, const View &r, const void *base_r) {
    int exact = 1;
    if (!wg_views_overlap_f32_u8(shape_of(w), (uint64_t)(uintptr_t)base_w, shape_of(r), (uint64_t)(uintptr_t)base_r, &exact)) return WG_OK;
    return aliased(op, wname, rname, exact);
}
inline View one_element() { return View{ 1, 1, 1, 1, 1, 0 }; } // the result scalar of a Reduce: element 0 of its buffer

// The reference's kernels bind every buffer as array<vec4<f32>> (gemm.wgsl:9-14, gemv.wgsl:9-14) and convert shapes with
// with_vec4_elts (shape.wgsl:64-66): rows, stride, stride_mat and offset must be multiples of 4 for that to address
// the same elements. (stride only matters with > 1 column, stride_mat with > 1 matrix: GpuMatrix::column sets
// stride = 1 and GpuCubeView::matrix sets stride_mat = 1, tensor.rs:474,574-584.) Views like that go to the kernels as they
// are (16-byte accesses); all others are staged (gemm_staged / gemv_staged below).
inline bool vec4_ok(const View &v) { return !(v.rows % 4 || v.offset % 4 || (v.cols > 1 && v.stride % 4) || (v.mats > 1 && v.stride_mat % 4)); }
int check_common(const char *op, const wg_ctx *ctx, wg_dtype dtype, const wg_buf *const *bufs, int n) {
    if (!ctx) return wg_set_error(WG_ERR_INVALID_ARG, "%s: ctx is NULL", op);
    if (dtype != WG_F32 && dtype != WG_F16 && dtype != WG_BF16) return wg_set_error(WG_ERR_INVALID_ARG, "%s: unknown dtype %d", op, (int)dtype);
    for (int i = 0; i < n; ++i) {
        if (!bufs[i]) return wg_set_error(WG_ERR_INVALID_ARG, "%s: buffer argument %d is NULL", op, i);
        if (bufs[i]->ctx->device != ctx->device)
            return wg_set_error(WG_ERR_INVALID_ARG, "%s: buffer argument %d lives on device %d, the context on device %d", op, i,
                                bufs[i]->ctx->device, ctx->device);
    }
    return WG_OK;
}

inline const void *elem_ptr(const wg_buf *b, uint64_t elem, wg_dtype dt) { return (const char *)b->ptr + elem * wg_dtype_size(dt); }

inline uint32_t up8(uint32_t x) { return (x + 7u) & ~7u; }

// Views that are not vec4-aligned. The reference's kernels cannot address them (they bind array<vec4<f32>> and divide rows, strides
// and offsets by 4, shape.wgsl:64-66: a slice at an odd row, a column block with an odd stride or a length that is not a multiple of
// 4 reads the wrong elements there), yet its own constructors hand them out (GpuMatrix::slice / rows / column, tensor.rs:574-626).
// Here they compute op(A) B exactly as the aligned call would. Offsets, leading dimensions and batch strides are free (the kernels' 16-byte
// accesses and LDS-DMA take element-aligned addresses); an operand that carries a LENGTH that is not a multiple of 4 is staged into a dense
// zero-padded copy (the length rounded up to 8; zeros add nothing to a dot product), the usual kernels run, and a padded result is copied back
// into the output view -- HBM-bound passes in a fourth context scratch (it cannot grow inside a recording).
// the Gemm launcher of an element type (f32; the 16-bit family compiled for f16 and for bf16)
// (odt: the element type of C -- dtype itself, or WG_F32 over 16-bit operands: wg_gemm_out32)
int gemm_launch(wg_ctx *ctx, bool tr, wg_dtype dtype, wg_dtype odt, uint32_t M, uint32_t N, uint32_t K, uint32_t mats, void *C, uint32_t ldc, uint64_t c_batch, wgk_mat A,
                wgk_mat B, float alpha, float beta) {
    if (odt != dtype) {
        if (dtype == WG_BF16) return wgk_gemm_bf16o32(ctx, tr, M, N, K, mats, (float *)C, ldc, c_batch, A, B, alpha, beta);
        return wgk_gemm_f16o32(ctx, tr, M, N, K, mats, (float *)C, ldc, c_batch, A, B, alpha, beta);
    }
    if (dtype == WG_F32) return wgk_gemm_f32(ctx, tr, M, N, K, mats, (float *)C, ldc, c_batch, A, B, alpha, beta);
    if (dtype == WG_BF16) return wgk_gemm_bf16(ctx, tr, M, N, K, mats, (wg_bf16 *)C, ldc, c_batch, A, B, alpha, beta);
    return wgk_gemm_f16(ctx, tr, M, N, K, mats, (__half *)C, ldc, c_batch, A, B, alpha, beta);
}

int gemm_staged(wg_ctx *ctx, bool tr, wg_dtype dtype, wg_dtype odt, float alpha, float beta, wg_buf *out, const View &o, const wg_buf *m1, const View &a, const wg_buf *m2,
                const View &b, uint32_t M, uint32_t N, uint32_t K) {
    const size_t es = wg_dtype_size(dtype), ces = wg_dtype_size(odt); // (one element size per operand: the output's may differ, wg_gemm_out32)
    // Only the operands that need it are copied (round 6: a 16384 x 16384 matrix times ONE column -- N % 4 != 0, nothing else -- paid 800 us for the copy
    // of the matrix, 177 us now): a dimension that is not a multiple of 4 is rounded up to 8 in the two operands that carry it, an operand
    // whose own view is not vec4-aligned is copied at the (possibly padded) sizes, the others are used where they lie.
    const uint32_t Mp = M % 4 ? up8(M) : M, Np = N % 4 && !(dtype != WG_F32 || M > 128u) ? up8(N) : N, Kp = K % 4 ? up8(K) : K, mats = o.mats; // (f16 / bf16: any N as it is)
    // (the kernels take any offset / leading dimension / batch stride -- element-aligned LDS-DMA and 16-byte accesses --: only lengths are padded)
    const bool sa = Mp != M || Kp != K, sb = Kp != K || Np != N, sc = Mp != M || Np != N;
    const uint64_t ae = sa ? (uint64_t)Mp * Kp : 0, be = sb ? (uint64_t)Kp * Np : 0, ce = sc ? (uint64_t)Mp * Np : 0;
    if (ae * mats >= (1ull << 32) || be * mats >= (1ull << 32) || ce * mats >= (1ull << 32))
        return wg_set_error(WG_ERR_UNSUPPORTED, "Gemm: operands too large for the staging path of views that are not vec4-aligned");
    void *ws = nullptr;
    // (a padded operand has a dimension rounded up to 8, so every region is a multiple of 16 bytes and the output's copy starts 16-byte aligned)
    if (int rc = wg_ctx_stage_workspace(ctx, (size_t)((ae + be) * mats * es + ce * mats * ces), &ws)) return rc;
    char *ap = (char *)ws, *bp = ap + ae * mats * es, *cp = bp + be * mats * es;
    wg_path(ctx, "stage%s>", !sc ? "" : beta != 0.f ? "/c=seed" : "/c");
    const uint32_t a_ld = tr ? Kp : Mp;
    wgk_mat A = { elem_ptr(m1, a.offset, dtype), a.stride, a.stride_mat }, B = { elem_ptr(m2, b.offset, dtype), b.stride, b.stride_mat };
    void *C = (void *)elem_ptr(out, o.offset, odt);
    uint32_t ldc = o.stride;
    uint64_t c_batch = o.stride_mat;
    if (sa) {
        if (int rc = wgk_stage_copy(ctx, dtype, ap, a_ld, ae, tr ? Kp : Mp, tr ? Mp : Kp, A.ptr, a.stride, a.stride_mat, a.rows, a.cols, mats)) return rc;
        A = wgk_mat{ ap, a_ld, ae };
    }
    if (sb) {
        if (int rc = wgk_stage_copy(ctx, dtype, bp, Kp, be, Kp, Np, B.ptr, b.stride, b.stride_mat, b.rows, b.cols, mats)) return rc;
        B = wgk_mat{ bp, Kp, be };
    }
    if (sc) {
        if (beta != 0.f)
            if (int rc = wgk_stage_copy(ctx, odt, cp, Mp, ce, Mp, Np, C, o.stride, o.stride_mat, M, N, mats)) return rc;
        C = cp; ldc = Mp; c_batch = ce;
    }
    if (int rc = gemm_launch(ctx, tr, dtype, odt, Mp, Np, Kp, mats, C, ldc, c_batch, A, B, alpha, beta)) return rc;
    if (!sc) return WG_OK;
    return wgk_stage_copy(ctx, odt, (void *)elem_ptr(out, o.offset, odt), o.stride, o.stride_mat, M, N, cp, Mp, ce, Mp, Np, mats);
}

int gemv_staged(wg_ctx *ctx, bool tr, wg_dtype dtype, wg_buf *out, const View &o, const wg_buf *m, const View &mm, const wg_buf *v, const View &vv,
                uint32_t rows_out, uint32_t k) {
    const size_t es = wg_dtype_size(dtype);
    // (as gemm_staged: only what needs it is copied -- a vector at an odd offset no longer costs a copy of the matrix)
    const uint32_t Op = rows_out % 4 ? up8(rows_out) : rows_out, Kp = k % 4 ? up8(k) : k, nrhs = o.cols, mats = o.mats;
    const uint32_t Rp = tr ? Kp : Op, Cp = tr ? Op : Kp;
    const bool sm = !vec4_ok(mm) || Op != rows_out || Kp != k, sv = !vec4_ok(vv) || Kp != k, so = !vec4_ok(o) || Op != rows_out;
    const uint64_t me = sm ? (uint64_t)Rp * Cp : 0, ve = sv ? (uint64_t)Kp * nrhs : 0, oe = so ? (uint64_t)Op * nrhs : 0;
    if (me * mats >= (1ull << 32) || ve * mats >= (1ull << 32) || oe * mats >= (1ull << 32))
        return wg_set_error(WG_ERR_UNSUPPORTED, "Gemv: operands too large for the staging path of views that are not vec4-aligned");
    // the matrix itself is off (offset, leading dimension or lengths): one pass over it where it lies, vectors and result addressed element by element (gemv_any.hip)
    if (sm) {
        if (k == 0) return wgk_stage_copy(ctx, dtype, (void *)elem_ptr(out, o.offset, dtype), o.stride, o.stride_mat, rows_out, nrhs, out->ptr, 1, 0, 0, 0, mats); // (an empty sum)
        return wgk_gemv_any(ctx, tr, dtype, mm.rows, mm.cols, nrhs, mats, (void *)elem_ptr(out, o.offset, dtype), o.stride, o.stride_mat,
                            wgk_mat{ elem_ptr(m, mm.offset, dtype), mm.stride, mm.stride_mat }, wgk_mat{ elem_ptr(v, vv.offset, dtype), vv.stride, vv.stride_mat });
    }
    void *ws = nullptr;
    if (int rc = wg_ctx_stage_workspace(ctx, (size_t)((me + ve + oe) * mats * es), &ws)) return rc;
    char *mp = (char *)ws, *vp = mp + me * mats * es, *op = vp + ve * mats * es;
    wgk_mat Mx = { elem_ptr(m, mm.offset, dtype), mm.stride, mm.stride_mat }, Vx = { elem_ptr(v, vv.offset, dtype), vv.stride, vv.stride_mat };
    void *O = (void *)elem_ptr(out, o.offset, dtype);
    uint32_t ldo = o.stride;
    uint64_t o_batch = o.stride_mat;
    if (sm) {
        if (int rc = wgk_stage_copy(ctx, dtype, mp, Rp, me, Rp, Cp, Mx.ptr, mm.stride, mm.stride_mat, mm.rows, mm.cols, mats)) return rc;
        Mx = wgk_mat{ mp, Rp, me };
    }
    if (sv) {
        if (int rc = wgk_stage_copy(ctx, dtype, vp, Kp, ve, Kp, nrhs, Vx.ptr, vv.stride, vv.stride_mat, k, nrhs, mats)) return rc;
        Vx = wgk_mat{ vp, Kp, ve };
    }
    if (so) { O = op; ldo = Op; o_batch = oe; }
    wg_path(ctx, "stage>");
    if (int rc = wgk_gemv(ctx, tr, dtype, Op, Kp, nrhs, mats, O, ldo, o_batch, Mx, Vx)) return rc;
    if (!so) return WG_OK;
    return wgk_stage_copy(ctx, dtype, (void *)elem_ptr(out, o.offset, dtype), o.stride, o.stride_mat, rows_out, nrhs, op, Op, oe, Op, nrhs, mats);
}

// wg_gemv_mixed on views the vec4 kernels cannot address: gemv_staged with an element type per operand (the matrix md, vectors and result f32)
int gemv_mixed_staged(wg_ctx *ctx, bool tr, wg_dtype md, wg_buf *out, const View &o, const wg_buf *m, const View &mm, const wg_buf *v, const View &vv, uint32_t rows_out,
                      uint32_t k) {
    const uint32_t Op = rows_out % 4 ? up8(rows_out) : rows_out, Kp = k % 4 ? up8(k) : k, nrhs = o.cols, mats = o.mats;
    const bool sm = !vec4_ok(mm) || Op != rows_out || Kp != k, sv = !vec4_ok(vv), so = !vec4_ok(o);
    const uint64_t ve = sv ? (uint64_t)Kp * nrhs : 0, oe = so ? (uint64_t)Op * nrhs : 0;
    if (ve * mats >= (1ull << 32) || oe * mats >= (1ull << 32))
        return wg_set_error(WG_ERR_UNSUPPORTED, "Gemv: operands too large for the staging path of views that are not vec4-aligned");
    float *O = (float *)elem_ptr(out, o.offset, WG_F32);
    wgk_mat Mx = { elem_ptr(m, mm.offset, md), mm.stride, mm.stride_mat }, Vx = { elem_ptr(v, vv.offset, WG_F32), vv.stride, vv.stride_mat };
    if (sm) { // the matrix where it lies, vectors and result element by element (gemv_any.hip)
        if (k == 0) return wgk_stage_copy(ctx, WG_F32, O, o.stride, o.stride_mat, rows_out, nrhs, out->ptr, 1, 0, 0, 0, mats); // (an empty sum)
        return wgk_gemv_any_mixed(ctx, tr, md, mm.rows, mm.cols, nrhs, mats, O, o.stride, o.stride_mat, Mx, Vx);
    }
    // (lengths are multiples of 4 here: Op == rows_out, Kp == k) f32 copies of the vectors / the result that are off
    void *ws = nullptr;
    if (int rc = wg_ctx_stage_workspace(ctx, (size_t)((ve + oe) * mats * sizeof(float)), &ws)) return rc;
    float *vp = (float *)ws, *op = vp + ve * mats;
    uint32_t ldo = o.stride;
    uint64_t o_batch = o.stride_mat;
    float *Ox = O;
    if (sv) {
        if (int rc = wgk_stage_copy(ctx, WG_F32, vp, Kp, ve, Kp, nrhs, Vx.ptr, vv.stride, vv.stride_mat, k, nrhs, mats)) return rc;
        Vx = wgk_mat{ vp, Kp, ve };
    }
    if (so) { Ox = op; ldo = Op; o_batch = oe; }
    wg_path(ctx, "stage>");
    if (int rc = wgk_gemv_mixed(ctx, tr, md, Op, Kp, nrhs, mats, Ox, ldo, o_batch, Mx, Vx)) return rc;
    if (!so) return WG_OK;
    return wgk_stage_copy(ctx, WG_F32, O, o.stride, o.stride_mat, rows_out, nrhs, op, Op, oe, Op, nrhs, mats);
}

} // namespace

int wg_check_alias(const char *op, wg_dtype dtype, const char *wname, wg_view_shape w, const void *base_w, const char *rname, wg_view_shape r, const void *base_r) {
    return check_alias(op, dtype, wname, mk(w), base_w, rname, mk(r), base_r);
}

int wg_gemm_f16_panels(wg_ctx *ctx, bool tr, void *out_panel0, uint32_t ldc, const wg_buf *m1, wg_view_shape m1_shape, const wg_buf *m2, wg_view_shape m2_shape,
                       const wgk_panels &panels) {
    const View a = mk(m1_shape), b = mk(m2_shape);
    const uint32_t m_rows = tr ? a.cols : a.rows, m_cols = tr ? a.rows : a.cols;
    if (m_cols != b.rows || a.mats != 1 || b.mats != 1 || m1->bytes == 0 || m2->bytes == 0) return WG_ERR_UNSUPPORTED;
    if (!vec4_ok(a) || !vec4_ok(b) || m_rows % 4 || m_cols % 4 || b.cols % 4) return WG_ERR_UNSUPPORTED;
    if (int rc = check_bounds("Gemm", "m1", a, m1, WG_F16)) return rc;
    if (int rc = check_bounds("Gemm", "m2", b, m2, WG_F16)) return rc;
    // the panels this launch writes (wgk_panels: panel p, np columns from column c0 on, is the dense m_rows x np block at out_panel0 + c0 * col_stride + slot_rows * (np - cols))
    // against the two operands: the communicator's staging cube is a buffer the caller can get hold of (wg_comm_stage_reserve)
    {
        uint64_t c0 = 0;
        for (uint32_t p = 0; p < panels.n_main + panels.n_tail; ++p) {
            const uint32_t np = p < panels.n_main ? panels.cols : panels.tail_cols[p - panels.n_main];
            const int64_t first = (int64_t)(c0 * panels.col_stride) + (int64_t)panels.slot_rows * ((int64_t)np - (int64_t)panels.cols);
            const char *base = (const char *)out_panel0 + first * (int64_t)wg_dtype_size(WG_F16);
            const View o = { m_rows, np, 1, ldc, 0, 0 };
            if (int rc = check_alias("Gemm", WG_F16, "out", o, base, "m1", a, m1->ptr)) return rc;
            if (int rc = check_alias("Gemm", WG_F16, "out", o, base, "m2", b, m2->ptr)) return rc;
            c0 += np;
        }
    }
    const wgk_mat A = { elem_ptr(m1, a.offset, WG_F16), a.stride, a.stride_mat }, B = { elem_ptr(m2, b.offset, WG_F16), b.stride, b.stride_mat };
    return wgk_gemm_f16(ctx, tr, m_rows, b.cols, m_cols, 1, (__half *)out_panel0, ldc, 0, A, B, 1.f, 0.f, &panels);
}

extern "C" {

int wg_gemm(wg_ctx *ctx, wg_gemm_variant variant, wg_dtype dtype, wg_buf *out, wg_view_shape out_shape, const wg_buf *m1,
            wg_view_shape m1_shape, const wg_buf *m2, wg_view_shape m2_shape) {
    return wg_gemm_ex(ctx, variant, dtype, 1.f, 0.f, out, out_shape, m1, m1_shape, m2, m2_shape);
}

int wg_gemm_ex(wg_ctx *ctx, wg_gemm_variant variant, wg_dtype dtype, float alpha, float beta, wg_buf *out, wg_view_shape out_shape,
               const wg_buf *m1, wg_view_shape m1_shape, const wg_buf *m2, wg_view_shape m2_shape) {
    const wg_buf *bufs[3] = { out, m1, m2 };
    if (int rc = check_common("Gemm", ctx, dtype, bufs, 3)) return rc;
    if ((int)variant < 0 || (int)variant > 3) return wg_set_error(WG_ERR_INVALID_ARG, "Gemm: unknown variant %d", (int)variant);
    const bool tr = variant == WG_GEMM_TR || variant == WG_GEMM_TR_FAST;
    const View o = mk(out_shape), a = mk(m1_shape), b = mk(m2_shape);

    // gemm.rs:81-96
    const uint32_t m_rows = tr ? a.cols : a.rows, m_cols = tr ? a.rows : a.cols;
    if (m_cols != b.rows || m_rows != o.rows || o.cols != b.cols || o.mats != a.mats || o.mats != b.mats)
        return wg_set_error(WG_ERR_DIM_MISMATCH,
                            "Gemm: dimension mismatch. (out [%u,%u,%u], m1 [%u,%u,%u]%s, m2 [%u,%u,%u])", o.rows, o.cols, o.mats,
                            a.rows, a.cols, a.mats, tr ? "^T" : "", b.rows, b.cols, b.mats);
    // kernel.rs:111-123 (zero-sized binding) and :144 (zero-sized grid): silently skipped
    if (out->bytes == 0 || m1->bytes == 0 || m2->bytes == 0) return WG_OK;
    if (o.rows == 0 || o.mats == 0) return WG_OK;
    if (o.cols == 0) return WG_OK; // the kernels' k-loop over m2 columns runs zero times

    if (int rc = check_bounds("Gemm", "out", o, out, dtype)) return rc;
    if (int rc = check_bounds("Gemm", "m1", a, m1, dtype)) return rc;
    if (int rc = check_bounds("Gemm", "m2", b, m2, dtype)) return rc;
    if (int rc = check_alias("Gemm", dtype, "out", o, out->ptr, "m1", a, m1->ptr)) return rc;
    if (int rc = check_alias("Gemm", dtype, "out", o, out->ptr, "m2", b, m2->ptr)) return rc;

    WG_HIP_TRY(hipSetDevice(ctx->device));
    // lengths the kernels' 4 x 4 blocks do not take (gemm.wgsl:87,94): zero-padded copies of the operands that carry them
    // (1 .. 7 columns that are not a multiple of 4 on otherwise aligned views: exactly a Gemv with that many right-hand sides -- no copy of anything)
    if (vec4_ok(o) && vec4_ok(a) && vec4_ok(b) && m_cols % 4 == 0 && m_rows % 4 == 0 && o.cols % 4 && o.cols < 8 && alpha == 1.f && beta == 0.f) // (the tuned Gemv kernels: aligned views)
        return wgk_gemv(ctx, tr, dtype, m_rows, m_cols, o.cols, o.mats, (void *)elem_ptr(out, o.offset, dtype), o.stride, o.stride_mat,
                        wgk_mat{ elem_ptr(m1, a.offset, dtype), a.stride, a.stride_mat }, wgk_mat{ elem_ptr(m2, b.offset, dtype), b.stride, b.stride_mat });
    // (the kernels take any offset, leading dimension and batch stride since round 6 -- gemm_f16.hip, gemm_f32*.hip: LDS-DMA and 16-byte accesses at element-aligned
    // addresses -- so only the lengths count)
    // (f16: the kernels take any number of columns -- they clamp their loads of m2 per column and skip the stores past N --, so N is as free as the offsets;
    //  f32: likewise from 129 rows on; the few-row forms of its launcher compute the transposed product and need N % 4 == 0 --
    //  tests/test_gpu_parity.py::test_gemm_f32_any_number_of_columns fails on them without the copies)
    const bool n_free = dtype != WG_F32 || m_rows > 128u; // (f32 with up to 128 rows: the few-row forms compute the transposed product, where N is the length that must be a multiple of 4)
    if ((o.cols % 4 && !n_free) || m_cols % 4 || m_rows % 4)
        return gemm_staged(ctx, tr, dtype, dtype, alpha, beta, out, o, m1, a, m2, b, m_rows, o.cols, m_cols);
    wgk_mat A = { elem_ptr(m1, a.offset, dtype), a.stride, a.stride_mat };
    wgk_mat B = { elem_ptr(m2, b.offset, dtype), b.stride, b.stride_mat };
    void *C = (void *)elem_ptr(out, o.offset, dtype);
    return gemm_launch(ctx, tr, dtype, dtype, m_rows, o.cols, m_cols, o.mats, C, o.stride, o.stride_mat, A, B, alpha, beta);
}

// wg_gemm_ex with an f32 `out` over 16-bit operands. The same checks in the same order with the same messages; bounds per operand's own element size; the aliasing
// rule on addresses (out against either 16-bit operand in 2-byte units). Never the Gemv kernels: the 16-bit tile kernels take any N as it is.
int wg_gemm_out32(wg_ctx *ctx, wg_gemm_variant variant, wg_dtype in_dtype, float alpha, float beta, wg_buf *out, wg_view_shape out_shape,
                  const wg_buf *m1, wg_view_shape m1_shape, const wg_buf *m2, wg_view_shape m2_shape) {
    const wg_buf *bufs[3] = { out, m1, m2 };
    if (int rc = check_common("Gemm", ctx, in_dtype, bufs, 3)) return rc;
    if (in_dtype == WG_F32) return wg_gemm_ex(ctx, variant, WG_F32, alpha, beta, out, out_shape, m1, m1_shape, m2, m2_shape); // (a caller generic over the operand type needs no branch)
    if ((int)variant < 0 || (int)variant > 3) return wg_set_error(WG_ERR_INVALID_ARG, "Gemm: unknown variant %d", (int)variant);
    const bool tr = variant == WG_GEMM_TR || variant == WG_GEMM_TR_FAST;
    const View o = mk(out_shape), a = mk(m1_shape), b = mk(m2_shape);

    const uint32_t m_rows = tr ? a.cols : a.rows, m_cols = tr ? a.rows : a.cols;
    if (m_cols != b.rows || m_rows != o.rows || o.cols != b.cols || o.mats != a.mats || o.mats != b.mats)
        return wg_set_error(WG_ERR_DIM_MISMATCH,
                            "Gemm: dimension mismatch. (out [%u,%u,%u], m1 [%u,%u,%u]%s, m2 [%u,%u,%u])", o.rows, o.cols, o.mats,
                            a.rows, a.cols, a.mats, tr ? "^T" : "", b.rows, b.cols, b.mats);
    if (out->bytes == 0 || m1->bytes == 0 || m2->bytes == 0) return WG_OK;
    if (o.rows == 0 || o.mats == 0) return WG_OK;
    if (o.cols == 0) return WG_OK;

    if (int rc = check_bounds("Gemm", "out", o, out, WG_F32)) return rc;
    if (int rc = check_bounds("Gemm", "m1", a, m1, in_dtype)) return rc;
    if (int rc = check_bounds("Gemm", "m2", b, m2, in_dtype)) return rc;
    if (int rc = check_alias_f32_u16("Gemm", "out", o, out->ptr, "m1", a, m1->ptr)) return rc;
    if (int rc = check_alias_f32_u16("Gemm", "out", o, out->ptr, "m2", b, m2->ptr)) return rc;

    WG_HIP_TRY(hipSetDevice(ctx->device));
    // lengths the kernels do not take as they are (M and K; any N runs as it is on the 16-bit kernels): zero-padded copies, the output's in f32
    if (m_cols % 4 || m_rows % 4) return gemm_staged(ctx, tr, in_dtype, WG_F32, alpha, beta, out, o, m1, a, m2, b, m_rows, o.cols, m_cols);
    wgk_mat A = { elem_ptr(m1, a.offset, in_dtype), a.stride, a.stride_mat };
    wgk_mat B = { elem_ptr(m2, b.offset, in_dtype), b.stride, b.stride_mat };
    void *C = (void *)elem_ptr(out, o.offset, WG_F32);
    return gemm_launch(ctx, tr, in_dtype, WG_F32, m_rows, o.cols, m_cols, o.mats, C, o.stride, o.stride_mat, A, B, alpha, beta);
}

int wg_gemv(wg_ctx *ctx, wg_gemv_variant variant, wg_dtype dtype, wg_buf *out, wg_view_shape out_shape, const wg_buf *m,
            wg_view_shape m_shape, const wg_buf *v, wg_view_shape v_shape) {
    const wg_buf *bufs[3] = { out, m, v };
    if (int rc = check_common("Gemv", ctx, dtype, bufs, 3)) return rc;
    if ((int)variant < 0 || (int)variant > 3) return wg_set_error(WG_ERR_INVALID_ARG, "Gemv: unknown variant %d", (int)variant);
    const bool tr = variant == WG_GEMV_TR || variant == WG_GEMV_TR_FAST;
    const View o = mk(out_shape), mm = mk(m_shape), vv = mk(v_shape);

    // gemv.rs:79-91 -- the reference checks exactly these two
    const uint32_t m_rows = tr ? mm.cols : mm.rows, m_cols = tr ? mm.rows : mm.cols;
    if (m_cols != vv.rows || m_rows != o.rows)
        return wg_set_error(WG_ERR_DIM_MISMATCH, "Gemv: dimension mismatch. (out [%u,%u,%u], m [%u,%u,%u]%s, v [%u,%u,%u])", o.rows,
                            o.cols, o.mats, mm.rows, mm.cols, mm.mats, tr ? "^T" : "", vv.rows, vv.cols, vv.mats);
    // gemv.rs:99-104: GemvTrFast silently becomes GemvTr when m.rows % 128 != 0 (same kernel here either way)
    if (variant == WG_GEMV_TR_FAST && mm.rows % 128u != 0) variant = WG_GEMV_TR;
    // gemv.rs:122: assert_eq!(out_nrows % 4, 0) on the fast paths
    if ((variant == WG_GEMV_FAST || variant == WG_GEMV_TR_FAST) && o.rows % 4u != 0)
        return wg_set_error(WG_ERR_PRECONDITION, "Gemv: assertion `left == right` failed (out_nrows %% 4 == 0, gemv.rs:122): out has %u rows",
                            o.rows);
    if (out->bytes == 0 || m->bytes == 0 || v->bytes == 0) return WG_OK;
    if (o.rows == 0 || o.cols == 0 || o.mats == 0) return WG_OK;

    // The grid is [.., out_ncols, out_nmats] and indexes m with z, v with (y, z) (gemv.wgsl:40,46,62): the views
    // that are actually addressed take their column / matrix counts from `out`.
    const View m_eff = { mm.rows, mm.cols, o.mats, mm.stride, mm.stride_mat, mm.offset };
    const View v_eff = { vv.rows, o.cols, o.mats, vv.stride, vv.stride_mat, vv.offset };
    if (int rc = check_bounds("Gemv", "out", o, out, dtype)) return rc;
    if (int rc = check_bounds("Gemv", "m", m_eff, m, dtype)) return rc;
    if (int rc = check_bounds("Gemv", "v", v_eff, v, dtype)) return rc;
    if (int rc = check_alias("Gemv", dtype, "out", o, out->ptr, "m", m_eff, m->ptr)) return rc;
    if (int rc = check_alias("Gemv", dtype, "out", o, out->ptr, "v", v_eff, v->ptr)) return rc;

    WG_HIP_TRY(hipSetDevice(ctx->device));
    // views / sizes the vec4 kernels cannot address as they are (shape.wgsl:64-66; gemv.wgsl:73,76): the any-alignment kernels (a matrix that is off), or copies of the vectors
    if (!vec4_ok(o) || !vec4_ok(m_eff) || !vec4_ok(v_eff) || m_cols % 4 || m_rows % 4)
        return gemv_staged(ctx, tr, dtype, out, o, m, m_eff, v, v_eff, m_rows, m_cols);
    wgk_mat M = { elem_ptr(m, mm.offset, dtype), mm.stride, mm.stride_mat };
    wgk_mat V = { elem_ptr(v, vv.offset, dtype), vv.stride, vv.stride_mat };
    return wgk_gemv(ctx, tr, dtype, o.rows, m_cols, o.cols, o.mats, (void *)elem_ptr(out, o.offset, dtype), o.stride, o.stride_mat, M, V);
}

// wg_gemv with an element type per operand: `m` holds m_dtype elements (f16 / bf16), `v` and `out` f32. The same checks in the same order with the same messages;
// bounds per operand's own element size; the aliasing rule on addresses (out against the 16-bit matrix in 2-byte units).
int wg_gemv_mixed(wg_ctx *ctx, wg_gemv_variant variant, wg_dtype m_dtype, wg_buf *out, wg_view_shape out_shape, const wg_buf *m, wg_view_shape m_shape,
                  const wg_buf *v, wg_view_shape v_shape) {
    const wg_buf *bufs[3] = { out, m, v };
    if (int rc = check_common("Gemv", ctx, m_dtype, bufs, 3)) return rc;
    if (m_dtype == WG_F32) return wg_gemv(ctx, variant, WG_F32, out, out_shape, m, m_shape, v, v_shape); // (a caller generic over the weight type needs no branch)
    if ((int)variant < 0 || (int)variant > 3) return wg_set_error(WG_ERR_INVALID_ARG, "Gemv: unknown variant %d", (int)variant);
    const bool tr = variant == WG_GEMV_TR || variant == WG_GEMV_TR_FAST;
    const View o = mk(out_shape), mm = mk(m_shape), vv = mk(v_shape);

    const uint32_t m_rows = tr ? mm.cols : mm.rows, m_cols = tr ? mm.rows : mm.cols;
    if (m_cols != vv.rows || m_rows != o.rows)
        return wg_set_error(WG_ERR_DIM_MISMATCH, "Gemv: dimension mismatch. (out [%u,%u,%u], m [%u,%u,%u]%s, v [%u,%u,%u])", o.rows,
                            o.cols, o.mats, mm.rows, mm.cols, mm.mats, tr ? "^T" : "", vv.rows, vv.cols, vv.mats);
    if (variant == WG_GEMV_TR_FAST && mm.rows % 128u != 0) variant = WG_GEMV_TR;
    if ((variant == WG_GEMV_FAST || variant == WG_GEMV_TR_FAST) && o.rows % 4u != 0)
        return wg_set_error(WG_ERR_PRECONDITION, "Gemv: assertion `left == right` failed (out_nrows %% 4 == 0, gemv.rs:122): out has %u rows",
                            o.rows);
    if (out->bytes == 0 || m->bytes == 0 || v->bytes == 0) return WG_OK;
    if (o.rows == 0 || o.cols == 0 || o.mats == 0) return WG_OK;

    const View m_eff = { mm.rows, mm.cols, o.mats, mm.stride, mm.stride_mat, mm.offset };
    const View v_eff = { vv.rows, o.cols, o.mats, vv.stride, vv.stride_mat, vv.offset };
    if (int rc = check_bounds("Gemv", "out", o, out, WG_F32)) return rc;
    if (int rc = check_bounds("Gemv", "m", m_eff, m, m_dtype)) return rc;
    if (int rc = check_bounds("Gemv", "v", v_eff, v, WG_F32)) return rc;
    if (int rc = check_alias_f32_u16("Gemv", "out", o, out->ptr, "m", m_eff, m->ptr)) return rc;
    if (int rc = check_alias("Gemv", WG_F32, "out", o, out->ptr, "v", v_eff, v->ptr)) return rc;

    WG_HIP_TRY(hipSetDevice(ctx->device));
    if (!vec4_ok(o) || !vec4_ok(m_eff) || !vec4_ok(v_eff) || m_cols % 4 || m_rows % 4)
        return gemv_mixed_staged(ctx, tr, m_dtype, out, o, m, m_eff, v, v_eff, m_rows, m_cols);
    wgk_mat M = { elem_ptr(m, mm.offset, m_dtype), mm.stride, mm.stride_mat };
    wgk_mat V = { elem_ptr(v, vv.offset, WG_F32), vv.stride, vv.stride_mat };
    return wgk_gemv_mixed(ctx, tr, m_dtype, o.rows, m_cols, o.cols, o.mats, (float *)elem_ptr(out, o.offset, WG_F32), o.stride, o.stride_mat, M, V);
}

// wg_gemv on an int8 matrix with f32 group scales (include/wgebra_hip.h): wg_gemv_mixed's checks in its order with its messages, the checks of group_rows and of the
// scales' shape behind the dimension check; bounds with 1 byte per element of `m`; `out` against `m` in 1-byte units. The kernels are the plan's (gemv_q8_plan.hip).
int wg_gemv_q8(wg_ctx *ctx, wg_gemv_variant variant, uint32_t group_rows, wg_buf *out, wg_view_shape out_shape, const wg_buf *m, wg_view_shape m_shape, const wg_buf *scales,
               wg_view_shape scales_shape, const wg_buf *v, wg_view_shape v_shape) {
    const wg_buf *bufs[4] = { out, m, scales, v };
    if (int rc = check_common("Gemv", ctx, WG_F32, bufs, 4)) return rc;
    if ((int)variant < 0 || (int)variant > 3) return wg_set_error(WG_ERR_INVALID_ARG, "Gemv: unknown variant %d", (int)variant);
    const bool tr = variant == WG_GEMV_TR || variant == WG_GEMV_TR_FAST;
    const View o = mk(out_shape), mm = mk(m_shape), ss = mk(scales_shape), vv = mk(v_shape);

    const uint32_t m_rows = tr ? mm.cols : mm.rows, m_cols = tr ? mm.rows : mm.cols;
    if (m_cols != vv.rows || m_rows != o.rows)
        return wg_set_error(WG_ERR_DIM_MISMATCH, "Gemv: dimension mismatch. (out [%u,%u,%u], m [%u,%u,%u]%s, v [%u,%u,%u])", o.rows,
                            o.cols, o.mats, mm.rows, mm.cols, mm.mats, tr ? "^T" : "", vv.rows, vv.cols, vv.mats);
    if (group_rows == 0 || (group_rows % 16u != 0 && group_rows < mm.rows))
        return wg_set_error(WG_ERR_INVALID_ARG, "Gemv: group_rows %u is neither a positive multiple of 16 nor at least the %u rows of m", group_rows, mm.rows);
    const uint32_t s_rows = mm.rows / group_rows + (mm.rows % group_rows != 0);
    if (ss.rows != s_rows || ss.cols != mm.cols || ss.mats != mm.mats)
        return wg_set_error(WG_ERR_DIM_MISMATCH, "Gemv: dimension mismatch. (m [%u,%u,%u], group_rows %u, scales [%u,%u,%u], expected [%u,%u,%u])", mm.rows, mm.cols, mm.mats,
                            group_rows, ss.rows, ss.cols, ss.mats, s_rows, mm.cols, mm.mats);
    if (variant == WG_GEMV_TR_FAST && mm.rows % 128u != 0) variant = WG_GEMV_TR;
    if ((variant == WG_GEMV_FAST || variant == WG_GEMV_TR_FAST) && o.rows % 4u != 0)
        return wg_set_error(WG_ERR_PRECONDITION, "Gemv: assertion `left == right` failed (out_nrows %% 4 == 0, gemv.rs:122): out has %u rows",
                            o.rows);
    if (out->bytes == 0 || m->bytes == 0 || scales->bytes == 0 || v->bytes == 0) return WG_OK;
    if (o.rows == 0 || o.cols == 0 || o.mats == 0) return WG_OK;

    const View m_eff = { mm.rows, mm.cols, o.mats, mm.stride, mm.stride_mat, mm.offset };
    const View s_eff = { ss.rows, ss.cols, o.mats, ss.stride, ss.stride_mat, ss.offset };
    const View v_eff = { vv.rows, o.cols, o.mats, vv.stride, vv.stride_mat, vv.offset };
    if (int rc = check_bounds("Gemv", "out", o, out, WG_F32)) return rc;
    if (int rc = check_bounds_es("Gemv", "m", m_eff, m, 1)) return rc;
    if (int rc = check_bounds("Gemv", "scales", s_eff, scales, WG_F32)) return rc;
    if (int rc = check_bounds("Gemv", "v", v_eff, v, WG_F32)) return rc;
    if (int rc = check_alias_f32_u8("Gemv", "out", o, out->ptr, "m", m_eff, m->ptr)) return rc;
    if (int rc = check_alias("Gemv", WG_F32, "out", o, out->ptr, "scales", s_eff, scales->ptr)) return rc;
    if (int rc = check_alias("Gemv", WG_F32, "out", o, out->ptr, "v", v_eff, v->ptr)) return rc;

    const wgk_mat M = { (const char *)m->ptr + mm.offset, mm.stride, mm.stride_mat };
    const wgk_mat S = { elem_ptr(scales, ss.offset, WG_F32), ss.stride, ss.stride_mat };
    const wgk_mat V = { elem_ptr(v, vv.offset, WG_F32), vv.stride, vv.stride_mat };
    float *O = (float *)elem_ptr(out, o.offset, WG_F32);
    wg_gemv_q8_query q = {};
    q.trans = tr; q.rows = mm.rows; q.cols = mm.cols; q.nrhs = o.cols; q.mats = o.mats; q.group_rows = group_rows;
    q.ldm = mm.stride; q.lds = ss.stride; q.ldv = vv.stride; q.ldo = o.stride;
    q.m_batch = mm.stride_mat; q.s_batch = ss.stride_mat; q.v_batch = vv.stride_mat; q.o_batch = o.stride_mat;
    q.m_addr16 = (uint32_t)((uintptr_t)M.ptr % 16u); q.v_addr16 = (uint32_t)((uintptr_t)V.ptr % 16u); q.o_addr16 = (uint32_t)((uintptr_t)O % 16u);
    q.cus = (uint32_t)wg_ctx_cus(ctx);
    const wg_gemv_q8_plan p = gemv_q8_plan(q);
    WG_HIP_TRY(hipSetDevice(ctx->device));
    return wgk_gemv_q8(ctx, p, tr, group_rows, mm.rows, mm.cols, o.cols, o.mats, O, o.stride, o.stride_mat, M, S, V);
}

// GemvTr on packed 4-bit weights with f32 group scales (include/wgebra_hip.h): wg_gemv_q8's checks in its order with its messages; `m` counts bytes (two weights
// each), so the contraction length is k = 2 m.rows; out = W v is refused behind the variant check. The kernels are the plan's (gemv_q4_plan.hip).
int wg_gemv_q4(wg_ctx *ctx, wg_gemv_variant variant, uint32_t group_rows, wg_buf *out, wg_view_shape out_shape, const wg_buf *m, wg_view_shape m_shape, const wg_buf *scales,
               wg_view_shape scales_shape, const wg_buf *v, wg_view_shape v_shape) {
    const wg_buf *bufs[4] = { out, m, scales, v };
    if (int rc = check_common("Gemv", ctx, WG_F32, bufs, 4)) return rc;
    if ((int)variant < 0 || (int)variant > 3) return wg_set_error(WG_ERR_INVALID_ARG, "Gemv: unknown variant %d", (int)variant);
    const View o = mk(out_shape), mm = mk(m_shape), ss = mk(scales_shape), vv = mk(v_shape);
    wg_gemv_q4_query q = {};
    q.trans = variant == WG_GEMV_TR || variant == WG_GEMV_TR_FAST;
    if (!q.trans) { // (the plan words the refusal)
        const wg_gemv_q4_plan p = gemv_q4_plan(q);
        return wg_set_error(p.status, "%s", p.message);
    }
    const uint64_t k64 = 2ull * mm.rows;
    if (k64 != vv.rows || mm.cols != o.rows)
        return wg_set_error(WG_ERR_DIM_MISMATCH, "Gemv: dimension mismatch. (out [%u,%u,%u], m [%u,%u,%u]^T packed: k %llu, v [%u,%u,%u])", o.rows, o.cols, o.mats, mm.rows,
                            mm.cols, mm.mats, (unsigned long long)k64, vv.rows, vv.cols, vv.mats);
    const uint32_t k = (uint32_t)k64;
    if (group_rows == 0 || (group_rows % 32u != 0 && group_rows < k))
        return wg_set_error(WG_ERR_INVALID_ARG, "Gemv: group_rows %u is neither a positive multiple of 32 nor at least the %u logical rows of m", group_rows, k);
    const uint32_t s_rows = k / group_rows + (k % group_rows != 0);
    if (ss.rows != s_rows || ss.cols != mm.cols || ss.mats != mm.mats)
        return wg_set_error(WG_ERR_DIM_MISMATCH, "Gemv: dimension mismatch. (m [%u,%u,%u] packed: k %u, group_rows %u, scales [%u,%u,%u], expected [%u,%u,%u])", mm.rows,
                            mm.cols, mm.mats, k, group_rows, ss.rows, ss.cols, ss.mats, s_rows, mm.cols, mm.mats);
    if (out->bytes == 0 || m->bytes == 0 || scales->bytes == 0 || v->bytes == 0) return WG_OK;
    if (o.rows == 0 || o.cols == 0 || o.mats == 0) return WG_OK;

    const View m_eff = { mm.rows, mm.cols, o.mats, mm.stride, mm.stride_mat, mm.offset };
    const View s_eff = { ss.rows, ss.cols, o.mats, ss.stride, ss.stride_mat, ss.offset };
    const View v_eff = { vv.rows, o.cols, o.mats, vv.stride, vv.stride_mat, vv.offset };
    if (int rc = check_bounds("Gemv", "out", o, out, WG_F32)) return rc;
    if (int rc = check_bounds_es("Gemv", "m", m_eff, m, 1)) return rc;
    if (int rc = check_bounds("Gemv", "scales", s_eff, scales, WG_F32)) return rc;
    if (int rc = check_bounds("Gemv", "v", v_eff, v, WG_F32)) return rc;
    if (int rc = check_alias_f32_u8("Gemv", "out", o, out->ptr, "m", m_eff, m->ptr)) return rc;
    if (int rc = check_alias("Gemv", WG_F32, "out", o, out->ptr, "scales", s_eff, scales->ptr)) return rc;
    if (int rc = check_alias("Gemv", WG_F32, "out", o, out->ptr, "v", v_eff, v->ptr)) return rc;

    const wgk_mat M = { (const char *)m->ptr + mm.offset, mm.stride, mm.stride_mat };
    const wgk_mat S = { elem_ptr(scales, ss.offset, WG_F32), ss.stride, ss.stride_mat };
    const wgk_mat V = { elem_ptr(v, vv.offset, WG_F32), vv.stride, vv.stride_mat };
    float *O = (float *)elem_ptr(out, o.offset, WG_F32);
    q.rows = mm.rows; q.cols = mm.cols; q.nrhs = o.cols; q.mats = o.mats; q.group_rows = group_rows;
    q.ldm = mm.stride; q.lds = ss.stride; q.ldv = vv.stride; q.ldo = o.stride;
    q.m_batch = mm.stride_mat; q.s_batch = ss.stride_mat; q.v_batch = vv.stride_mat; q.o_batch = o.stride_mat;
    q.m_addr16 = (uint32_t)((uintptr_t)M.ptr % 16u); q.v_addr16 = (uint32_t)((uintptr_t)V.ptr % 16u);
    q.cus = (uint32_t)wg_ctx_cus(ctx);
    const wg_gemv_q4_plan p = gemv_q4_plan(q);
    WG_HIP_TRY(hipSetDevice(ctx->device));
    return wgk_gemv_q4(ctx, p, group_rows, k, mm.cols, o.cols, o.mats, O, o.stride, o.stride_mat, M, S, V);
}

// wg_gemm on wg_gemv_q8's int8 matrix and scales with 16-bit columns (include/wgebra_hip.h): wg_gemm_out32's checks in its order with its messages, then wg_gemv_q8's
// checks of group_rows and of the scales' shape behind the dimension check; bounds with 1 / 4 / 2 / 4 bytes per element of m / scales / x / out; `out` against `m` in
// 1-byte and against `x` in 2-byte units. The kernels are the plan's (gemm_q8_plan.hip).
int wg_gemm_q8(wg_ctx *ctx, wg_gemm_variant variant, uint32_t group_rows, wg_dtype x_dtype, wg_buf *out, wg_view_shape out_shape, const wg_buf *m, wg_view_shape m_shape,
               const wg_buf *scales, wg_view_shape scales_shape, const wg_buf *x, wg_view_shape x_shape) {
    const wg_buf *bufs[4] = { out, m, scales, x };
    if (int rc = check_common("Gemm", ctx, x_dtype, bufs, 4)) return rc;
    if (x_dtype == WG_F32)
        return wg_set_error(WG_ERR_UNSUPPORTED, "Gemm: wg_gemm_q8 takes f16 or bf16 columns (f32 activations stay with wg_gemv_q8, which never narrows them)");
    if ((int)variant < 0 || (int)variant > 3) return wg_set_error(WG_ERR_INVALID_ARG, "Gemm: unknown variant %d", (int)variant);
    if (variant != WG_GEMM_TR && variant != WG_GEMM_TR_FAST)
        return wg_set_error(WG_ERR_UNSUPPORTED, "Gemm: wg_gemm_q8 computes out = W^T x only (WG_GEMM_TR); wg_gemv_q8 computes out = W v, whose scales cannot leave the contraction");
    const View o = mk(out_shape), mm = mk(m_shape), ss = mk(scales_shape), xx = mk(x_shape);

    if (mm.rows != xx.rows || mm.cols != o.rows || o.cols != xx.cols || o.mats != mm.mats || o.mats != xx.mats)
        return wg_set_error(WG_ERR_DIM_MISMATCH, "Gemm: dimension mismatch. (out [%u,%u,%u], m1 [%u,%u,%u]^T, m2 [%u,%u,%u])", o.rows, o.cols, o.mats, mm.rows, mm.cols,
                            mm.mats, xx.rows, xx.cols, xx.mats);
    if (group_rows == 0 || (group_rows % 16u != 0 && group_rows < mm.rows))
        return wg_set_error(WG_ERR_INVALID_ARG, "Gemm: group_rows %u is neither a positive multiple of 16 nor at least the %u rows of m", group_rows, mm.rows);
    const uint32_t s_rows = mm.rows / group_rows + (mm.rows % group_rows != 0);
    if (ss.rows != s_rows || ss.cols != mm.cols || ss.mats != mm.mats)
        return wg_set_error(WG_ERR_DIM_MISMATCH, "Gemm: dimension mismatch. (m [%u,%u,%u], group_rows %u, scales [%u,%u,%u], expected [%u,%u,%u])", mm.rows, mm.cols, mm.mats,
                            group_rows, ss.rows, ss.cols, ss.mats, s_rows, mm.cols, mm.mats);
    if (out->bytes == 0 || m->bytes == 0 || scales->bytes == 0 || x->bytes == 0) return WG_OK;
    if (o.rows == 0 || o.cols == 0 || o.mats == 0) return WG_OK;

    if (int rc = check_bounds("Gemm", "out", o, out, WG_F32)) return rc;
    if (int rc = check_bounds_es("Gemm", "m", mm, m, 1)) return rc;
    if (int rc = check_bounds("Gemm", "scales", ss, scales, WG_F32)) return rc;
    if (int rc = check_bounds("Gemm", "x", xx, x, x_dtype)) return rc;
    if (int rc = check_alias_f32_u8("Gemm", "out", o, out->ptr, "m", mm, m->ptr)) return rc;
    if (int rc = check_alias("Gemm", WG_F32, "out", o, out->ptr, "scales", ss, scales->ptr)) return rc;
    if (int rc = check_alias_f32_u16("Gemm", "out", o, out->ptr, "x", xx, x->ptr)) return rc;

    const wgk_mat M = { (const char *)m->ptr + mm.offset, mm.stride, mm.stride_mat };
    const wgk_mat S = { elem_ptr(scales, ss.offset, WG_F32), ss.stride, ss.stride_mat };
    const wgk_mat X = { elem_ptr(x, xx.offset, x_dtype), xx.stride, xx.stride_mat };
    float *O = (float *)elem_ptr(out, o.offset, WG_F32);
    wg_gemm_q8_query q = {};
    q.k = mm.rows; q.outputs = mm.cols; q.n = o.cols; q.mats = o.mats; q.group_rows = group_rows; q.x_bf16 = x_dtype == WG_BF16;
    q.ldm = mm.stride; q.lds = ss.stride; q.ldx = xx.stride; q.ldo = o.stride;
    q.m_batch = mm.stride_mat; q.s_batch = ss.stride_mat; q.x_batch = xx.stride_mat; q.o_batch = o.stride_mat;
    q.m_addr16 = (uint32_t)((uintptr_t)M.ptr % 16u); q.x_addr16 = (uint32_t)((uintptr_t)X.ptr % 16u); q.o_addr16 = (uint32_t)((uintptr_t)O % 16u);
    q.cus = (uint32_t)wg_ctx_cus(ctx);
    const wg_gemm_q8_plan p = gemm_q8_plan(q);
    WG_HIP_TRY(hipSetDevice(ctx->device));
    return wgk_gemm_q8(ctx, p, x_dtype == WG_BF16, group_rows, mm.rows, mm.cols, o.cols, o.mats, O, o.stride, o.stride_mat, M, S, X);
}

// wg_gemm_q8 on wg_gemv_q4's packed matrix (include/wgebra_hip.h): wg_gemm_q8's checks in its order with its statuses; `m` counts bytes (two weights each), so the
// contraction length is k = 2 m.rows and wg_gemv_q4's rule for group_rows applies; both refusals (f32 columns, out = W x) come before any dimension is looked at.
// The kernels are the plan's (gemm_q4_plan.hip).
int wg_gemm_q4(wg_ctx *ctx, wg_gemm_variant variant, uint32_t group_rows, wg_dtype x_dtype, wg_buf *out, wg_view_shape out_shape, const wg_buf *m, wg_view_shape m_shape,
               const wg_buf *scales, wg_view_shape scales_shape, const wg_buf *x, wg_view_shape x_shape) {
    const wg_buf *bufs[4] = { out, m, scales, x };
    if (int rc = check_common("Gemm", ctx, x_dtype, bufs, 4)) return rc;
    if (x_dtype == WG_F32)
        return wg_set_error(WG_ERR_UNSUPPORTED, "Gemm: wg_gemm_q4 takes f16 or bf16 columns (f32 activations stay with wg_gemv_q4, which never narrows them)");
    if ((int)variant < 0 || (int)variant > 3) return wg_set_error(WG_ERR_INVALID_ARG, "Gemm: unknown variant %d", (int)variant);
    if (variant != WG_GEMM_TR && variant != WG_GEMM_TR_FAST)
        return wg_set_error(WG_ERR_UNSUPPORTED, "Gemm: wg_gemm_q4 computes out = W^T x only (WG_GEMM_TR); wg_gemv_q8 computes out = W v, on a layout with the groups along the outputs");
    const View o = mk(out_shape), mm = mk(m_shape), ss = mk(scales_shape), xx = mk(x_shape);

    const uint64_t k64 = 2ull * mm.rows;
    if (k64 != xx.rows || mm.cols != o.rows || o.cols != xx.cols || o.mats != mm.mats || o.mats != xx.mats)
        return wg_set_error(WG_ERR_DIM_MISMATCH, "Gemm: dimension mismatch. (out [%u,%u,%u], m1 [%u,%u,%u]^T packed: k %llu, m2 [%u,%u,%u])", o.rows, o.cols, o.mats, mm.rows,
                            mm.cols, mm.mats, (unsigned long long)k64, xx.rows, xx.cols, xx.mats);
    const uint32_t k = (uint32_t)k64;
    if (group_rows == 0 || (group_rows % 32u != 0 && group_rows < k))
        return wg_set_error(WG_ERR_INVALID_ARG, "Gemm: group_rows %u is neither a positive multiple of 32 nor at least the %u logical rows of m", group_rows, k);
    const uint32_t s_rows = k / group_rows + (k % group_rows != 0);
    if (ss.rows != s_rows || ss.cols != mm.cols || ss.mats != mm.mats)
        return wg_set_error(WG_ERR_DIM_MISMATCH, "Gemm: dimension mismatch. (m [%u,%u,%u] packed: k %u, group_rows %u, scales [%u,%u,%u], expected [%u,%u,%u])", mm.rows,
                            mm.cols, mm.mats, k, group_rows, ss.rows, ss.cols, ss.mats, s_rows, mm.cols, mm.mats);
    if (out->bytes == 0 || m->bytes == 0 || scales->bytes == 0 || x->bytes == 0) return WG_OK;
    if (o.rows == 0 || o.cols == 0 || o.mats == 0) return WG_OK;

    if (int rc = check_bounds("Gemm", "out", o, out, WG_F32)) return rc;
    if (int rc = check_bounds_es("Gemm", "m", mm, m, 1)) return rc;
    if (int rc = check_bounds("Gemm", "scales", ss, scales, WG_F32)) return rc;
    if (int rc = check_bounds("Gemm", "x", xx, x, x_dtype)) return rc;
    if (int rc = check_alias_f32_u8("Gemm", "out", o, out->ptr, "m", mm, m->ptr)) return rc;
    if (int rc = check_alias("Gemm", WG_F32, "out", o, out->ptr, "scales", ss, scales->ptr)) return rc;
    if (int rc = check_alias_f32_u16("Gemm", "out", o, out->ptr, "x", xx, x->ptr)) return rc;

    const wgk_mat M = { (const char *)m->ptr + mm.offset, mm.stride, mm.stride_mat };
    const wgk_mat S = { elem_ptr(scales, ss.offset, WG_F32), ss.stride, ss.stride_mat };
    const wgk_mat X = { elem_ptr(x, xx.offset, x_dtype), xx.stride, xx.stride_mat };
    float *O = (float *)elem_ptr(out, o.offset, WG_F32);
    wg_gemm_q4_query q = {};
    q.k = k; q.outputs = mm.cols; q.n = o.cols; q.mats = o.mats; q.group_rows = group_rows; q.x_bf16 = x_dtype == WG_BF16;
    q.ldm = mm.stride; q.lds = ss.stride; q.ldx = xx.stride; q.ldo = o.stride;
    q.m_batch = mm.stride_mat; q.s_batch = ss.stride_mat; q.x_batch = xx.stride_mat; q.o_batch = o.stride_mat;
    q.m_addr16 = (uint32_t)((uintptr_t)M.ptr % 16u); q.x_addr16 = (uint32_t)((uintptr_t)X.ptr % 16u); q.o_addr16 = (uint32_t)((uintptr_t)O % 16u);
    q.cus = (uint32_t)wg_ctx_cus(ctx);
    const wg_gemm_q4_plan p = gemm_q4_plan(q);
    WG_HIP_TRY(hipSetDevice(ctx->device));
    return wgk_gemm_q4(ctx, p, x_dtype == WG_BF16, group_rows, k, mm.cols, o.cols, o.mats, O, o.stride, o.stride_mat, M, S, X);
}

int wg_reduce(wg_ctx *ctx, wg_reduce_op op, wg_dtype dtype, const wg_buf *value, wg_view_shape value_shape, wg_buf *result) {
    const wg_buf *bufs[2] = { value, result };
    if (int rc = check_common("Reduce", ctx, dtype, bufs, 2)) return rc;
    if ((int)op < 0 || (int)op > 4) return wg_set_error(WG_ERR_INVALID_ARG, "Reduce: unknown op %d", (int)op);
    if (value->bytes == 0 || result->bytes == 0) return WG_OK; // kernel.rs:111-123
    if (result->bytes < wg_dtype_size(dtype)) return wg_set_error(WG_ERR_OUT_OF_BOUNDS, "Reduce: result buffer smaller than one element");
    // reduce.wgsl:71-72: input[offset + i], i < nrows; stride / ncols / nmats are ignored
    const View vec = { value_shape.size[0], 1, 1, 1, 1, value_shape.offset };
    if (int rc = check_bounds("Reduce", "value", vec, value, dtype)) return rc;
    if (int rc = check_alias("Reduce", dtype, "result", one_element(), result->ptr, "value", vec, value->ptr)) return rc;
    WG_HIP_TRY(hipSetDevice(ctx->device));
    return wgk_reduce(ctx, (int)op, dtype, elem_ptr(value, vec.offset, dtype), vec.rows, 1, 1, 0, 0, result->ptr);
}

int wg_reduce_fast(wg_ctx *ctx, wg_reduce_op op, wg_dtype dtype, const wg_buf *value, wg_view_shape value_shape, wg_buf *result) {
    const wg_buf *bufs[2] = { value, result };
    if (int rc = check_common("Reduce", ctx, dtype, bufs, 2)) return rc;
    if ((int)op < 0 || (int)op > 4) return wg_set_error(WG_ERR_INVALID_ARG, "Reduce: unknown op %d", (int)op);
    if (value->bytes == 0 || result->bytes == 0) return WG_OK; // kernel.rs:111-123
    if (result->bytes < wg_dtype_size(dtype)) return wg_set_error(WG_ERR_OUT_OF_BOUNDS, "Reduce: result buffer smaller than one element");
    const View vec = { value_shape.size[0], 1, 1, 1, 1, value_shape.offset };
    if (int rc = check_bounds("Reduce", "value", vec, value, dtype)) return rc;
    if (int rc = check_alias("Reduce", dtype, "result", one_element(), result->ptr, "value", vec, value->ptr)) return rc;
    WG_HIP_TRY(hipSetDevice(ctx->device));
    return wgk_reduce_fast(ctx, (int)op, dtype, elem_ptr(value, vec.offset, dtype), vec.rows, result->ptr);
}

int wg_gemv_reduce(wg_ctx *ctx, wg_gemv_variant variant, wg_reduce_op op, wg_dtype dtype, wg_buf *result, const wg_buf *m,
                   wg_view_shape m_shape, const wg_buf *v, wg_view_shape v_shape) {
    // result[0] = reduce(op, op(m) v): Gemv into a context-owned scratch vector, then Reduce in the reference order on the same
    // stream -- one call, no intermediate tensor for the caller; bit-identical to wg_gemv followed by wg_reduce.
    const wg_buf *bufs[3] = { result, m, v };
    if (int rc = check_common("Gemv", ctx, dtype, bufs, 3)) return rc;
    if ((int)op < 0 || (int)op > 4) return wg_set_error(WG_ERR_INVALID_ARG, "Reduce: unknown op %d", (int)op);
    if ((int)variant < 0 || (int)variant > 3) return wg_set_error(WG_ERR_INVALID_ARG, "Gemv: unknown variant %d", (int)variant);
    if (result->bytes < wg_dtype_size(dtype)) return wg_set_error(WG_ERR_OUT_OF_BOUNDS, "Reduce: result buffer smaller than one element");
    const bool tr = variant == WG_GEMV_TR || variant == WG_GEMV_TR_FAST;
    const View mm = mk(m_shape), vv = mk(v_shape);
    if (vv.cols != 1 || vv.mats != 1 || mm.mats != 1)
        return wg_set_error(WG_ERR_UNSUPPORTED, "gemv_reduce: one matrix and one vector only");
    const uint32_t out_rows = tr ? mm.cols : mm.rows;
    // The result scalar against the matrix and the vector -- before anything is allocated, launched or logged. (The two launches below see `result` only next to the
    // context's scratch vector, which aliases nothing of the caller's.) For a call wg_gemv would neither refuse for its dimensions nor skip: its bounds checks first.
    if ((tr ? mm.rows : mm.cols) == vv.rows && out_rows != 0 && m->bytes != 0 && v->bytes != 0) {
        const View m_eff = { mm.rows, mm.cols, 1, mm.stride, mm.stride_mat, mm.offset }, v_eff = { vv.rows, 1, 1, vv.stride, vv.stride_mat, vv.offset };
        if (int rc = check_bounds("Gemv", "m", m_eff, m, dtype)) return rc;
        if (int rc = check_bounds("Gemv", "v", v_eff, v, dtype)) return rc;
        if (int rc = check_alias("GemvReduce", dtype, "result", one_element(), result->ptr, "m", m_eff, m->ptr)) return rc;
        if (int rc = check_alias("GemvReduce", dtype, "result", one_element(), result->ptr, "v", v_eff, v->ptr)) return rc;
    }
    void *ws = nullptr;
    if (int rc = wg_ctx_tr_workspace(ctx, (size_t)(out_rows ? out_rows : 4) * sizeof(float), &ws)) return rc;
    // Launch-bound sizes (the single-kernel Gemv family): ONE launch -- the last workgroup to finish folds y in the reference order
    // (gemv.hip, gemv_n_small_reduce_kernel) -- for exactly the calls wg_gemv would run on its single-kernel leaf (gemv_plan.hip). Same checks as wg_gemv would make;
    // everything else falls through to the two launches.
    if (!tr && dtype == WG_F32 && mm.cols == vv.rows && out_rows % 4u == 0 && mm.cols % 4u == 0 && mm.cols > 0 &&
        m->bytes && v->bytes && mm.offset % 4u == 0 && vv.offset % 4u == 0 && (mm.cols == 1 || mm.stride % 4u == 0)) {
        const wgk_mat M = { elem_ptr(m, mm.offset, dtype), mm.stride, mm.stride_mat }, V = { elem_ptr(v, vv.offset, dtype), vv.stride, vv.stride_mat };
        const wg_gemv_plan p = gemv_plan(wgk_gemv_query(ctx, false, dtype, dtype, false, out_rows, mm.cols, 1, 1, out_rows, out_rows, M, V));
        if (p.leaf == WG_GEMV_SMALL) {
            const View m_eff = { mm.rows, mm.cols, 1, mm.stride, mm.stride_mat, mm.offset }, v_eff = { vv.rows, 1, 1, vv.stride, vv.stride_mat, vv.offset };
            if (int rc = check_bounds("Gemv", "m", m_eff, m, dtype)) return rc;
            if (int rc = check_bounds("Gemv", "v", v_eff, v, dtype)) return rc;
            if (!ctx->flags) {
                if (ctx->recording) return wg_set_error(WG_ERR_WORKSPACE, "gemv_reduce: arrival counter needed while recording: run the call once outside the recording first");
                WG_HIP_TRY(hipSetDevice(ctx->device));
                WG_HIP_TRY(hipMalloc((void **)&ctx->flags, 256));
                WG_HIP_TRY(hipMemsetAsync(ctx->flags, 0, 256, ctx->stream));
            }
            return wgk_gemv_small_reduce(ctx, p, (int)op, out_rows, mm.cols, (float *)ws, M, V, ctx->flags, (float *)result->ptr);
        }
    }
    wg_path(ctx, "gemv_reduce.two>");
    wg_buf tmp;
    tmp.ctx = ctx; tmp.ptr = ws; tmp.bytes = (size_t)(out_rows ? out_rows : 4) * sizeof(float); tmp.usage = 0; tmp.owned = false; tmp.host_pinned = false;
    wg_view_shape os;
    os.size[0] = out_rows; os.size[1] = 1; os.size[2] = 1; os.stride = out_rows; os.stride_mat = out_rows; os.offset = 0;
    if (int rc = wg_gemv(ctx, variant, dtype, &tmp, os, m, m_shape, v, v_shape)) return rc;
    return wg_reduce(ctx, op, dtype, &tmp, os, result);
}

int wg_reduce_batched(wg_ctx *ctx, wg_reduce_op op, wg_dtype dtype, const wg_buf *values, wg_view_shape values_shape, wg_buf *results) {
    const wg_buf *bufs[2] = { values, results };
    if (int rc = check_common("Reduce", ctx, dtype, bufs, 2)) return rc;
    if ((int)op < 0 || (int)op > 4) return wg_set_error(WG_ERR_INVALID_ARG, "Reduce: unknown op %d", (int)op);
    const View v = mk(values_shape);
    const uint64_t nvec = (uint64_t)v.cols * v.mats;
    if (nvec == 0 || results->bytes == 0) return WG_OK;
    if (results->bytes / wg_dtype_size(dtype) < nvec)
        return wg_set_error(WG_ERR_OUT_OF_BOUNDS, "Reduce: results buffer holds %zu elements but %llu vectors are reduced",
                            results->bytes / wg_dtype_size(dtype), (unsigned long long)nvec);
    if (values->bytes == 0 && v.rows != 0) return WG_OK;
    if (int rc = check_bounds("Reduce", "values", v, values, dtype)) return rc;
    // results[c + t * cols]: cols x mats elements back to back from element 0 of their buffer
    if (int rc = check_alias("Reduce", dtype, "results", View{ v.cols, v.mats, 1, v.cols, 0, 0 }, results->ptr, "values", v, values->ptr)) return rc;
    WG_HIP_TRY(hipSetDevice(ctx->device));
    return wgk_reduce(ctx, (int)op, dtype, elem_ptr(values, v.offset, dtype), v.rows, v.cols, v.mats, v.stride, v.stride_mat,
                      results->ptr);
}

int wg_op_assign(wg_ctx *ctx, wg_op_assign_variant op, wg_dtype dtype, wg_buf *a, wg_view_shape a_shape, const wg_buf *b,
                 wg_view_shape b_shape) {
    const wg_buf *bufs[2] = { a, b };
    if (int rc = check_common("OpAssign", ctx, dtype, bufs, 2)) return rc;
    if ((int)op < 0 || (int)op > 4) return wg_set_error(WG_ERR_INVALID_ARG, "OpAssign: unknown variant %d", (int)op);
    // op_assign.rs:82-86
    if (a_shape.size[0] != b_shape.size[0])
        return wg_set_error(WG_ERR_DIM_MISMATCH, "Op-assign: dimension mismatch. (a has %u rows, b has %u)", a_shape.size[0],
                            b_shape.size[0]);
    if (a->bytes == 0 || b->bytes == 0) return WG_OK; // kernel.rs:111-123
    const uint32_t n = a_shape.size[0];
    if (n == 0) return WG_OK; // kernel.rs:144
    // op_assign.wgsl:43-45: a[offset_a + i], b[offset_b + i]
    const View va = { n, 1, 1, 1, 1, a_shape.offset }, vb = { n, 1, 1, 1, 1, b_shape.offset };
    if (int rc = check_bounds("OpAssign", "a", va, a, dtype)) return rc;
    if (int rc = check_bounds("OpAssign", "b", vb, b, dtype)) return rc;
    // the identical view as `a` and `b` (same address; the lengths are equal) is defined: every lane of op_assign.hip's kernels loads its a[i] and b[i] before it
    // stores a[i], in the 16-byte body and in the scalar head and tail alike. Any other overlap is a race between lanes.
    if (elem_ptr(a, va.offset, dtype) != elem_ptr(b, vb.offset, dtype))
        if (int rc = check_alias("OpAssign", dtype, "a", va, a->ptr, "b", vb, b->ptr)) return rc;
    WG_HIP_TRY(hipSetDevice(ctx->device));
    return wgk_op_assign(ctx, (int)op, dtype, (void *)elem_ptr(a, va.offset, dtype), elem_ptr(b, vb.offset, dtype), n);
}

int wg_axpy(wg_ctx *ctx, float alpha, wg_dtype dtype, wg_buf *y, wg_view_shape y_shape, const wg_buf *x, wg_view_shape x_shape) {
    const wg_buf *bufs[2] = { y, x };
    if (int rc = check_common("Axpy", ctx, dtype, bufs, 2)) return rc;
    if (y_shape.size[0] != x_shape.size[0])
        return wg_set_error(WG_ERR_DIM_MISMATCH, "Axpy: dimension mismatch. (y has %u rows, x has %u)", y_shape.size[0], x_shape.size[0]);
    if (y->bytes == 0 || x->bytes == 0) return WG_OK;
    const uint32_t n = y_shape.size[0];
    if (n == 0) return WG_OK;
    const View vy = { n, 1, 1, 1, 1, y_shape.offset }, vx = { n, 1, 1, 1, 1, x_shape.offset };
    if (int rc = check_bounds("Axpy", "y", vy, y, dtype)) return rc;
    if (int rc = check_bounds("Axpy", "x", vx, x, dtype)) return rc;
    if (elem_ptr(y, vy.offset, dtype) != elem_ptr(x, vx.offset, dtype)) // (the identical view: defined, as in wg_op_assign)
        if (int rc = check_alias("Axpy", dtype, "y", vy, y->ptr, "x", vx, x->ptr)) return rc;
    WG_HIP_TRY(hipSetDevice(ctx->device));
    return wgk_op_assign(ctx, 5 /* axpy */, dtype, (void *)elem_ptr(y, vy.offset, dtype), elem_ptr(x, vx.offset, dtype), n, alpha);
}

int wg_copy_view(wg_ctx *ctx, wg_dtype dtype, wg_buf *dst, wg_view_shape dst_shape, const wg_buf *src, wg_view_shape src_shape) {
    const wg_buf *bufs[2] = { dst, src };
    if (int rc = check_common("CopyView", ctx, dtype, bufs, 2)) return rc;
    const View d = mk(dst_shape), s = mk(src_shape);
    if (d.mats != s.mats) return wg_set_error(WG_ERR_DIM_MISMATCH, "CopyView: dimension mismatch. (dst has %u matrices, src has %u)", d.mats, s.mats);
    if (dst->bytes == 0 || d.rows == 0 || d.cols == 0 || d.mats == 0) return WG_OK;
    if (int rc = check_bounds("CopyView", "dst", d, dst, dtype)) return rc;
    const bool empty_src = src->bytes == 0 || s.rows == 0 || s.cols == 0;
    if (!empty_src)
        if (int rc = check_bounds("CopyView", "src", s, src, dtype)) return rc;
    if (!empty_src)
        if (int rc = check_alias("CopyView", dtype, "dst", d, dst->ptr, "src", s, src->ptr)) return rc;
    WG_HIP_TRY(hipSetDevice(ctx->device));
    return wgk_stage_copy(ctx, dtype, (void *)elem_ptr(dst, d.offset, dtype), d.stride, d.stride_mat, d.rows, d.cols, empty_src ? dst->ptr : elem_ptr(src, s.offset, dtype),
                          s.stride, s.stride_mat, empty_src ? 0u : s.rows, empty_src ? 0u : s.cols, d.mats);
}

// ---------------------------------------------------------------------------------------------------------------
// ROW_MAJOR operator surface. The reference's `Shape` is row-major when its shaders are composed with
// `row_major_shader_defs()` (shape.rs:11-15; shape.wgsl:49-57: index = t*stride_mat + offset + i*stride + j). A row-major
// R x C view is the same memory as the column-major C x R view with the same stride, so:
//   out = m1 m2      <=>  out^T = m2^T m1^T      : the column-major Gemm on the re-labelled views, operands swapped;
//   out = m1^T m2    <=>  out^T = m2^T (m1^T)^T  : needs the second operand transposed in memory: one HBM-bound transpose
//                                                  (transpose.hip) into a scratch buffer, then the column-major Gemm;
//   out = m v        <=>  column-major GemvTr on the re-labelled matrix;   out = m^T v  <=>  column-major Gemv.
// Vector views (Reduce, OpAssign) index `offset + i` in both orderings: nothing to do.
// ---------------------------------------------------------------------------------------------------------------
static wg_view_shape relabel(wg_view_shape s) {
    const uint32_t r = s.size[0];
    s.size[0] = s.size[1];
    s.size[1] = r;
    return s;
}

// The aliasing rule of a row-major product, under the caller's operator and operand names: a row-major view covers the same elements as its column-major twin. For a
// call that is not skipped: bounds first, as everywhere.
static int check_alias_rm(const char *op, wg_dtype dtype, const wg_buf *out, wg_view_shape out_shape, const char *n1, const wg_buf *m1, wg_view_shape m1_shape, const char *n2,
                          const wg_buf *m2, wg_view_shape m2_shape) {
    const View o = mk(relabel(out_shape)), a = mk(relabel(m1_shape)), b = mk(relabel(m2_shape));
    if (out->bytes == 0 || m1->bytes == 0 || m2->bytes == 0 || o.rows == 0 || o.cols == 0 || o.mats == 0) return WG_OK;
    if (int rc = check_bounds(op, "out", o, out, dtype)) return rc;
    if (int rc = check_bounds(op, n1, a, m1, dtype)) return rc;
    if (int rc = check_bounds(op, n2, b, m2, dtype)) return rc;
    if (int rc = check_alias(op, dtype, "out", o, out->ptr, n1, a, m1->ptr)) return rc;
    return check_alias(op, dtype, "out", o, out->ptr, n2, b, m2->ptr);
}

int wg_gemm_rm(wg_ctx *ctx, wg_gemm_variant variant, wg_dtype dtype, wg_buf *out, wg_view_shape out_shape, const wg_buf *m1,
               wg_view_shape m1_shape, const wg_buf *m2, wg_view_shape m2_shape) {
    const wg_buf *bufs[3] = { out, m1, m2 };
    if (int rc = check_common("Gemm", ctx, dtype, bufs, 3)) return rc;
    if ((int)variant < 0 || (int)variant > 3) return wg_set_error(WG_ERR_INVALID_ARG, "Gemm: unknown variant %d", (int)variant);
    const bool tr = variant == WG_GEMM_TR || variant == WG_GEMM_TR_FAST;
    const View o = mk(out_shape), a = mk(m1_shape), b = mk(m2_shape);
    const uint32_t m_rows = tr ? a.cols : a.rows, m_cols = tr ? a.rows : a.cols; // gemm.rs:81-96, on the row-major shapes
    if (m_cols != b.rows || m_rows != o.rows || o.cols != b.cols || o.mats != a.mats || o.mats != b.mats)
        return wg_set_error(WG_ERR_DIM_MISMATCH,
                            "Gemm: dimension mismatch. (out [%u,%u,%u], m1 [%u,%u,%u]%s, m2 [%u,%u,%u])", o.rows, o.cols, o.mats,
                            a.rows, a.cols, a.mats, tr ? "^T" : "", b.rows, b.cols, b.mats);
    // The aliasing rule under this entry point's own operand names: the forwarded calls swap m1 and m2, and the GemmTr that copies m1 into scratch would never see
    // `out` next to it.
    if (int rc = check_alias_rm("Gemm", dtype, out, out_shape, "m1", m1, m1_shape, "m2", m2, m2_shape)) return rc;
    if (!tr) return wg_gemm_ex(ctx, WG_GEMM, dtype, 1.f, 0.f, out, relabel(out_shape), m2, relabel(m2_shape), m1, relabel(m1_shape));

    // m1 is K x M row-major == column-major M x K (ld = stride); the column-major Gemm needs it as K x M column-major
    if (out->bytes == 0 || m1->bytes == 0 || m2->bytes == 0 || o.rows == 0 || o.cols == 0 || o.mats == 0) return WG_OK;
    const View a_cm = mk(relabel(m1_shape)); // M x K column-major
    if (int rc = check_bounds("Gemm", "m1", a_cm, m1, dtype)) return rc;
    const size_t es = wg_dtype_size(dtype);
    const uint32_t K = a.rows, M = a.cols;
    WG_HIP_TRY(hipSetDevice(ctx->device));
    // From about a round of tiles on: the kernels that take m1 where it lies (gemm_f16_nt.hip; gemm_f32.hip's B_NC tile bodies) -- out^T (N x M) = m2^T (N x K,
    // contiguous along N) * m1 (K x M, contiguous along M); no scratch, no extra pass over m1. WG_TUNE_RM_TR_NATIVE = 0 forces the copy below (tests compare the
    // two ways), 1 the kernels at any size.
    if (ctx->tuning[WG_TUNE_RM_TR_NATIVE] != 0) {
        const View o_cm = mk(relabel(out_shape)), b_cm = mk(relabel(m2_shape)); // N x M and N x K column-major
        const uint32_t tile_n = dtype != WG_F32 ? 256u : 128u;                   // 256 x 256 (f16, bf16) / 256 x 128 (f32) tiles
        const uint64_t tiles = (uint64_t)((o_cm.rows + 255u) / 256u) * ((o_cm.cols + tile_n - 1u) / tile_n) * o_cm.mats;
        const uint64_t cus = (uint64_t)(ctx->compute_units > 0 ? ctx->compute_units : 256);
        // (f32: the copy path's launcher cuts K / takes small tiles below a round of big tiles, which this launch does not: only from a full round on.
        //  f16: the native launcher has the mid-size tiles too (gemm_f16_t128.hip's B_NC instances): from half a round of 128 x 128 tiles on -- below that the copy
        //  path's launcher would cut K over the idle CUs, which the native kernels do not)
        const uint64_t tiles128 = (uint64_t)((o_cm.rows + 127u) / 128u) * ((o_cm.cols + 127u) / 128u) * o_cm.mats;
        if (ctx->tuning[WG_TUNE_RM_TR_NATIVE] == 1 || (dtype != WG_F32 ? 2u * tiles128 >= cus : tiles >= cus)) {
            if (int rc = check_bounds("Gemm", "m2", b_cm, m2, dtype)) return rc;
            if (int rc = check_bounds("Gemm", "out", o_cm, out, dtype)) return rc;
            const wgk_mat A = { elem_ptr(m2, b_cm.offset, dtype), b_cm.stride, b_cm.stride_mat }, B = { elem_ptr(m1, a_cm.offset, dtype), a_cm.stride, a_cm.stride_mat };
            void *o = (void *)elem_ptr(out, o_cm.offset, dtype);
            const int rc = dtype == WG_F16    ? wgk_gemm_f16_nt(ctx, o_cm.rows, o_cm.cols, K, o_cm.mats, (__half *)o, o_cm.stride, o_cm.stride_mat, A, B)
                           : dtype == WG_BF16 ? wgk_gemm_bf16_nt(ctx, o_cm.rows, o_cm.cols, K, o_cm.mats, (wg_bf16 *)o, o_cm.stride, o_cm.stride_mat, A, B)
                                              : wgk_gemm_f32_nt(ctx, o_cm.rows, o_cm.cols, K, o_cm.mats, (float *)o, o_cm.stride, o_cm.stride_mat, A, B);
            if (rc != WG_ERR_UNSUPPORTED) return rc;
        }
    }
    void *ws = nullptr;
    if (int rc = wg_ctx_tr_workspace(ctx, (size_t)K * M * a.mats * es, &ws)) return rc;
    if (int rc = wgk_transpose(ctx, dtype, M, K, a.mats, elem_ptr(m1, a_cm.offset, dtype), a_cm.stride, a_cm.stride_mat, ws, K, (uint64_t)K * M))
        return rc;
    wg_buf tmp;
    tmp.ctx = ctx; tmp.ptr = ws; tmp.bytes = (size_t)K * M * a.mats * es; tmp.usage = 0; tmp.owned = false; tmp.host_pinned = false;
    wg_view_shape ts;
    ts.size[0] = K; ts.size[1] = M; ts.size[2] = a.mats; ts.stride = K; ts.stride_mat = K * M; ts.offset = 0;
    return wg_gemm_ex(ctx, WG_GEMM, dtype, 1.f, 0.f, out, relabel(out_shape), m2, relabel(m2_shape), &tmp, ts);
}

int wg_gemv_rm(wg_ctx *ctx, wg_gemv_variant variant, wg_dtype dtype, wg_buf *out, wg_view_shape out_shape, const wg_buf *m,
               wg_view_shape m_shape, const wg_buf *v, wg_view_shape v_shape) {
    const wg_buf *bufs[3] = { out, m, v };
    if (int rc = check_common("Gemv", ctx, dtype, bufs, 3)) return rc;
    if ((int)variant < 0 || (int)variant > 3) return wg_set_error(WG_ERR_INVALID_ARG, "Gemv: unknown variant %d", (int)variant);
    const bool tr = variant == WG_GEMV_TR || variant == WG_GEMV_TR_FAST;
    const View o = mk(out_shape), mm = mk(m_shape), vv = mk(v_shape);
    const uint32_t m_rows = tr ? mm.cols : mm.rows, m_cols = tr ? mm.rows : mm.cols; // gemv.rs:79-91, on the row-major shapes
    if (m_cols != vv.rows || m_rows != o.rows)
        return wg_set_error(WG_ERR_DIM_MISMATCH, "Gemv: dimension mismatch. (out [%u,%u,%u], m [%u,%u,%u]%s, v [%u,%u,%u])", o.rows,
                            o.cols, o.mats, mm.rows, mm.cols, mm.mats, tr ? "^T" : "", vv.rows, vv.cols, vv.mats);
    if ((variant == WG_GEMV_FAST || variant == WG_GEMV_TR_FAST) && o.rows % 4u != 0)
        return wg_set_error(WG_ERR_PRECONDITION, "Gemv: assertion `left == right` failed (out_nrows %% 4 == 0, gemv.rs:122): out has %u rows",
                            o.rows);
    // Several right-hand sides (grid.y of gemv.wgsl:40,46,62 with the row-major `im`, shape.wgsl:49-57): a row-major matrix of
    // right-hand sides has its columns 1 element apart, which no GEMV kernel streams -- but out (R x n) = op(m) * v (C x n) on row-major
    // views IS the row-major Gemm / GemmTr, i.e. the column-major product out^T (n x R) = v^T * op(m)^T with few rows (the few-row and
    // few-column MFMA kernels). The matrix is shared by the columns and the batch count comes from `out`, as in wg_gemv.
    if (o.cols > 1 || vv.cols > 1) {
        wg_view_shape os = out_shape, ms = m_shape, vs = v_shape;
        ms.size[2] = o.mats;
        vs.size[1] = o.cols;
        vs.size[2] = o.mats;
        if (int rc = check_alias_rm("Gemv", dtype, out, os, "m", m, ms, "v", v, vs)) return rc; // (the refusal names the call that was made, not the Gemm it becomes)
        return wg_gemm_rm(ctx, tr ? WG_GEMM_TR : WG_GEMM, dtype, out, os, m, ms, v, vs);
    }
    return wg_gemv(ctx, tr ? WG_GEMV : WG_GEMV_TR, dtype, out, out_shape, m, relabel(m_shape), v, v_shape);
}

// wg_gemm_q8 with int8 columns and their f32 group scales (include/wgebra_hip.h): wg_gemm_q8's checks in its order with its statuses, the refusal of out = W x before
// any dimension is looked at; both group sizes behind the Gemm dimension check, then the shape of `scales`, then of `x_scales`; bounds with 1 / 4 / 1 / 4 / 4 bytes per
// element of m / scales / x / x_scales / out; `out` against `m` and `x` in 1-byte units. The kernels are the plan's (gemm_q8a8_plan.hip).
int wg_gemm_q8a8(wg_ctx *ctx, wg_gemm_variant variant, uint32_t group_rows, uint32_t x_group_rows, wg_buf *out, wg_view_shape out_shape, const wg_buf *m, wg_view_shape m_shape,
                 const wg_buf *scales, wg_view_shape scales_shape, const wg_buf *x, wg_view_shape x_shape, const wg_buf *x_scales, wg_view_shape x_scales_shape) {
    const wg_buf *bufs[5] = { out, m, scales, x, x_scales };
    if (int rc = check_common("Gemm", ctx, WG_F32, bufs, 5)) return rc;
    if ((int)variant < 0 || (int)variant > 3) return wg_set_error(WG_ERR_INVALID_ARG, "Gemm: unknown variant %d", (int)variant);
    if (variant != WG_GEMM_TR && variant != WG_GEMM_TR_FAST)
        return wg_set_error(WG_ERR_UNSUPPORTED, "Gemm: wg_gemm_q8a8 computes out = W^T x only (WG_GEMM_TR); wg_gemv_q8 computes out = W v, whose scales cannot leave the contraction");
    const View o = mk(out_shape), mm = mk(m_shape), ss = mk(scales_shape), xx = mk(x_shape), xs = mk(x_scales_shape);

    if (mm.rows != xx.rows || mm.cols != o.rows || o.cols != xx.cols || o.mats != mm.mats || o.mats != xx.mats)
        return wg_set_error(WG_ERR_DIM_MISMATCH, "Gemm: dimension mismatch. (out [%u,%u,%u], m1 [%u,%u,%u]^T, m2 [%u,%u,%u])", o.rows, o.cols, o.mats, mm.rows, mm.cols,
                            mm.mats, xx.rows, xx.cols, xx.mats);
    const uint32_t k = mm.rows;
    if (group_rows == 0 || (group_rows % 16u != 0 && group_rows < k))
        return wg_set_error(WG_ERR_INVALID_ARG, "Gemm: group_rows %u is neither a positive multiple of 16 nor at least the %u rows of m", group_rows, k);
    if (x_group_rows == 0 || (x_group_rows % 16u != 0 && x_group_rows < k))
        return wg_set_error(WG_ERR_INVALID_ARG, "Gemm: x_group_rows %u is neither a positive multiple of 16 nor at least the %u rows of x", x_group_rows, k);
    if (group_rows < k && x_group_rows < k && group_rows % x_group_rows != 0 && x_group_rows % group_rows != 0)
        return wg_set_error(WG_ERR_INVALID_ARG, "Gemm: of group_rows %u and x_group_rows %u, both below the %u rows, neither divides the other", group_rows, x_group_rows, k);
    const uint32_t s_rows = k / group_rows + (k % group_rows != 0);
    if (ss.rows != s_rows || ss.cols != mm.cols || ss.mats != mm.mats)
        return wg_set_error(WG_ERR_DIM_MISMATCH, "Gemm: dimension mismatch. (m [%u,%u,%u], group_rows %u, scales [%u,%u,%u], expected [%u,%u,%u])", mm.rows, mm.cols, mm.mats,
                            group_rows, ss.rows, ss.cols, ss.mats, s_rows, mm.cols, mm.mats);
    const uint32_t xs_rows = k / x_group_rows + (k % x_group_rows != 0);
    if (xs.rows != xs_rows || xs.cols != xx.cols || xs.mats != xx.mats)
        return wg_set_error(WG_ERR_DIM_MISMATCH, "Gemm: dimension mismatch. (x [%u,%u,%u], x_group_rows %u, x_scales [%u,%u,%u], expected [%u,%u,%u])", xx.rows, xx.cols, xx.mats,
                            x_group_rows, xs.rows, xs.cols, xs.mats, xs_rows, xx.cols, xx.mats);
    if (out->bytes == 0 || m->bytes == 0 || scales->bytes == 0 || x->bytes == 0 || x_scales->bytes == 0) return WG_OK;
    if (o.rows == 0 || o.cols == 0 || o.mats == 0) return WG_OK;

    if (int rc = check_bounds("Gemm", "out", o, out, WG_F32)) return rc;
    if (int rc = check_bounds_es("Gemm", "m", mm, m, 1)) return rc;
    if (int rc = check_bounds("Gemm", "scales", ss, scales, WG_F32)) return rc;
    if (int rc = check_bounds_es("Gemm", "x", xx, x, 1)) return rc;
    if (int rc = check_bounds("Gemm", "x_scales", xs, x_scales, WG_F32)) return rc;
    if (int rc = check_alias_f32_u8("Gemm", "out", o, out->ptr, "m", mm, m->ptr)) return rc;
    if (int rc = check_alias("Gemm", WG_F32, "out", o, out->ptr, "scales", ss, scales->ptr)) return rc;
    if (int rc = check_alias_f32_u8("Gemm", "out", o, out->ptr, "x", xx, x->ptr)) return rc;
    if (int rc = check_alias("Gemm", WG_F32, "out", o, out->ptr, "x_scales", xs, x_scales->ptr)) return rc;

    const wgk_mat M = { (const char *)m->ptr + mm.offset, mm.stride, mm.stride_mat };
    const wgk_mat S = { elem_ptr(scales, ss.offset, WG_F32), ss.stride, ss.stride_mat };
    const wgk_mat X = { (const char *)x->ptr + xx.offset, xx.stride, xx.stride_mat };
    const wgk_mat XS = { elem_ptr(x_scales, xs.offset, WG_F32), xs.stride, xs.stride_mat };
    float *O = (float *)elem_ptr(out, o.offset, WG_F32);
    wg_gemm_q8a8_query q = {};
    q.k = k; q.outputs = mm.cols; q.n = o.cols; q.mats = o.mats; q.group_rows = group_rows; q.x_group_rows = x_group_rows;
    q.ldm = mm.stride; q.lds = ss.stride; q.ldx = xx.stride; q.ldxs = xs.stride; q.ldo = o.stride;
    q.m_batch = mm.stride_mat; q.s_batch = ss.stride_mat; q.x_batch = xx.stride_mat; q.xs_batch = xs.stride_mat; q.o_batch = o.stride_mat;
    q.m_addr16 = (uint32_t)((uintptr_t)M.ptr % 16u); q.x_addr16 = (uint32_t)((uintptr_t)X.ptr % 16u); q.o_addr16 = (uint32_t)((uintptr_t)O % 16u);
    q.cus = (uint32_t)wg_ctx_cus(ctx);
    const wg_gemm_q8a8_plan p = gemm_q8a8_plan(q);
    WG_HIP_TRY(hipSetDevice(ctx->device));
    return wgk_gemm_q8a8(ctx, p, group_rows, x_group_rows, k, mm.cols, o.cols, o.mats, O, o.stride, o.stride_mat, M, S, X, XS);
}

namespace {
// Two views of any element sizes (1, 2 or 4 bytes), both in 1-byte units (views_overlap.hpp's scaling, for either side): a view with rows, stride and stride_mat
// multiplied by its element size and its offset folded into the byte base has the same footprint as a view of 1-byte elements. A scaled field that leaves 32 bits
// leaves the intervals: disjoint intervals are disjoint footprints, anything else is refused as "may overlap".
bool bytes_view(const View &v, const void *base, uint32_t es, wg_view_shape &out, uint64_t &byte_base) {
    const uint64_t rows = (uint64_t)es * v.rows, stride = v.cols > 1 ? (uint64_t)es * v.stride : rows, stride_mat = v.mats > 1 ? (uint64_t)es * v.stride_mat : 0;
    byte_base = (uint64_t)(uintptr_t)base + (uint64_t)es * v.offset;
    if (rows > 0xffffffffull || stride > 0xffffffffull || stride_mat > 0xffffffffull) return false;
    out = wg_view_shape{ { (uint32_t)rows, v.cols, v.mats }, (uint32_t)stride, (uint32_t)stride_mat, 0 };
    return true;
}
int check_alias_bytes(const char *op, const char *wname, const View &w, const void *base_w, uint32_t wes, const char *rname, const View &r, const void *base_r, uint32_t res) {
    if (extent(w) == 0 || extent(r) == 0) return WG_OK;
    wg_view_shape a, b;
    uint64_t ba, bb;
    const bool oka = bytes_view(w, base_w, wes, a, ba), okb = bytes_view(r, base_r, res, b, bb);
    int exact = 1;
    if (oka && okb) {
        if (!wg_views_overlap(a, ba, b, bb, 1, &exact)) return WG_OK;
        return aliased(op, wname, rname, exact);
    }
    typedef unsigned __int128 u128;
    const u128 lo_a = ba, hi_a = lo_a + (u128)wes * (extent(w) - w.offset), lo_b = bb, hi_b = lo_b + (u128)res * (extent(r) - r.offset);
    if (hi_a <= lo_b || hi_b <= lo_a) return WG_OK;
    return aliased(op, wname, rname, 0);
}
} // namespace

// The device-side quantiser (include/wgebra_hip.h): q and scales from src. The checks: context, dtype and buffers; q against src, group_rows, the scales' shape; empty
// operands skipped; bounds with 1 / 4 / src bytes per element; q and scales against src and against each other, on addresses. The kernels: quantize_q8.hip.
int wg_quantize_q8(wg_ctx *ctx, wg_dtype src_dtype, uint32_t group_rows, wg_buf *q, wg_view_shape q_shape, wg_buf *scales, wg_view_shape scales_shape, const wg_buf *src,
                   wg_view_shape src_shape) {
    const wg_buf *bufs[3] = { q, scales, src };
    if (int rc = check_common("Quantize", ctx, src_dtype, bufs, 3)) return rc;
    const View qq = mk(q_shape), ss = mk(scales_shape), sv = mk(src_shape);
    if (qq.rows != sv.rows || qq.cols != sv.cols || qq.mats != sv.mats)
        return wg_set_error(WG_ERR_DIM_MISMATCH, "Quantize: dimension mismatch. (q [%u,%u,%u], src [%u,%u,%u])", qq.rows, qq.cols, qq.mats, sv.rows, sv.cols, sv.mats);
    if (group_rows == 0 || (group_rows % 16u != 0 && group_rows < qq.rows))
        return wg_set_error(WG_ERR_INVALID_ARG, "Quantize: group_rows %u is neither a positive multiple of 16 nor at least the %u rows of src", group_rows, qq.rows);
    const uint32_t s_rows = qq.rows / group_rows + (qq.rows % group_rows != 0);
    if (ss.rows != s_rows || ss.cols != qq.cols || ss.mats != qq.mats)
        return wg_set_error(WG_ERR_DIM_MISMATCH, "Quantize: dimension mismatch. (q [%u,%u,%u], group_rows %u, scales [%u,%u,%u], expected [%u,%u,%u])", qq.rows, qq.cols, qq.mats,
                            group_rows, ss.rows, ss.cols, ss.mats, s_rows, qq.cols, qq.mats);
    if (q->bytes == 0 || scales->bytes == 0 || src->bytes == 0) return WG_OK;
    if (qq.rows == 0 || qq.cols == 0 || qq.mats == 0) return WG_OK;

    const uint32_t es = (uint32_t)wg_dtype_size(src_dtype);
    if (int rc = check_bounds_es("Quantize", "q", qq, q, 1)) return rc;
    if (int rc = check_bounds("Quantize", "scales", ss, scales, WG_F32)) return rc;
    if (int rc = check_bounds("Quantize", "src", sv, src, src_dtype)) return rc;
    if (int rc = check_alias_bytes("Quantize", "q", qq, q->ptr, 1, "src", sv, src->ptr, es)) return rc;
    if (int rc = check_alias_bytes("Quantize", "scales", ss, scales->ptr, 4, "src", sv, src->ptr, es)) return rc;
    if (int rc = check_alias_bytes("Quantize", "q", qq, q->ptr, 1, "scales", ss, scales->ptr, 4)) return rc;

    int8_t *Q = (int8_t *)q->ptr + qq.offset;
    float *S = (float *)elem_ptr(scales, ss.offset, WG_F32);
    const wgk_mat SRC = { elem_ptr(src, sv.offset, src_dtype), sv.stride, sv.stride_mat };
    wg_quantize_q8_query qu = {};
    qu.rows = qq.rows; qu.cols = qq.cols; qu.mats = qq.mats; qu.group_rows = group_rows; qu.src_elem = es;
    qu.ldq = qq.stride; qu.ldsrc = sv.stride; qu.q_batch = qq.stride_mat; qu.src_batch = sv.stride_mat;
    qu.q_addr16 = (uint32_t)((uintptr_t)Q % 16u); qu.src_addr16 = (uint32_t)((uintptr_t)SRC.ptr % 16u);
    const wg_quantize_q8_plan p = quantize_q8_plan(qu);
    WG_HIP_TRY(hipSetDevice(ctx->device));
    return wgk_quantize_q8(ctx, p, src_dtype, group_rows, qq.rows, qq.cols, qq.mats, Q, qq.stride, qq.stride_mat, S, ss.stride, ss.stride_mat, SRC);
}

} // extern "C"
