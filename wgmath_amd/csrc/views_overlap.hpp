// Do two operator views share memory? (views_overlap.hip: host arithmetic on two wg_view_shape and two byte addresses -- no kernel, no device call, no context,
// nothing else of the library.) The operator front-end (api.hip) asks it for every (written, read) pair of a call and refuses the call with WG_ERR_ALIASED when the
// answer is yes; tests read it through wg_debug_views_overlap, and tests/cpp/overlap_check.cpp links the unit alone under the host sanitizers.
#pragma once
#include <cstdint>

#include "../../include/wgebra_hip.h"

// The footprint of a view: the bytes [base + e * elem_size, + elem_size) of every element e = t * stride_mat + offset + i + j * stride it addresses
// (i < size[0], j < size[1], t < size[2]); `base` is the byte address of element 0 of the buffer the view indexes. A view with a zero size has no footprint.
// Returns 1 when the two footprints share a byte, 0 when they do not. Decided in three steps:
//   1. the byte intervals [first byte, last byte] of the two views: disjoint intervals are disjoint footprints (the common case: a few integer comparisons);
//   2. each view as column runs -- one contiguous run per (column, matrix); columns at most `rows` apart and matrices at most one matrix apart are folded into one run
//      first, so a dense matrix or cube is ONE run --: while the two views have at most WG_VIEWS_OVERLAP_MAX_RUNS runs between them the runs are walked in address
//      order and the answer is exact (*exact = 1);
//   3. above that bound the answer is 1 ("overlaps") whatever the truth, and *exact = 0.
// `exact` may be NULL. Never answers 0 for footprints that intersect.
int wg_views_overlap(const wg_view_shape &a, uint64_t byte_base_a, const wg_view_shape &b, uint64_t byte_base_b, uint32_t elem_size, int *exact);

// Views of DIFFERENT element sizes (wg_gemv_mixed: an f32 `out` against a 16-bit matrix, possibly in one buffer): both are compared in 2-byte units. A column of r
// f32 elements is one contiguous run of 2 r units, so the f32 view with rows, stride and stride_mat doubled -- and its offset folded into the byte base -- has the
// same footprint as a view of 2-byte elements, and the exact comparison above applies with elem_size 2. A doubled field that no longer fits the 32 bits of
// wg_view_shape (an f32 view of 2^31 rows and more, or strides that large where they count) leaves the intervals: disjoint intervals are disjoint footprints,
// anything else is answered 1 with *exact = 0, like a pair past the run bound.
inline int wg_views_overlap_f32_u16(const wg_view_shape &f32_view, uint64_t byte_base_f32, const wg_view_shape &u16_view, uint64_t byte_base_u16, int *exact) {
    if (exact) *exact = 1;
    const wg_view_shape &s = f32_view;
    if (s.size[0] == 0 || s.size[1] == 0 || s.size[2] == 0) return 0;
    const uint64_t rows = 2ull * s.size[0], stride = s.size[1] > 1 ? 2ull * s.stride : rows, stride_mat = s.size[2] > 1 ? 2ull * s.stride_mat : 0;
    const uint64_t base = byte_base_f32 + 4ull * s.offset; // (a device address plus at most 16 GiB: no wrap)
    if (rows <= 0xffffffffull && stride <= 0xffffffffull && stride_mat <= 0xffffffffull) {
        const wg_view_shape scaled = { { (uint32_t)rows, s.size[1], s.size[2] }, (uint32_t)stride, (uint32_t)stride_mat, 0 };
        return wg_views_overlap(scaled, base, u16_view, byte_base_u16, 2, exact);
    }
    // the intervals alone: each view as ONE dense column of its whole extent (extents in 128 bits; a view whose extent does not fit a column of 2^32 - 1 elements
    // cannot be stated that way either and is answered conservatively)
    typedef unsigned __int128 u128;
    const u128 ext_f = (u128)(s.size[2] - 1) * s.stride_mat + (u128)(s.size[1] - 1) * s.stride + s.size[0]; // f32 elements from the first one on
    const wg_view_shape &h = u16_view;
    if (h.size[0] == 0 || h.size[1] == 0 || h.size[2] == 0) return 0;
    const u128 ext_h = (u128)(h.size[2] - 1) * h.stride_mat + (u128)(h.size[1] - 1) * h.stride + h.size[0];
    const u128 lo_f = base, hi_f = lo_f + 4 * ext_f, lo_h = (u128)byte_base_u16 + 2ull * h.offset, hi_h = lo_h + 2 * ext_h;
    if (hi_f <= lo_h || hi_h <= lo_f) return 0;
    if (exact) *exact = 0;
    return 1;
}

// ... and an f32 view against a view of 1-BYTE elements (wg_gemv_q8: an f32 `out` against the int8 matrix, possibly in one buffer): both are compared in 1-byte units.
// The f32 view with rows, stride and stride_mat scaled by 4 -- and its offset folded into the byte base -- has the same footprint as a view of 1-byte elements, and
// the exact comparison applies with elem_size 1. A scaled field that leaves 32 bits (an f32 view of 2^30 rows and more, or strides that large where they count) leaves
// the intervals, as above: disjoint intervals are disjoint footprints, anything else is answered 1 with *exact = 0.
inline int wg_views_overlap_f32_u8(const wg_view_shape &f32_view, uint64_t byte_base_f32, const wg_view_shape &u8_view, uint64_t byte_base_u8, int *exact) {
    if (exact) *exact = 1;
    const wg_view_shape &s = f32_view;
    if (s.size[0] == 0 || s.size[1] == 0 || s.size[2] == 0) return 0;
    const uint64_t rows = 4ull * s.size[0], stride = s.size[1] > 1 ? 4ull * s.stride : rows, stride_mat = s.size[2] > 1 ? 4ull * s.stride_mat : 0;
    const uint64_t base = byte_base_f32 + 4ull * s.offset; // (a device address plus at most 16 GiB: no wrap)
    if (rows <= 0xffffffffull && stride <= 0xffffffffull && stride_mat <= 0xffffffffull) {
        const wg_view_shape scaled = { { (uint32_t)rows, s.size[1], s.size[2] }, (uint32_t)stride, (uint32_t)stride_mat, 0 };
        return wg_views_overlap(scaled, base, u8_view, byte_base_u8, 1, exact);
    }
    typedef unsigned __int128 u128;
    const u128 ext_f = (u128)(s.size[2] - 1) * s.stride_mat + (u128)(s.size[1] - 1) * s.stride + s.size[0]; // f32 elements from the first one on
    const wg_view_shape &h = u8_view;
    if (h.size[0] == 0 || h.size[1] == 0 || h.size[2] == 0) return 0;
    const u128 ext_h = (u128)(h.size[2] - 1) * h.stride_mat + (u128)(h.size[1] - 1) * h.stride + h.size[0];
    const u128 lo_f = base, hi_f = lo_f + 4 * ext_f, lo_h = (u128)byte_base_u8 + h.offset, hi_h = lo_h + ext_h;
    if (hi_f <= lo_h || hi_h <= lo_f) return 0;
    if (exact) *exact = 0;
    return 1;
}
