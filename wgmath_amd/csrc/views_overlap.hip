// The overlap predicate of the operator front-end (views_overlap.hpp): do the footprints of two views share a byte? Host arithmetic only; compiled once, linked
// into the library for api.hip and wg_debug_views_overlap, and alone into tests/cpp/overlap_check.cpp.
#include "views_overlap.hpp"

#include <algorithm>
#include <vector>

namespace {

// (byte addresses in 128 bits: base + (mats - 1) * stride_mat * elem_size of an arbitrary wg_view_shape does not fit 64, and a wrapped address would be a wrong answer)
typedef unsigned __int128 u128;

// A view as nc x nm runs of `len` bytes: run (j, t) starts at first + j * step_c + t * step_m. n == 0: no footprint.
struct Runs {
    u128 first = 0, len = 0, step_c = 0, step_m = 0, end = 0; // end: one past the last byte of the view
    uint64_t nc = 0, nm = 0, n = 0;
};

Runs runs_of(const wg_view_shape &s, uint64_t base, uint32_t es) {
    Runs r;
    const u128 rows = s.size[0], cols = s.size[1], mats = s.size[2];
    if (rows == 0 || cols == 0 || mats == 0 || es == 0) return r;
    u128 len = rows; // elements of one run
    r.nc = s.size[1];
    r.nm = s.size[2];
    if (cols == 1 || s.stride <= rows) { // columns that touch or overlap each other: one run per matrix
        len = (cols - 1) * s.stride + rows;
        r.nc = 1;
        if (mats == 1 || s.stride_mat <= len) { // and matrices that do: one run
            len = (mats - 1) * s.stride_mat + len;
            r.nm = 1;
        }
    }
    r.first = (u128)base + (u128)s.offset * es;
    r.len = len * es;
    r.step_c = (u128)s.stride * es;
    r.step_m = (u128)s.stride_mat * es;
    r.n = r.nc * r.nm;
    r.end = r.first + (r.nm - 1) * r.step_m + (r.nc - 1) * r.step_c + r.len;
    return r;
}

struct Run {
    u128 lo, hi;
    int who;
};

} // namespace

int wg_views_overlap(const wg_view_shape &a, uint64_t byte_base_a, const wg_view_shape &b, uint64_t byte_base_b, uint32_t elem_size, int *exact) {
    if (exact) *exact = 1;
    const Runs ra = runs_of(a, byte_base_a, elem_size), rb = runs_of(b, byte_base_b, elem_size);
    if (ra.n == 0 || rb.n == 0) return 0;
    if (ra.end <= rb.first || rb.end <= ra.first) return 0; // 1. the intervals
    if (ra.n == 1 && rb.n == 1) return 1;                   // (two runs whose intervals intersect)
    if (ra.n > WG_VIEWS_OVERLAP_MAX_RUNS || rb.n > WG_VIEWS_OVERLAP_MAX_RUNS || ra.n + rb.n > WG_VIEWS_OVERLAP_MAX_RUNS) { // 3. too many runs to walk
        if (exact) *exact = 0;
        return 1;
    }
    // 2. every run of both views that reaches into the other view's interval, in address order: a run that starts before the furthest end seen so far of the OTHER
    // view's runs shares its first byte with one of them (runs are never empty); runs of one view may overlap each other freely
    std::vector<Run> all;
    all.reserve((size_t)(ra.n + rb.n));
    const Runs *rs[2] = { &ra, &rb };
    for (int w = 0; w < 2; ++w) {
        const Runs &r = *rs[w], &o = *rs[1 - w];
        for (uint64_t t = 0; t < r.nm; ++t)
            for (uint64_t j = 0; j < r.nc; ++j) {
                const u128 lo = r.first + t * r.step_m + j * r.step_c, hi = lo + r.len;
                if (hi > o.first && lo < o.end) all.push_back(Run{ lo, hi, w });
            }
    }
    std::sort(all.begin(), all.end(), [](const Run &x, const Run &y) { return x.lo < y.lo; });
    u128 seen_end[2] = { 0, 0 };
    for (const Run &r : all) {
        if (r.lo < seen_end[1 - r.who]) return 1;
        if (r.hi > seen_end[r.who]) seen_end[r.who] = r.hi;
    }
    return 0;
}

extern "C" int wg_debug_views_overlap(wg_view_shape shape_a, uint64_t byte_base_a, wg_view_shape shape_b, uint64_t byte_base_b, uint32_t elem_size, int *exact) {
    return wg_views_overlap(shape_a, byte_base_a, shape_b, byte_base_b, elem_size, exact);
}
