// The overlap predicate alone (wgmath_amd/csrc/views_overlap.hip, nothing else of the library) under the host sanitizers, against a naive double loop over the
// elements of both views: the grid of tests/test_operand_overlap.py::test_predicate_matches_brute_force (sizes, strides, offsets, matrix counts, element sizes
// and byte bases that make the views disjoint, touching, shifted by one element, shifted by a few, or identical), seeded, plus views past the run bound and at
// the ends of the 32-bit shape fields. Host code only: built and run by tests/test_cpp_overlap.py on the CPU, never on a GPU.
#include <cstdint>
#include <cstdio>

#include "wgebra_hip.h"

static int failures = 0;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) { // xorshift64*, seeded above: the same pairs on every run
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (uint32_t)(((rng_state * 0x2545F4914F6CDD1Dull) >> 33) % n);
}

static uint64_t extent(const wg_view_shape &s) { // one past the last element index (0: no footprint)
    if (!s.size[0] || !s.size[1] || !s.size[2]) return 0;
    return (uint64_t)(s.size[2] - 1) * s.stride_mat + s.offset + (s.size[0] - 1) + (uint64_t)(s.size[1] - 1) * s.stride + 1;
}

static int naive(const wg_view_shape &a, uint64_t ba, const wg_view_shape &b, uint64_t bb, uint32_t es) {
    for (uint32_t ta = 0; ta < a.size[2]; ++ta) for (uint32_t ja = 0; ja < a.size[1]; ++ja) for (uint32_t ia = 0; ia < a.size[0]; ++ia) {
        const uint64_t pa = ba + ((uint64_t)ta * a.stride_mat + a.offset + ia + (uint64_t)ja * a.stride) * es;
        for (uint32_t tb = 0; tb < b.size[2]; ++tb) for (uint32_t jb = 0; jb < b.size[1]; ++jb) for (uint32_t ib = 0; ib < b.size[0]; ++ib) {
            const uint64_t pb = bb + ((uint64_t)tb * b.stride_mat + b.offset + ib + (uint64_t)jb * b.stride) * es;
            if (pa < pb + es && pb < pa + es) return 1;
        }
    }
    return 0;
}

static wg_view_shape random_view() {
    static const uint32_t sizes[] = { 0, 1, 3, 4, 5, 8 }, offsets[] = { 0, 1, 3, 4, 7 };
    wg_view_shape s;
    const uint32_t rows = sizes[rnd(6)], cols = sizes[rnd(6)];
    s.size[0] = rows; s.size[1] = cols; s.size[2] = 1 + rnd(3);
    const uint32_t strides[] = { rows, rows + 1, rows + 3, 2 * rows };
    s.stride = strides[rnd(4)];
    const uint32_t mat = s.stride * (cols ? cols : 1);
    const uint32_t stride_mats[] = { rows * cols, mat, mat + 3, 2 * mat, 1 }; // dense, whole columns, a gap, room for another view between, GpuCubeView::matrix's 1
    s.stride_mat = stride_mats[rnd(5)];
    s.offset = offsets[rnd(5)];
    return s;
}

static void expect(int got, int exact, int want, int want_exact, const char *what) {
    if (got == want && exact == want_exact) return;
    fprintf(stderr, "%s: got %d (exact %d), expected %d (exact %d)\n", what, got, exact, want, want_exact);
    ++failures;
}

int main() {
    unsigned long pairs = 0, overlapping = 0, inexact = 0;
    for (int it = 0; it < 40000; ++it) {
        const wg_view_shape a = random_view(), b = random_view();
        const uint32_t es = rnd(2) ? 4u : 2u;
        const uint64_t ba = 1ull << 20, ea = extent(a), eb = extent(b);
        uint64_t bb = ba;
        switch (rnd(6)) {
        case 0: bb = ba + (ea + 16) * es; break;                                       // disjoint, b behind a
        case 1: bb = ba + (ea - b.offset) * es; break;                                 // touching: b's first byte is a's end (unsigned wrap is fine: + offset follows)
        case 2: bb = ba + es; break;                                                   // shifted by one element
        case 3: bb = ba - es; break;
        case 4: bb = ba + ((uint64_t)rnd((uint32_t)(ea + eb + 1)) - eb) * es; break;   // anywhere from wholly in front to wholly behind
        default: break;                                                                // the same buffer
        }
        int exact = -1;
        const int got = wg_debug_views_overlap(a, ba, b, bb, es, &exact), want = naive(a, ba, b, bb, es);
        const int sym = wg_debug_views_overlap(b, bb, a, ba, es, nullptr);
        ++pairs;
        overlapping += want;
        inexact += exact == 0;
        if (got != sym || (exact != 0 && exact != 1) || (exact && got != want) || (want && !got)) {
            fprintf(stderr, "a [%u,%u,%u] s=%u sm=%u off=%u @%llu  b [%u,%u,%u] s=%u sm=%u off=%u @%llu  es=%u: got %d (swapped %d, exact %d), the double loop says %d\n",
                    a.size[0], a.size[1], a.size[2], a.stride, a.stride_mat, a.offset, (unsigned long long)ba, b.size[0], b.size[1], b.size[2], b.stride, b.stride_mat,
                    b.offset, (unsigned long long)bb, es, got, sym, exact, want);
            ++failures;
        }
    }
    if (inexact) { fprintf(stderr, "%lu small pairs were answered conservatively\n", inexact); ++failures; }
    if (overlapping < pairs / 10 || pairs - overlapping < pairs / 10) { fprintf(stderr, "the grid is lopsided: %lu of %lu pairs overlap\n", overlapping, pairs); ++failures; }

    int exact = -1, r;
    // past the run bound: two one-row views of 3000 columns two elements apart, the second shifted by one element -- they interleave without touching
    const wg_view_shape comb = { { 1, 3000, 1 }, 2, 6000, 0 };
    r = wg_debug_views_overlap(comb, 4096, comb, 4096 + 4, 4, &exact);
    expect(r, exact, 1, 0, "interleaved combs past the run bound");
    r = wg_debug_views_overlap(comb, 4096, comb, 4096 + 6000 * 4, 4, &exact);
    expect(r, exact, 0, 1, "combs past the run bound with disjoint intervals");
    // just under the bound (2048 + 2047 runs): walked, and exact both ways
    const wg_view_shape c1 = { { 1, 2048, 1 }, 2, 4096, 0 }, c2 = { { 1, 2047, 1 }, 2, 4096, 0 };
    r = wg_debug_views_overlap(c1, 4096, c2, 4096 + 4, 4, &exact);
    expect(r, exact, 0, 1, "interleaved combs under the run bound");
    r = wg_debug_views_overlap(c1, 4096, c2, 4096 + 8, 4, &exact);
    expect(r, exact, 1, 1, "coinciding combs under the run bound");
    // a dense cube is one run however many columns it has
    const wg_view_shape cube = { { 64, 100000, 7 }, 64, 6400000, 5 }, one = { { 1, 1, 1 }, 1, 1, 0 };
    r = wg_debug_views_overlap(cube, 0, one, (5ull + 44799999ull) * 2, 2, &exact);
    expect(r, exact, 1, 1, "the last element of a dense cube");
    r = wg_debug_views_overlap(cube, 0, one, (5ull + 44800000ull) * 2, 2, &exact);
    expect(r, exact, 0, 1, "the element behind a dense cube");
    // the ends of the 32-bit fields: addresses past 2^64 must not wrap into a wrong answer
    const uint32_t big = 0xFFFFFFFFu;
    const wg_view_shape huge = { { big, big, big }, big, big, big };
    r = wg_debug_views_overlap(huge, ~0ull, one, 0, 4, &exact);
    expect(r, exact, 0, 1, "a view whose addresses pass 2^64 against element 0");
    r = wg_debug_views_overlap(huge, 0, huge, 0, 4, &exact);
    expect(r, exact, 1, 1, "the largest view against itself");
    const wg_view_shape sparse = { { 1, big, big }, big, big, 0 }; // 2^64 runs
    r = wg_debug_views_overlap(sparse, 0, sparse, 4, 4, &exact);
    expect(r, exact, 1, 0, "about 2^64 runs");
    // zero-sized views and a zero element size overlap nothing
    const wg_view_shape empty = { { 0, 5, 1 }, 8, 40, 0 };
    r = wg_debug_views_overlap(empty, 0, cube, 0, 2, &exact);
    expect(r, exact, 0, 1, "an empty view");
    r = wg_debug_views_overlap(cube, 0, cube, 0, 0, nullptr);
    expect(r, 1, 0, 1, "element size 0");

    printf("%lu pairs (%lu overlapping), %d failures\n", pairs, overlapping, failures);
    if (!failures) puts("OVERLAP OK");
    return failures ? 1 : 0;
}
