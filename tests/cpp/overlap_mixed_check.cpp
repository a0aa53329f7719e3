// The overlap predicate between views of DIFFERENT element sizes (wg_gemv_mixed: an f32 `out` against a 16-bit matrix, possibly in one buffer): the 2-byte-unit
// scaling of the f32 view (wgmath_amd/csrc/views_overlap.hpp, wg_views_overlap_f32_u16) against a brute-force intersection of the two byte sets, on seeded small
// random pairs -- disjoint, touching, shifted by one byte, by a few, interleaved, identical -- plus f32 views too large for the scaled 32-bit fields. Host code
// only: built with the host sanitizers and run by tests/test_cpp_overlap_mixed.py on the CPU, never on a GPU.
#include <cstdint>
#include <cstdio>
#include <set>

#include "views_overlap.hpp"

static int failures = 0;

static uint64_t rng_state = 0xD1B54A32D192ED03ull;
static uint32_t rnd(uint32_t n) { // xorshift64*, seeded above: the same pairs on every run
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (uint32_t)(((rng_state * 0x2545F4914F6CDD1Dull) >> 33) % n);
}

static uint64_t extent(const wg_view_shape &s) { // one past the last element index counted from element 0 of the buffer (0: no footprint)
    if (!s.size[0] || !s.size[1] || !s.size[2]) return 0;
    return (uint64_t)(s.size[2] - 1) * s.stride_mat + s.offset + (s.size[0] - 1) + (uint64_t)(s.size[1] - 1) * s.stride + 1;
}

static std::set<uint64_t> bytes_of(const wg_view_shape &s, uint64_t base, uint32_t es) {
    std::set<uint64_t> out;
    for (uint32_t t = 0; t < s.size[2]; ++t)
        for (uint32_t j = 0; j < s.size[1]; ++j)
            for (uint32_t i = 0; i < s.size[0]; ++i) {
                const uint64_t p = base + ((uint64_t)t * s.stride_mat + s.offset + i + (uint64_t)j * s.stride) * es;
                for (uint32_t b = 0; b < es; ++b) out.insert(p + b);
            }
    return out;
}

static int brute(const wg_view_shape &f, uint64_t bf, const wg_view_shape &h, uint64_t bh) {
    const std::set<uint64_t> a = bytes_of(f, bf, 4), b = bytes_of(h, bh, 2);
    for (uint64_t p : a)
        if (b.count(p)) return 1;
    return 0;
}

static wg_view_shape random_view() {
    static const uint32_t sizes[] = { 0, 1, 3, 4, 5, 8 }, offsets[] = { 0, 1, 3, 4, 7 };
    wg_view_shape s;
    const uint32_t rows = sizes[rnd(6)], cols = sizes[rnd(6)];
    s.size[0] = rows; s.size[1] = cols; s.size[2] = 1 + rnd(3);
    const uint32_t strides[] = { rows, rows + 1, rows + 3, 2 * rows, 3 * rows + 2 };
    s.stride = strides[rnd(5)];
    const uint32_t mat = s.stride * (cols ? cols : 1);
    const uint32_t stride_mats[] = { rows * cols, mat, mat + 3, 2 * mat, 1 };
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
    unsigned long pairs = 0, overlapping = 0, touching = 0, interleaved = 0;
    for (int it = 0; it < 6000; ++it) {
        const wg_view_shape f = random_view(), h = random_view(); // f: f32 elements, h: 16-bit elements
        const uint64_t bf = 1ull << 20, ef = extent(f) * 4, eh = extent(h) * 2;
        uint64_t bh = bf;
        const uint32_t how = rnd(7);
        switch (how) {
        case 0: bh = bf + ef + 32; break;                                     // disjoint, h behind f
        case 1: bh = bf + ef - 2ull * h.offset; break;                        // touching: h's first byte is the byte behind f's last
        case 2: bh = bf + ef - 2ull * h.offset - 1; break;                    // ONE byte of overlap (an odd address: decided on addresses, never dereferenced)
        case 3: bh = bf + 4ull * f.offset - eh; break;                           // touching from the front: h ends where f begins
        case 4: bh = bf + 2 * rnd((uint32_t)(ef / 2 + eh / 2 + 1)) - eh; break; // anywhere from wholly in front to wholly behind, 2-byte steps
        case 5: bh = bf + rnd((uint32_t)(ef + eh + 1)) - eh; break;           // ... any byte
        default: break;                                                       // the same buffer: interleaved where the strides leave room
        }
        int exact = -1;
        const int got = wg_views_overlap_f32_u16(f, bf, h, bh, &exact), want = brute(f, bf, h, bh);
        ++pairs;
        overlapping += want;
        if (!want && ef && eh) {
            const uint64_t lo_f = bf + 4ull * f.offset, hi_f = bf + ef, lo_h = bh + 2ull * h.offset, hi_h = bh + eh;
            if (hi_f == lo_h || hi_h == lo_f) ++touching;
            else if (lo_f < hi_h && lo_h < hi_f) ++interleaved;
        }
        if (exact != 1 || got != want) {
            fprintf(stderr, "f32 [%u,%u,%u] s=%u sm=%u off=%u @%llu  u16 [%u,%u,%u] s=%u sm=%u off=%u @%llu (case %u): got %d (exact %d), the byte sets say %d\n", f.size[0],
                    f.size[1], f.size[2], f.stride, f.stride_mat, f.offset, (unsigned long long)bf, h.size[0], h.size[1], h.size[2], h.stride, h.stride_mat, h.offset,
                    (unsigned long long)bh, how, got, exact, want);
            ++failures;
        }
    }
    if (overlapping < pairs / 10 || pairs - overlapping < pairs / 10) { fprintf(stderr, "the grid is lopsided: %lu of %lu pairs overlap\n", overlapping, pairs); ++failures; }
    if (touching < 100 || interleaved < 30) { fprintf(stderr, "too few touching (%lu) or interleaved (%lu) disjoint pairs\n", touching, interleaved); ++failures; }

    // the cases of tests/test_gpu_gemv_mixed.py::test_aliasing: out = 64 floats at byte 0, the matrix (64 x 256, 16-bit) from 16-bit element 128 on
    int exact = -1, r;
    const wg_view_shape out = { { 64, 1, 1 }, 64, 64, 0 };
    wg_view_shape m = { { 64, 256, 1 }, 64, 64 * 256, 128 };
    r = wg_views_overlap_f32_u16(out, 4096, m, 4096, &exact);
    expect(r, exact, 0, 1, "out ends exactly where m begins");
    m.offset = 127;
    r = wg_views_overlap_f32_u16(out, 4096, m, 4096, &exact);
    expect(r, exact, 1, 1, "m one 16-bit element earlier");
    m.offset = 0;
    r = wg_views_overlap_f32_u16(out, 4096, m, 4096 + 255, &exact);
    expect(r, exact, 1, 1, "one byte of overlap");
    r = wg_views_overlap_f32_u16(out, 4096, m, 4096 + 256, &exact);
    expect(r, exact, 0, 1, "one byte further");
    // out in the leading-dimension padding of m: m 8 x 16 with ld 24, out 8 x 3 floats at f32 offset 4, 12 floats apart
    const wg_view_shape m2 = { { 8, 16, 1 }, 24, 0, 0 };
    wg_view_shape o2 = { { 8, 3, 1 }, 12, 0, 4 };
    r = wg_views_overlap_f32_u16(o2, 4096, m2, 4096, &exact);
    expect(r, exact, 0, 1, "out interleaved between the columns of m");
    o2.offset = 3;
    r = wg_views_overlap_f32_u16(o2, 4096, m2, 4096, &exact);
    expect(r, exact, 1, 1, "interleaved out one float earlier");
    // an f32 view whose doubled fields do not fit 32 bits: the intervals decide what they can, the rest is answered conservatively
    const wg_view_shape big = { { 0x80000000u, 1, 1 }, 0x80000000u, 0, 0 }, one = { { 1, 1, 1 }, 1, 1, 0 };
    r = wg_views_overlap_f32_u16(big, 1ull << 40, one, (1ull << 40) + 4ull * 0x80000000ull, &exact);
    expect(r, exact, 0, 1, "the element behind a column of 2^31 floats");
    r = wg_views_overlap_f32_u16(big, 1ull << 40, one, (1ull << 40) + 4ull * 0x80000000ull - 1, &exact);
    expect(r, exact, 1, 0, "the last byte of a column of 2^31 floats (conservative)");
    const wg_view_shape wide = { { 4, 2, 1 }, 0xC0000000u, 0, 0 }; // two columns 12 GiB apart: the doubled stride does not fit
    r = wg_views_overlap_f32_u16(wide, 1ull << 40, one, (1ull << 40) + 64, &exact);
    expect(r, exact, 1, 0, "between two far columns (conservative: may overlap)");
    r = wg_views_overlap_f32_u16(wide, 1ull << 40, one, (1ull << 40) - 2, &exact);
    expect(r, exact, 0, 1, "directly in front of a view with a stride past 2^31");
    const wg_view_shape empty = { { 0, 5, 1 }, 8, 40, 0 };
    r = wg_views_overlap_f32_u16(empty, 4096, m2, 4096, &exact);
    expect(r, exact, 0, 1, "an empty f32 view");
    r = wg_views_overlap_f32_u16(big, 4096, empty, 4096, &exact);
    expect(r, exact, 0, 1, "an empty 16-bit view");

    printf("%lu pairs (%lu overlapping; %lu touching and %lu interleaved among the disjoint ones), %d failures\n", pairs, overlapping, touching, interleaved, failures);
    if (!failures) puts("OVERLAP MIXED OK");
    return failures ? 1 : 0;
}
