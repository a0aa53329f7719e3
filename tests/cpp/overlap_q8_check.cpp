// The overlap predicate between an f32 view and a view of 1-byte elements (wg_gemv_q8: an f32 `out` against the int8 matrix, possibly in one buffer): the 1-byte-unit
// scaling of the f32 view (wgmath_amd/csrc/views_overlap.hpp, wg_views_overlap_f32_u8) against a brute-force intersection of the two byte sets, on seeded small
// random pairs -- disjoint, touching, one byte of overlap, shifted by a few, interleaved, identical -- plus f32 views too large for the scaled 32-bit fields. Host code
// only: built with the host sanitizers and run by tests/test_cpp_overlap_q8.py on the CPU, never on a GPU.
#include <cstdint>
#include <cstdio>
#include <set>

#include "views_overlap.hpp"

static int failures = 0;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
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
    const std::set<uint64_t> a = bytes_of(f, bf, 4), b = bytes_of(h, bh, 1);
    for (uint64_t p : a)
        if (b.count(p)) return 1;
    return 0;
}

static wg_view_shape random_view(bool bytes) { // (a view of bytes gets sizes four times as long: footprints of a like length on both sides)
    static const uint32_t sizes[] = { 0, 1, 3, 4, 5, 8 }, offsets[] = { 0, 1, 3, 4, 7 };
    wg_view_shape s;
    const uint32_t rows = sizes[rnd(6)] * (bytes ? 1 + rnd(4) : 1), cols = sizes[rnd(6)];
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
        const wg_view_shape f = random_view(false), h = random_view(true); // f: f32 elements, h: 1-byte elements
        const uint64_t bf = 1ull << 20, ef = extent(f) * 4, eh = extent(h);
        uint64_t bh = bf;
        const uint32_t how = rnd(6);
        switch (how) {
        case 0: bh = bf + ef + 32; break;                            // disjoint, h behind f
        case 1: bh = bf + ef - h.offset; break;                      // touching: h's first byte is the byte behind f's last
        case 2: bh = bf + ef - h.offset - 1; break;                  // ONE byte of overlap
        case 3: bh = bf + 4ull * f.offset - eh; break;               // touching from the front: h ends where f begins
        case 4: bh = bf + rnd((uint32_t)(ef + eh + 1)) - eh; break;  // anywhere from wholly in front to wholly behind, any byte
        default: break;                                              // the same buffer: interleaved where the strides leave room
        }
        int exact = -1;
        const int got = wg_views_overlap_f32_u8(f, bf, h, bh, &exact), want = brute(f, bf, h, bh);
        ++pairs;
        overlapping += want;
        if (!want && ef && eh) {
            const uint64_t lo_f = bf + 4ull * f.offset, hi_f = bf + ef, lo_h = bh + h.offset, hi_h = bh + eh;
            if (hi_f == lo_h || hi_h == lo_f) ++touching;
            else if (lo_f < hi_h && lo_h < hi_f) ++interleaved;
        }
        if (exact != 1 || got != want) {
            fprintf(stderr, "f32 [%u,%u,%u] s=%u sm=%u off=%u @%llu  u8 [%u,%u,%u] s=%u sm=%u off=%u @%llu (case %u): got %d (exact %d), the byte sets say %d\n", f.size[0],
                    f.size[1], f.size[2], f.stride, f.stride_mat, f.offset, (unsigned long long)bf, h.size[0], h.size[1], h.size[2], h.stride, h.stride_mat, h.offset,
                    (unsigned long long)bh, how, got, exact, want);
            ++failures;
        }
    }
    if (overlapping < pairs / 10 || pairs - overlapping < pairs / 10) { fprintf(stderr, "the grid is lopsided: %lu of %lu pairs overlap\n", overlapping, pairs); ++failures; }
    if (touching < 100 || interleaved < 30) { fprintf(stderr, "too few touching (%lu) or interleaved (%lu) disjoint pairs\n", touching, interleaved); ++failures; }

    // the cases of tests/test_gpu_gemv_q8.py::test_aliasing: out = 64 floats at byte 0, the matrix (64 x 256 bytes) from byte 256 on
    int exact = -1, r;
    const wg_view_shape out = { { 64, 1, 1 }, 64, 64, 0 };
    wg_view_shape m = { { 64, 256, 1 }, 64, 64 * 256, 256 };
    r = wg_views_overlap_f32_u8(out, 4096, m, 4096, &exact);
    expect(r, exact, 0, 1, "out ends exactly where m begins");
    m.offset = 255;
    r = wg_views_overlap_f32_u8(out, 4096, m, 4096, &exact);
    expect(r, exact, 1, 1, "m one byte earlier: one byte of overlap");
    m.offset = 0;
    r = wg_views_overlap_f32_u8(out, 4096, m, 4096 + 256, &exact);
    expect(r, exact, 0, 1, "a second handle that begins where out ends");
    // out in the leading-dimension padding of m: m 16 x 16 bytes with ld 48, out 8 x 3 floats at f32 offset 4 (byte 16), 12 floats (48 bytes) apart
    const wg_view_shape m2 = { { 16, 16, 1 }, 48, 0, 0 };
    wg_view_shape o2 = { { 8, 3, 1 }, 12, 0, 4 };
    r = wg_views_overlap_f32_u8(o2, 4096, m2, 4096, &exact);
    expect(r, exact, 0, 1, "out interleaved between the columns of m");
    o2.offset = 3;
    r = wg_views_overlap_f32_u8(o2, 4096, m2, 4096, &exact);
    expect(r, exact, 1, 1, "interleaved out one float earlier");
    o2.offset = 5;
    r = wg_views_overlap_f32_u8(o2, 4096, m2, 4096, &exact);
    expect(r, exact, 1, 1, "interleaved out one float later: its last float is the next column's first four bytes");
    // an f32 view whose scaled fields do not fit 32 bits: the intervals decide what they can, the rest is answered conservatively
    const wg_view_shape big = { { 0x40000000u, 1, 1 }, 0x40000000u, 0, 0 }, one = { { 1, 1, 1 }, 1, 1, 0 };
    r = wg_views_overlap_f32_u8(big, 1ull << 40, one, (1ull << 40) + 4ull * 0x40000000ull, &exact);
    expect(r, exact, 0, 1, "the byte behind a column of 2^30 floats");
    r = wg_views_overlap_f32_u8(big, 1ull << 40, one, (1ull << 40) + 4ull * 0x40000000ull - 1, &exact);
    expect(r, exact, 1, 0, "the last byte of a column of 2^30 floats (conservative)");
    const wg_view_shape nearly = { { 0x3fffffffu, 1, 1 }, 0x3fffffffu, 0, 0 }; // the longest column whose scaled length still fits: decided exactly
    r = wg_views_overlap_f32_u8(nearly, 1ull << 40, one, (1ull << 40) + 4ull * 0x3fffffffull - 1, &exact);
    expect(r, exact, 1, 1, "the last byte of a column of 2^30 - 1 floats (exact)");
    const wg_view_shape wide = { { 4, 2, 1 }, 0x60000000u, 0, 0 }; // two columns 6 GiB apart: the scaled stride does not fit
    r = wg_views_overlap_f32_u8(wide, 1ull << 40, one, (1ull << 40) + 64, &exact);
    expect(r, exact, 1, 0, "between two far columns (conservative: may overlap)");
    r = wg_views_overlap_f32_u8(wide, 1ull << 40, one, (1ull << 40) - 1, &exact);
    expect(r, exact, 0, 1, "directly in front of a view with a stride past 2^30");
    const wg_view_shape empty = { { 0, 5, 1 }, 8, 40, 0 };
    r = wg_views_overlap_f32_u8(empty, 4096, m2, 4096, &exact);
    expect(r, exact, 0, 1, "an empty f32 view");
    r = wg_views_overlap_f32_u8(big, 4096, empty, 4096, &exact);
    expect(r, exact, 0, 1, "an empty 1-byte view");

    printf("%lu pairs (%lu overlapping; %lu touching and %lu interleaved among the disjoint ones), %d failures\n", pairs, overlapping, touching, interleaved, failures);
    if (!failures) puts("OVERLAP Q8 OK");
    return failures ? 1 : 0;
}
