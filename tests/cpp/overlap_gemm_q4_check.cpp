// wg_gemm_q4's aliasing rule on the host: an f32 `out` against the packed matrix (bytes of two 4-bit weights) in 1-byte units, against the f32 scales, and against the 16-bit columns in 2-byte units
// (wgmath_amd/csrc/views_overlap.hpp), on the layout of tests/test_gpu_gemm_q4.py::test_aliasing -- out | m | scales | x touching in ONE buffer -- and on every shift of
// `out` by whole floats across it, each compared with a brute-force intersection of the two byte sets. Host code only: built with the host sanitizers and run by
// tests/test_cpp_overlap_gemm_q4.py on the CPU, never on a GPU.
#include <cstdint>
#include <cstdio>
#include <set>

#include "views_overlap.hpp"

static int failures = 0;

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
static int brute(const wg_view_shape &f, const wg_view_shape &h, uint64_t base, uint32_t es) {
    const std::set<uint64_t> a = bytes_of(f, base, 4), b = bytes_of(h, base, es);
    for (uint64_t p : a)
        if (b.count(p)) return 1;
    return 0;
}
static int predicate(const wg_view_shape &f, const wg_view_shape &h, uint64_t base, uint32_t es, int *exact) {
    if (es == 1) return wg_views_overlap_f32_u8(f, base, h, base, exact);
    if (es == 2) return wg_views_overlap_f32_u16(f, base, h, base, exact);
    return wg_views_overlap(f, base, h, base, 4, exact);
}
static void expect(const char *what, const wg_view_shape &f, const wg_view_shape &h, uint32_t es, int want) {
    int exact = -1;
    const uint64_t base = 1ull << 32;
    const int got = predicate(f, h, base, es, &exact), truth = brute(f, h, base, es);
    if (got != want || truth != want || exact != 1) {
        fprintf(stderr, "%s: got %d (exact %d), the byte sets say %d, expected %d\n", what, got, exact, truth, want);
        ++failures;
    }
}

int main() {
    // k = 128 logical rows, outputs = 16, N = 4, G = 64, one buffer: out 16 x 4 floats at byte 0 (256 bytes), then 256 bytes nobody reads, m 64 BYTES x 16 from byte 512,
    // scales 2 x 16 floats from byte 1536 (float 384), x 128 x 4 two-byte elements from byte 1664 (element 832)
    const uint32_t K = 128, B = K / 2, O = 16, N = 4;
    wg_view_shape out = { { O, N, 1 }, O, O * N, 64 };
    const wg_view_shape m = { { B, O, 1 }, B, B * O, 512 }, s = { { 2, O, 1 }, 2, 2 * O, 384 }, x = { { K, N, 1 }, K, K * N, 832 };
    expect("out ends where m begins", out, m, 1, 0);
    expect("out against scales", out, s, 4, 0);
    expect("out against x", out, x, 2, 0);
    wg_view_shape m1 = m;
    m1.offset = 511;
    expect("m one byte earlier", out, m1, 1, 1);
    out.offset = 384 - O * N + 1; // the last float of out is the first scale
    expect("the last float of out is the first scale", out, s, 4, 1);
    expect("... and that out lies inside m", out, m, 1, 1);
    out.offset = 384 + 2 * O; // out begins where the scales end: on x's first two elements
    expect("out on the first elements of x", out, x, 2, 1);
    expect("... touching the scales", out, s, 4, 0);
    out.offset = (1664 + 2 * K * N) / 4; // behind x
    expect("out behind x", out, x, 2, 0);
    out.offset -= 1;
    expect("out on the last two elements of x", out, x, 2, 1);
    // out with a padded leading dimension in the gaps of a padded x: x 8 x 4 elements with leading dimension 24 (16 bytes of data, 32 of padding per column), out 4 x 4
    // floats with leading dimension 12 at float offset 4 + 12 j: bytes 16 .. 31 of every 48
    const wg_view_shape xp = { { 8, 4, 1 }, 24, 0, 0 };
    wg_view_shape op = { { 4, 4, 1 }, 12, 0, 4 };
    expect("out interleaved between the columns of x", op, xp, 2, 0);
    op.offset = 3;
    expect("interleaved out one float earlier", op, xp, 2, 1);
    // every shift of a small out across the whole layout, against each read operand
    unsigned long pairs = 0, overlapping = 0;
    for (uint32_t off = 0; off < 700; ++off) {
        const wg_view_shape o = { { 3, 2, 1 }, 5, 10, off };
        const struct { const wg_view_shape *v; uint32_t es; } reads[] = { { &m, 1 }, { &s, 4 }, { &x, 2 } };
        for (const auto &r : reads) {
            int exact = -1;
            const int got = predicate(o, *r.v, 4096, r.es, &exact), truth = brute(o, *r.v, 4096, r.es);
            ++pairs;
            overlapping += truth;
            if (got != truth || exact != 1) {
                fprintf(stderr, "out at float %u against %u-byte elements: got %d (exact %d), the byte sets say %d\n", off, r.es, got, exact, truth);
                ++failures;
            }
        }
    }
    if (overlapping < pairs / 10 || pairs - overlapping < pairs / 10) { fprintf(stderr, "the shifts are lopsided: %lu of %lu overlap\n", overlapping, pairs); ++failures; }
    printf("%lu pairs (%lu overlapping), %d failures\n", pairs, overlapping, failures);
    if (!failures) puts("OVERLAP GEMM Q4 OK");
    return failures ? 1 : 0;
}
