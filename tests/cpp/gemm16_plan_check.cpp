// The 16-bit Gemm planner alone (wgmath_amd/csrc/gemm16_plan.hip, nothing else of the library) under the host sanitizers: the sweep and the rules of
// tests/test_gemm16_plan_host.py over the same grid of sizes. The cost models convert double to uint32_t and subtract unsigned values; an out-of-range
// conversion or a wrapped difference that only shows as a strange plan in Python is an error report here. Host code only: built and run by
// tests/test_cpp_gemm16_plan.py on the CPU, never on a GPU.
#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "wgebra_hip.h"

// the one symbol the planner unit takes from the rest of the library (runtime.hip: records the message of a failing call)
int wg_set_error(int status, const char *, ...) { return status; }

static int failures = 0;
static void fail(const wg_gemm16_query &q, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    fprintf(stderr, "%s %u x %u x %u x %u beta=%g cus=%u: ", q.trans ? "tr" : "nn", q.M, q.K, q.N, q.nmats, q.beta, q.cus);
    vfprintf(stderr, fmt, ap);
    fputc('\n', stderr);
    va_end(ap);
    ++failures;
}
#define CHECK(cond, ...) do { if (!(cond)) fail(q, __VA_ARGS__); } while (0)

static void check(const wg_gemm16_query &q) {
    wg_gemm16_plan p, p2;
    wg_gemm16_query inner, unused;
    char tags[256];
    if (wg_debug_gemm16_plan(&q, "f16", &p, tags, sizeof tags, &inner) != WG_OK) return fail(q, "wg_debug_gemm16_plan failed");
    if (p.leaf == WG_GEMM16_UNSUPPORTED) return;
    CHECK(tags[0] != 0, "no tags");
    const uint64_t K = q.K, krem = q.K % 64u, MiB = 1ull << 20;
    if (p.leaf == WG_GEMM16_PAD) {
        wg_debug_gemm16_plan(&inner, "f16", &p2, nullptr, 0, &unused);
        CHECK(p2.leaf != WG_GEMM16_PAD && p2.leaf != WG_GEMM16_UNSUPPORTED, "the padded call's inner call is leaf %u (%s)", p2.leaf, p2.message);
        CHECK(inner.M % 8 == 0 && inner.K % 8 == 0 && inner.K >= 64 && inner.padded == 1, "inner query %u x %u", inner.M, inner.K);
        return;
    }
    const uint64_t ns = p.nsplit, kps = p.k_per_split;
    CHECK(ns >= 1 && q.nmats * ns <= 65535, "%u matrices x %u splits", q.nmats, p.nsplit);
    CHECK((ns - 1) * kps < K && K <= ns * kps + krem, "%u splits of %u do not cover K", p.nsplit, p.k_per_split);
    if (ns > 1) {
        CHECK(kps % 64 == 0, "%u splits of %u", p.nsplit, p.k_per_split);
        if (p.leaf != WG_GEMM16_SKINNY) { // whole k of every split, the last one included: one stage (128 x 128 tiles), three (256 x 256)
            const uint64_t floor = p.leaf == WG_GEMM16_M16 ? 192 : 64;
            CHECK(kps >= floor && K - krem >= (ns - 1) * kps + floor && K - krem <= ns * kps, "%u splits of %u", p.nsplit, p.k_per_split);
        }
        CHECK(p.workspace_bytes == 4 * ns * q.M * q.N * q.nmats, "workspace %llu", (unsigned long long)p.workspace_bytes);
    }
    CHECK(p.workspace_bytes <= 512 * MiB, "workspace %llu", (unsigned long long)p.workspace_bytes);
    if (p.leaf != WG_GEMM16_M16) return;
    const uint64_t tiles = (uint64_t)p.tiles_m * p.tiles_n;
    CHECK(p.tiles_m == (q.M + 255) / 256 && p.tiles_n == (q.N + 255) / 256 && K - krem >= 192 && p.tail < tiles, "tiles %u x %u, tail %u", p.tiles_m, p.tiles_n, p.tail);
    if (p.tail) {
        const uint64_t ts = p.tail_split, tk = p.tail_kps;
        CHECK(ns == 1 && q.nmats == 1 && 2 * p.tail <= q.cus && (tiles - p.tail) % q.cus == 0, "tail of %u tiles", p.tail);
        CHECK(ts >= 2 && tk % 64 == 0 && tk >= 192 && K - krem >= (ts - 1) * tk + 192 && K - krem <= ts * tk, "tail of %u splits of %u", p.tail_split, p.tail_kps);
        CHECK(p.workspace_bytes == ts * p.tail * 65536 * 4, "tail workspace %llu", (unsigned long long)p.workspace_bytes);
    }
    if (p.cont) CHECK(q.beta == 0.f && krem == 0 && (tiles - p.tail) * q.nmats > q.cus && ns == 1 && p.nwg == q.cus && !p.queues, "continuous walk");
    if (p.queues) CHECK(ns == 1 && q.nmats == 1 && p.nwg % 8 == 0 && p.nwg >= tiles - p.tail, "tile queues with %u workgroups", p.nwg);
}

int main() {
    const uint32_t sizes[] = { 8, 64, 72, 192, 200, 256, 512, 1000, 1024, 1028, 4096, 4352, 8192, 16384 }, mats[] = { 1, 2, 8 }, cus[] = { 8, 256 };
    // forced families too (WG_TUNE_F16_TILE / _CONT / _SCHED / _BALANCE), and a context with one short XCD
    const int knobs[][4] = { { 0, -1, -1, 0 }, { 128, -1, -1, 0 }, { 256, -1, 0, 0 }, { 256128, -1, -1, 0 }, { 256, 1, -1, 0 }, { 256, -1, 1, 0 }, { 256, -1, -1, 1 } };
    unsigned long plans = 0;
    for (uint32_t M : sizes) for (uint32_t N : sizes) for (uint32_t K : sizes) for (uint32_t z : mats) for (uint32_t tr = 0; tr < 2; ++tr)
        for (int beta = 0; beta < 2; ++beta) for (uint32_t c : cus) for (const auto &kn : knobs) {
            wg_gemm16_query q = {};
            q.trans = tr; q.M = M; q.N = N; q.K = K; q.nmats = z;
            q.lda = tr ? K : M; q.ldb = K; q.ldc = M;
            q.a_batch = (uint64_t)M * K; q.b_batch = (uint64_t)K * N; q.c_batch = (uint64_t)M * N;
            q.alpha = 1.f; q.beta = (float)beta; q.cus = c;
            q.tile = kn[0]; q.sched = kn[1]; q.cont = kn[2]; q.balance = kn[3];
            check(q);
            if (kn[0] == 0 && c == 256) { // the same product on views at odd offsets with odd leading dimensions, on 248 CUs with one short XCD
                q.lda += 1 + q.lda % 2; q.ldb += 1 + q.ldb % 2; q.ldc += 3;
                q.a_addr = q.b_addr = q.c_addr = 2; q.cus = 248; q.uneven_xcds = 1;
                check(q);
                ++plans;
            }
            ++plans;
        }
    printf("%lu plans, %d failures\n", plans, failures);
    if (!failures) puts("PLAN OK");
    return failures ? 1 : 0;
}
