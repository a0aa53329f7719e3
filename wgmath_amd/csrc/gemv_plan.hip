// The planner of the Gemv launchers: which kernel a call takes, with what right-hand-side tile, cut of the contraction, grids and workspace (gemv_plan.hpp).
// Host arithmetic on sizes, strides, addresses modulo 16, the CU count and one tuning value. No kernel, no device call, no context -- the launchers (gemv.hip,
// gemv_any.hip) execute the plan, tests read it through wg_debug_gemv_plan / wg_debug_gemv_any_plan and tests/cpp/gemv_plan_check.cpp links this unit with
// gemm32_plan.hip alone (under the host sanitizers). The kernels the comments below speak of are gemv.hip's.
#include "gemv_plan.hpp"
#include "gemm32_plan.hpp"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>

int wg_set_error(int status, const char *fmt, ...) __attribute__((format(printf, 2, 3))); // (runtime.hip)

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr uint32_t kMaxRhs = (uint32_t)kGemvMaxRhs;

inline uint32_t ceil_div(uint32_t a, uint32_t b) { return a / b + (a % b != 0); }

wg_gemv_plan no_launch(wg_gemv_plan p, int status, const char *fmt, ...) {
    p.leaf = WG_GEMV_UNSUPPORTED;
    p.status = status;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(p.message, sizeof p.message, fmt, ap);
    va_end(ap);
    return p;
}

#ifndef GEMV_SMALL
#define GEMV_SMALL 1
#endif
// gemv_n_small_kernel, rows per workgroup = 4 RL: as few as gives the chip >= 128 workgroups
int gemv_small_rl(uint32_t rows_out) {
    static const int forced = [] { const char *e = getenv("WG_GEMV_SMALL_RL"); return e ? atoi(e) : 0; }(); // experiments: 2 / 4 / 8 lanes x float4 of rows per workgroup
    if (forced == 2 || forced == 4 || forced == 8) return forced;
    return rows_out >= 4096u ? 8 : (rows_out >= 2048u ? 4 : 2);
}

// blocks along the output, and how finely the contraction must be split to give every CU ~4 workgroups
#ifndef WG_GEMVT_COLS
#define WG_GEMVT_COLS 1 // 0: T with one right-hand side on the 4-columns-per-wave kernel as well (the form before round 3)
#endif
// T with ONE right-hand side runs on gemv_t_cols_kernel (a half-wave per column): measured over 17 shapes x 2 element types against the
// 4-columns-per-wave kernel (tools/gemvtr_sweep.py, profiles/r03_evidence.md section 10): f32 -1...-40 % time (4096^2 16.5 -> 10 us, 65536 x 4096
// 169 -> 162), f16 -5...-45 % (65536 x 4096 95 -> 83 us = 6.5 TB/s) -- except f32 columns exactly 64 KiB apart with k <= 16384 (16384 x 2048 ...
// x 16384: +5...+13 %; 15360 and 17408 rows are fine, f16 and longer columns at that stride are fine), which stay on the old kernel.
// gemv_t_cols_kernel with 4 instead of 8 loads in flight per lane (half the registers, twice the half-waves per CU): columns of at most 8 chunks (a chunk: 32 lanes x 16 bytes),
// and up to 31 chunks when the 8-deep form would end in a partial trip. Measured (tools/gemvtr_sweep.py, f16, us): 1024 x 65536 55 -> 20 (vendor 22), 1280 x 32768 25.4 -> 13.8,
// 3072 x 65536 74.2 -> 57.0; whole trips of 8 stay (4096 x 65536 f16 75.0 against 79.0, 2048 x 65536 f32 76.5 against 79.5).
bool t_cols_u4(uint32_t k_per_split, uint32_t e) {
    const uint32_t chunks = k_per_split / (32u * e);
    return chunks <= 8u || (chunks < 32u && chunks % 8u != 0);
}
// GemvTr with TWO right-hand sides on the half-wave-per-column kernel's 2-vector form (gemv_t_cols_kernel<.., 4, 2>, round 5): every piece of the matrix meets the same rows
// of both vectors, no LDS, no barrier. Measured against what took these shapes before (tools/misc_sweep.py with MISC_GEMV_SHAPES, us, before -> after | vendor) -- f16 (the
// 4-columns-per-wave kernel): 4096^2 14.0 -> 7.7 | 18, 4096 x 11008 24.0 -> 18.5 | 18.5, 11008 x 4096 23.4 -> 18.1 | 19, 8192^2 36.3 -> 25.0 | 22-27, 65536 x 4096 111 -> 88 | 108,
// 16384^2 104 -> 91 | 98, but few outputs lose (32768 x 1536 28.8 -> 38.7): from 2048 outputs on. f32 (the vectors-in-LDS kernel): only where that kernel's one barrier per chunk
// shows -- 4096 x 11008 41.8 -> 33.3 | 30, 4096^2 12.8 -> 12.0 -- and worse elsewhere (16384^2 163 -> 188, 11008 x 4096 32.3 -> 34.7): contractions of 2049 .. 8192 rows onto
// 4096 .. 16384 outputs.
#ifndef WG_GEMVT_COLS2
#define WG_GEMVT_COLS2 1
#endif
bool uses_t_cols2(const wg_gemv_query &q) {
    if (!WG_GEMVT_COLS2 || !q.trans || q.nrhs != 2u) return false;
    if (q.m_elem == 2u) return q.rows_out >= 2048u;
    return q.k > 2048u && q.k <= 8192u && q.rows_out >= 4096u && q.rows_out <= 16384u;
}
bool uses_t_cols(const wg_gemv_query &q) {
    if (!WG_GEMVT_COLS || !q.trans || q.nrhs != 1) return false;
    if (q.m_elem == 4u && q.ldm % 16384u == 0 && q.k <= 16384u) return false;
    return true;
}
// cols: the call runs on gemv_t_cols_kernel; gx: its blocks along the output; gz: matrices x groups of right-hand sides
uint32_t plan_nsplit(const wg_gemv_query &q, bool cols, uint32_t gx, uint32_t gz) {
    const bool trans = q.trans != 0;
    const uint32_t rows_out = q.rows_out, k = q.k, nrhs = q.nrhs;
    const int cus = (int)q.cus;
    const uint32_t min_k_per_split = trans ? 2048u : 64u; // T: >= 8 row-steps per lane; N: >= 16 columns per wave
    const uint64_t blocks_xy = (uint64_t)gx * gz;
    const uint32_t max_split = k == 0 ? 1u : ceil_div(k, min_k_per_split);
    // ~4 workgroups per CU (measured at 1 / 2 / 4 per CU: GemvTr 65536 x 4096 5.4 / 6.0 / 6.4 TB/s; Gemv 4096 x 11008 43 / - / 33 us),
    // except a tall matrix with a short contraction whose row blocks alone give every CU a workgroup: splitting 65536 x 256 four ways
    // costs 18 us with the combine pass against 10 us unsplit.
    // N: matrices of 256 MiB and more stream best with 2 workgroups per CU and four times the columns per workgroup (4096 x 32768 f32: 103 -> 83 us,
    // 16384^2: 167 -> 158, 4096 x 65536: 165.9 -> 162.5; f16 alike), smaller ones with 4 (tools/gemvtr_sweep.py with SWEEP_N=1, r03 evidence section 10)
    // (round 5: tall matrices from 128 MiB on as well -- 32768 x 1536 f32 39.3 -> 35.9 us, 16384 x 2048 30.4 -> 27.4; not the squarer ones: 8192 x 4096 23.1 -> 27.4, 11008 x 4096 31.2 -> 33.4)
    const uint64_t n_bytes = (uint64_t)rows_out * k * q.m_elem;
    const bool big_n = !trans && (n_bytes >= (256ull << 20) || (q.m_elem == 4u && n_bytes >= (128ull << 20) && rows_out >= 16384u));
    const uint32_t per_cu = cols ? 2u : trans ? 4u : big_n ? 2u : 4u; // (the half-wave-per-column kernel: 2 / 4 / 8 per CU measured the same within 2 %; fewer splits, smaller combine)
    uint32_t want = blocks_xy >= (uint64_t)cus * per_cu ? 1u : ceil_div((uint32_t)cus * per_cu, (uint32_t)blocks_xy);
    if (!trans && blocks_xy >= (uint64_t)cus && k <= 1024u) want = 1u;
    if (trans && !cols && blocks_xy >= 2ull * (uint64_t)cus) want = 1u; // T with >= 2 workgroups per CU already: 8192 x 8192 47 us unsplit, 57 split in two + combine
    uint32_t nsplit = want > max_split ? max_split : want;
    if (nsplit < 1u) nsplit = 1u;
    if (nsplit > 65535u) nsplit = 65535u;
    if (nrhs > 65535u) nsplit = 1u; // the combine pass puts the right-hand sides on grid.y; that many columns fill the chip unsplit
    return nsplit;
}
// launch-bound Gemvs run as ONE kernel without partials (gemv_n_small_kernel); the fused Gemv+Reduce takes exactly the calls whose plan is this leaf
bool uses_small_kernel(const wg_gemv_query &q, uint32_t nsplit) {
    return GEMV_SMALL && !q.trans && nsplit > 1 && (uint64_t)q.rows_out * q.k <= (4ull << 20) && q.rows_out >= 128u && q.nrhs <= 65535u;
}

// The Gemv kernels proper: small, n, t, tcols, each of the last three with or without the combine pass. The plan is made with the MATRIX's element size, so a mixed call
// has the plan of the 16-bit call of the same shape, views and context.
wg_gemv_plan own_kernels(wg_gemv_plan p, const wg_gemv_query &q) {
    const bool trans = q.trans != 0;
    const uint32_t rows_out = q.rows_out, k = q.k, nrhs = q.nrhs, nmats = q.nmats;
    p.rhs_groups = ceil_div(nrhs, kMaxRhs);
    const uint64_t gz64 = (uint64_t)nmats * p.rhs_groups;
    if (gz64 > 65535) return no_launch(p, WG_ERR_UNSUPPORTED, "Gemv: nmats * ceil(nrhs/8) = %llu exceeds 65535", (unsigned long long)gz64);
    const uint32_t gz = (uint32_t)gz64;

    const bool t_cols = uses_t_cols(q) || uses_t_cols2(q);
    const uint32_t gx = t_cols ? ceil_div(rows_out, 8u) : trans ? ceil_div(rows_out, 4u * kWaves) : ceil_div(rows_out, 256u);
    uint32_t nsplit = plan_nsplit(q, t_cols, gx, gz);
    const uint32_t k_per_split = k == 0 ? 4u : ceil_div(ceil_div(k, nsplit), 4u) * 4u; // vec4 granularity
    nsplit = k == 0 ? 1u : ceil_div(k, k_per_split);
    p.block = kThreads;

    // launch-bound sizes: one kernel without partials beats split + combine (1024 x 1024: 12.6 -> ~9 us per eager dispatch); it needs no workspace
    // (so that a recording on a fresh context does not ask for one)
    if (uses_small_kernel(q, nsplit)) {
        p.leaf = WG_GEMV_SMALL;
        p.rl = (uint32_t)gemv_small_rl(rows_out);
        p.grid[0] = ceil_div(rows_out, 4u * p.rl); p.grid[1] = nrhs; p.grid[2] = nmats;
        return p; // (nsplit 1, k_per_split k: every workgroup sweeps all columns)
    }
    p.nsplit = nsplit; p.k_per_split = k_per_split;
    p.grid[0] = gx; p.grid[1] = nsplit; p.grid[2] = gz;
    if (nsplit > 1) { // f32 partial sums whatever the element type
        p.workspace_bytes = (uint64_t)nmats * nsplit * nrhs * rows_out * sizeof(float);
        p.combine_grid[0] = ceil_div(rows_out / 4u, 4u); p.combine_grid[1] = nrhs; p.combine_grid[2] = nmats;
    }
    // kMaxRhs RHS columns per group (grid.z); the kernel template is the per-pass register tile: the smallest of 1, 2, 4, 8 that
    // holds min(nrhs, 8) columns (a group of 3 uses tile 4, of 5..7 tile 8)
    const uint32_t per_group = nrhs < kMaxRhs ? nrhs : kMaxRhs;
    p.rhs_tile = per_group > 4 ? 8 : (per_group > 2 ? 4 : per_group);
    if (!t_cols) {
        p.leaf = trans ? WG_GEMV_T : WG_GEMV_N;
        return p;
    }
    p.leaf = WG_GEMV_TCOLS;
    // f16: 16-byte loads (8 rows per lane) where every column, split and batch keeps them aligned; 8-byte loads (the view contract) otherwise
    // (v16: elements of the vectors' type per 16 bytes -- f32 vectors beside a 16-bit matrix are read as two 16-byte loads per 8 rows)
    bool wide = false;
    const uint32_t v16 = 16u / q.v_elem;
    if (q.m_elem == 2u)
        wide = q.m_addr16 % 16 == 0 && q.v_addr16 % 16 == 0 && q.ldm % 8 == 0 && k_per_split % 8 == 0 && (nmats == 1 || (q.m_batch % 8 == 0 && q.v_batch % v16 == 0)) &&
               (nrhs == 1 || q.ldv % v16 == 0);
    // the instance: elements per load, loads in flight, right-hand sides (the 2-vector form has 4 in flight only)
    p.e = wide ? 8 : 4;
    p.u = nrhs == 2 || t_cols_u4(k_per_split, p.e) ? 4 : WG_GEMVT_U;
    p.v = nrhs;
    return p;
}

// 3 .. 8 right-hand sides on a matrix that is not launch-bound: the GEMV kernels re-read the vectors once per matrix piece (GemvTr) or give every
// right-hand side its own accumulators (f16 Gemv), and fall well behind one pass on the matrix cores -- measured against both and against the
// vendor's skinny GEMMs (tools/misc_sweep.py, profiles/r03_evidence.md section 12): f16 GemvTr 65536 x 4096 x 8 373 -> 135 us, f32 GemvTr 4096^2 x 8
// 33 -> 18 us, f16 Gemv 65536 x 4096 x 8 138 -> 123 us. Kept on the GEMV kernels: 2 right-hand sides, matrices under 48 MiB (one launch instead
// of several), f32 Gemv (the N kernel streams 8 right-hand sides at 6.2 TB/s), and f32 GemvTr with >= 8 outputs per contracted row (212 vs 279 us).
bool few_rhs_as_gemm(const wg_gemv_query &q) {
    const bool f16 = q.m_elem == 2u;
    const uint32_t rows_out = q.rows_out, k = q.k, nrhs = q.nrhs;
    const uint64_t bytes = (uint64_t)rows_out * k * q.m_elem;
    if (nrhs < 3u || bytes < ((nrhs >= 7u ? 16ull : 48ull) << 20)) return false; // (7-8 right-hand sides pay from 16 MiB: 4096^2 f16 x 8 26 -> 19 us)
    if (q.trans) return f16 || (uint64_t)rows_out < 8ull * k;
    // f32 Gemv: since the few-column Gemm kernel multiplies N <= 16 on 16-wide MFMAs (round 5) it is ahead of the 8-accumulator N kernel on everything but a few
    // rows with a long contraction (11008 x 4096 x 4: 36.4 -> 33.2 us, 65536 x 4096 x 8: 187 -> 176, 8192^2 x 3: 47.7 -> 42.9; 4096 x 65536 x 8: 173 stays, Gemm 180)
    // (With the non-temporal hint on its streamed pieces -- gemm_f32_skinny.hip tr_dma_streamed, round 5 -- the Gemm form of 4096 x 65536 x 8 takes 160 us in a replayed
    // command buffer and 175 +- 14 us, at 1.79 GHz, as eager dispatches in bench.py, against the N kernel's steady 173 at 2.39 GHz: it stays on the N kernel.)
    return f16 || (uint64_t)k < 8ull * rows_out;
}

#ifndef WG_GEMVT_LDS
#define WG_GEMVT_LDS 1
#endif
// GemvTr with 2 .. 8 right-hand sides on gemv_t_lds_kernel: shape of the workgroups, chunk of k in the LDS, grid.
wg_gemv_plan t_lds(wg_gemv_plan p, const wg_gemv_query &q) {
    const uint32_t cus = q.cus, rows_out = q.rows_out, k = q.k;
    const uint32_t tile = q.nrhs > 4u ? 8u : (q.nrhs > 2u ? 4u : 2u);
    p.leaf = WG_GEMV_TLDS;
    p.rhs_tile = tile;
    // the vectors whole when k x tile floats fit 128 KiB (then they are staged once per workgroup), else chunks of 64 KiB (two workgroups per CU)
    const uint32_t whole = (128u << 10) / (tile * 4u), chunk = (64u << 10) / (tile * 4u);
    p.lds_kc = k <= whole ? k : chunk;
    const size_t lds = (size_t)p.lds_kc * tile * sizeof(float);
    p.lds_bytes = (uint32_t)lds;
    static const int shapes[5][2] = { { 4, 1024 }, { 2, 1024 }, { 1, 1024 }, { 1, 512 }, { 1, 256 } }; // 128, 64, 32, 16, 8 columns per trip
    double best = 1e30;
    p.lds_cols = 1; p.lds_threads = 256;
    uint32_t best_grid = 1;
    for (const auto &sh : shapes) {
        const uint32_t per_wg = (uint32_t)sh[0] * (uint32_t)sh[1] / 32u;
        const uint32_t groups = ceil_div(rows_out, per_wg);
        uint32_t per_cu = (uint32_t)((160u << 10) / (lds ? lds : 1));
        if (per_cu > 2048u / (uint32_t)sh[1]) per_cu = 2048u / (uint32_t)sh[1];
        if (per_cu < 1u) per_cu = 1u;
        const uint32_t slots = cus * per_cu, grid = groups < slots ? groups : slots;
        const uint32_t trips = ceil_div(groups, grid);
        // relative time: work per workgroup slot in column-trips, against an even share; a grid that leaves CUs without a workgroup pays for them;
        // narrower shapes pay a little for re-reading the vectors from the LDS per column (COLS = 1) and for staging them per workgroup
        double f = (double)trips * grid / (double)groups;
        if (groups < cus) f *= (double)cus / groups;
        // (staging: tile floats of the vectors per contracted row against per_wg floats of the matrix, from the L2; once per workgroup when k is one chunk)
        f *= 1.0 + 0.02 * (4 - sh[0]) + 0.5 * (double)tile / per_wg * (k > p.lds_kc ? 1.0 : 1.0 / trips);
        if (f < best) { best = f; p.lds_cols = (uint32_t)sh[0]; p.lds_threads = (uint32_t)sh[1]; best_grid = grid; }
    }
    p.grid[0] = best_grid; p.grid[1] = 1; p.grid[2] = q.nmats;
    p.block = p.lds_threads;
    return p;
}
// Where it runs (f32 only: f16 gains nothing over the f16 Gemm kernels, 120 vs 111 us at 4096 x 65536 x 8), measured with tools/misc_sweep.py
// (profiles/r05_evidence.md section 5):
//   * from 128 outputs per CU on, the vectors whole in the LDS: 4096 x 65536 x 8 178 us against 212 on the
//     4-columns-per-wave kernel and 279 on the few-column Gemm kernel (vendor 178);
//   * TWO right-hand sides from 8 outputs per CU on (the narrow workgroup shapes of round 5): 4096^2 x 2 18.2 -> 12.8 us (vendor 18.9);
//   * NOT 3 .. 8 right-hand sides on fewer outputs: every workgroup shape loses to the matrix-core path there (4096 x 11008 x 4: 55 us on 344 workgroups
//     of 32 columns, 86 with twice the loads in flight, against 40 on the few-column Gemm kernel; 4096^2 x 8 26.5 against 18.1) -- a column is 16 KiB,
//     each half-wave's whole life is a few dependent round trips behind the staging of the vectors.
bool uses_t_lds(const wg_gemv_query &q) {
    const uint32_t rows_out = q.rows_out, k = q.k, nrhs = q.nrhs;
    if (!WG_GEMVT_LDS || !q.trans || q.m_elem != 4u || nrhs < 2u || nrhs > 8u || q.nmats > 65535u) return false;
    if (!q.gemvt_lds && uses_t_cols2(q)) return false; // (two right-hand sides on the column kernel's 2-vector form)
    const uint32_t forced = (uint32_t)q.gemvt_lds, min_cols = forced ? forced : 128u; // (forced: tests, experiments -- wg_ctx_set_tuning)
    const uint32_t cus = q.cus;
    const uint32_t tile = nrhs > 4u ? 8u : (nrhs > 2u ? 4u : 2u);
    if (rows_out % 4u || k % 4u || k < 128u) return false;
    const bool whole = (uint64_t)k * tile * 4u <= (128u << 10);                       // one chunk: staged once per workgroup
    const bool chunks_ok = whole || (uint64_t)k * tile * 4u <= 4ull * (64u << 10);     // at most 4 chunks (two barriers per chunk and trip)
    if ((uint64_t)rows_out >= (uint64_t)min_cols * cus) return forced ? chunks_ok : whole;
    return nrhs == 2u && whole && (uint64_t)rows_out >= 8ull * cus;
}

#ifndef WG_ANY_PER_CU
#define WG_ANY_PER_CU 0 // workgroups per CU the splits of gemv_any aim at; 0: 2, and 4 for N on matrices of 1 GiB and more (cliff sweep A/B, profiles/r06_gemv_any_ab.txt)
#endif

void join(std::string &log, const char *tag) { // as wg_path joins them
    if (!log.empty() && log.back() != '>') log += ' ';
    log += tag;
}

} // namespace

// (Round 5 also carried the half-wave-per-column shape of gemv_t_cols_kernel over to 2 .. 8 right-hand sides -- four adjacent columns per half-wave, the
// vectors re-read through the L1 -- and measured it slower than every path above on all eight sweep cases (4096^2 x 4: 35.8 us against 18.3 on the few-column
// Gemm kernel; 4096 x 11008 x 4: 47 against 39): the re-reads cost the L1 as much as the matrix itself. Removed; profiles/r05_evidence.md section 5.)
wg_gemv_plan gemv_plan(const wg_gemv_query &q) {
    wg_gemv_plan p = {};
    p.nsplit = 1; p.k_per_split = q.k; p.rhs_tile = 1; p.rhs_groups = 1; p.block = kThreads;
    if (q.rows_out == 0 || q.nrhs == 0 || q.nmats == 0) { p.leaf = WG_GEMV_NOTHING; return p; }
    if (uses_t_lds(q)) return t_lds(p, q);
    // 16-bit elements (extensions; the reference kernel is f32, gemv.wgsl:9-14): the same HBM-bound kernels (8-byte loads of 4 rows, f32 accumulation in the same order,
    // one rounding at the store; split partials stay f32). More than 8 right-hand sides are a Gemm with few columns: the 16-bit Gemm kernels take any column count (one
    // pass over the matrix on the matrix cores). Not the mixed call: the Gemm kernels would round v to 16 bits -- more than 8 right-hand sides run as groups of 8 in
    // grid.z, one pass over the matrix per group.
    if (q.m_elem == 2u) {
        if (q.gemm16 && (q.nrhs > kMaxRhs || few_rhs_as_gemm(q))) { p.leaf = WG_GEMV_AS_GEMM16; return p; }
        return own_kernels(p, q);
    }
    // 9 .. 64 right-hand sides are a Gemm with few columns: one pass over the matrix on the matrix cores (gemm_f32_skinny.hip) instead of
    // one GEMV pass per 8 columns. (The 32-bit DMA offsets of that kernel must suffice for both operands, in both variants.)
    if ((q.nrhs > kMaxRhs || few_rhs_as_gemm(q)) && q.nrhs <= 64u && q.rows_out >= 512u && q.k >= 128u && (uint64_t)q.ldm * 32u * 4u < (1ull << 31) &&
        (uint64_t)q.ldv * 64u * 4u < (1ull << 31)) {
        p.gemm32 = gemm32_skinny_plan(q.rows_out, q.nrhs, q.k, q.nmats, q.cus); // its K cut
        if (p.gemm32.leaf == WG_GEMM32_UNSUPPORTED) return no_launch(p, p.gemm32.status, "%s", p.gemm32.message);
        p.leaf = WG_GEMV_AS_GEMM32;
        p.nsplit = p.gemm32.nsplit; p.k_per_split = p.gemm32.k_per_split;
        p.workspace_bytes = p.gemm32.workspace_bytes;
        return p;
    }
    return own_kernels(p, q);
}

// gemv_any.hip's kernels (V != T: wg_gemv_mixed -- splits, workgroups per CU and the non-temporal threshold follow the MATRIX's element size)
wg_gemv_any_plan gemv_any_plan(const wg_gemv_query &q) {
    wg_gemv_any_plan p = {};
    const bool trans = q.trans != 0;
    const uint32_t R = trans ? q.k : q.rows_out, C = trans ? q.rows_out : q.k, nrhs = q.nrhs, nmats = q.nmats; // the matrix view as stored
    if (R == 0 || C == 0 || nrhs == 0 || nmats == 0) return p;
    const uint32_t E = 16u / q.m_elem; // elements per 16-byte load: the rows a lane owns
    const uint64_t gz = (uint64_t)nmats * nrhs;
    if (gz > 0xffffffffull) {
        p.status = WG_ERR_UNSUPPORTED;
        snprintf(p.message, sizeof p.message, "Gemv: matrices x right-hand sides = %llu exceeds 2^32 - 1", (unsigned long long)gz);
        return p;
    }
    p.zchunk = gz < 65535u ? (uint32_t)gz : 65535u; // grid.z (grid.y of the combine pass) per launch: the pairs go in chunks of up to 65535
    // ~per_cu workgroups per CU; a split is whole 64-column chunks (N) / whole 64 E-row steps (T)
    const uint32_t gx = trans ? (C + 4u * kWaves - 1u) / (4u * kWaves) : (R + 64u * E - 1u) / (64u * E);
    const uint32_t unit = trans ? 64u * E : 64u * kWaves, len = trans ? R : C, units = (len + unit - 1u) / unit;
    const uint64_t per_cu = WG_ANY_PER_CU ? WG_ANY_PER_CU : (!trans && (uint64_t)R * C * q.m_elem >= (1ull << 30) ? 4u : 2u);
    uint32_t nsplit = (uint32_t)((per_cu * q.cus + (uint64_t)gx * gz - 1u) / ((uint64_t)gx * gz));
    if (nsplit > units) nsplit = units;
    if (nsplit < 1u) nsplit = 1u;
    p.per_split = ((units + nsplit - 1u) / nsplit) * unit;
    nsplit = (len + p.per_split - 1u) / p.per_split;
    if (nsplit > 65535u) {
        p.status = WG_ERR_UNSUPPORTED;
        snprintf(p.message, sizeof p.message, "Gemv: too many splits");
        return p;
    }
    p.launch = 1;
    p.grid_x = gx;
    p.nsplit = nsplit;
    if (nsplit > 1u) p.workspace_bytes = (uint64_t)p.zchunk * nsplit * q.rows_out * sizeof(float); // (one chunk's partials: the chunks run in stream order)
    // the non-temporal hint for a matrix that cannot stay in the Infinity Cache anyway (gemv_any.hip ld16)
    p.nt = (uint64_t)R * C * q.m_elem >= (512ull << 20);
    p.nchunks = (uint32_t)((gz + p.zchunk - 1u) / p.zchunk);
    if (p.nchunks > 1u) snprintf(p.tag, sizeof p.tag, "gemv_any/%s,ns=%u,chunks=%u", trans ? "t" : "n", nsplit, p.nchunks);
    else snprintf(p.tag, sizeof p.tag, "gemv_any/%s,ns=%u", trans ? "t" : "n", nsplit);
    return p;
}

const char *gemv_elem_tag(const wg_gemv_query &q) {
    if (q.m_elem == 4u) return "f32.gemv";
    if (q.v_elem == 4u) return q.bf16 ? "bf16w.gemv" : "f16w.gemv";
    return q.bf16 ? "bf16.gemv" : "f16.gemv";
}

GemvTags gemv_tags(const wg_gemv_plan &p) {
    GemvTags t = {};
    switch (p.leaf) {
    case WG_GEMV_SMALL: snprintf(t.tag[t.n++], sizeof t.tag[0], "gemv.small/rl=%u", p.rl); break;
    case WG_GEMV_N: snprintf(t.tag[t.n++], sizeof t.tag[0], "gemv.n/t=%u,ns=%u", p.rhs_tile, p.nsplit); break;
    case WG_GEMV_T: snprintf(t.tag[t.n++], sizeof t.tag[0], "gemv.t/t=%u,ns=%u", p.rhs_tile, p.nsplit); break;
    case WG_GEMV_TCOLS: snprintf(t.tag[t.n++], sizeof t.tag[0], "gemv.tcols/e=%u,u=%u,v=%u,ns=%u", p.e, p.u, p.v, p.nsplit); break;
    case WG_GEMV_TLDS: snprintf(t.tag[t.n++], sizeof t.tag[0], "gemv.tlds/nr=%u,c=%u,th=%u", p.rhs_tile, p.lds_cols, p.lds_threads); return t;
    default: return t;
    }
    if (p.nsplit > 1) snprintf(t.tag[t.n++], sizeof t.tag[0], "gemv.combine/ns=%u", p.nsplit);
    return t;
}

// Host-side view of gemv_plan (tests/test_gemv_plan_host.py; no context, no device): the plan of a query and the launch log such a call leaves.
extern "C" int wg_debug_gemv_plan(const wg_gemv_query *query, wg_gemv_plan *plan, char *tags, size_t cap) {
    if (!query || !plan || (cap && !tags)) return wg_set_error(WG_ERR_INVALID_ARG, "wg_debug_gemv_plan: NULL argument");
    *plan = gemv_plan(*query);
    std::string log;
    if (plan->leaf == WG_GEMV_UNSUPPORTED) { // (the launcher has logged its wrapper, and in front of its own kernels the element prefix, when the plan refuses)
        log = "gemv>";
        if (plan->gemm32.leaf != WG_GEMM32_UNSUPPORTED) join(log, gemv_elem_tag(*query));
    } else if (plan->leaf != WG_GEMV_NOTHING) {
        log = "gemv>";
        if (plan->leaf == WG_GEMV_AS_GEMM32) {
            const Gemm32Tags t = gemm32_tags(plan->gemm32);
            for (int i = 0; i < t.n; ++i) join(log, t.tag[i]);
            if (plan->gemm32.nsplit > 1) join(log, ("splitk.reduce/ns=" + std::to_string(plan->gemm32.nsplit)).c_str()); // (logged by wg_splitk_reduce, splitk.hip)
        } else if (plan->leaf != WG_GEMV_AS_GEMM16) {
            if (plan->leaf != WG_GEMV_TLDS) join(log, gemv_elem_tag(*query));
            const GemvTags t = gemv_tags(*plan);
            for (int i = 0; i < t.n; ++i) join(log, t.tag[i]);
        }
    }
    if (cap) snprintf(tags, cap, "%s", log.c_str());
    return WG_OK;
}

extern "C" int wg_debug_gemv_any_plan(const wg_gemv_query *query, wg_gemv_any_plan *plan, char *tags, size_t cap) {
    if (!query || !plan || (cap && !tags)) return wg_set_error(WG_ERR_INVALID_ARG, "wg_debug_gemv_any_plan: NULL argument");
    *plan = gemv_any_plan(*query);
    if (cap) snprintf(tags, cap, "%s", plan->tag);
    return WG_OK;
}
