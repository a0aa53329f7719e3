// The q4 GemvTr through include/wgebra.hpp: Gemv::dispatch_q4_tr / dispatch_q4_generic on GpuTensor<uint8_t> packed weights, run on a 64-row x 256-column matrix (32
// bytes per column) whose first bytes hold every byte value -- all 16 nibbles in both positions -- with power-of-two group scales in [1/4, 4] (groups of 32 logical
// rows) against integer vectors in [-4, 4]: (max scale / min scale) * sum |q||v| <= 16 * 64 * 8 * 4 < 2^24, so every partial sum in any order and with any placement
// of the scale is exact and the result is fixed by construction.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "wgebra.hpp"

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static void gpu_gemv_q4(const wg::GpuInstance &gpu) {
    using namespace wg;
    auto gemv = Gemv::from_device(gpu.device());
    auto shapes = ViewShapeBuffers::create();
    const uint32_t RB = 32, K = 2 * RB, C = 256, G = 32, NG = K / G;
    std::mt19937 rng(17);
    std::uniform_int_distribution<int> db(0, 255), dv(-4, 4), de(-2, 2);
    std::vector<uint8_t> m(RB * C);
    std::vector<float> s(NG * C), v(K), out0(C);
    for (uint32_t i = 0; i < RB * C; ++i) m[i] = (uint8_t)(i < 256 ? i : (uint32_t)db(rng)); // every byte value at least once
    for (auto &x : s) x = std::ldexp(1.0f, de(rng));
    for (auto &x : v) x = (float)dv(rng);
    uint32_t nan_bits = 0x7FC00000u;
    for (auto &x : out0) std::memcpy(&x, &nan_bits, 4); // the output starts as NaN: it is overwritten, never read
    auto tm = TensorBuilder::matrix(RB, C, BufferUsages::STORAGE).build_init(gpu.device(), m);
    auto ts = TensorBuilder::matrix(NG, C, BufferUsages::STORAGE).build_init(gpu.device(), s);
    auto tv = TensorBuilder::vector(K, BufferUsages::STORAGE).build_init(gpu.device(), v);
    auto staging = TensorBuilder::vector(C, BufferUsages::MAP_READ | BufferUsages::COPY_DST).build<float>(gpu.device());
    for (int generic = 0; generic < 2; ++generic) {
        auto to = TensorBuilder::vector(C, BufferUsages::STORAGE | BufferUsages::COPY_SRC).build_init(gpu.device(), out0);
        auto encoder = gpu.create_command_encoder();
        auto pass = encoder.compute_pass("q4", nullptr);
        if (generic)
            gemv.dispatch_q4_generic(gpu.device(), shapes, pass, to.as_embedded_view(), tm.as_embedded_view(), ts.as_embedded_view(), tv.as_embedded_view(), G,
                                     GemvVariant::GemvTr);
        else
            gemv.dispatch_q4_tr(gpu.device(), shapes, pass, to.as_embedded_view(), tm.as_embedded_view(), ts.as_embedded_view(), tv.as_embedded_view(), G);
        staging.copy_from(encoder, to);
        gpu.queue().submit(encoder.finish());
        auto got = staging.read(gpu.device());
        uint32_t wrong = 0;
        for (uint32_t c = 0; c < C; ++c) {
            double acc = 0; // (multiples of 1/4 below 2^24: exact in a double)
            for (uint32_t r = 0; r < K; ++r) {
                const uint8_t b = m[r / 2 + c * RB];
                const int q = (int)((r & 1) ? b >> 4 : b & 15) - 8; // low nibble: the even row
                acc += (double)s[r / G + c * NG] * (double)q * (double)v[r];
            }
            wrong += !((double)got[c] == acc);
        }
        EXPECT(wrong == 0, "GemvTr%s: %u of %u results are not the exact product", generic ? " (generic)" : "", wrong, C);
    }
}

int main(int argc, char **argv) {
    if (argc > 1 && std::strcmp(argv[1], "--host-only") == 0) { // (built and linked: the two operators are referenced below)
        std::printf("HOST OK\n");
        return 0;
    }
    auto gpu = wg::GpuInstance::create();
    gpu_gemv_q4(gpu);
    std::printf(failures ? "FAILED\n" : "ALL OK\n");
    return failures ? 1 : 0;
}
