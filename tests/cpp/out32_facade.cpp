// The f32-output Gemm through include/wgebra.hpp: Gemm::dispatch_out32 / dispatch_out32_tr / dispatch_out32_generic instantiated for every operand type the facade
// knows (wg::bf16, _Float16 where the host compiler has it, float) and run on a 64 x 256 by 256 x 32 product of integers 7 and 8 with one sign per row of op(m1) and per
// column of m2: every partial sum stays below 2^24, so the result is the exact integer product whatever the order -- around 15000 in magnitude and odd half of the
// time, which neither 16-bit type can hold -- unless `out` passes through 16 bits anywhere. With -DWG_OUT32_OUT_NOT_FLOAT the file must NOT compile: `out` is a view
// of float by its type.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "wgebra.hpp"

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

template <typename W> W elem(int x);
template <> wg::bf16 elem<wg::bf16>(int x) { return wg::bf16::from_float((float)x); }
template <> float elem<float>(int x) { return (float)x; }
#if defined(__FLT16_MANT_DIG__)
template <> _Float16 elem<_Float16>(int x) { return (_Float16)x; }
#endif

template <typename W>
static void gpu_gemm_out32(const wg::GpuInstance &gpu, const char *name) {
    using namespace wg;
    auto gemm = Gemm::from_device(gpu.device());
    auto shapes = ViewShapeBuffers::create();
    const uint32_t M = 64, K = 256, N = 32;
    std::mt19937 rng(11);
    std::uniform_int_distribution<int> mag(0, 3), sg(0, 1);
    std::vector<int> rs(M), cs(N), ai(M * K), bi(K * N); // A[i + k M], B[k + j K]
    for (auto &x : rs) x = sg(rng) ? 1 : -1;
    for (auto &x : cs) x = sg(rng) ? 1 : -1;
    for (uint32_t k = 0; k < K; ++k)
        for (uint32_t i = 0; i < M; ++i) ai[i + k * M] = rs[i] * (mag(rng) ? 8 : 7);
    for (uint32_t j = 0; j < N; ++j)
        for (uint32_t k = 0; k < K; ++k) bi[k + j * K] = cs[j] * (mag(rng) ? 8 : 7);
    std::vector<W> b(K * N);
    for (uint32_t i = 0; i < K * N; ++i) b[i] = elem<W>(bi[i]);
    auto tb = TensorBuilder::matrix(K, N, BufferUsages::STORAGE).build_init(gpu.device(), b);
    for (bool tr : { false, true }) {
        std::vector<W> a(M * K); // stored M x K (Gemm) or K x M (GemmTr), column-major
        for (uint32_t i = 0; i < M; ++i)
            for (uint32_t k = 0; k < K; ++k) a[tr ? k + i * K : i + k * M] = elem<W>(ai[i + k * M]);
        auto ta = TensorBuilder::matrix(tr ? K : M, tr ? M : K, BufferUsages::STORAGE).build_init(gpu.device(), a);
        std::vector<float> out0(M * N);
        uint32_t nan_bits = 0x7FC00000u;
        for (auto &x : out0) std::memcpy(&x, &nan_bits, 4); // the output starts as NaN: beta = 0 overwrites it, never reads it
        auto staging = TensorBuilder::matrix(M, N, BufferUsages::MAP_READ | BufferUsages::COPY_DST).build<float>(gpu.device());
        for (int form = 0; form < 3; ++form) { // the short form, the generic form, the generic form with (alpha, beta) = (-0.375, 0.5) on an old out of 4097
            const float alpha = form == 2 ? -0.375f : 1.f, beta = form == 2 ? 0.5f : 0.f;
            if (form == 2) for (auto &x : out0) x = 4097.f;
            auto to = TensorBuilder::matrix(M, N, BufferUsages::STORAGE | BufferUsages::COPY_SRC).build_init(gpu.device(), out0);
            auto encoder = gpu.create_command_encoder();
            auto pass = encoder.compute_pass("out32", nullptr);
            if (form)
                gemm.dispatch_out32_generic<W>(gpu.device(), shapes, pass, to.as_embedded_view(), ta.as_embedded_view(), tb.as_embedded_view(),
                                               tr ? GemmVariant::GemmTr : GemmVariant::Gemm, alpha, beta);
            else if (tr)
                gemm.dispatch_out32_tr<W>(gpu.device(), shapes, pass, to.as_embedded_view(), ta.as_embedded_view(), tb.as_embedded_view());
            else
                gemm.dispatch_out32<W>(gpu.device(), shapes, pass, to.as_embedded_view(), ta.as_embedded_view(), tb.as_embedded_view());
            staging.copy_from(encoder, to);
            gpu.queue().submit(encoder.finish());
            auto got = staging.read(gpu.device());
            uint32_t wrong = 0, odd_big = 0;
            for (uint32_t j = 0; j < N; ++j)
                for (uint32_t i = 0; i < M; ++i) {
                    long long acc = 0;
                    for (uint32_t k = 0; k < K; ++k) acc += (long long)ai[i + k * M] * bi[k + j * K];
                    const double want = form == 2 ? -0.375 * (double)acc + 0.5 * 4097.0 : (double)acc; // (multiples of 1/8 below 2^14: exact in f32)
                    wrong += !((double)got[i + j * M] == want);
                    odd_big += (acc % 2 != 0) && (acc > 2048 || acc < -2048);
                }
            EXPECT(wrong == 0, "%s %s form %d: %u of %u results are not the exact value", name, tr ? "GemmTr" : "Gemm", form, wrong, M * N);
            EXPECT(4 * odd_big >= M * N, "%s %s: fewer than a quarter of the results are odd integers above 2048 (the case shows nothing)", name, tr ? "GemmTr" : "Gemm");
        }
    }
}

// every template for every operand type, whether or not a GPU is there to run them
template <typename W>
static void instantiate(const wg::Device &d, const wg::ViewShapeBuffers &s, wg::ComputePass &p, wg::GpuTensorView<float> out, wg::GpuTensorView<W> m1, wg::GpuTensorView<W> m2) {
    const wg::Gemm g{};
    g.dispatch_out32<W>(d, s, p, out, m1, m2);
    g.dispatch_out32_tr<W>(d, s, p, out, m1, m2);
    g.dispatch_out32_generic<W>(d, s, p, out, m1, m2, wg::GemmVariant::Gemm);
    g.dispatch_out32_generic<W>(d, s, p, out, m1, m2, wg::GemmVariant::GemmTr, 2.f, -1.f);
}
template void instantiate<wg::bf16>(const wg::Device &, const wg::ViewShapeBuffers &, wg::ComputePass &, wg::GpuTensorView<float>, wg::GpuTensorView<wg::bf16>, wg::GpuTensorView<wg::bf16>);
template void instantiate<float>(const wg::Device &, const wg::ViewShapeBuffers &, wg::ComputePass &, wg::GpuTensorView<float>, wg::GpuTensorView<float>, wg::GpuTensorView<float>);
#if defined(__FLT16_MANT_DIG__)
template void instantiate<_Float16>(const wg::Device &, const wg::ViewShapeBuffers &, wg::ComputePass &, wg::GpuTensorView<float>, wg::GpuTensorView<_Float16>, wg::GpuTensorView<_Float16>);
#endif

#ifdef WG_OUT32_OUT_NOT_FLOAT
// must be refused by the compiler: an `out` of the operands' 16-bit type
void out_not_float(const wg::Device &d, const wg::ViewShapeBuffers &s, wg::ComputePass &p, wg::GpuTensorView<wg::bf16> out, wg::GpuTensorView<wg::bf16> m1, wg::GpuTensorView<wg::bf16> m2) {
    wg::Gemm{}.dispatch_out32<wg::bf16>(d, s, p, out, m1, m2);
}
#endif

int main(int argc, char **argv) {
    static_assert(wg::dtype_of<wg::bf16>::value == WG_BF16 && wg::dtype_of<float>::value == WG_F32, "the operand types of the out32 call");
    if (argc > 1 && std::strcmp(argv[1], "--host-only") == 0) { // (built and linked: the templates are instantiated above for every operand type)
        std::printf("HOST OK\n");
        return 0;
    }
    auto gpu = wg::GpuInstance::create();
    gpu_gemm_out32<wg::bf16>(gpu, "bf16");
#if defined(__FLT16_MANT_DIG__)
    gpu_gemm_out32<_Float16>(gpu, "f16");
#endif
    gpu_gemm_out32<float>(gpu, "f32");
    std::printf(failures ? "FAILED\n" : "ALL OK\n");
    return failures ? 1 : 0;
}
