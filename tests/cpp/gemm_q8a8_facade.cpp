// The q8a8 Gemm and the device-side quantiser through include/wgebra.hpp: Gemm::dispatch_q8a8_tr / dispatch_q8a8_generic on GpuTensorView<int8_t> weights and columns
// with GpuTensorView<float> scales and result, and QuantizeQ8::dispatch<X> for X = float, _Float16 and wg::bf16 -- instantiated (their addresses are taken) and
// type-checked: the operand types are part of the signatures, so f16 columns, an f16 `out` or int8 scales do not compile. Built with -Wall -Wextra -Werror and linked
// against the library by tests/test_cpp_gemm_q8a8.py.
#include <cstdint>
#include <cstdio>
#include <type_traits>

#include "wgebra.hpp"

using namespace wg;

using TrFn = void (Gemm::*)(const Device &, const ViewShapeBuffers &, ComputePass &, GpuTensorView<float>, GpuTensorView<int8_t>, GpuTensorView<float>, GpuTensorView<int8_t>,
                            GpuTensorView<float>, uint32_t, uint32_t) const;
using GenericFn = void (Gemm::*)(const Device &, const ViewShapeBuffers &, ComputePass &, GpuTensorView<float>, GpuTensorView<int8_t>, GpuTensorView<float>,
                                 GpuTensorView<int8_t>, GpuTensorView<float>, uint32_t, uint32_t, GemmVariant) const;
template <typename X>
using QuantFn = void (QuantizeQ8::*)(const Device &, const ViewShapeBuffers &, ComputePass &, GpuTensorView<int8_t>, GpuTensorView<float>, GpuTensorView<X>, uint32_t) const;

// a call with these argument types is well-formed
template <typename O, typename M, typename S, typename X, typename XS, typename = void>
struct callable : std::false_type {};
template <typename O, typename M, typename S, typename X, typename XS>
struct callable<O, M, S, X, XS,
                std::void_t<decltype(std::declval<const Gemm &>().dispatch_q8a8_tr(std::declval<const Device &>(), std::declval<const ViewShapeBuffers &>(),
                                                                                    std::declval<ComputePass &>(), std::declval<GpuTensorView<O>>(),
                                                                                    std::declval<GpuTensorView<M>>(), std::declval<GpuTensorView<S>>(),
                                                                                    std::declval<GpuTensorView<X>>(), std::declval<GpuTensorView<XS>>(), 32u, 32u))>>
    : std::true_type {};
template <typename Q, typename S, typename X, typename = void>
struct quantizes : std::false_type {};
template <typename Q, typename S, typename X>
struct quantizes<Q, S, X,
                 std::void_t<decltype(std::declval<const QuantizeQ8 &>().dispatch(std::declval<const Device &>(), std::declval<const ViewShapeBuffers &>(),
                                                                                   std::declval<ComputePass &>(), std::declval<GpuTensorView<Q>>(),
                                                                                   std::declval<GpuTensorView<S>>(), std::declval<GpuTensorView<X>>(), 32u))>>
    : std::true_type {};

static_assert(callable<float, int8_t, float, int8_t, float>::value, "int8 on both sides");
static_assert(!callable<float, int8_t, float, bf16, float>::value, "`x` is int8_t by its type (16-bit columns are dispatch_q8*)");
static_assert(!callable<float, uint8_t, float, int8_t, float>::value, "`m` is int8_t by its type");
static_assert(!callable<bf16, int8_t, float, int8_t, float>::value, "`out` is float by its type");
static_assert(!callable<float, int8_t, bf16, int8_t, float>::value, "`scales` is float by its type");
static_assert(!callable<float, int8_t, float, int8_t, int8_t>::value, "`x_scales` is float by its type");
static_assert(quantizes<int8_t, float, float>::value && quantizes<int8_t, float, bf16>::value, "f32 and bf16 sources");
static_assert(!quantizes<uint8_t, float, float>::value && !quantizes<int8_t, bf16, float>::value, "`q` is int8_t and `scales` float by their types");
#if defined(__FLT16_MANT_DIG__) // (a host compiler without _Float16 has no dtype_of<_Float16> either: include/wgebra.hpp)
static_assert(quantizes<int8_t, float, _Float16>::value, "f16 sources");
#endif

int main() {
    TrFn a = &Gemm::dispatch_q8a8_tr;
    GenericFn b = &Gemm::dispatch_q8a8_generic;
    QuantFn<float> c = &QuantizeQ8::dispatch<float>;
    QuantFn<bf16> d = &QuantizeQ8::dispatch<bf16>;
#if defined(__FLT16_MANT_DIG__)
    QuantFn<_Float16> e = &QuantizeQ8::dispatch<_Float16>;
#else
    QuantFn<bf16> e = d;
#endif
    // the library's answers without a context, through the symbols the facade calls
    wg_view_shape s = {};
    const int rc = wg_gemm_q8a8(nullptr, WG_GEMM_TR, 32, 32, nullptr, s, nullptr, s, nullptr, s, nullptr, s, nullptr, s);
    const int rq = wg_quantize_q8(nullptr, WG_F16, 32, nullptr, s, nullptr, s, nullptr, s);
    if (!a || !b || !c || !d || !e || rc != WG_ERR_INVALID_ARG || rq != WG_ERR_INVALID_ARG) {
        std::printf("FAILED: rc = %d, rq = %d\n", rc, rq);
        return 1;
    }
    std::printf("HOST OK\n");
    return 0;
}
