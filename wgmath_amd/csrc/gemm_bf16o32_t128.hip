// wg_gemm_out32 (bf16 operands, f32 result): the 128 x 128 / 256 x 128 kernel, compiled with the output-element switch of gemm_f16_common.hpp
#define WG_GEMM16_BF16
#define WG_GEMM16_OUT32
#include "gemm_f16_t128.hip"
