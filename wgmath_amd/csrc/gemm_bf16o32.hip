// wg_gemm_out32 (bf16 operands, f32 result): the 256 x 256 kernel, the tail reduce and the launcher, compiled with the output-element switch of gemm_f16_common.hpp
#define WG_GEMM16_BF16
#define WG_GEMM16_OUT32
#include "gemm_f16.hip"
