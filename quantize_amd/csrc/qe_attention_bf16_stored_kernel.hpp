// qe_attention_bf16_stored_kernel.hpp -- the types and small device functions of the bf16 attention kernel on bf16 rows,
// for its two kernels: attn_bf16_stored_kernel (qe_attention_bf16_stored.hip: fp32 context) and attn_bf16_ctx_kernel
// (qe_attention_bf16_ctx.hip: bf16 context, for a consumer that reads bf16 rows -- qe_quantlinear_bf16_input).  The kernels'
// statements are qe_attention_bf16_stored_body.hpp; how the operands reach their fragments is described at the top of
// qe_attention_bf16_stored.hip.
#pragma once
#include "qe_attention_common.hpp"

namespace qe {

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));

// eight fp32 -> one MFMA fragment, round to nearest even (v_cvt_pk_bf16_f32)
__device__ __forceinline__ bf16x8 pack8(float x0, float x1, float x2, float x3, float x4, float x5, float x6, float x7)
{
    bf16x8 f;
    f[0] = (__bf16)x0; f[1] = (__bf16)x1; f[2] = (__bf16)x2; f[3] = (__bf16)x3;
    f[4] = (__bf16)x4; f[5] = (__bf16)x5; f[6] = (__bf16)x6; f[7] = (__bf16)x7;
    return f;
}

// the two bf16 of a fragment register as fp32 (exact: a bf16 is the upper half of an fp32)
__device__ __forceinline__ float bf_lo(uint32_t w) { return __builtin_bit_cast(float, w << 16); }
__device__ __forceinline__ float bf_hi(uint32_t w) { return __builtin_bit_cast(float, w & 0xffff0000u); }

}  // namespace

}  // namespace qe
