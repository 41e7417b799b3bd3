// qe_attention_bf16_ctx.hip -- qe_attention_bf16_ctx: qe_attention_bf16_stored with a bf16 context.  The kernel is
// attn_bf16_stored_kernel's text (qe_attention_bf16_stored_kernel.hpp, OUT16 = true): the same operands, fragments, softmax
// and accumulation; where that kernel stores four fp32 quotients as one float4, this one rounds the same four quotients to
// bf16 (nearest even, a NaN stays a NaN) and stores them as one 8-byte piece.  out is therefore qe_attention_bf16_stored's
// out rounded elementwise, for every head size, operand mode and layout (tests/test_attention_bf16_ctx_gpu.py).
// A unit of its own: the 112 instances of the fp32-out kernel keep their code object.
// The argument checks are attn_prepare's, with 2-byte input AND output elements.
#include "qe_attention_bf16_stored_kernel.hpp"

namespace qe {

template <int D, int MODE = 0>
__global__ __launch_bounds__(64 * attn_wpb(D)) void attn_bf16_ctx_kernel(const AttnArgs a)
{
    constexpr bool OUT16 = true;
#include "qe_attention_bf16_stored_body.hpp"
}

struct AttnBf16Ctx {
    template <int D, int MODE> static constexpr auto kernel = &attn_bf16_ctx_kernel<D, MODE>;
};

}  // namespace qe

// the operands choose the kernel's instance, not the kernel
extern "C" int qe_attention_bf16_ctx_path(int32_t L, int32_t S, int32_t H, int32_t d, int has_mask, int has_key_bias, int causal)
{
    (void)has_mask; (void)has_key_bias; (void)causal;
    return qe::attn_bf16_path(L, S, H, d);
}

extern "C" int qe_attention_bf16_ctx(const uint16_t *q, const uint16_t *k, const uint16_t *v, uint16_t *out, int32_t N, int32_t L,
                                     int32_t S, int32_t H, int32_t d, int64_t q_rn, int64_t q_rt, int64_t kv_rn, int64_t kv_rt,
                                     int64_t o_rn, int64_t o_rt, float scale, const float *mask, int64_t mask_sn,
                                     int64_t mask_sh, const float *key_bias, int causal, qe_stream_t stream)
{
    using namespace qe;
    AttnArgs a;
    int mode;
    // a head size without a bf16 instance is refused here: never another kernel instead
    if (const int e = attn_prepare(q, k, v, sizeof(uint16_t), out, sizeof(uint16_t), N, L, S, H, d, q_rn, q_rt, kv_rn, kv_rt, o_rn,
                                   o_rt, scale, mask, mask_sn, mask_sh, key_bias, causal, attn_bf16_path(L, S, H, d), a, mode))
        return e;
    attn_dispatch_mode(mode, [&](auto m) { attn_launch_rows32<AttnBf16Ctx, decltype(m)::value>(a, static_cast<hipStream_t>(stream)); });
    QE_LAUNCH_CHECK();
    return QE_OK;
}
