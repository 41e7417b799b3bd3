// qe_attention_bf16_stored.hip -- qe_attention_bf16_stored: attn_bf16_kernel (qe_attention_bf16.hip) on q, k, v that are
// already bf16 in memory (rows of H*d bf16 elements, e.g. what qe_quantlinear_bf16 wrote).  Same geometry (32 query rows
// per wave, attn_wpb waves of one (image, head) per workgroup, no LDS, no barrier, no workspace), same two products on
// v_mfma_f32_32x32x16_bf16 with the same fragments, same fp32 out / mask / key_bias / causal operands and the same 14 MODE
// instances x 8 head sizes; what changes is how an operand reaches its fragment:
//
//   Q^T   fragment s of a lane is ONE 16-byte load (elements hi D/2 + 8s .. + 7 of the query row); it is widened to fp32,
//         multiplied by scale in fp32 and rounded back to bf16 (nearest even), once per wave.  With scale == 1.0f that
//         returns the stored value.
//   K     fragment s of the next tile is one 16-byte load per lane and is the MFMA operand as loaded: no conversion in
//         the tile loop (attn_bf16_kernel rounds D/2 floats per lane and tile).
//   V^T   element j of fragment (s, b) is v[key crow(8s + j, hi)][32 b + lo]: a 2-byte load per element, two of them
//         joined into one fragment register (attn_bf16_kernel: a 4-byte load and a rounding per element).
//
// Every lane loads from a clamped, valid address (key S - 1, column D - 1) and a select zeroes what lies beyond S or D --
// K rows included: never a load under a per-lane condition.
//
// Numerics contract (include/quant_engine.h): q^ = bf16(fp32(q) scale), k^ = k, v^ = v, and everything after that is
// qe_attention_bf16's contract.  On inputs that are bf16 values, and with the same scale, the fragments of the two kernels
// hold the same bits, and the text from the score accumulator on (mask / bias add, online softmax, P rounding, rescale,
// O^T += V^T P^T, store) is attn_bf16_kernel's, written out for this kernel as well: the outputs are bit-identical
// (tests/test_attention_bf16_stored_gpu.py).  The kernel's statements are qe_attention_bf16_stored_body.hpp, included inside
// the kernel below and inside attn_bf16_ctx_kernel (qe_attention_bf16_ctx.hip), which differs in its store alone.
//
// The argument struct (its q / k / v pointers carry the bf16 rows), the MODE bits, the argument checks with 2-byte input
// elements, the mode and head-size switches and the launch geometry are qe_attention_common.hpp's.
#include "qe_attention_bf16_stored_kernel.hpp"

namespace qe {

template <int D, int MODE = 0>
__global__ __launch_bounds__(64 * attn_wpb(D)) void attn_bf16_stored_kernel(const AttnArgs a)
{
    constexpr bool OUT16 = false;
#include "qe_attention_bf16_stored_body.hpp"
}

struct AttnBf16Stored {
    template <int D, int MODE> static constexpr auto kernel = &attn_bf16_stored_kernel<D, MODE>;
};

static int attn_bf16_stored_run(const uint16_t *q, const uint16_t *k, const uint16_t *v, float *out, int32_t N, int32_t L,
                                int32_t S, int32_t H, int32_t d, int64_t q_rn, int64_t q_rt, int64_t kv_rn, int64_t kv_rt,
                                int64_t o_rn, int64_t o_rt, float scale, const float *mask, int64_t mask_sn, int64_t mask_sh,
                                const float *key_bias, int causal, qe_stream_t stream)
{
    AttnArgs a;
    int mode;
    // a head size without a bf16 instance is refused here: never another kernel instead
    if (const int e = attn_prepare(q, k, v, sizeof(uint16_t), out, sizeof(float), N, L, S, H, d, q_rn, q_rt, kv_rn, kv_rt, o_rn, o_rt, scale, mask,
                                   mask_sn, mask_sh, key_bias, causal, attn_bf16_path(L, S, H, d), a, mode))
        return e;
    attn_dispatch_mode(mode, [&](auto m) { attn_launch_rows32<AttnBf16Stored, decltype(m)::value>(a, static_cast<hipStream_t>(stream)); });
    QE_LAUNCH_CHECK();
    return QE_OK;
}

}  // namespace qe

// the operands choose the kernel's instance, not the kernel
extern "C" int qe_attention_bf16_stored_path(int32_t L, int32_t S, int32_t H, int32_t d, int has_mask, int has_key_bias, int causal)
{
    (void)has_mask; (void)has_key_bias; (void)causal;
    return qe::attn_bf16_path(L, S, H, d);
}

extern "C" int qe_attention_bf16_stored(const uint16_t *q, const uint16_t *k, const uint16_t *v, float *out, int32_t N, int32_t L,
                                        int32_t S, int32_t H, int32_t d, int64_t q_rn, int64_t q_rt, int64_t kv_rn, int64_t kv_rt,
                                        int64_t o_rn, int64_t o_rt, float scale, const float *mask, int64_t mask_sn,
                                        int64_t mask_sh, const float *key_bias, int causal, qe_stream_t stream)
{
    return qe::attn_bf16_stored_run(q, k, v, out, N, L, S, H, d, q_rn, q_rt, kv_rn, kv_rt, o_rn, o_rt, scale, mask, mask_sn, mask_sh,
                                    key_bias, causal, stream);
}
