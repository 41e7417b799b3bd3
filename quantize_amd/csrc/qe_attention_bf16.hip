// qe_attention_bf16.hip -- the opt-in bf16 matrix-core form of the attention core (qe_attention_bf16): the structure of
// attn_mfma_kernel (qe_attention.hip: 32 query rows per wave, up to 8 waves of one (image, head) per workgroup, no LDS, no
// barrier, S^T = K Q^T so that a lane owns 16 scores of ONE query row, the score accumulator reused as the B operand of
// O^T += V^T P^T) with both products on v_mfma_f32_32x32x16_bf16 instead of v_mfma_f32_32x32x2_f32.  The 32x32 C/D layout
// is the same for both instructions, so the online softmax, the lane-local mask / key-bias / causal code, the tile
// skipping, the tails and the store are those of the fp32 kernel, line for line.  q, k, v and out stay fp32 in memory and
// are read in place: no workspace, no pre-pass.
//
//   S^T = K Q^T   D/16 steps.  Lane half hi holds dims [hi D/2, hi D/2 + D/2) of its row (contiguous 16-byte loads); step s
//                 takes elements 8s .. 8s+7 of that run on BOTH operands, so the k pairing is the same for A and B (a sum
//                 over k is order-free).  q is multiplied by scale in fp32, then q scale and k are rounded to bf16.
//   softmax       fp32, unchanged; the row sum l adds the fp32 p, before they are rounded.
//   O^T += V^T P^T  2 steps per 32-column block.  The B fragment of step s is registers 8s .. 8s+7 of the score accumulator
//                 rounded to bf16: element j of lane half h is key 16s + 8(j>>2) + 4h + (j&3) = crow(8s + j, h) of the
//                 tile, so the A fragment's element j is v[that key][32b + lo] -- vr[8s + j][b], the fp32 kernel's own
//                 loads -- rounded to bf16.  O stays fp32; alpha rescale and the one division by l as in the fp32 kernel.
//
// Numerics contract (include/quant_engine.h): q^ = bf16(fp32(q scale)), k^ = bf16(k), v^ = bf16(v), round to nearest even;
// scores are fp32 sums of exact bf16 products plus the fp32 mask / bias (summed first); p in fp32, rounded to bf16 only as
// the operand of P.V; l the fp32 sum of the unrounded p; O accumulated in fp32, one fp32 division at the end.
//
// The argument struct, the MODE bits, the argument checks, the mode and head-size switches and the launch geometry are
// qe_attention_common.hpp's, shared with the fp32 core.  The kernel's prologue, K-row load, accumulator zeroing, online
// softmax and store are attn_mfma_kernel's text, written out here as well (marked below): a device helper for any of them
// changed some instance's code in one of the two units.
#include "qe_attention_common.hpp"

namespace qe {

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// eight fp32 -> one MFMA fragment, round to nearest even (v_cvt_pk_bf16_f32)
__device__ __forceinline__ bf16x8 pack8(float x0, float x1, float x2, float x3, float x4, float x5, float x6, float x7)
{
    bf16x8 f;
    f[0] = (__bf16)x0; f[1] = (__bf16)x1; f[2] = (__bf16)x2; f[3] = (__bf16)x3;
    f[4] = (__bf16)x4; f[5] = (__bf16)x5; f[6] = (__bf16)x6; f[7] = (__bf16)x7;
    return f;
}

}  // namespace

template <int D, int MODE = 0>
__global__ __launch_bounds__(64 * attn_wpb(D)) void attn_bf16_kernel(const AttnArgs a)
{
    constexpr bool MASK = (MODE & kMask) != 0, BIAS = (MODE & kBias) != 0, CAUSAL = (MODE & kCausal) != 0;
    constexpr bool VEC4 = (MODE & kVec4) != 0;
    constexpr int HALF = D / 2;                 // dims [h*HALF, h*HALF + HALF) on lane half h
    constexpr int KS = D / 16;                  // k-steps of S^T: step s takes elements 8s .. 8s+7 of the lane's run
    constexpr int NB = (D + 31) / 32;           // 32-column blocks of O^T
    constexpr int WPB = attn_wpb(D);
    // this block / wave / lane decode is also attn_mfma_kernel's
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int lo = lane & 31, hi = lane >> 5;
    const int64_t bid = blockIdx.x;
    const int qg = (int)(bid % a.qgroups);
    const int64_t nh = bid / a.qgroups;
    const int h = (int)(nh % a.H);
    const int n = (int)(nh / a.H);
    const int q0 = (qg * WPB + wave) * 32;
    if (q0 >= a.L) return;                      // wave-uniform; no barrier in this kernel
    const int64_t E = (int64_t)a.H * a.d;
    const int64_t col = (int64_t)h * a.d;

    // Q^T operand: fragment s holds bf16(q[query q0 + lo][hi*HALF + 8s + j] * scale)
    bf16x8 qf[KS];
    {
        const int t = q0 + lo;
        if (t < a.L) {
            const float4 *src = reinterpret_cast<const float4 *>(a.q + (n * a.q_rn + t * a.q_rt) * E + col + hi * HALF);
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const float4 x = src[2 * s], y = src[2 * s + 1];
                qf[s] = pack8(x.x * a.scale, x.y * a.scale, x.z * a.scale, x.w * a.scale, y.x * a.scale, y.y * a.scale,
                              y.z * a.scale, y.w * a.scale);
            }
        } else {
#pragma unroll
            for (int s = 0; s < KS; ++s) qf[s] = pack8(0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f);
        }
    }
    const float *kbase = a.k + n * a.kv_rn * E + col;
    const float *vbase = a.v + n * a.kv_rn * E + col;
    const int64_t kv_step = a.kv_rt * E;

    // additive operands of a tile, in the score accumulator's own order: ar[r] belongs to key crow(r, hi) of query q0 + lo
    const float *mrow = nullptr, *brow = nullptr;
    if constexpr (MASK) mrow = a.mask + n * a.mask_sn + h * a.mask_sh + (int64_t)(q0 + lo < a.L ? q0 + lo : 0) * a.S;
    if constexpr (BIAS) brow = a.key_bias + (int64_t)n * a.S;
    float ar[(MASK || BIAS) ? 16 : 1];
    // as the V loads below: every lane loads from a clamped, valid address and a select zeroes what lies beyond S
    auto load_add = [&](int k0) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int key = k0 + 8 * g + 4 * hi;
            if constexpr (VEC4) {                   // S % 4 == 0: a run lies wholly below S or wholly beyond it
                const int kc = min(key, a.S - 4);
                float4 x = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if constexpr (MASK) x = *reinterpret_cast<const float4 *>(mrow + kc);
                if constexpr (BIAS) {
                    const float4 y = *reinterpret_cast<const float4 *>(brow + kc);
                    if constexpr (MASK) { x.x += y.x; x.y += y.y; x.z += y.z; x.w += y.w; } else x = y;
                }
                const bool in = key < a.S;
                ar[4 * g] = in ? x.x : 0.0f; ar[4 * g + 1] = in ? x.y : 0.0f; ar[4 * g + 2] = in ? x.z : 0.0f;
                ar[4 * g + 3] = in ? x.w : 0.0f;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int kc = min(key + j, a.S - 1);
                    float x = 0.0f;
                    if constexpr (MASK) x = mrow[kc];
                    if constexpr (BIAS) { if constexpr (MASK) x += brow[kc]; else x = brow[kc]; }
                    ar[4 * g + j] = key + j < a.S ? x : 0.0f;
                }
            }
        }
    };
    // causal: the last tile that holds a key <= q0 + 31 is the wave's diagonal tile; the tiles above it are not visited
    const int kend = CAUSAL ? min(a.S, q0 + 32) : a.S;

    // K of the next tile waits in fp32 registers (the loads stay in flight over the softmax); it is rounded as it is used
    float kr[HALF];
    auto load_k = [&](int k0) {
        if constexpr (MASK || BIAS) load_add(k0);
        const int key = k0 + lo;                    // this K-row load is also attn_mfma_kernel's
        if (key < a.S) {
            const float4 *src = reinterpret_cast<const float4 *>(kbase + key * kv_step + hi * HALF);
#pragma unroll
            for (int i = 0; i < HALF / 4; ++i) {
                const float4 x = src[i];
                kr[4 * i] = x.x; kr[4 * i + 1] = x.y; kr[4 * i + 2] = x.z; kr[4 * i + 3] = x.w;
            }
        } else {
#pragma unroll
            for (int i = 0; i < HALF; ++i) kr[i] = 0.0f;
        }
    };

    f32x16 o[NB];                               // zeroed as in attn_mfma_kernel
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[b][r] = 0.0f;
    float m = -INFINITY, lsum = 0.0f;

    load_k(0);
    for (int k0 = 0; k0 < kend; k0 += 32) {
        // V^T operand of this tile, still fp32: vr[s][b] = v[key k0 + crow(s, hi)][32 b + lo].  Every lane loads from a
        // clamped, valid address (key S - 1, column D - 1) and the tail is zeroed by a select: 16 NB loads in flight
        // together, where a load under a per-lane condition becomes a branch with its own wait
        float vr[16][NB];
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const int key = k0 + (s & 3) + 8 * (s >> 2) + 4 * hi;
            const float *src = vbase + min(key, a.S - 1) * kv_step;
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const int c = 32 * b + lo;
                const float x = src[32 * b + 31 < D ? c : min(c, D - 1)];
                vr[s][b] = (key < a.S && c < D) ? x : 0.0f;
            }
        }
        f32x16 sc;
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[r] = 0.0f;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const bf16x8 kf = pack8(kr[8 * s], kr[8 * s + 1], kr[8 * s + 2], kr[8 * s + 3], kr[8 * s + 4], kr[8 * s + 5],
                                    kr[8 * s + 6], kr[8 * s + 7]);
            sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[s], sc, 0, 0, 0);
        }
        if constexpr (MASK || BIAS) {
#pragma unroll
            for (int r = 0; r < 16; ++r) sc[r] += ar[r];
        }
        if (k0 + 32 < kend) load_k(k0 + 32);

        // online softmax over this tile's 32 keys of query q0 + lo; also attn_mfma_kernel's
        float tmax = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = k0 + (r & 3) + 8 * (r >> 2) + 4 * hi;
            if (key >= a.S) sc[r] = -INFINITY;
            if constexpr (CAUSAL) { if (key > q0 + lo) sc[r] = -INFINITY; }
            tmax = fmaxf(tmax, sc[r]);
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
        const float mn = fmaxf(m, tmax);
        float alpha = exp2f((m - mn) * kLog2e);
        float msub = mn;
        if constexpr (MASK || BIAS) {              // every key so far masked: -inf - -inf is NaN; keep the empty state
            if (mn == -INFINITY) { alpha = 1.0f; msub = 0.0f; }
        }
        m = mn;
        float psum = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            sc[r] = exp2f((sc[r] - msub) * kLog2e);
            psum += sc[r];
        }
        lsum = lsum * alpha + psum;
        // P^T operand: registers 8s .. 8s+7 of the score accumulator are the B fragment of k-step s
        bf16x8 pf[2];
#pragma unroll
        for (int s = 0; s < 2; ++s)
            pf[s] = pack8(sc[8 * s], sc[8 * s + 1], sc[8 * s + 2], sc[8 * s + 3], sc[8 * s + 4], sc[8 * s + 5], sc[8 * s + 6],
                          sc[8 * s + 7]);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
#pragma unroll
            for (int r = 0; r < 16; ++r) o[b][r] *= alpha;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const bf16x8 vf = pack8(vr[8 * s][b], vr[8 * s + 1][b], vr[8 * s + 2][b], vr[8 * s + 3][b], vr[8 * s + 4][b],
                                        vr[8 * s + 5][b], vr[8 * s + 6][b], vr[8 * s + 7][b]);
                o[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf[s], o[b], 0, 0, 0);
            }
        }
    }

    const int t = q0 + lo;
    const float l = lsum + __shfl_xor(lsum, 32);
    if (t >= a.L) return;
    float *dst = a.out + (n * a.o_rn + t * a.o_rt) * E + col;      // from the row-sum exchange on, also attn_mfma_kernel's
#pragma unroll
    for (int b = 0; b < NB; ++b) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c = 32 * b + 8 * g + 4 * hi;       // O^T rows (r&3) + 8(r>>2) + 4 hi of register r = 4 g + j
            if (c < D)
                *reinterpret_cast<float4 *>(dst + c) =
                    make_float4(o[b][4 * g] / l, o[b][4 * g + 1] / l, o[b][4 * g + 2] / l, o[b][4 * g + 3] / l);
        }
    }
}

struct AttnBf16 {
    template <int D, int MODE> static constexpr auto kernel = &attn_bf16_kernel<D, MODE>;
};

static int attn_bf16_run(const float *q, const float *k, const float *v, float *out, int32_t N, int32_t L, int32_t S, int32_t H,
                         int32_t d, int64_t q_rn, int64_t q_rt, int64_t kv_rn, int64_t kv_rt, int64_t o_rn, int64_t o_rt,
                         float scale, const float *mask, int64_t mask_sn, int64_t mask_sh, const float *key_bias, int causal,
                         qe_stream_t stream)
{
    AttnArgs a;
    int mode;
    // a head size without a bf16 instance is refused here: never the fp32 kernels instead
    if (const int e = attn_prepare(q, k, v, sizeof(float), out, sizeof(float), N, L, S, H, d, q_rn, q_rt, kv_rn, kv_rt, o_rn, o_rt, scale, mask, mask_sn,
                                   mask_sh, key_bias, causal, attn_bf16_path(L, S, H, d), a, mode))
        return e;
    attn_dispatch_mode(mode, [&](auto m) { attn_launch_rows32<AttnBf16, decltype(m)::value>(a, static_cast<hipStream_t>(stream)); });
    QE_LAUNCH_CHECK();
    return QE_OK;
}

}  // namespace qe

// the operands choose the kernel's instance, not the kernel
extern "C" int qe_attention_bf16_path(int32_t L, int32_t S, int32_t H, int32_t d, int has_mask, int has_key_bias, int causal)
{
    (void)has_mask; (void)has_key_bias; (void)causal;
    return qe::attn_bf16_path(L, S, H, d);
}

extern "C" int qe_attention_bf16(const float *q, const float *k, const float *v, float *out, int32_t N, int32_t L, int32_t S,
                                 int32_t H, int32_t d, int64_t q_rn, int64_t q_rt, int64_t kv_rn, int64_t kv_rt, int64_t o_rn,
                                 int64_t o_rt, float scale, const float *mask, int64_t mask_sn, int64_t mask_sh,
                                 const float *key_bias, int causal, qe_stream_t stream)
{
    return qe::attn_bf16_run(q, k, v, out, N, L, S, H, d, q_rn, q_rt, kv_rn, kv_rt, o_rn, o_rt, scale, mask, mask_sn, mask_sh,
                             key_bias, causal, stream);
}
