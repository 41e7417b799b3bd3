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
// O^T += V^T P^T, store) is attn_bf16_kernel's, written out here as well: the outputs are bit-identical
// (tests/test_attention_bf16_stored_gpu.py).
//
// The argument struct (its q / k / v pointers carry the bf16 rows), the MODE bits, the argument checks with 2-byte input
// elements, the mode and head-size switches and the launch geometry are qe_attention_common.hpp's.
#include "qe_attention_common.hpp"

namespace qe {

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
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

template <int D, int MODE = 0>
__global__ __launch_bounds__(64 * attn_wpb(D)) void attn_bf16_stored_kernel(const AttnArgs a)
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
    const uint16_t *q16 = reinterpret_cast<const uint16_t *>(a.q);      // the rows are bf16 (AttnArgs)
    const uint16_t *k16 = reinterpret_cast<const uint16_t *>(a.k);
    const uint16_t *v16 = reinterpret_cast<const uint16_t *>(a.v);

    // Q^T operand: fragment s holds bf16(fp32(q[query q0 + lo][hi*HALF + 8s + j]) * scale); rows beyond L are zero
    bf16x8 qf[KS];
    {
        const int t = q0 + lo;
        const uint4 *src = reinterpret_cast<const uint4 *>(q16 + (n * a.q_rn + min(t, a.L - 1) * a.q_rt) * E + col + hi * HALF);
        const float sc = a.scale;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const uint4 x = src[s];
            qf[s] = t < a.L ? pack8(bf_lo(x.x) * sc, bf_hi(x.x) * sc, bf_lo(x.y) * sc, bf_hi(x.y) * sc, bf_lo(x.z) * sc,
                                    bf_hi(x.z) * sc, bf_lo(x.w) * sc, bf_hi(x.w) * sc)
                            : pack8(0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f);
        }
    }
    const uint16_t *kbase = k16 + n * a.kv_rn * E + col;
    const uint16_t *vbase = v16 + n * a.kv_rn * E + col;
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

    // K of the next tile waits as MFMA fragments (the loads stay in flight over the softmax): fragment s of key k0 + lo is
    // elements hi*HALF + 8s .. + 7 of its row, zero beyond S
    uint4 kr[KS];
    auto load_k = [&](int k0) {
        if constexpr (MASK || BIAS) load_add(k0);
        const int key = k0 + lo;
        const uint4 *src = reinterpret_cast<const uint4 *>(kbase + min(key, a.S - 1) * kv_step + hi * HALF);
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const uint4 x = src[s];
            kr[s] = key < a.S ? x : make_uint4(0u, 0u, 0u, 0u);
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
        // V^T operand of this tile: register vr[i][b] holds elements 2 i (low half) and 2 i + 1 (high half) of the fragments,
        // v[key k0 + crow(2 i, hi)][32 b + lo] and the same column of the next key.  Every lane loads from a clamped, valid
        // address (key S - 1, column D - 1) and one mask per register zeroes the tail: 16 NB loads in flight together,
        // where a load under a per-lane condition becomes a branch with its own wait
        uint32_t vr[8][NB];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int key = k0 + (2 * i & 3) + 8 * (i >> 1) + 4 * hi;       // crow(2 i, hi); crow(2 i + 1, hi) is key + 1
            const uint16_t *src0 = vbase + min(key, a.S - 1) * kv_step, *src1 = vbase + min(key + 1, a.S - 1) * kv_step;
            const uint32_t keep = key + 1 < a.S ? 0xffffffffu : key < a.S ? 0xffffu : 0u;
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const int c = 32 * b + lo;
                const int cc = 32 * b + 31 < D ? c : min(c, D - 1);
                u16x2 w;
                w.x = src0[cc];
                w.y = src1[cc];
                vr[i][b] = __builtin_bit_cast(uint32_t, w) & (c < D ? keep : 0u);
            }
        }
        f32x16 sc;
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[r] = 0.0f;
#pragma unroll
        for (int s = 0; s < KS; ++s) sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, kr[s]), qf[s], sc, 0, 0, 0);
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
                // elements 2i, 2i + 1 of the A fragment share a register: low and high half
                const uint4 vf = make_uint4(vr[4 * s][b], vr[4 * s + 1][b], vr[4 * s + 2][b], vr[4 * s + 3][b]);
                o[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, vf), pf[s], o[b], 0, 0, 0);
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
    if (const int e = attn_prepare(q, k, v, sizeof(uint16_t), out, N, L, S, H, d, q_rn, q_rt, kv_rn, kv_rt, o_rn, o_rt, scale, mask,
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
