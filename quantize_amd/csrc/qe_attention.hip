// qe_attention.hip -- the fp32 attention core of a ViT / nn.MultiheadAttention for gfx950 (MI355X):
//   out[n, t, h*d + c] = sum_s softmax_s(scale * q[n, t, h] . k[n, s, h]) v[n, s, h*d + c]
// read in place from rows of H*d floats (row n*rn + t*rt), never storing the L x S score matrix.
//
// attn_mfma_kernel<D> (d % 16 == 0, d <= 128): flash-style forward on the exact fp32 matrix pipe (v_mfma_f32_32x32x2_f32:
// a k-ordered fmaf chain, one rounding per product).  A wave owns 32 query rows of one (image, head); a workgroup holds up to
// 8 such waves of the same head, so the K / V rows they all stream are shared in the CU's L1.  Per 32-key tile:
//   S^T = K Q^T   A = K (lane: key lane&31), B = Q^T (lane: query lane&31); the k order is permuted (step s takes dim s from
//                 lane half 0, dim s + d/2 from half 1: both operands use the same pairing, and a sum over k is order-free),
//                 so each lane loads d/2 CONTIGUOUS floats of its row.  The accumulator gives lane l the 16 scores of query
//                 l&31 for keys crow(r, l>>5) = (r&3) + 8(r>>2) + 4(l>>5): a row max is 15 fmaxf and one exchange with
//                 lane l^32.
//   online softmax  m' = max(m, tile max); p = exp2f((s - m') log2e); l = l alpha + sum p; O = O alpha with
//                 alpha = exp2f((m - m') log2e).  The row sum stays split between the two lane halves until the end.
//   O^T += V^T P^T  A = V^T (lane: column lane&31 of a 32-column block, key crow(s, l>>5)), B = P^T: register s of the score
//                 accumulator IS the B operand of k-step s -- no lane movement.  O^T has the query on the lane, so the
//                 rescale by alpha and the final division by l are lane-local; the store is 4 float4 per 32-column block.
// K for the next tile is loaded while the softmax and P.V of this one run, V while S^T is computed.
// attn_valu_kernel<NO> (every d <= 256; QE_ATTN=0 takes it for every shape): one wave per query row, 64 keys per step (a
// lane per key: an fmaf chain over c = 0..d-1), the same online softmax, column c of the output on lane c % 64.
//
// Numerics (both kernels): q is multiplied by `scale` once as it is loaded (fp32); scores are fp32 fmaf sums; the softmax
// uses exp2f with the log2(e) factor applied to the max-subtracted score, (s - m) * log2e, so the subtraction stays exact
// near the max; products P.V and the row sum in fp32; one division by the row sum at the end.
// Non-finite inputs: fmaxf skips a NaN score, and exp2f(NaN) = NaN reaches that row's sum and output: a NaN in a query
// row poisons that row of that head only, a NaN in a key or value row that (image, head) only.
//
// Masked form (qe_attention_masked): the score becomes scale q.k + mask[n, h, t, s] + key_bias[n, s], restricted to
// s <= t under `causal`.  Both kernels add mask and key_bias to each other first, in fp32, then their sum to the score: a
// call with both returns the bits of a call with the mask alone that holds that sum.  Which operands exist is the template
// parameter MODE of both kernels (kMask | kBias | kCausal, plus kVec4 where every mask / bias run of four keys is 16-byte
// aligned), never a branch in the tile loop: MODE 0 is the unmasked kernel, instruction for instruction.  In the MFMA
// kernel a lane's 16 scores are four runs of four consecutive keys of ONE query row, so the mask adds lane-locally; its
// loads are issued with the K prefetch, a tile ahead.  Causal waves stop at the diagonal tile (the tiles above it are never
// loaded) and mask that tile by index.  While a row's running max is still -inf (every key so far masked) the rescale
// factor is 1 and p is 0, so a later visible key starts the row cleanly; a row with no visible key at all ends as
// 0 / 0 = NaN, that row of that head only.
//
// The argument struct, the MODE bits, the argument checks, the mode and head-size switches and the launch geometry of
// attn_mfma_kernel are qe_attention_common.hpp's, shared with the bf16 core (qe_attention_bf16.hip).  attn_bf16_kernel
// repeats parts of attn_mfma_kernel's text (marked below): a device helper for any of them changed some instance's code.
#include "qe_attention_common.hpp"

#include <cstdlib>

namespace qe {

template <int D, int MODE = 0>
__global__ __launch_bounds__(64 * attn_wpb(D)) void attn_mfma_kernel(const AttnArgs a)
{
    constexpr bool MASK = (MODE & kMask) != 0, BIAS = (MODE & kBias) != 0, CAUSAL = (MODE & kCausal) != 0;
    constexpr bool VEC4 = (MODE & kVec4) != 0;
    constexpr int HALF = D / 2;                 // k-steps of S^T; dims [h*HALF, h*HALF + HALF) on lane half h
    constexpr int NB = (D + 31) / 32;           // 32-column blocks of O^T
    constexpr int WPB = attn_wpb(D);
    // this block / wave / lane decode is also attn_bf16_kernel's
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

    // Q^T operand: lane holds q[query q0 + lo][hi*HALF + s] * scale
    float qr[HALF];
    {
        const int t = q0 + lo;
        if (t < a.L) {
            const float4 *src = reinterpret_cast<const float4 *>(a.q + (n * a.q_rn + t * a.q_rt) * E + col + hi * HALF);
#pragma unroll
            for (int i = 0; i < HALF / 4; ++i) {
                const float4 x = src[i];
                qr[4 * i] = x.x * a.scale; qr[4 * i + 1] = x.y * a.scale; qr[4 * i + 2] = x.z * a.scale; qr[4 * i + 3] = x.w * a.scale;
            }
        } else {
#pragma unroll
            for (int i = 0; i < HALF; ++i) qr[i] = 0.0f;
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
    auto load_add = [&](int k0) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int key = k0 + 8 * g + 4 * hi;
            if constexpr (VEC4) {                   // S % 4 == 0: a run lies wholly below S or wholly beyond it
                float4 x = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (key < a.S) {
                    if constexpr (MASK) x = *reinterpret_cast<const float4 *>(mrow + key);
                    if constexpr (BIAS) {
                        const float4 y = *reinterpret_cast<const float4 *>(brow + key);
                        if constexpr (MASK) { x.x += y.x; x.y += y.y; x.z += y.z; x.w += y.w; } else x = y;
                    }
                }
                ar[4 * g] = x.x; ar[4 * g + 1] = x.y; ar[4 * g + 2] = x.z; ar[4 * g + 3] = x.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float x = 0.0f;
                    if (key + j < a.S) {
                        if constexpr (MASK) x = mrow[key + j];
                        if constexpr (BIAS) { if constexpr (MASK) x += brow[key + j]; else x = brow[key + j]; }
                    }
                    ar[4 * g + j] = x;
                }
            }
        }
    };
    // causal: the last tile that holds a key <= q0 + 31 is the wave's diagonal tile; the tiles above it are not visited
    const int kend = CAUSAL ? min(a.S, q0 + 32) : a.S;

    float kr[HALF];
    auto load_k = [&](int k0) {
        if constexpr (MASK || BIAS) load_add(k0);
        const int key = k0 + lo;                    // this K-row load is also attn_bf16_kernel's
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

    f32x16 o[NB];                               // zeroed as in attn_bf16_kernel
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[b][r] = 0.0f;
    float m = -INFINITY, lsum = 0.0f;

    load_k(0);
    for (int k0 = 0; k0 < kend; k0 += 32) {
        // V^T operand of this tile: vr[s][b] = v[key k0 + crow(s, hi)][32 b + lo]
        float vr[16][NB];
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const int key = k0 + (s & 3) + 8 * (s >> 2) + 4 * hi;
            const float *src = vbase + key * kv_step;
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const int c = 32 * b + lo;
                vr[s][b] = (key < a.S && c < D) ? src[c] : 0.0f;
            }
        }
        f32x16 sc;
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[r] = 0.0f;
#pragma unroll
        for (int s = 0; s < HALF; ++s) sc = __builtin_amdgcn_mfma_f32_32x32x2f32(kr[s], qr[s], sc, 0, 0, 0);
        if constexpr (MASK || BIAS) {
#pragma unroll
            for (int r = 0; r < 16; ++r) sc[r] += ar[r];
        }
        if (k0 + 32 < kend) load_k(k0 + 32);

        // online softmax over this tile's 32 keys of query q0 + lo; also attn_bf16_kernel's
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
#pragma unroll
        for (int b = 0; b < NB; ++b) {
#pragma unroll
            for (int r = 0; r < 16; ++r) o[b][r] *= alpha;
#pragma unroll
            for (int s = 0; s < 16; ++s) o[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(vr[s][b], sc[s], o[b], 0, 0, 0);
        }
    }

    const int t = q0 + lo;
    const float l = lsum + __shfl_xor(lsum, 32);
    if (t >= a.L) return;
    float *dst = a.out + (n * a.o_rn + t * a.o_rt) * E + col;      // from the row-sum exchange on, also attn_bf16_kernel's
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

__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m));
    return v;
}

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

template <int NO, int MODE = 0>
__global__ __launch_bounds__(256) void attn_valu_kernel(const AttnArgs a)
{
    constexpr bool MASK = (MODE & kMask) != 0, BIAS = (MODE & kBias) != 0, CAUSAL = (MODE & kCausal) != 0;
    __shared__ float qs[4][NO * 64];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int64_t row = (int64_t)blockIdx.x * 4 + wave;      // over N * H * L
    const int64_t rows = (int64_t)a.N * a.H * a.L;
    const bool live = row < rows;
    const int t = live ? (int)(row % a.L) : 0;
    const int h = live ? (int)((row / a.L) % a.H) : 0;
    const int n = live ? (int)(row / ((int64_t)a.L * a.H)) : 0;
    const int64_t E = (int64_t)a.H * a.d;
    const int64_t col = (int64_t)h * a.d;
    const float *qrow = a.q + (n * a.q_rn + t * a.q_rt) * E + col;
#pragma unroll
    for (int i = 0; i < NO; ++i) {
        const int c = lane + 64 * i;
        qs[wave][c] = (live && c < a.d) ? qrow[c] * a.scale : 0.0f;
    }
    __syncthreads();
    if (!live) return;                                        // wave-uniform, after the only barrier
    const float *kbase = a.k + n * a.kv_rn * E + col;
    const float *vbase = a.v + n * a.kv_rn * E + col;
    const int64_t kv_step = a.kv_rt * E;
    float o[NO];
#pragma unroll
    for (int i = 0; i < NO; ++i) o[i] = 0.0f;
    float m = -INFINITY, l = 0.0f;
    const float *mrow = nullptr, *brow = nullptr;
    if constexpr (MASK) mrow = a.mask + n * a.mask_sn + h * a.mask_sh + (int64_t)t * a.S;
    if constexpr (BIAS) brow = a.key_bias + (int64_t)n * a.S;
    const int kend = CAUSAL ? min(a.S, t + 1) : a.S;           // causal: keys above the diagonal are not visited
    for (int k0 = 0; k0 < kend; k0 += 64) {
        const int key = k0 + lane;
        float s = -INFINITY;
        if (key < kend) {
            const float *kr = kbase + key * kv_step;
            s = 0.0f;
            for (int c = 0; c < a.d; ++c) s = fmaf(qs[wave][c], kr[c], s);
            if constexpr (MASK && BIAS) s += mrow[key] + brow[key];      // summed first, as the MFMA kernel does
            else if constexpr (MASK) s += mrow[key];
            else if constexpr (BIAS) s += brow[key];
        }
        const float mn = fmaxf(m, wave_max(s));
        float alpha = exp2f((m - mn) * kLog2e);
        float msub = mn;
        if constexpr (MASK || BIAS) {              // every key so far masked: keep the empty state (see the MFMA kernel)
            if (mn == -INFINITY) { alpha = 1.0f; msub = 0.0f; }
        }
        m = mn;
        const float p = key < kend ? exp2f((s - msub) * kLog2e) : 0.0f;
        l = l * alpha + wave_sum(p);
#pragma unroll
        for (int i = 0; i < NO; ++i) o[i] *= alpha;
        const int nk = min(64, kend - k0);
        for (int j = 0; j < nk; ++j) {
            const float pj = __shfl(p, j);
            const float *vr = vbase + (k0 + j) * kv_step;
#pragma unroll
            for (int i = 0; i < NO; ++i) {
                const int c = lane + 64 * i;
                if (c < a.d) o[i] = fmaf(pj, vr[c], o[i]);
            }
        }
    }
    float *dst = a.out + (n * a.o_rn + t * a.o_rt) * E + col;
#pragma unroll
    for (int i = 0; i < NO; ++i) {
        const int c = lane + 64 * i;
        if (c < a.d) dst[c] = o[i] / l;
    }
}

static int attn_path(int L, int S, int H, int d)
{
    if (L <= 0 || S <= 0 || H <= 0 || d <= 0 || d > 256) return -1;
    if (d % 16 != 0 || d > 128) return 0;
    if (const char *e = env_get("QE_ATTN")) { if (atoi(e) == 0) return 0; }
    return 1;
}

struct AttnMfma {
    template <int D, int MODE> static constexpr auto kernel = &attn_mfma_kernel<D, MODE>;
};

template <int NO, int MODE>
static void launch_valu(const AttnArgs &a, hipStream_t s)
{
    const int64_t blocks = ceil_div64((int64_t)a.N * a.H * a.L, 4);
    hipLaunchKernelGGL((attn_valu_kernel<NO, MODE>), dim3((unsigned)blocks), dim3(256), 0, s, a);
}

template <int MODE>
static void launch_mode(const AttnArgs &a, int path, hipStream_t s)
{
    if (path == 1) {
        attn_launch_rows32<AttnMfma, MODE>(a, s);
    } else {
        constexpr int VM = MODE & ~kVec4;        // the VALU kernel reads one float per lane: no 16-byte form
        const int no = ceil_div(a.d, 64);
        if (no == 1) launch_valu<1, VM>(a, s);
        else if (no == 2) launch_valu<2, VM>(a, s);
        else if (no == 3) launch_valu<3, VM>(a, s);
        else launch_valu<4, VM>(a, s);
    }
}

static int attn_run(const float *q, const float *k, const float *v, float *out, int32_t N, int32_t L, int32_t S, int32_t H,
                    int32_t d, int64_t q_rn, int64_t q_rt, int64_t kv_rn, int64_t kv_rt, int64_t o_rn, int64_t o_rt, float scale,
                    const float *mask, int64_t mask_sn, int64_t mask_sh, const float *key_bias, int causal, qe_stream_t stream)
{
    const int path = attn_path(L, S, H, d);
    AttnArgs a;
    int mode;
    if (const int e = attn_prepare(q, k, v, sizeof(float), out, sizeof(float), N, L, S, H, d, q_rn, q_rt, kv_rn, kv_rt, o_rn, o_rt, scale, mask, mask_sn,
                                   mask_sh, key_bias, causal, path, a, mode))
        return e;
    attn_dispatch_mode(mode, [&](auto m) { launch_mode<decltype(m)::value>(a, path, static_cast<hipStream_t>(stream)); });
    QE_LAUNCH_CHECK();
    return QE_OK;
}

}  // namespace qe

extern "C" int qe_attention_path(int32_t L, int32_t S, int32_t H, int32_t d)
{
    return qe::attn_path(L, S, H, d);
}

// the operands choose the kernel's instance, not the kernel: the answer is qe_attention_path's for every combination
extern "C" int qe_attention_masked_path(int32_t L, int32_t S, int32_t H, int32_t d, int has_mask, int has_key_bias, int causal)
{
    (void)has_mask; (void)has_key_bias; (void)causal;
    return qe::attn_path(L, S, H, d);
}

extern "C" int qe_attention(const float *q, const float *k, const float *v, float *out, int32_t N, int32_t L, int32_t S,
                            int32_t H, int32_t d, int64_t q_rn, int64_t q_rt, int64_t kv_rn, int64_t kv_rt, int64_t o_rn,
                            int64_t o_rt, float scale, qe_stream_t stream)
{
    return qe::attn_run(q, k, v, out, N, L, S, H, d, q_rn, q_rt, kv_rn, kv_rt, o_rn, o_rt, scale, nullptr, 0, 0, nullptr, 0,
                        stream);
}

extern "C" int qe_attention_masked(const float *q, const float *k, const float *v, float *out, int32_t N, int32_t L, int32_t S,
                                   int32_t H, int32_t d, int64_t q_rn, int64_t q_rt, int64_t kv_rn, int64_t kv_rt,
                                   int64_t o_rn, int64_t o_rt, float scale, const float *mask, int64_t mask_sn,
                                   int64_t mask_sh, const float *key_bias, int causal, qe_stream_t stream)
{
    return qe::attn_run(q, k, v, out, N, L, S, H, d, q_rn, q_rt, kv_rn, kv_rt, o_rn, o_rt, scale, mask, mask_sn, mask_sh,
                        key_bias, causal, stream);
}
