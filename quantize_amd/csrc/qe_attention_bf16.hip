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
// The argument struct, the mode bits and the argument checks restate qe_attention.hip's: that translation unit stays as it
// is (its 144 instances compile to the same code), so nothing is shared through a header.
#include "qe_common.h"

#include <algorithm>

namespace qe {

struct AttnBf16Args {
    const float *q, *k, *v;
    float *out;
    int64_t q_rn, q_rt, kv_rn, kv_rt, o_rn, o_rt;    // in rows of H*d floats
    int N, L, S, H, d;
    int qgroups;                                     // workgroups per (image, head)
    float scale;
    const float *mask, *key_bias;                    // masked instances only (MODE != 0)
    int64_t mask_sn, mask_sh;                        // element strides of the (L, S) mask block per image / head
};

namespace {

enum : int { kMask = 1, kBias = 2, kCausal = 4, kVec4 = 8 };    // as qe_attention.hip

constexpr float kLog2e = 1.4426950408889634f;

typedef float f32x16 __attribute__((ext_vector_type(16)));
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
__global__ __launch_bounds__(D <= 64 ? 512 : 256) void attn_bf16_kernel(const AttnBf16Args a)
{
    constexpr bool MASK = (MODE & kMask) != 0, BIAS = (MODE & kBias) != 0, CAUSAL = (MODE & kCausal) != 0;
    constexpr bool VEC4 = (MODE & kVec4) != 0;
    constexpr int HALF = D / 2;                 // dims [h*HALF, h*HALF + HALF) on lane half h
    constexpr int KS = D / 16;                  // k-steps of S^T: step s takes elements 8s .. 8s+7 of the lane's run
    constexpr int NB = (D + 31) / 32;           // 32-column blocks of O^T
    constexpr int WPB = D <= 64 ? 8 : 4;
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
        const int key = k0 + lo;
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

    f32x16 o[NB];
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

        // online softmax over this tile's 32 keys of query q0 + lo
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
    float *dst = a.out + (n * a.o_rn + t * a.o_rt) * E + col;
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

// 2 = the bf16 MFMA kernel, -1 = no kernel.  QE_ATTN is not read: it chooses between the two fp32 kernels only.
static int attn_bf16_path(int L, int S, int H, int d)
{
    if (L <= 0 || S <= 0 || H <= 0 || d <= 0) return -1;
    if (d % 16 != 0 || d > 128) return -1;
    return 2;
}

template <int D, int MODE>
static void launch_bf16(const AttnBf16Args &a, hipStream_t s)
{
    constexpr int WPB = D <= 64 ? 8 : 4;
    AttnBf16Args b = a;
    const int tiles = ceil_div(a.L, 32);
    const int wpb = std::min(WPB, tiles);        // a short sequence launches only the waves it has rows for
    b.qgroups = ceil_div(tiles, WPB);
    const int64_t blocks = (int64_t)b.qgroups * a.H * a.N;
    hipLaunchKernelGGL((attn_bf16_kernel<D, MODE>), dim3((unsigned)blocks), dim3(64 * (b.qgroups == 1 ? wpb : WPB)), 0, s, b);
}

template <int MODE>
static void launch_bf16_mode(const AttnBf16Args &a, hipStream_t s)
{
    switch (a.d) {
    case 16: launch_bf16<16, MODE>(a, s); break;
    case 32: launch_bf16<32, MODE>(a, s); break;
    case 48: launch_bf16<48, MODE>(a, s); break;
    case 64: launch_bf16<64, MODE>(a, s); break;
    case 80: launch_bf16<80, MODE>(a, s); break;
    case 96: launch_bf16<96, MODE>(a, s); break;
    case 112: launch_bf16<112, MODE>(a, s); break;
    default: launch_bf16<128, MODE>(a, s); break;
    }
}

// [lo, hi) byte range the rows of (n < N, t < T) span
static void row_span(const float *p, int N, int T, int64_t rn, int64_t rt, int64_t E, uintptr_t &lo, uintptr_t &hi)
{
    const int64_t last = (int64_t)(N - 1) * rn + (int64_t)(T - 1) * rt;
    lo = reinterpret_cast<uintptr_t>(p);
    hi = lo + (uintptr_t)((last + 1) * E) * sizeof(float);
}

// qe_attention_masked's checks, in its order (attn_run of qe_attention.hip), then the bf16 kernel's instance
static int attn_bf16_run(const float *q, const float *k, const float *v, float *out, int32_t N, int32_t L, int32_t S, int32_t H,
                         int32_t d, int64_t q_rn, int64_t q_rt, int64_t kv_rn, int64_t kv_rt, int64_t o_rn, int64_t o_rt,
                         float scale, const float *mask, int64_t mask_sn, int64_t mask_sh, const float *key_bias, int causal,
                         qe_stream_t stream)
{
    if (N <= 0 || L <= 0 || S <= 0 || H <= 0 || d <= 0) return QE_ERR_ARG;
    if (q_rn < 0 || q_rt < 0 || kv_rn < 0 || kv_rt < 0 || o_rn < 0 || o_rt < 0) return QE_ERR_ARG;
    if (q == nullptr || k == nullptr || v == nullptr || out == nullptr) return QE_ERR_ARG;
    if (((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v) |
          reinterpret_cast<uintptr_t>(out)) & 15) != 0)
        return QE_ERR_ARG;
    if (mask_sn < 0 || mask_sh < 0) return QE_ERR_ARG;
    if (mask == nullptr && (mask_sn != 0 || mask_sh != 0)) return QE_ERR_ARG;
    if (((reinterpret_cast<uintptr_t>(mask) | reinterpret_cast<uintptr_t>(key_bias)) & 15) != 0) return QE_ERR_ARG;
    if (attn_bf16_path(L, S, H, d) < 0) return QE_ERR_UNSUPPORTED;      // never the fp32 kernels instead
    const int64_t E = (int64_t)H * d;
    uintptr_t olo, ohi;
    row_span(out, N, L, o_rn, o_rt, E, olo, ohi);
    const float *ins[3] = {q, k, v};
    const int64_t rn[3] = {q_rn, kv_rn, kv_rn}, rt[3] = {q_rt, kv_rt, kv_rt};
    const int len[3] = {L, S, S};
    for (int i = 0; i < 3; ++i) {
        uintptr_t lo, hi;
        row_span(ins[i], N, len[i], rn[i], rt[i], E, lo, hi);
        if (lo < ohi && olo < hi) return QE_ERR_ARG;
    }
    if (mask != nullptr) {                       // the (L, S) blocks of (n < N, h < H) span up to this many floats
        const uintptr_t lo = reinterpret_cast<uintptr_t>(mask);
        const uintptr_t hi = lo + (uintptr_t)((N - 1) * mask_sn + (H - 1) * mask_sh + (int64_t)L * S) * sizeof(float);
        if (lo < ohi && olo < hi) return QE_ERR_ARG;
    }
    if (key_bias != nullptr) {
        const uintptr_t lo = reinterpret_cast<uintptr_t>(key_bias);
        const uintptr_t hi = lo + (uintptr_t)((int64_t)N * S) * sizeof(float);
        if (lo < ohi && olo < hi) return QE_ERR_ARG;
    }
    // the second limit is the fp32 VALU kernel's grid: kept so that both entry points answer every argument list alike
    // (tests/test_attention_bf16_cpu.py compares them)
    if ((int64_t)N * H * ceil_div(L, 32) > 0x7fffffffLL || ceil_div64((int64_t)N * H * L, 4) > 0x7fffffffLL)
        return QE_ERR_UNSUPPORTED;
    AttnBf16Args a = {};
    a.q = q; a.k = k; a.v = v; a.out = out;
    a.q_rn = q_rn; a.q_rt = q_rt; a.kv_rn = kv_rn; a.kv_rt = kv_rt; a.o_rn = o_rn; a.o_rt = o_rt;
    a.N = N; a.L = L; a.S = S; a.H = H; a.d = d; a.scale = scale;
    a.mask = mask; a.key_bias = key_bias; a.mask_sn = mask_sn; a.mask_sh = mask_sh;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int mode = (mask != nullptr ? kMask : 0) | (key_bias != nullptr ? kBias : 0) | (causal ? kCausal : 0);
    // every run of four keys a lane reads starts at a multiple of four floats from a 16-byte aligned base
    if ((mode & (kMask | kBias)) != 0 && S % 4 == 0 && mask_sn % 4 == 0 && mask_sh % 4 == 0) mode |= kVec4;
    switch (mode) {
    case 0: launch_bf16_mode<0>(a, s); break;
    case kMask: launch_bf16_mode<kMask>(a, s); break;
    case kBias: launch_bf16_mode<kBias>(a, s); break;
    case kMask | kBias: launch_bf16_mode<kMask | kBias>(a, s); break;
    case kCausal: launch_bf16_mode<kCausal>(a, s); break;
    case kCausal | kMask: launch_bf16_mode<kCausal | kMask>(a, s); break;
    case kCausal | kBias: launch_bf16_mode<kCausal | kBias>(a, s); break;
    case kCausal | kMask | kBias: launch_bf16_mode<kCausal | kMask | kBias>(a, s); break;
    case kVec4 | kMask: launch_bf16_mode<kVec4 | kMask>(a, s); break;
    case kVec4 | kBias: launch_bf16_mode<kVec4 | kBias>(a, s); break;
    case kVec4 | kMask | kBias: launch_bf16_mode<kVec4 | kMask | kBias>(a, s); break;
    case kVec4 | kCausal | kMask: launch_bf16_mode<kVec4 | kCausal | kMask>(a, s); break;
    case kVec4 | kCausal | kBias: launch_bf16_mode<kVec4 | kCausal | kBias>(a, s); break;
    default: launch_bf16_mode<kVec4 | kCausal | kMask | kBias>(a, s); break;
    }
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
