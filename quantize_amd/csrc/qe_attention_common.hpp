// qe_attention_common.hpp -- what the attention cores (qe_attention.hip: fp32, qe_attention_bf16.hip: bf16 MFMA on fp32
// rows, qe_attention_bf16_stored.hip: the same on bf16 rows, qe_attention_bf16_ctx.hip: that one with a bf16 context) share: the
// argument struct and the MODE bits, every check an entry point makes before it launches (attn_prepare), and the two
// switches that turn the runtime mode and head size into a kernel instance (attn_dispatch_mode, attn_launch_rows32), with
// the launch geometry of the kernels that give a wave 32 query rows.  No device code: attn_mfma_kernel and attn_bf16_kernel
// keep their common text (prologue, K-row load, accumulator zeroing, online softmax, store) written out in each, because
// every helper tried changed the instructions of some instance.
#pragma once
#include "qe_common.h"

#include <algorithm>
#include <type_traits>

namespace qe {

struct AttnArgs {
    const float *q, *k, *v;                          // attn_bf16_stored_kernel: rows of bf16 behind the same three pointers
    float *out;                                      // attn_bf16_ctx_kernel: rows of bf16 behind this pointer
    int64_t q_rn, q_rt, kv_rn, kv_rt, o_rn, o_rt;    // in rows of H*d elements
    int N, L, S, H, d;
    int qgroups;                                     // workgroups per (image, head)
    float scale;
    const float *mask, *key_bias;                    // masked instances only (MODE != 0)
    int64_t mask_sn, mask_sh;                        // element strides of the (L, S) mask block per image / head
};

enum : int { kMask = 1, kBias = 2, kCausal = 4, kVec4 = 8 };

constexpr float kLog2e = 1.4426950408889634f;

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- the kernels with 32 query rows per wave (attn_mfma_kernel, attn_bf16_kernel, attn_bf16_stored_kernel) ----

// waves of one (image, head) per workgroup (they share the K / V rows they stream in the CU's L1): the kernels' block size
// and query decode, and the grid below
constexpr int attn_wpb(int D) { return D <= 64 ? 8 : 4; }

// CORE names a kernel family: struct { template <int D, int MODE> static constexpr auto kernel = &some_kernel<D, MODE>; }
template <class CORE, int D, int MODE>
inline void attn_launch_d(const AttnArgs &a, hipStream_t s)
{
    constexpr int WPB = attn_wpb(D);
    AttnArgs b = a;
    const int tiles = ceil_div(a.L, 32);
    const int wpb = std::min(WPB, tiles);        // a short sequence launches only the waves it has rows for
    b.qgroups = ceil_div(tiles, WPB);
    const int64_t blocks = (int64_t)b.qgroups * a.H * a.N;
    launch_instance<CORE::template kernel<D, MODE>>((unsigned)blocks, 64 * (b.qgroups == 1 ? wpb : WPB), 0, 0, s, b);
}

// the head sizes of these kernels: d % 16 == 0, d <= 128 (the caller's path function has checked it)
template <class CORE, int MODE>
inline void attn_launch_rows32(const AttnArgs &a, hipStream_t s)
{
    switch (a.d) {
    case 16: attn_launch_d<CORE, 16, MODE>(a, s); break;
    case 32: attn_launch_d<CORE, 32, MODE>(a, s); break;
    case 48: attn_launch_d<CORE, 48, MODE>(a, s); break;
    case 64: attn_launch_d<CORE, 64, MODE>(a, s); break;
    case 80: attn_launch_d<CORE, 80, MODE>(a, s); break;
    case 96: attn_launch_d<CORE, 96, MODE>(a, s); break;
    case 112: attn_launch_d<CORE, 112, MODE>(a, s); break;
    default: attn_launch_d<CORE, 128, MODE>(a, s); break;
    }
}

// ---- one mode switch and one set of checks for every entry point ----

// f(std::integral_constant<int, MODE>) for the runtime mode: the 14 instances of a kernel (kVec4 needs a mask or a bias)
template <class F>
inline void attn_dispatch_mode(int mode, F &&f)
{
    switch (mode) {
    case 0: f(std::integral_constant<int, 0>()); break;
    case kMask: f(std::integral_constant<int, kMask>()); break;
    case kBias: f(std::integral_constant<int, kBias>()); break;
    case kMask | kBias: f(std::integral_constant<int, kMask | kBias>()); break;
    case kCausal: f(std::integral_constant<int, kCausal>()); break;
    case kCausal | kMask: f(std::integral_constant<int, kCausal | kMask>()); break;
    case kCausal | kBias: f(std::integral_constant<int, kCausal | kBias>()); break;
    case kCausal | kMask | kBias: f(std::integral_constant<int, kCausal | kMask | kBias>()); break;
    case kVec4 | kMask: f(std::integral_constant<int, kVec4 | kMask>()); break;
    case kVec4 | kBias: f(std::integral_constant<int, kVec4 | kBias>()); break;
    case kVec4 | kMask | kBias: f(std::integral_constant<int, kVec4 | kMask | kBias>()); break;
    case kVec4 | kCausal | kMask: f(std::integral_constant<int, kVec4 | kCausal | kMask>()); break;
    case kVec4 | kCausal | kBias: f(std::integral_constant<int, kVec4 | kCausal | kBias>()); break;
    default: f(std::integral_constant<int, kVec4 | kCausal | kMask | kBias>()); break;
    }
}

// 2 = a bf16 matrix-core kernel (either storage), -1 = no kernel.  QE_ATTN is not read: it chooses between the two fp32
// kernels only.
inline int attn_bf16_path(int L, int S, int H, int d)
{
    if (L <= 0 || S <= 0 || H <= 0 || d <= 0) return -1;
    if (d % 16 != 0 || d > 128) return -1;
    return 2;
}

// [lo, hi) byte range the rows of (n < N, t < T) span; elem = bytes per element
inline void row_span(const void *p, int N, int T, int64_t rn, int64_t rt, int64_t E, size_t elem, uintptr_t &lo, uintptr_t &hi)
{
    const int64_t last = (int64_t)(N - 1) * rn + (int64_t)(T - 1) * rt;
    lo = reinterpret_cast<uintptr_t>(p);
    hi = lo + (uintptr_t)((last + 1) * E) * elem;
}

// Everything qe_attention, qe_attention_masked, qe_attention_bf16, qe_attention_bf16_stored and qe_attention_bf16_ctx check
// before a launch, in one
// order, so that an argument list that breaks two rules gets one answer from all of them.  in_elem = bytes per element of
// q, k and v (4: fp32 rows, 2: bf16 rows), out_elem = bytes per element of out (4, or 2: qe_attention_bf16_ctx's bf16 rows);
// mask and key_bias are fp32 for every entry point.  `path` is the entry point's own path function's
// answer for (L, S, H, d), < 0: no kernel.  On QE_OK `a` is filled (but for qgroups) and `mode` is the instance's MODE.
// Both grid limits hold for every entry point: the second is the fp32 VALU kernel's.
inline int attn_prepare(const void *q, const void *k, const void *v, size_t in_elem, void *out, size_t out_elem, int32_t N, int32_t L, int32_t S, int32_t H,
                        int32_t d, int64_t q_rn, int64_t q_rt, int64_t kv_rn, int64_t kv_rt, int64_t o_rn, int64_t o_rt,
                        float scale, const float *mask, int64_t mask_sn, int64_t mask_sh, const float *key_bias, int causal,
                        int path, AttnArgs &a, int &mode)
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
    if (path < 0) return QE_ERR_UNSUPPORTED;
    const int64_t E = (int64_t)H * d;
    uintptr_t olo, ohi;
    row_span(out, N, L, o_rn, o_rt, E, out_elem, olo, ohi);
    const void *ins[3] = {q, k, v};
    const int64_t rn[3] = {q_rn, kv_rn, kv_rn}, rt[3] = {q_rt, kv_rt, kv_rt};
    const int len[3] = {L, S, S};
    for (int i = 0; i < 3; ++i) {
        uintptr_t lo, hi;
        row_span(ins[i], N, len[i], rn[i], rt[i], E, in_elem, lo, hi);
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
    const int64_t rows = (int64_t)N * H * L;
    if ((int64_t)N * H * ceil_div(L, 32) > 0x7fffffffLL || ceil_div64(rows, 4) > 0x7fffffffLL) return QE_ERR_UNSUPPORTED;
    a = {};
    a.q = static_cast<const float *>(q); a.k = static_cast<const float *>(k); a.v = static_cast<const float *>(v); a.out = static_cast<float *>(out);
    a.q_rn = q_rn; a.q_rt = q_rt; a.kv_rn = kv_rn; a.kv_rt = kv_rt; a.o_rn = o_rn; a.o_rt = o_rt;
    a.N = N; a.L = L; a.S = S; a.H = H; a.d = d; a.scale = scale;
    a.mask = mask; a.key_bias = key_bias; a.mask_sn = mask_sn; a.mask_sh = mask_sh;
    mode = (mask != nullptr ? kMask : 0) | (key_bias != nullptr ? kBias : 0) | (causal ? kCausal : 0);
    // every run of four keys a lane reads starts at a multiple of four floats from a 16-byte aligned base
    if ((mode & (kMask | kBias)) != 0 && S % 4 == 0 && mask_sn % 4 == 0 && mask_sh % 4 == 0) mode |= kVec4;
    return QE_OK;
}

}  // namespace qe
