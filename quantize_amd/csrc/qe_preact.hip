// qe_preact.hip -- the boundary between two convolutions of a pre-activation network (WideResNet):
//   s = x + identity ;  a = relu(s * alpha[c] + shift[c]) ;  codes[i] = qe_quantize_pack(a, rq[i])
// in one pass over x and identity: the residual add, an eval-mode BatchNorm as the per-channel affine the Python layer derives
// from it, the ReLU and up to two consumer quantisers (conv1 and convShortcut of the next block), with the residual stream s and
// the activated tensor a as optional fp32 outputs.  Two instances, which the host-side plan (qe_preact.hpp) picks:
//   fast   every consumer 8-bit and P % 16 == 0: a thread owns 16 consecutive elements of one plane;
//   plain  everything else: a thread owns 8 consecutive elements of the flat tensor, whose b-bit codes are b whole bytes.
//
// The contract is an fp32 operation SEQUENCE (include/quant_engine.h), so nothing in this file may be contracted into an fma.
#include "qe_preact.hpp"
#include "qe_conv_span.hpp"
#include "qe_elementwise.hpp"

#pragma clang fp contract(off)

namespace qe {

struct PreactArgs {
    const float *x, *identity;             // identity NULL: s = x
    const float *alpha, *shift;
    float *sum_out, *act_out;              // NULL: not stored.  sum_out may be x or identity: a thread reads its elements first
    RqArgs rq[PREACT_MAX_OUT];             // fast: the 8-bit consumers (rq[i].out: their codes)
    QeRq q[PREACT_MAX_OUT];                // plain: the consumers at any width
    uint8_t *codes[PREACT_MAX_OUT];
    int n_bits[PREACT_MAX_OUT], rq_pt[PREACT_MAX_OUT];
    int32_t *status;
    int n_out, C, P;
    int64_t n;
};

__device__ __forceinline__ float preact_value(float s, float al, float sh)
{
    const float m = s * al;
    const float t = m + sh;
    return span_relu(t);
}

__device__ __forceinline__ void preact_report(const PreactArgs &a, bool bad)
{
    if (__builtin_amdgcn_ballot_w64(bad) != 0 && (threadIdx.x & 63) == 0 && a.status != nullptr) atomicOr(a.status, 1);
}

// ---- fast: 16 consecutive elements of one plane per thread ---------------------------------------------------------------------
// Four 16-byte loads of x (and of identity) and four 16-byte stores of each fp32 output at the tensors' own 4-byte alignment, one
// 16-byte store of codes per consumer at any byte alignment (the hardware splits a piece that straddles a line).  The channel is
// the thread's: alpha, shift and the consumers' scales are read once.  n is a multiple of 16: there is no ragged group.
__global__ __launch_bounds__(PREACT_THREADS) void preact_fast_kernel(const PreactArgs a)
{
    const int64_t e0 = ((int64_t)blockIdx.x * PREACT_THREADS + threadIdx.x) * PREACT_FAST_VEC;
    bool bad = false;
    if (e0 < a.n) {
        const int c = (int)((e0 / a.P) % a.C);
        float v[PREACT_FAST_VEC];
#pragma unroll
        for (int k = 0; k < 4; ++k) __builtin_memcpy(v + 4 * k, a.x + e0 + 4 * k, 16);
        if (a.identity != nullptr) {
            float d[PREACT_FAST_VEC];
#pragma unroll
            for (int k = 0; k < 4; ++k) __builtin_memcpy(d + 4 * k, a.identity + e0 + 4 * k, 16);
#pragma unroll
            for (int j = 0; j < PREACT_FAST_VEC; ++j) v[j] = v[j] + d[j];
        }
        if (a.sum_out != nullptr) {
#pragma unroll
            for (int k = 0; k < 4; ++k) __builtin_memcpy(a.sum_out + e0 + 4 * k, v + 4 * k, 16);
        }
        const float al = a.alpha[c], sh = a.shift[c];
#pragma unroll
        for (int j = 0; j < PREACT_FAST_VEC; ++j) v[j] = preact_value(v[j], al, sh);
        if (a.act_out != nullptr) {
#pragma unroll
            for (int k = 0; k < 4; ++k) __builtin_memcpy(a.act_out + e0 + 4 * k, v + 4 * k, 16);
        }
        for (int i = 0; i < a.n_out; ++i) {
            const RqConst rc = span_rq_setup(a.rq[i], a.rq_pt[i] ? 0 : c);
            uint32_t cw[4] = {0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < PREACT_FAST_VEC; ++j) cw[j >> 2] |= ((unsigned)rq_value(rc, v[j], bad) & 0xffu) << (8 * (j & 3));
            const uint4 w = make_uint4(cw[0], cw[1], cw[2], cw[3]);
            __builtin_memcpy(a.codes[i] + e0, &w, 16);
        }
    }
    if (a.n_out > 0) preact_report(a, bad);
}

// ---- plain: 8 consecutive elements of the flat tensor per thread, grid-stride ----------------------------------------------------
// A whole group moves in 16-byte pieces, the last ragged one element by element; the lanes past the tensor's end compute nothing,
// so they raise no flag.  The group's 8 b-bit codes are b whole bytes of each consumer's stream, which no other thread touches.
__global__ __launch_bounds__(PREACT_THREADS) void preact_plain_kernel(const PreactArgs a)
{
    const int64_t n_groups = (a.n + PREACT_PLAIN_VEC - 1) / PREACT_PLAIN_VEC;
    bool bad = false;
    for (int64_t g = (int64_t)blockIdx.x * PREACT_THREADS + threadIdx.x; g < n_groups; g += (int64_t)gridDim.x * PREACT_THREADS) {
        const int64_t e0 = PREACT_PLAIN_VEC * g;
        const int cnt = (a.n - e0) < PREACT_PLAIN_VEC ? (int)(a.n - e0) : PREACT_PLAIN_VEC;
        const bool whole = cnt == PREACT_PLAIN_VEC;
        float v[PREACT_PLAIN_VEC], d[PREACT_PLAIN_VEC];
        if (whole) {
            __builtin_memcpy(v, a.x + e0, 16);
            __builtin_memcpy(v + 4, a.x + e0 + 4, 16);
        } else {
#pragma unroll
            for (int j = 0; j < PREACT_PLAIN_VEC; ++j) v[j] = j < cnt ? a.x[e0 + j] : 0.0f;
        }
        if (a.identity != nullptr) {
            if (whole) {
                __builtin_memcpy(d, a.identity + e0, 16);
                __builtin_memcpy(d + 4, a.identity + e0 + 4, 16);
            } else {
#pragma unroll
                for (int j = 0; j < PREACT_PLAIN_VEC; ++j) d[j] = j < cnt ? a.identity[e0 + j] : 0.0f;
            }
#pragma unroll
            for (int j = 0; j < PREACT_PLAIN_VEC; ++j) v[j] = v[j] + d[j];
        }
        if (a.sum_out != nullptr) {
            if (whole) {
                __builtin_memcpy(a.sum_out + e0, v, 16);
                __builtin_memcpy(a.sum_out + e0 + 4, v + 4, 16);
            } else {
                for (int j = 0; j < cnt; ++j) a.sum_out[e0 + j] = v[j];
            }
        }
        // plane and channel of the group's first element once, then walked
        const int64_t pl = e0 / a.P;
        int rem = (int)(e0 - pl * a.P), c0 = (int)(pl % a.C);
        int ch[PREACT_PLAIN_VEC];
        {
            int c = c0;
#pragma unroll
            for (int j = 0; j < PREACT_PLAIN_VEC; ++j) {
                ch[j] = c;
                if (++rem == a.P) {
                    rem = 0;
                    c = c + 1 == a.C ? 0 : c + 1;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < PREACT_PLAIN_VEC; ++j)
            if (j < cnt) v[j] = preact_value(v[j], a.alpha[ch[j]], a.shift[ch[j]]);
        if (a.act_out != nullptr) {
            if (whole) {
                __builtin_memcpy(a.act_out + e0, v, 16);
                __builtin_memcpy(a.act_out + e0 + 4, v + 4, 16);
            } else {
                for (int j = 0; j < cnt; ++j) a.act_out[e0 + j] = v[j];
            }
        }
        for (int i = 0; i < a.n_out; ++i) {
            const QeRq &q = a.q[i];
            const int nbits = a.n_bits[i];
            uint64_t bits = 0;
#pragma unroll
            for (int j = 0; j < PREACT_PLAIN_VEC; ++j) {
                if (j < cnt) {
                    const int ci = a.rq_pt[i] ? 0 : ch[j];
                    bits |= (uint64_t)qe_rq_code(v[j], q.scale[ci], q.zero[ci], q, bad) << (j * nbits);
                }
            }
            uint8_t *dst = a.codes[i] + g * nbits;                       // 8 elements fill n_bits whole bytes
            const int nb = (cnt * nbits + 7) >> 3;                       // the last group: the stream ends inside it
            if (nb == 8) __builtin_memcpy(dst, &bits, 8);
            else for (int b = 0; b < nb; ++b) dst[b] = (uint8_t)(bits >> (8 * b));
        }
    }
    if (a.n_out > 0) preact_report(a, bad);
}

// the instances by the plan's kernel number
static constexpr SpanLaunch<PreactArgs> kPreactInstances[] = {&launch_instance<&preact_plain_kernel, PreactArgs>,
                                                              &launch_instance<&preact_fast_kernel, PreactArgs>};
static_assert(sizeof(kPreactInstances) / sizeof(kPreactInstances[0]) == PREACT_KERNELS, "one launcher per instance number");

int launch_preact(const PreactPlan &p, const float *x, const float *identity, int N, int C, int P, const float *alpha, const float *shift,
                  int n_out, const qe_requant *rq, uint8_t *const *codes, float *sum_out, float *act_out, int32_t *status, hipStream_t s)
{
    if (p.kernel < 0 || p.kernel >= PREACT_KERNELS) return QE_ERR_UNSUPPORTED;
    PreactArgs a;
    a.x = x; a.identity = identity; a.alpha = alpha; a.shift = shift; a.sum_out = sum_out; a.act_out = act_out;
    a.status = status; a.n_out = n_out; a.C = C; a.P = P;
    a.n = (int64_t)N * C * P;
    for (int i = 0; i < PREACT_MAX_OUT; ++i) {
        const bool on = i < n_out;
        a.codes[i] = on ? codes[i] : nullptr;
        a.rq[i] = make_rq_args(on && rq[i].n_bits == 8 ? &rq[i] : nullptr, a.codes[i], status);
        a.q[i] = on ? make_qe_rq(rq[i]) : QeRq{nullptr, nullptr, 0.0f, 0.0f, 0.0f, 0.0f, 0u, 0u};
        a.n_bits[i] = on ? rq[i].n_bits : 8;
        a.rq_pt[i] = !on || rq[i].n_param == 1;
    }
    kPreactInstances[p.kernel]((unsigned)p.blocks, PREACT_THREADS, 0, 0, s, a);
    QE_LAUNCH_CHECK();
    return QE_OK;
}

}  // namespace qe
