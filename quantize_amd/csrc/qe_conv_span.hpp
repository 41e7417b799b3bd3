// qe_conv_span.hpp -- what the kernels on contiguous spans of NCHW byte planes share (the depthwise kernels of
// qe_conv_dw.hip and the grouped kernels of qe_conv_grp.hip): the operand half of their kernel argument, the pieces of their
// arithmetic (zero split, float half of the sum, border classes, ReLU, the consumer's quantiser at a channel) and the bodies of
// the 16-byte chunk copies.  The loops around the chunk bodies, the staging order, the re-centring and the epilogues' f
// formulas stay with each kernel.
#pragma once
#include "qe_conv_common.hpp"

namespace qe {

// ---- the operands of a kernel argument -----------------------------------------------------------------------------------
struct SpanOperands {
    const uint8_t *x, *w;
    const float *xs, *xz, *ws, *wz, *bias;
    float *out;
    RqArgs rq;                 // rq.out: the 8-bit codes (NULL: none)
    int x_pt, w_pt, rq_pt;     // per tensor
    int x_bits, x_sign, w_bits, w_sign;
    int N;                     // the batch closes the block: with it DwArgs and GrpArgs keep the layout they had on their own, and
};                             // a moved field (relu was tried) compiles all 32 kernels to other code

inline SpanOperands span_operands(const qe_qparam *x, const qe_qparam *w, const float *bias, int N, float *out, const qe_requant *rq,
                                  uint8_t *codes, int32_t *status)
{
    SpanOperands a;
    a.x = x->data; a.w = w->data;
    a.xs = x->scale; a.xz = x->zero; a.ws = w->scale; a.wz = w->zero; a.bias = bias;
    a.out = out;
    a.rq = make_rq_args(rq, codes, status);
    a.x_pt = x->n_param == 1; a.w_pt = w->n_param == 1; a.rq_pt = rq == nullptr || rq->n_param == 1;
    a.x_bits = x->n_bits; a.x_sign = x->sign; a.w_bits = w->n_bits; a.w_sign = w->sign;
    a.N = N;
    return a;
}

// a row of a family's instance table, indexed by the plan's kernel number: launch_instance<&kernel, Args> (qe_common.h)
template <class Args>
using SpanLaunch = void (*)(unsigned blocks, unsigned threads, size_t lds, size_t lds_attr, hipStream_t s, const Args &a);

constexpr int round16(int v) { return (v + 15) & ~15; }

// ---- arithmetic ------------------------------------------------------------------------------------------------------------
// zero point -> integer part (less `shift`) and remainder; a zero that is NaN or beyond +-1024 keeps its value in the remainder
__device__ __forceinline__ void span_split_zero(float z, int shift, int &zi, float &dz)
{
    if (fabsf(z) <= 1024.0f) {
        const float r = rintf(z);
        zi = (int)r - shift;
        dz = z - r;
    } else {
        zi = -shift;
        dz = z;
    }
}

__device__ __forceinline__ float span_relu(float v) { return (v > 0.0f || v != v) ? v : 0.0f; }   // torch.relu: NaN passes

// the consumer's quantiser of channel idx (0: per tensor)
__device__ __forceinline__ RqConst span_rq_setup(const RqArgs &a, int idx)
{
    RqArgs t = a;
    t.scale = a.scale + idx;
    t.zero = a.zero + idx;
    return rq_setup(t);
}

// the float half of the sum, shared by the fast and the plain kernels: B = sum (qw - zwi), n products
__device__ __forceinline__ float span_cf(int n, int B, float dzx, float dzw) { return fmaf((float)n * dzx, dzw, -dzx * (float)B); }

// border classes of a 3x3, padding 1 window: bit 0 top, 1 bottom, 2 left, 3 right taps out of bounds
__device__ __forceinline__ bool span_tap_off(int cls, int kh, int kw)
{
    return (kh == 0 && (cls & 1)) || (kh == 2 && (cls & 2)) || (kw == 0 && (cls & 4)) || (kw == 2 && (cls & 8));
}
__device__ __forceinline__ int span_row_cls(int oh, int S, int H) { return (oh * S - 1 < 0 ? 1 : 0) | (oh * S + 1 >= H ? 2 : 0); }
__device__ __forceinline__ int span_out_cls(int row_cls, int ow, int S, int W) { return row_cls | (ow == 0 ? 4 : 0) | (ow * S + 1 >= W ? 8 : 0); }

// ---- 16-byte chunks on 16-byte aligned addresses -----------------------------------------------------------------------------
// the chunk at src, raw bytes; outside [x_lo, x_hi) (the tensor) nothing is read and the bytes are 0
__device__ __forceinline__ uint4 span_load16(const uint8_t *src, const uint8_t *x_lo, const uint8_t *x_hi)
{
    uint4 v;
    if (src >= x_lo && src + 16 <= x_hi) {
        v = *reinterpret_cast<const uint4 *>(src);
    } else {
        unsigned d[4] = {0, 0, 0, 0};
        for (int b = 0; b < 16; ++b)
            if (src + b >= x_lo && src + b < x_hi) d[b >> 2] |= (unsigned)src[b] << (8 * (b & 3));
        v = make_uint4(d[0], d[1], d[2], d[3]);
    }
    return v;
}

// the chunk at dst, inside [lo, hi) (the span) only: whole, else word by word, else byte by byte (codes)
__device__ __forceinline__ void span_store16_bytes(uint8_t *dst, const uint4 v, const uint8_t *lo, const uint8_t *hi)
{
    if (dst >= lo && dst + 16 <= hi) {
        *reinterpret_cast<uint4 *>(dst) = v;
    } else {
        const unsigned d[4] = {v.x, v.y, v.z, v.w};
        for (int q = 0; q < 4; ++q) {
            uint8_t *dq = dst + 4 * q;
            if (dq >= lo && dq + 4 <= hi) {
                *reinterpret_cast<unsigned *>(dq) = d[q];
            } else {
                for (int b = 0; b < 4; ++b)
                    if (dq + b >= lo && dq + b < hi) dq[b] = (uint8_t)(d[q] >> (8 * b));
            }
        }
    }
}

// the same for a span of whole words (fp32)
__device__ __forceinline__ void span_store16_words(uint8_t *dst, const uint4 v, const uint8_t *lo, const uint8_t *hi)
{
    if (dst >= lo && dst + 16 <= hi) {
        *reinterpret_cast<uint4 *>(dst) = v;
    } else {
        const unsigned d[4] = {v.x, v.y, v.z, v.w};
        for (int q = 0; q < 4; ++q)
            if (dst + 4 * q >= lo && dst + 4 * q + 4 <= hi) *reinterpret_cast<unsigned *>(dst + 4 * q) = d[q];
    }
}

}  // namespace qe
