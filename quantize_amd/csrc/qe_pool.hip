// qe_pool.hip -- the quantised ReLU and pooling layers.
//
// Module forms (fp32 NCHW in, fp32 out): the packed forwards of the reference's QuantReLU, QuantMaxPool2d and
// QuantAdaptiveAvgPool2d in one pass each -- qdq(v) = (clamp(rint(v / scale - zero), qmin, qmax) + zero) * scale per element, then
// relu, the window maximum or the window mean.  Codes-domain form: qe_avgpool2d_codes, a windowed average of 8-bit stored codes
// with the consumer's quantiser fused (rq_value of qe_conv_common.hpp, qe_rq_code of qe_elementwise.hpp: the arithmetic of
// qe_quantize_pack), in three instances that the host-side plan (qe_pool.hpp) picks.
//
// At the end of the file, with their entry points: the two older pooling kernels, qe_global_avgpool (fp32 planes) and
// qe_maxpool2d_codes (8-bit codes).
//
// The contracts are fp32 operation SEQUENCES (include/quant_engine.h), so nothing in this file may be contracted into an fma.
#include "qe_pool.hpp"
#include "qe_conv_span.hpp"
#include "qe_elementwise.hpp"

#pragma clang fp contract(off)

namespace qe {

// ---- shared arithmetic -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float pool_qdq(float v, float sc, float zr, float qmin, float qmax)
{
    return (tp_quantize(v, sc, zr, qmin, qmax) + zr) * sc;
}

// y of a window without ReLU from its exact integer sum S of q
__device__ __forceinline__ float pool_value(float sc, float zp, int S, int cnt)
{
    const float fc = (float)cnt;
    const float t = fc * zp;
    const float d = (float)S - t;
    const float m = sc * d;
    return m / fc;
}

// y of a window with ReLU from the fp32 sum R of its taps
__device__ __forceinline__ float pool_relu_value(float sc, float R, int cnt)
{
    const float m = sc * R;
    return m / (float)cnt;
}

// one tap under ReLU, in fp32: q the decoded code
__device__ __forceinline__ float pool_relu_tap(int q, float zp) { return span_relu((float)q - zp); }

// the x operand at a plane: scale, zero', and the integer shortcut of the ReLU sum (zb: zero' in stored-code units)
struct PoolQ {
    float sc, zp;
    int off, zb;
    bool int_ok;
};

struct PoolArgs {
    const uint8_t *x;
    const float *xs, *xz;
    float *out;
    RqArgs rq;                 // rq.out: the codes (NULL: none)
    QeRq q;                    // the sub-8-bit consumer (plain kernel, vec 8)
    int n_bits;
    int x_pt, x_sign, rq_pt;
    int C, H, W, OH, OW, kernel, stride, relu;
    int T, logT, ncx;
    int64_t NP;
};

__device__ __forceinline__ PoolQ pool_xq(const PoolArgs &a, int c, int cnt)
{
    PoolQ q;
    q.sc = a.xs[a.x_pt ? 0 : c];
    q.zp = a.xz[a.x_pt ? 0 : c];
    q.off = a.x_sign ? 128 : 0;
    q.int_ok = fabsf(q.zp) <= 256.0f && q.zp == rintf(q.zp) && (int64_t)cnt * 512 < (1 << 24);
    q.zb = q.int_ok ? (int)q.zp + q.off : 0;
    return q;
}

// a window of the plane at xp, tap by tap: every instance's definition, and what the plain kernel runs
__device__ __forceinline__ float pool_window(const PoolArgs &a, const uint8_t *xp, const PoolQ &q, int h0, int h1, int w0, int w1)
{
    const int cnt = (h1 - h0) * (w1 - w0);
    if (!a.relu) {
        int S = 0;
        for (int ih = h0; ih < h1; ++ih)
            for (int iw = w0; iw < w1; ++iw) S += (int)xp[ih * a.W + iw];
        return pool_value(q.sc, q.zp, S - q.off * cnt, cnt);
    }
    if (q.int_ok) {
        int R = 0;
        for (int ih = h0; ih < h1; ++ih)
            for (int iw = w0; iw < w1; ++iw) R += max((int)xp[ih * a.W + iw] - q.zb, 0);
        return pool_relu_value(q.sc, (float)R, cnt);
    }
    float R = 0.0f;
    for (int ih = h0; ih < h1; ++ih)
        for (int iw = w0; iw < w1; ++iw) R += pool_relu_tap((int)xp[ih * a.W + iw] - q.off, q.zp);
    return pool_relu_value(q.sc, R, cnt);
}

// ---- plain: one thread per output (V == 1), or per 8 consecutive outputs whose sub-8-bit codes fill whole bytes (V == 8) --------
template <int V>
__global__ __launch_bounds__(POOL_THREADS) void pool_plain_kernel(const PoolArgs a)
{
    const int64_t OHW = (int64_t)a.OH * a.OW, n = a.NP * OHW;
    const int64_t o0 = ((int64_t)blockIdx.x * POOL_THREADS + threadIdx.x) * V;
    bool bad = false;
    if (o0 < n) {
        int64_t p = o0 / OHW;
        const int rem = (int)(o0 - p * OHW);
        int oh = rem / a.OW, ow = rem - oh * a.OW;
        uint64_t bits = 0;
        int made = 0;
#pragma unroll 1
        for (int j = 0; j < V && o0 + j < n; ++j) {
            const int c = (int)(p % a.C);
            int h0, h1, w0, w1;
            if (a.kernel > 0) {
                h0 = oh * a.stride; h1 = h0 + a.kernel; w0 = ow * a.stride; w1 = w0 + a.kernel;
            } else {
                h0 = pool_win_lo(oh, a.H, a.OH); h1 = pool_win_hi(oh, a.H, a.OH);
                w0 = pool_win_lo(ow, a.W, a.OW); w1 = pool_win_hi(ow, a.W, a.OW);
            }
            const PoolQ q = pool_xq(a, c, (h1 - h0) * (w1 - w0));
            const float y = pool_window(a, a.x + p * a.H * a.W, q, h0, h1, w0, w1);
            if (a.out != nullptr) a.out[o0 + j] = y;
            if (a.rq.out != nullptr) {
                if constexpr (V == 1) {
                    const RqConst rc = span_rq_setup(a.rq, a.rq_pt ? 0 : c);
                    a.rq.out[o0] = (uint8_t)(unsigned)rq_value(rc, y, bad);
                } else {
                    const int ci = a.rq_pt ? 0 : c;
                    bits |= (uint64_t)qe_rq_code(y, a.q.scale[ci], a.q.zero[ci], a.q, bad) << (j * a.n_bits);
                }
            }
            ++made;
            if (++ow == a.OW) {
                ow = 0;
                if (++oh == a.OH) { oh = 0; ++p; }
            }
        }
        if constexpr (V != 1) {
            if (a.rq.out != nullptr) {
                uint8_t *dst = a.rq.out + (o0 / 8) * a.n_bits;           // 8 elements fill n_bits whole bytes
                const int nb = (made * a.n_bits + 7) >> 3;
                for (int b = 0; b < nb; ++b) dst[b] = (uint8_t)(bits >> (8 * b));
            }
        }
    }
    if (a.rq.out != nullptr) rq_report(a.rq, bad);
}

// ---- pair: kernel == stride == 2.  A thread makes 16 adjacent outputs of a row from 32 bytes of each of its two input rows ------
// 16-byte pieces at whatever alignment the row has (the hardware splits a piece that straddles a line).  A ragged last chunk of a
// row loads the same 32 bytes while they lie inside the tensor and writes its own outputs one by one: nothing outside the tensors
// is touched.
__global__ __launch_bounds__(POOL_THREADS) void pool_pair_kernel(const PoolArgs a)
{
    const int64_t t = (int64_t)blockIdx.x * POOL_THREADS + threadIdx.x;
    bool bad = false;
    if (t < a.NP * a.OH * a.ncx) {
        const int64_t prow = t / a.ncx;                                   // plane * OH + oh
        const int cx = (int)(t - prow * a.ncx);
        const int64_t p = prow / a.OH;
        const int oh = (int)(prow - p * a.OH);
        const int c = (int)(p % a.C);
        const int ow0 = cx * POOL_PAIR_VEC;
        const int nv = min(POOL_PAIR_VEC, a.OW - ow0);
        const uint8_t *r0 = a.x + p * a.H * a.W + (int64_t)(2 * oh) * a.W + 2 * ow0, *r1 = r0 + a.W;
        uint32_t w0[8], w1[8];
        // 32 bytes of each row: past a ragged chunk's own 2 * nv bytes they are the next rows' (unused); only where they would
        // leave the tensor -- its last rows -- the chunk reads its own bytes one by one
        if (r1 + 32 <= a.x + a.NP * a.H * a.W) {
            uint4 v[4];
            __builtin_memcpy(&v[0], r0, 16);
            __builtin_memcpy(&v[1], r0 + 16, 16);
            __builtin_memcpy(&v[2], r1, 16);
            __builtin_memcpy(&v[3], r1 + 16, 16);
            __builtin_memcpy(w0, &v[0], 32);
            __builtin_memcpy(w1, &v[2], 32);
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                uint32_t d0 = 0, d1 = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if (4 * k + b < 2 * nv) {
                        d0 |= (uint32_t)r0[4 * k + b] << (8 * b);
                        d1 |= (uint32_t)r1[4 * k + b] << (8 * b);
                    }
                w0[k] = d0; w1[k] = d1;
            }
        }
        const PoolQ q = pool_xq(a, c, 4);
        float y[POOL_PAIR_VEC];
#pragma unroll
        for (int j = 0; j < POOL_PAIR_VEC; ++j) {
            const uint32_t d0 = w0[j >> 1], d1 = w1[j >> 1];
            if (!a.relu) {
                const uint32_t sel = (j & 1) ? 0x01010000u : 0x00000101u;           // the two bytes of this output's columns
                int S = (int)__builtin_amdgcn_udot4(d0, sel, 0u, false);
                S = (int)__builtin_amdgcn_udot4(d1, sel, (uint32_t)S, false);
                y[j] = pool_value(q.sc, q.zp, S - 4 * q.off, 4);
            } else {
                const int sh = 16 * (j & 1);
                const int b00 = (d0 >> sh) & 0xff, b01 = (d0 >> (sh + 8)) & 0xff, b10 = (d1 >> sh) & 0xff, b11 = (d1 >> (sh + 8)) & 0xff;
                if (q.int_ok) {
                    const int R = max(b00 - q.zb, 0) + max(b01 - q.zb, 0) + max(b10 - q.zb, 0) + max(b11 - q.zb, 0);
                    y[j] = pool_relu_value(q.sc, (float)R, 4);
                } else {
                    float R = 0.0f;
                    R += pool_relu_tap(b00 - q.off, q.zp);
                    R += pool_relu_tap(b01 - q.off, q.zp);
                    R += pool_relu_tap(b10 - q.off, q.zp);
                    R += pool_relu_tap(b11 - q.off, q.zp);
                    y[j] = pool_relu_value(q.sc, R, 4);
                }
            }
        }
        const int64_t o = prow * a.OW + ow0;
        if (a.out != nullptr) {
            if (nv == POOL_PAIR_VEC) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float4 v = make_float4(y[4 * k], y[4 * k + 1], y[4 * k + 2], y[4 * k + 3]);
                    __builtin_memcpy(a.out + o + 4 * k, &v, 16);
                }
            } else {
#pragma unroll
                for (int j = 0; j < POOL_PAIR_VEC; ++j)
                    if (j < nv) a.out[o + j] = y[j];
            }
        }
        if (a.rq.out != nullptr) {
            const RqConst rc = span_rq_setup(a.rq, a.rq_pt ? 0 : c);
            uint32_t cw[4] = {0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < POOL_PAIR_VEC; ++j)
                if (j < nv) cw[j >> 2] |= ((unsigned)rq_value(rc, y[j], bad) & 0xffu) << (8 * (j & 3));
            if (nv == POOL_PAIR_VEC) {
                const uint4 v = make_uint4(cw[0], cw[1], cw[2], cw[3]);
                __builtin_memcpy(a.rq.out + o, &v, 16);
            } else {
#pragma unroll
                for (int j = 0; j < POOL_PAIR_VEC; ++j)
                    if (j < nv) a.rq.out[o + j] = (uint8_t)(cw[j >> 2] >> (8 * (j & 3)));
            }
        }
    }
    if (a.rq.out != nullptr) rq_report(a.rq, bad);
}

// ---- plane: the window is the whole plane.  T = 2^logT lanes share a plane and read its aligned 16-byte pieces (span_load16:
// bytes outside the plane read as 0 and are not loaded at the tensor's ends), 256 / T consecutive planes per workgroup: a wave's
// loads cover one contiguous stretch of the tensor.  Partial sums are exact integers and meet by shuffles; lane 0 of the plane
// finishes.  A ReLU sum whose zero' is no small integer is the fp32 sequence of the contract: lane 0 adds it up alone.
__global__ __launch_bounds__(POOL_THREADS) void pool_plane_kernel(const PoolArgs a)
{
    const int g = threadIdx.x >> a.logT, l = threadIdx.x & (a.T - 1);
    const int64_t p = (int64_t)blockIdx.x * (POOL_THREADS >> a.logT) + g;
    const bool live = p < a.NP;
    const int P = a.H * a.W;
    const int c = live ? (int)(p % a.C) : 0;
    const PoolQ q = pool_xq(a, c, P);
    const bool seq = a.relu && !q.int_ok;
    int S = 0;
    const uint8_t *lo = a.x + (live ? p : 0) * P, *hi = lo + P;
    if (live && !seq) {
        const uint8_t *A = lo - (reinterpret_cast<uintptr_t>(lo) & 15);
        const int chunks = (int)((hi - A + 15) >> 4);
        for (int i = l; i < chunks; i += a.T) {
            const uint8_t *src = A + 16 * i;
            const uint4 v = span_load16(src, lo, hi);
            const uint32_t d[4] = {v.x, v.y, v.z, v.w};
            if (!a.relu) {
#pragma unroll
                for (int k = 0; k < 4; ++k) S = (int)__builtin_amdgcn_udot4(d[k], 0x01010101u, (uint32_t)S, false);
            } else {
#pragma unroll
                for (int b = 0; b < 16; ++b)
                    if (src + b >= lo && src + b < hi) S += max((int)((d[b >> 2] >> (8 * (b & 3))) & 0xff) - q.zb, 0);
            }
        }
    }
    for (int m = 1; m < a.T; m <<= 1) S += __shfl_xor(S, m);
    bool bad = false;
    if (live && l == 0) {
        float y;
        if (!a.relu) {
            y = pool_value(q.sc, q.zp, S - q.off * P, P);
        } else if (!seq) {
            y = pool_relu_value(q.sc, (float)S, P);
        } else {
            float R = 0.0f;
            for (int i = 0; i < P; ++i) R += pool_relu_tap((int)lo[i] - q.off, q.zp);
            y = pool_relu_value(q.sc, R, P);
        }
        if (a.out != nullptr) a.out[p] = y;
        if (a.rq.out != nullptr) {
            const RqConst rc = span_rq_setup(a.rq, a.rq_pt ? 0 : c);
            a.rq.out[p] = (uint8_t)(unsigned)rq_value(rc, y, bad);
        }
    }
    if (a.rq.out != nullptr) rq_report(a.rq, bad);
}

// the instances by the plan's kernel number; the plain kernel has the two vector widths
static constexpr SpanLaunch<PoolArgs> kPoolInstances[] = {
    &launch_instance<&pool_plain_kernel<1>, PoolArgs>, &launch_instance<&pool_pair_kernel, PoolArgs>,
    &launch_instance<&pool_plane_kernel, PoolArgs>};
static_assert(sizeof(kPoolInstances) / sizeof(kPoolInstances[0]) == POOL_KERNELS, "one launcher per instance number");

int launch_pool_codes(const PoolPlan &p, const qe_qparam *x, int N, int C, int H, int W, int kernel, int stride, int relu, float *out,
                      const qe_requant *rq, uint8_t *codes, int32_t *status, hipStream_t s)
{
    if (p.kernel < 0 || p.kernel >= POOL_KERNELS) return QE_ERR_UNSUPPORTED;
    PoolArgs a;
    a.x = x->data; a.xs = x->scale; a.xz = x->zero; a.out = out;
    a.x_pt = x->n_param == 1; a.x_sign = x->sign; a.rq_pt = rq == nullptr || rq->n_param == 1;
    a.rq = make_rq_args(rq, codes, status);
    a.q = rq != nullptr ? make_qe_rq(*rq) : QeRq{nullptr, nullptr, 0.0f, 0.0f, 0.0f, 0.0f, 0u, 0u};
    a.n_bits = rq != nullptr ? rq->n_bits : 8;
    a.C = C; a.H = H; a.W = W; a.OH = p.OH; a.OW = p.OW; a.kernel = kernel; a.stride = stride; a.relu = relu ? 1 : 0;
    a.T = p.T; a.logT = p.logT; a.ncx = p.ncx;
    a.NP = (int64_t)N * C;
    if (p.kernel == POOL_PLAIN && p.vec == POOL_SUB8_VEC)
        launch_instance<&pool_plain_kernel<POOL_SUB8_VEC>, PoolArgs>((unsigned)p.blocks, POOL_THREADS, 0, 0, s, a);
    else
        kPoolInstances[p.kernel]((unsigned)p.blocks, POOL_THREADS, 0, 0, s, a);
    QE_LAUNCH_CHECK();
    return QE_OK;
}

// ---- module forms -------------------------------------------------------------------------------------------------------------
// Threads own groups of 4 consecutive elements that start on a 16-byte boundary of OUT: `lead` = elements between that boundary
// and out, so group t is elements 4t - lead .. 4t - lead + 3 and every whole group is one aligned 16-byte store.  The loads are
// 16-byte pieces at x's own (4-byte) alignment.
struct QdqArgs {
    const float *x;
    float *out;
    const float *scale, *zero;
    int n_param;
    float qmin, qmax;
    int64_t n, inner;
    int lead;
    int C, H, W, OH, OW, kernel, stride, pad;
};

__global__ __launch_bounds__(POOL_THREADS) void quant_relu_kernel(const QdqArgs a)
{
    const int64_t e0 = ((int64_t)blockIdx.x * POOL_THREADS + threadIdx.x) * 4 - a.lead;
    if (e0 >= a.n) return;
    const int64_t first = e0 < 0 ? 0 : e0;
    int64_t row = a.n_param > 1 ? first / a.inner : 0;                    // element / inner, walked from the first one
    int64_t rem = a.n_param > 1 ? first - row * a.inner : 0;
    int c = a.n_param > 1 ? (int)(row % a.n_param) : 0;
    const bool whole = e0 >= 0 && e0 + 4 <= a.n;
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (whole) {
        __builtin_memcpy(v, a.x + e0, 16);
    } else {
        for (int j = 0; j < 4; ++j)
            if (e0 + j >= 0 && e0 + j < a.n) v[j] = a.x[e0 + j];
    }
    float sc = a.scale[c], zr = a.zero[c];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (e0 + j < 0) continue;
        v[j] = span_relu(pool_qdq(v[j], sc, zr, a.qmin, a.qmax));
        if (a.n_param > 1 && ++rem == a.inner) {
            rem = 0;
            c = c + 1 == a.n_param ? 0 : c + 1;
            sc = a.scale[c]; zr = a.zero[c];
        }
    }
    if (whole) {
        *reinterpret_cast<float4 *>(a.out + e0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int j = 0; j < 4; ++j)
            if (e0 + j >= 0 && e0 + j < a.n) a.out[e0 + j] = v[j];
    }
}

// the maximum of a window of raw taps, a NaN tap winning; mono: qdq once at the end, else tap by tap
__device__ __forceinline__ float quant_max_window(const QdqArgs &a, const float *xp, int oh, int ow, float sc, float zr)
{
    const int h0 = oh * a.stride - a.pad, w0 = ow * a.stride - a.pad;
    const int hlo = h0 < 0 ? 0 : h0, hhi = h0 + a.kernel < a.H ? h0 + a.kernel : a.H;
    const int wlo = w0 < 0 ? 0 : w0, whi = w0 + a.kernel < a.W ? w0 + a.kernel : a.W;
    const bool mono = sc > 0.0f;
    float m = -INFINITY, nan = 0.0f;
    bool any = false, has_nan = false;
    for (int ih = hlo; ih < hhi; ++ih)
        for (int iw = wlo; iw < whi; ++iw) {
            float v = xp[ih * a.W + iw];
            if (!mono) v = pool_qdq(v, sc, zr, a.qmin, a.qmax);
            if (v != v) { has_nan = true; nan = v; }
            else if (!any || v > m) m = v;
            any = true;
        }
    if (has_nan) m = nan;
    return mono ? pool_qdq(m, sc, zr, a.qmin, a.qmax) : m;
}

__global__ __launch_bounds__(POOL_THREADS) void quant_maxpool2d_kernel(const QdqArgs a)
{
    const int64_t e0 = ((int64_t)blockIdx.x * POOL_THREADS + threadIdx.x) * 4 - a.lead;
    if (e0 >= a.n) return;
    const int64_t first = e0 < 0 ? 0 : e0;
    const int64_t OHW = (int64_t)a.OH * a.OW;
    int64_t p = first / OHW;
    const int r = (int)(first - p * OHW);
    int oh = r / a.OW, ow = r - oh * a.OW;
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (e0 + j < 0 || e0 + j >= a.n) continue;
        const int c = a.n_param > 1 ? (int)(p % a.C) : 0;
        v[j] = quant_max_window(a, a.x + p * a.H * a.W, oh, ow, a.scale[c], a.zero[c]);
        if (++ow == a.OW) {
            ow = 0;
            if (++oh == a.OH) { oh = 0; ++p; }
        }
    }
    if (e0 >= 0 && e0 + 4 <= a.n) {
        *reinterpret_cast<float4 *>(a.out + e0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int j = 0; j < 4; ++j)
            if (e0 + j >= 0 && e0 + j < a.n) a.out[e0 + j] = v[j];
    }
}

// one thread per output: the contract's sequence, rows outer, columns inner
__global__ __launch_bounds__(POOL_THREADS) void quant_adaptive_avgpool2d_kernel(const QdqArgs a)
{
    const int64_t o = (int64_t)blockIdx.x * POOL_THREADS + threadIdx.x;
    if (o >= a.n) return;
    const int64_t OHW = (int64_t)a.OH * a.OW;
    const int64_t p = o / OHW;
    const int r = (int)(o - p * OHW);
    const int oh = r / a.OW, ow = r - oh * a.OW;
    const int c = a.n_param > 1 ? (int)(p % a.C) : 0;
    const float sc = a.scale[c], zr = a.zero[c];
    const int h0 = pool_win_lo(oh, a.H, a.OH), h1 = pool_win_hi(oh, a.H, a.OH);
    const int w0 = pool_win_lo(ow, a.W, a.OW), w1 = pool_win_hi(ow, a.W, a.OW);
    const float *xp = a.x + p * a.H * a.W;
    float sum = 0.0f;
    for (int ih = h0; ih < h1; ++ih)
        for (int iw = w0; iw < w1; ++iw) sum += pool_qdq(xp[ih * a.W + iw], sc, zr, a.qmin, a.qmax);
    a.out[o] = sum / (float)((h1 - h0) * (w1 - w0));
}

// The global case (OH == OW == 1): a workgroup takes 64 consecutive planes and walks them in tiles of up to 241 elements per
// plane: all 256 threads copy a tile into LDS with coalesced loads (planes of at most 241 elements: the 64 planes are one
// contiguous run, copied in 16-byte pieces, as global_avgpool_kernel does), then one thread per plane adds its tile up in the
// contract's order, the running sum staying in its register.  The row stride in LDS is odd: the 64 adding threads hit 64 banks.
constexpr int QAP_PLANES = 64, QAP_TILE = 241;
__global__ __launch_bounds__(POOL_THREADS) void quant_global_avgpool_kernel(const QdqArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float qap[];
    const int P = a.H * a.W;
    const int64_t plane0 = (int64_t)blockIdx.x * QAP_PLANES;
    const int np = (int)((a.n - plane0) < QAP_PLANES ? (a.n - plane0) : QAP_PLANES);
    const float *src = a.x + plane0 * P;
    const int64_t p = plane0 + threadIdx.x;
    const int c = (a.n_param > 1 && (int)threadIdx.x < np) ? (int)(p % a.C) : 0;
    const float sc = a.scale[c], zr = a.zero[c];
    const bool run = P <= QAP_TILE && (P & 1) && (reinterpret_cast<uintptr_t>(src) & 15) == 0;   // one contiguous, conflict-free run
    const int stride = run ? P : (P < QAP_TILE ? P : QAP_TILE) | 1;
    float sum = 0.0f;
    for (int t0 = 0; t0 < P; t0 += QAP_TILE) {
        const int tl = P - t0 < QAP_TILE ? P - t0 : QAP_TILE;
        if (run) {
            const int nf = np * P;
            for (int i = threadIdx.x * 4; i < nf; i += POOL_THREADS * 4) {
                if (i + 4 <= nf) *reinterpret_cast<float4 *>(qap + i) = *reinterpret_cast<const float4 *>(src + i);
                else for (int j = i; j < nf; ++j) qap[j] = src[j];
            }
        } else {
            for (int i = threadIdx.x; i < np * tl; i += POOL_THREADS) {
                const int pl = i / tl, e = i - pl * tl;
                qap[pl * stride + e] = src[(int64_t)pl * P + t0 + e];
            }
        }
        __syncthreads();
        if ((int)threadIdx.x < np)
            for (int i = 0; i < tl; ++i) sum += pool_qdq(qap[threadIdx.x * stride + i], sc, zr, a.qmin, a.qmax);
        __syncthreads();
    }
    if ((int)threadIdx.x < np) a.out[p] = sum / (float)P;
}

static QdqArgs qdq_args(const float *x, float *out, const qe_requant *rq, int64_t n)
{
    QdqArgs a = {};
    a.x = x; a.out = out; a.scale = rq->scale; a.zero = rq->zero; a.n_param = rq->n_param; a.qmin = rq->qmin; a.qmax = rq->qmax;
    a.n = n; a.inner = 1;
    a.lead = (int)((reinterpret_cast<uintptr_t>(out) & 15) >> 2);
    return a;
}

int launch_quant_relu(const float *x, int64_t n, int64_t inner, const qe_requant *rq, float *out, hipStream_t s)
{
    QdqArgs a = qdq_args(x, out, rq, n);
    a.inner = inner;
    const int64_t blocks = ceil_div64(ceil_div64(n + a.lead, 4), POOL_THREADS);
    if (blocks > 0x7fffffffLL) return QE_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(quant_relu_kernel, dim3((unsigned)blocks), dim3(POOL_THREADS), 0, s, a);
    QE_LAUNCH_CHECK();
    return QE_OK;
}

int launch_quant_maxpool2d(const float *x, int N, int C, int H, int W, int kernel, int stride, int padding, int OH, int OW,
                           const qe_requant *rq, float *out, hipStream_t s)
{
    QdqArgs a = qdq_args(x, out, rq, (int64_t)N * C * OH * OW);
    a.C = C; a.H = H; a.W = W; a.OH = OH; a.OW = OW; a.kernel = kernel; a.stride = stride; a.pad = padding;
    const int64_t blocks = ceil_div64(ceil_div64(a.n + a.lead, 4), POOL_THREADS);
    if (blocks > 0x7fffffffLL) return QE_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(quant_maxpool2d_kernel, dim3((unsigned)blocks), dim3(POOL_THREADS), 0, s, a);
    QE_LAUNCH_CHECK();
    return QE_OK;
}

int launch_quant_adaptive_avgpool2d(const float *x, int N, int C, int H, int W, int OH, int OW, const qe_requant *rq, float *out,
                                    hipStream_t s)
{
    QdqArgs a = qdq_args(x, out, rq, (int64_t)N * C * OH * OW);
    a.C = C; a.H = H; a.W = W; a.OH = OH; a.OW = OW;
    const int P = H * W;
    const size_t lds = (size_t)QAP_PLANES * ((P < QAP_TILE ? P : QAP_TILE) | 1) * sizeof(float);      // at most 61.7 KB
    if (OH == 1 && OW == 1) {
        const int64_t blocks = ceil_div64(a.n, QAP_PLANES);
        if (blocks > 0x7fffffffLL) return QE_ERR_UNSUPPORTED;
        hipLaunchKernelGGL(quant_global_avgpool_kernel, dim3((unsigned)blocks), dim3(POOL_THREADS), lds, s, a);
    } else {
        const int64_t blocks = ceil_div64(a.n, POOL_THREADS);
        if (blocks > 0x7fffffffLL) return QE_ERR_UNSUPPORTED;
        hipLaunchKernelGGL(quant_adaptive_avgpool2d_kernel, dim3((unsigned)blocks), dim3(POOL_THREADS), 0, s, a);
    }
    QE_LAUNCH_CHECK();
    return QE_OK;
}

}  // namespace qe

// ---------------------------------------------------------------------------------------------
// Global average pool (bench.py's top-1 tail): a workgroup copies 64 planes (64 * P contiguous floats) into LDS with
// coalesced 16-byte loads, then 4 threads per plane add up a quarter each (P is small: 49 for ResNet-50) and the
// quarters are combined with two shuffles.  HBM-bound: 103 MB for (256, 2048, 7, 7).
// ---------------------------------------------------------------------------------------------
namespace qe {
constexpr int AP_PLANES = 64;
__global__ __launch_bounds__(256) void global_avgpool_kernel(const float *__restrict__ x, float *__restrict__ out,
                                                             int64_t n_planes, int P)
{
    extern __shared__ __attribute__((aligned(16))) float sp[];
    const int64_t plane0 = (int64_t)blockIdx.x * AP_PLANES;
    const int np = (int)((n_planes - plane0) < AP_PLANES ? (n_planes - plane0) : AP_PLANES);
    const int nf = np * P;
    const float *src = x + plane0 * P;
    const bool al = (reinterpret_cast<uintptr_t>(src) & 15) == 0;
    if (al) {
        for (int i = threadIdx.x * 4; i < nf; i += 256 * 4) {
            if (i + 4 <= nf) *reinterpret_cast<float4 *>(sp + i) = *reinterpret_cast<const float4 *>(src + i);
            else for (int j = i; j < nf; ++j) sp[j] = src[j];
        }
    } else {
        for (int i = threadIdx.x; i < nf; i += 256) sp[i] = src[i];
    }
    __syncthreads();
    const int pl = threadIdx.x >> 2, part = threadIdx.x & 3;
    float sum = 0.0f;
    if (pl < np) {
        const int per = (P + 3) >> 2;
        const int lo = part * per, hi = (lo + per < P) ? lo + per : P;
        for (int i = lo; i < hi; ++i) sum += sp[pl * P + i];
    }
    sum += __shfl_xor(sum, 1);
    sum += __shfl_xor(sum, 2);
    if (pl < np && part == 0) out[plane0 + pl] = sum / (float)P;
}
}  // namespace qe

extern "C" int qe_global_avgpool(const float *x, int64_t n_planes, int32_t P, float *out, qe_stream_t stream)
{
    using namespace qe;
    if (n_planes < 0 || P <= 0) return QE_ERR_ARG;
    if (n_planes == 0) return QE_OK;
    if (x == nullptr || out == nullptr) return QE_ERR_ARG;
    if ((size_t)AP_PLANES * P * sizeof(float) > 60 * 1024) return QE_ERR_UNSUPPORTED;   // planes of at most 240 pixels
    const int64_t blocks = (n_planes + AP_PLANES - 1) / AP_PLANES;
    if (blocks > 0x7fffffffLL) return QE_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(global_avgpool_kernel, dim3((unsigned)blocks), dim3(256), (size_t)AP_PLANES * P * sizeof(float),
                       static_cast<hipStream_t>(stream), x, out, n_planes, (int)P);
    QE_LAUNCH_CHECK();
    return QE_OK;
}

// ---------------------------------------------------------------------------------------------
// Max pooling of 8-bit stored codes (the stem's MaxPool2d after its quantised ReLU).  The stored code (q, or q + 128 when
// signed) is order-preserving and the quantiser is non-decreasing, so max over codes == code of the max.  A thread makes
// 16 consecutive outputs of the flat (N, C, OH, OW) tensor and stores them as one 16-byte piece where it can; padding
// taps are skipped (torch pads with -inf).
// ---------------------------------------------------------------------------------------------
namespace qe {
__global__ __launch_bounds__(256) void maxpool2d_codes_kernel(const uint8_t *__restrict__ x, uint8_t *__restrict__ out, int64_t n_out,
                                                              int H, int W, int OH, int OW, int k, int stride, int pad, int vec)
{
    const int64_t o0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16;
    if (o0 >= n_out) return;
    // the first output's (plane, row, column) once (one 64-bit division per 16 outputs), then walked along the row
    const int64_t plane0 = o0 / ((int64_t)OH * OW);
    const int rem = (int)(o0 - plane0 * OH * OW);
    int oh = rem / OW, ow = rem - oh * OW;
    const uint8_t *xp = x + plane0 * H * W;
    uint8_t r[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        uint32_t m = 0;
        if (o0 + j < n_out) {
            const int h0 = oh * stride - pad, w0 = ow * stride - pad;
            const int hlo = h0 < 0 ? 0 : h0, hhi = h0 + k < H ? h0 + k : H;
            const int wlo = w0 < 0 ? 0 : w0, whi = w0 + k < W ? w0 + k : W;
            for (int ih = hlo; ih < hhi; ++ih)
                for (int iw = wlo; iw < whi; ++iw) m = max(m, (uint32_t)xp[ih * W + iw]);
        }
        r[j] = (uint8_t)m;
        if (++ow == OW) {
            ow = 0;
            if (++oh == OH) { oh = 0; xp += (int64_t)H * W; }
        }
    }
    if (vec && o0 + 16 <= n_out) {
        uint4 v;
        __builtin_memcpy(&v, r, 16);
        *reinterpret_cast<uint4 *>(out + o0) = v;
    } else {
        for (int j = 0; j < 16 && o0 + j < n_out; ++j) out[o0 + j] = r[j];
    }
}
}  // namespace qe

extern "C" int qe_maxpool2d_codes(const uint8_t *x, int32_t N, int32_t C, int32_t H, int32_t W, int32_t kernel, int32_t stride,
                                  int32_t padding, uint8_t *out, qe_stream_t stream)
{
    using namespace qe;
    int OH, OW;
    if (check_pool_window(N, C, H, W, kernel, stride, padding, OH, OW) != QE_OK) return QE_ERR_ARG;
    const int64_t n_out = (int64_t)N * C * OH * OW;
    if (n_out == 0) return QE_OK;
    if (x == nullptr || out == nullptr) return QE_ERR_ARG;
    const int64_t blocks = (n_out + 16 * 256 - 1) / (16 * 256);
    if (blocks > 0x7fffffffLL) return QE_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(maxpool2d_codes_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), x, out, n_out,
                       (int)H, (int)W, OH, OW, (int)kernel, (int)stride, (int)padding, (reinterpret_cast<uintptr_t>(out) & 15) == 0 ? 1 : 0);
    QE_LAUNCH_CHECK();
    return QE_OK;
}
