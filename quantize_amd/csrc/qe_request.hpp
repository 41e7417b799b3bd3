// qe_request.hpp -- what a request check of the C ABI needs, once: the bit-width and operand tests, the stored-code range of
// (n_bits, sign), the aliasing pieces and the pool window.  Plain C++17 on quant_engine.h and the standard headers, nothing
// from HIP: the entry points of every .hip file, the torch binding and tools/check_request_host.cpp read the same lines.
// The ORDER inside a check decides which code a caller sees (tests/test_api_refusals_cpu.py pins it).
#pragma once
#include <stdint.h>
#include "../../include/quant_engine.h"

namespace qe {

// ---- operands ------------------------------------------------------------------------------------------------------------
inline bool bits_ok(int n_bits) { return n_bits > 0 && n_bits <= 8; }

// null pointers, then n_bits
inline int check_operand(const qe_qparam *q)
{
    if (q == nullptr || q->data == nullptr || q->scale == nullptr || q->zero == nullptr) return QE_ERR_ARG;
    return bits_ok(q->n_bits) ? QE_OK : QE_ERR_NBITS;
}
// ... then n_param < 1
inline int check_qparam(const qe_qparam *q)
{
    const int rc = check_operand(q);
    if (rc != QE_OK) return rc;
    return q->n_param < 1 ? QE_ERR_ARG : QE_OK;
}
inline int check_requant(const qe_requant *rq)
{
    if (rq == nullptr || rq->scale == nullptr || rq->zero == nullptr) return QE_ERR_ARG;
    if (!bits_ok(rq->n_bits)) return QE_ERR_NBITS;
    return rq->n_param < 1 ? QE_ERR_ARG : QE_OK;
}
// one scale, or one per channel
inline bool one_or_per_channel(int64_t n_param, int64_t channels) { return n_param == 1 || n_param == channels; }

// ---- the stored code of (n_bits, sign) (tpack.cu:108-111) ------------------------------------------------------------------
// stored code = (q + offset) & mask; [lo, hi] is the representable range of q (tpack's range test).  n_bits in 1 .. 8.
struct CodeRange {
    unsigned offset, mask;
    float lo, hi;
};
inline CodeRange code_range(int n_bits, int sign)
{
    CodeRange r;
    r.offset = sign ? (1u << (n_bits - 1)) : 0u;
    r.mask = (1u << n_bits) - 1u;
    r.lo = sign ? -(float)(1 << (n_bits - 1)) : 0.0f;
    r.hi = sign ? (float)((1 << (n_bits - 1)) - 1) : (float)((1 << n_bits) - 1);
    return r;
}

// ---- aliasing --------------------------------------------------------------------------------------------------------------
struct Span { uintptr_t lo, hi; };
inline Span span_of(const void *p, int64_t bytes) { return Span{reinterpret_cast<uintptr_t>(p), reinterpret_cast<uintptr_t>(p) + (uintptr_t)bytes}; }
// a null span overlaps nothing; neither do two spans that only touch
inline bool overlaps(const Span &a, const Span &b) { return a.lo != 0 && b.lo != 0 && a.lo < b.hi && b.lo < a.hi; }

// no output overlaps an operand or another output
inline bool outputs_clear(const Span *outs, int n_outs, const Span *ins, int n_ins)
{
    for (int i = 0; i < n_outs; ++i) {
        for (int j = 0; j < n_ins; ++j)
            if (overlaps(outs[i], ins[j])) return false;
        for (int j = i + 1; j < n_outs; ++j)
            if (overlaps(outs[i], outs[j])) return false;
    }
    return true;
}

// two buffers of `bytes` each: the same address (in place) or disjoint
inline bool same_or_disjoint(const void *a, const void *b, int64_t bytes) { return a == b || !overlaps(span_of(a, bytes), span_of(b, bytes)); }

// ---- pool window -----------------------------------------------------------------------------------------------------------
// a kernel x kernel window at `stride` over (N, C, H, W) planes padded by `padding` (at most half the window, as torch asks):
// QE_OK and the output plane, or QE_ERR_ARG
inline int check_pool_window(int N, int C, int H, int W, int kernel, int stride, int padding, int &OH, int &OW)
{
    if (N < 0 || C < 0 || H <= 0 || W <= 0 || kernel <= 0 || stride <= 0 || padding < 0 || 2 * padding > kernel) return QE_ERR_ARG;
    OH = (H + 2 * padding - kernel) / stride + 1;
    OW = (W + 2 * padding - kernel) / stride + 1;
    if (H + 2 * padding < kernel || W + 2 * padding < kernel || OH <= 0 || OW <= 0) return QE_ERR_ARG;
    return QE_OK;
}

}  // namespace qe
