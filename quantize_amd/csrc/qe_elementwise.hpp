// qe_elementwise.hpp -- per-element device arithmetic shared by the quantise+pack kernels (qe_tpack.hip), the linear
// epilogues (qe_linear.hip) and the ViT kernels (qe_layernorm.hip).  A fused epilogue and the two-pass form it replaces
// call the SAME functions here, which is what makes them bit-identical.
#pragma once
#include "qe_common.h"

namespace qe {

// (char)x of tpack.cu:50 for in-range values, plus the range test of tpack.cu:211-215
// evaluated on the value as float (x.min().item<float>()).
template <typename T>
__device__ __forceinline__ unsigned tp_code(T v, float lo, float hi, unsigned offset, unsigned mask, bool &bad)
{
    const float f = (float)v;
    bad |= !(f >= lo && f <= hi);  // NaN fails both comparisons, like TORCH_CHECK
    const int iv = (int)v;         // truncation toward zero == (char)v while in range
    return ((unsigned)iv + offset) & mask;
}

// Fused activation quantisation: the Quantizer's
//   q = round(x / scale - zero).clamp(qmin, qmax)      (modelzoo/modules/quantizer.py:31, :215; zero in the MODULE's
// convention, i.e. subtracted here and added back on dequantisation) in front of the packer, so the fp32 integer-valued
// tensor the reference materialises between Quantizer and tpack (4 B/element written + read again) never exists.
// Same fp32 operations in the same order as torch: IEEE division, subtraction, round-half-even, clamp (NaN passes
// through the clamp and trips the range flag like it trips CHECK_RANGE).
__device__ __forceinline__ float tp_quantize(float v, float sc, float zr, float qmin, float qmax)
{
    const float r = rintf(v / sc - zr);
    return (r != r) ? r : fminf(fmaxf(r, qmin), qmax);
}

// torchvision's nn.GELU() (approximate='none'), written as torch's kernel writes it: x * 0.5 * (1 + erf(x / sqrt(2))) in fp32.
__device__ __forceinline__ float qe_gelu(float x)
{
    return x * 0.5f * (1.0f + erff(x * (float)M_SQRT1_2));
}

template <int ACT>
__device__ __forceinline__ float qe_act(float x)
{
    if constexpr (ACT == QE_ACT_GELU) return qe_gelu(x);
    else return x;
}

// One per-tensor consumer quantiser, everything an epilogue needs (8-bit or narrower stored codes).
struct QeRq {
    const float *scale, *zero;
    float qmin, qmax, lo, hi;    // clamp; representable range of the stored code (tpack's range test)
    unsigned offset, mask;       // stored code = (q + offset) & mask
};

// the kernel operand of the C ABI's quantiser, as qe_quantize_pack describes its codes
inline QeRq make_qe_rq(const qe_requant &r)
{
    const CodeRange cr = code_range(r.n_bits, r.sign);
    return QeRq{r.scale, r.zero, r.qmin, r.qmax, cr.lo, cr.hi, cr.offset, cr.mask};
}

// v -> stored code of a per-tensor quantiser with the arithmetic of qe_quantize_pack (bit-identical)
__device__ __forceinline__ unsigned qe_rq_code(float v, float sc, float zr, const QeRq &q, bool &bad)
{
    return tp_code<float>(tp_quantize(v, sc, zr, q.qmin, q.qmax), q.lo, q.hi, q.offset, q.mask, bad);
}

}  // namespace qe
