// qe_grp_common.hpp -- what the group-quantised (AWQ layout) units share: qe_linear_grp.hip (fp32 rows, bf16 matrix cores),
// qe_linear_grp_i8.hip and qe_conv_awq.hip (8-bit codes, int8 MFMA).  The host layer -- the weight operand's check and its
// side of fast eligibility, the int8 kernels' <WB, WZ, XZ> instance and its switch, the operand fields of a kernel argument,
// the launch tail -- and the device leaves of the two int8 units.  Each unit stays a translation unit of its own with its
// own kernels; a device piece lives here only while every kernel that uses it keeps its instruction stream (DESIGN.md,
// "Group-quantised (AWQ) kernels: one host layer, shared device pieces").
#pragma once
#include <type_traits>
#include "qe_common.h"

namespace qe {

// ---- host: the weight operand ------------------------------------------------------------------------------------------
// a group-quantised weight operand of O rows x K codes (a conv: OC x IC): the operand, then G, then one scale and zero per
// (row, group).  Every test after the operand's answers QE_ERR_ARG, so a caller's own QE_ERR_ARG tests may follow this one.
inline int check_grp_weights(const qe_qparam *w, int G, int K, int O)
{
    if (int rc = check_operand(w)) return rc;
    if (G <= 0 || K % G != 0) return QE_ERR_ARG;
    return (int64_t)w->n_param == (int64_t)O * (K / G) ? QE_OK : QE_ERR_ARG;
}

// the weight side of every fast kernel's eligibility; a plan ANDs its own conditions onto it
inline bool grp_weights_fast(const qe_qparam *w, int G)
{
    return (w->n_bits == 4 || w->n_bits == 8) && (G == 32 || G == 64 || G == 128) && aligned16(w->data);
}

// ---- host: the instance of an int8 fast kernel ---------------------------------------------------------------------------
struct GrpI8Instance {
    int w4;                 // 4-bit weight codes (else 8-bit)
    int wz, xz;             // residual weight / activation zeros: the operand was not declared symmetric
};

inline GrpI8Instance grp_i8_instance(const qe_qparam *w, int x_symmetric, int w_symmetric)
{
    return GrpI8Instance{w->n_bits == 4, w_symmetric == 0, x_symmetric == 0};
}

// f(std::true_type | std::false_type) for a runtime flag
template <class F>
inline void dispatch_flag(int flag, F &&f)
{
    if (flag) f(std::true_type()); else f(std::false_type());
}

// f(WB, WZ, XZ) as std::integral_constants for the runtime instance: the 8 instances of a kernel
template <class F>
inline void dispatch_grp_i8(const GrpI8Instance &in, F &&f)
{
    dispatch_flag(in.w4, [&](auto w4) { dispatch_flag(in.wz, [&](auto wz) { dispatch_flag(in.xz, [&](auto xz) {
        f(std::integral_constant<int, decltype(w4)::value ? 4 : 8>(), wz, xz);
    }); }); });
}

// the operand fields of an int8 unit's kernel argument; K: codes per weight row (a conv: IC)
template <class Args>
inline void fill_grp_operands(Args &a, const qe_qparam *x, const qe_qparam *w, const float *bias, int G, int K)
{
    a.x = x->data; a.w = w->data; a.x_scale = x->scale; a.x_zero = x->zero; a.w_scale = w->scale; a.w_zero = w->zero;
    a.bias = bias;
    a.x_bits = x->n_bits; a.x_sign = x->sign; a.w_bits = w->n_bits; a.w_sign = w->sign;
    a.G = G; a.NG = K / G;
}

// ---- host: the launch tail -------------------------------------------------------------------------------------------------
// The grid limit, the plain kernel (one thread per output, 256 per block) or the fast kernel `run_fast` launches, the check.
template <auto PLAIN, class Args, class F>
inline int launch_grp(int fast, int64_t blocks, const Args &a, hipStream_t s, F &&run_fast)
{
    if (blocks > 0x7fffffffLL) return QE_ERR_UNSUPPORTED;
    if (!fast) launch_instance<PLAIN>((unsigned)blocks, 256, 0, 0, s, a);
    else run_fast();
    QE_LAUNCH_CHECK();
    return QE_OK;
}

// ---- device leaves of the int8 units -------------------------------------------------------------------------------------
// stored u of an n_bits stream -> the centred integer u - 2^(bits-1)
__device__ __forceinline__ int centred_elem(const uint8_t *__restrict__ p, int64_t i, int n_bits)
{
    return unpack_elem(p, i, n_bits, 0) - (1 << (n_bits - 1));
}
__device__ __forceinline__ uint4 xor80(uint4 v)
{
    return make_uint4(v.x ^ 0x80808080u, v.y ^ 0x80808080u, v.z ^ 0x80808080u, v.w ^ 0x80808080u);
}
__device__ __forceinline__ int dot_ones(uint4 v)          // the sum of 16 int8
{
    int s = __builtin_amdgcn_sdot4((int)v.x, 0x01010101, 0, false);
    s = __builtin_amdgcn_sdot4((int)v.y, 0x01010101, s, false);
    s = __builtin_amdgcn_sdot4((int)v.z, 0x01010101, s, false);
    return __builtin_amdgcn_sdot4((int)v.w, 0x01010101, s, false);
}
// 8 nibbles (low first) of `w` -> 8 bytes of u - 8
__device__ __forceinline__ void widen_nibbles(uint32_t w, uint32_t &lo, uint32_t &hi)
{
    const uint32_t e = w & 0x0f0f0f0fu, o = (w >> 4) & 0x0f0f0f0fu;          // codes 0 2 4 6, codes 1 3 5 7
    lo = (__builtin_amdgcn_perm(o, e, 0x05010400u) + 0x78787878u) ^ 0x80808080u;   // u + 0x78 <= 0x87: no carry; ^ 0x80: u - 8
    hi = (__builtin_amdgcn_perm(o, e, 0x07030602u) + 0x78787878u) ^ 0x80808080u;
}

// ---- device block of the two linear fast kernels -----------------------------------------------------------------------------
// A group ends: the fold of the group accumulator (int32, or fp32 in the bf16 unit) into the total,
//   acco = fma(sw, accg - zw' Sx, acco);   accg = 0,   Sx = sx_of(row tile i, register r) (read only with WZ)
// conv_awq_mfma_kernel writes the same loop out: with this function its instruction stream moves.
template <bool WZ, int MI, class AccG, class AccO, class SxOf>
__device__ __forceinline__ void grp_fold(AccG (&accg)[MI][2], AccO (&acco)[MI][2], const float (&gsw)[2], const float (&gdz)[2], SxOf sx_of)
{
#pragma unroll
    for (int i = 0; i < MI; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float s = 0.0f;
            if constexpr (WZ) s = sx_of(i, r);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const float p = (float)accg[i][j][r];
                const float t = WZ ? fmaf(-gdz[j], s, p) : p;
                acco[i][j][r] = fmaf(gsw[j], t, acco[i][j][r]);
                accg[i][j][r] = 0;
            }
        }
    }
}

}  // namespace qe
