// qe_linear_bf16in.hpp -- what qe_linear.hip (the host plan and the entry points) and qe_linear_bf16in.hip (the kernels of
// qe_quantlinear_bf16_input, a unit of their own so that no other code object moves) share: the weight centre of the
// float-input linear kernels, the geometry the plan needs, the kernel arguments and the two launches.
#pragma once
#include "qe_common.h"

namespace qe {

// The integer c a column's weight codes are centred on before the bf16 conversion: rint(zw), clamped to the code range so
// that |q - c| <= 255 stays exact in bf16.  The MFMAs then sum x (q - c), and the epilogue subtracts only (zw - c) S_x: with
// zw itself there (zw ~ 128 for unsigned codes, asymmetric weights) the two fp32 terms sw (S_xq - zw S_x) are large and
// cancel, and their rounding error was many times the reference chain's on non-zero-mean activations.
__device__ __forceinline__ float linf_centre(float zw, int w_sign)
{
    const float c = rintf(zw);
    return w_sign ? fminf(fmaxf(c, -128.0f), 127.0f) : fminf(fmaxf(c, 0.0f), 255.0f);
}

// linear_bf16in_kernel: tile 128 x 128, 32-deep stages, two stage buffers of an activation and a weight image
// ([128][32] bf16 each), the row sums and the column constants
constexpr int LB_T = 128, LB_K = 32;
constexpr int LB_PLANE = LB_T * LB_K * 2;                 // bytes of one [128][32] bf16 image (8 KB)
constexpr size_t linb_lds_bytes() { return (size_t)4 * LB_PLANE + LB_T * sizeof(float) + LB_T * 4 * sizeof(float); }

struct LinBf16Args {
    const uint16_t *x;      // B x K bf16 bit patterns
    const uint8_t *w;       // O x K stored 8-bit codes
    const float *w_scale, *w_zero, *bias;
    const float *res;       // residual instance: out = y + res (res == out allowed)
    float *out;
    int w_sign, w_per_tensor;
    int64_t B;
    int K, O;
};

// Grid of a linear's elementwise pass (widen_bf16_kernel, round_bf16_kernel, add_residual_kernel: 256-thread blocks, grid
// stride) over n > 0 elements: `width` elements per thread and trip where every address is 16-byte aligned (`addrs`: their
// bitwise OR), one otherwise; at most 16 blocks per CU.
struct ElementwiseGrid { int vec, blocks; };
inline ElementwiseGrid elementwise_grid(int64_t n, int width, uintptr_t addrs)
{
    const int vec = (addrs & 15) == 0;
    const int64_t want = ((vec ? n / width : n) + 255) / 256;
    return {vec, (int)(want < 1 ? 1 : want > kNumCU * 16 ? kNumCU * 16 : want)};
}

// blocks = ceil(B / 128) ceil(O / 128); residual chooses the template instance
void launch_linear_bf16in(const LinBf16Args &a, bool residual, int64_t blocks, hipStream_t s);
// out[i] = fp32 of the bf16 bit pattern x[i] (exact): path 0 of qe_quantlinear_bf16_input
void launch_widen_bf16(const uint16_t *x, float *out, int64_t n, hipStream_t s);

}  // namespace qe
