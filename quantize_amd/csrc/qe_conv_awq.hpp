// qe_conv_awq.hpp -- the kernel argument of qe_quantconv2d_awq (qe_conv_awq.hip): both kernels read the same block.
#pragma once
#include "qe_common.h"

namespace qe {

struct ConvAwqArgs {
    const uint8_t *x, *w;      // packed NCHW activation codes, packed OIHW weight codes
    const float *x_scale, *x_zero, *w_scale, *w_zero, *bias;
    float *out;                // [N][OC][OH][OW] fp32
    int x_bits, x_sign, w_bits, w_sign;
    int G, NG;                 // input channels per group, groups per output channel (IC / G)
    int N, IC, H, W, OC, KH, KW, stride, padding, OH, OW;
    int P;                     // fast kernel: the plane, H * W
    int tiles;                 // fast kernel: pixel tiles per image
    int relu;
};

}  // namespace qe
