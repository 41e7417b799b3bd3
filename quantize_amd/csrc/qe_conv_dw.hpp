// qe_conv_dw.hpp -- host interface of the depthwise packed convolutions (qe_conv_dw.hip): the one plan that
// qe_quantconv2d_depthwise_path / _plan_info and the launcher read, and the launcher.
#pragma once
#include "qe_common.h"

namespace qe {

// what the plan depends on: the shape, the operand formats, the epilogue and (for the reported store forms) the addresses
struct DwRequest {
    const qe_conv_shape *sh;
    int x_bits, x_sign, w_bits, w_sign;
    int rq_bits;               // 0: no codes
    bool has_out;
    uintptr_t out, codes;      // 0 reads as aligned
};

// fast: 1 + 3 * (stride - 1) + (0 out, 1 codes, 2 out + codes)
enum DwKernel { DW_NONE = -1, DW_PLAIN = 0, DW_FAST_FIRST = 1, DW_KERNELS = 7 };

struct DwPlan {
    int kernel = DW_NONE;
    int symmetric = 0;         // both operands signed: a plane whose zeros are 0 has no zero-point term at all
    int G = 1, TH = 0;         // planes of a workgroup (whole planes), or output rows of a band (G == 1)
    int vec = 1;               // consecutive outputs of a thread
    int store16 = 0, codes4 = 0;
    int two_pass = 0;          // sub-8-bit codes: fp32 out, then qe_quantize_pack
    int OH = 0, OW = 0, bands = 1, ncg = 1;
    unsigned m_ncg = 0, m_oh = 0;          // floor(2^31 / d) + 1: u / d == umulhi(2 u, m) while u d < 2^31
    int in_off = 0, codes_off = 0, out_off = 0;   // LDS regions (bytes) behind the per-plane table
    int64_t blocks = 0, lds = 0;
};

constexpr int DW_THREADS = 256;
constexpr int DW_VEC = 4;
constexpr int DW_MAX_G = 32;
constexpr int DW_MAX_OUTPUTS = 4096;        // outputs of a workgroup
constexpr int DW_LDS_BUDGET = 32 * 1024;    // five workgroups of a CU's 160 KB
constexpr int DW_MAX_K = 7;

DwPlan plan_dw(const DwRequest &r);

// the kernel of the plan on (x, w, bias): fp32 out and / or the 8-bit codes of rq (rq == NULL or out-only when two_pass)
int launch_dw(const DwPlan &p, const qe_qparam *x, const qe_qparam *w, const float *bias, const qe_conv_shape *sh, int relu,
              float *out, const qe_requant *rq, uint8_t *codes, int32_t *status, hipStream_t s);

}  // namespace qe
