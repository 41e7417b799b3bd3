// qe_conv_grp.hpp -- host interface of the grouped packed convolutions (qe_conv_grp.hip): the one plan that
// qe_quantconv2d_grouped_path / _plan_info and the launcher read, and the launcher.
#pragma once
#include "qe_common.h"

namespace qe {

// what the plan depends on: the shape, the groups, the operand formats, the epilogue and (for the reported store forms) the
// addresses
struct GrpRequest {
    const qe_conv_shape *sh;
    int groups;
    int x_bits, x_sign, x_n_param, w_bits, w_sign;
    int rq_bits;               // 0: no codes
    bool has_out;
    uintptr_t out, codes;      // 0 reads as aligned
};

// fast: 1 + 6 * log2(Cg / 4) + 3 * (stride - 1) + (0 out, 1 codes, 2 out + codes)
enum GrpKernel { GRP_NONE = -1, GRP_PLAIN = 0, GRP_FAST_FIRST = 1, GRP_KERNELS = 25 };

struct GrpPlan {
    int kernel = GRP_NONE;
    int slab = 1;              // consecutive channels of a workgroup (fast: 32 = 32 / Cg whole groups; plain: 1)
    int TH = 1, TW = 1;        // output rows and columns of a workgroup's pixel tile (fast: a band of TH whole rows)
    int tiles = 1;             // tiles per plane
    int out16 = 0, codes16 = 0;
    int two_pass = 0;          // sub-8-bit codes: fp32 out, then qe_quantize_pack
    int OH = 0, OW = 0, nslabs = 1;
    int wps = 1;               // workgroups of a slab: each walks N * tiles / wps tiles (fast)
    int in_rows = 0, raw_stride = 0, codes_stride = 0, out_stride = 0;   // LDS geometry (bytes per channel)
    int tile_off = 0, stage_off = 0, ostage_off = 0;                     // LDS regions (bytes) behind the per-channel table
    int64_t blocks = 0, lds = 0;
};

constexpr int GRP_THREADS = 256;
constexpr int GRP_SLAB = 32;
constexpr int GRP_MAX_PIXELS = 256;          // outputs per channel of a workgroup
constexpr int GRP_LDS_BUDGET = 64 * 1024;    // two workgroups of a CU's 160 KB
constexpr int GRP_MAX_K = 7;

GrpPlan plan_grp(const GrpRequest &r);

// the kernel of the plan on (x, w, bias): fp32 out and / or the 8-bit codes of rq (rq == NULL or out-only when two_pass)
int launch_grp(const GrpPlan &p, const qe_qparam *x, const qe_qparam *w, const float *bias, const qe_conv_shape *sh, int groups,
               int relu, float *out, const qe_requant *rq, uint8_t *codes, int32_t *status, hipStream_t s);

}  // namespace qe
