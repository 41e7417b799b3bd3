// qe_preact.hpp -- host side of the pre-activation boundary kernels (qe_preact.hip): the request check and the one plan that
// qe_affine_relu_quantize_pack_path and qe_affine_relu_quantize_pack both read.  Host-only and header-only apart from the launcher.
#pragma once
#include "qe_common.h"

namespace qe {

enum PreactKernel { PREACT_NONE = -1, PREACT_PLAIN = 0, PREACT_FAST = 1, PREACT_KERNELS = 2 };
constexpr int PREACT_THREADS = 256;
constexpr int PREACT_FAST_VEC = 16;        // consecutive elements of one plane a fast thread owns: one 16-byte store of 8-bit codes
constexpr int PREACT_PLAIN_VEC = 8;        // consecutive elements a plain thread owns: their b-bit codes fill b whole bytes
constexpr int PREACT_MAX_OUT = 2;          // consumers (conv1 and convShortcut of a WideResNet block)
constexpr int PREACT_MAX_BLOCKS = kNumCU * 8;      // the plain kernel's grid cap (as TP_MAX_BLOCKS): grid-stride beyond it

struct PreactRequest {
    int N, C, P;
    int n_out;
    int rq_bits[PREACT_MAX_OUT];
    bool has_sum, has_act;
};

struct PreactPlan {
    int kernel = PREACT_NONE;
    int rc = QE_ERR_ARG;                   // what the call answers when kernel == PREACT_NONE
    int vec = 0;                           // consecutive elements of a thread
    int64_t groups = 0;                    // threads' worth of work
    int64_t blocks = 0;                    // the grid
};

inline PreactPlan plan_preact(const PreactRequest &r)
{
    PreactPlan p;
    if (r.n_out < 0 || r.n_out > PREACT_MAX_OUT) return p;
    for (int i = 0; i < r.n_out; ++i)
        if (!bits_ok(r.rq_bits[i])) { p.rc = QE_ERR_NBITS; return p; }
    if (r.N <= 0 || r.C <= 0 || r.P <= 0) return p;
    if (r.n_out == 0 && !r.has_sum && !r.has_act) return p;
    const int64_t n = (int64_t)r.N * r.C * r.P;
    bool all8 = true;
    for (int i = 0; i < r.n_out; ++i) all8 = all8 && r.rq_bits[i] == 8;
    p.rc = QE_ERR_UNSUPPORTED;
    if (all8 && r.P % PREACT_FAST_VEC == 0) {
        p.vec = PREACT_FAST_VEC;
        p.groups = n / PREACT_FAST_VEC;
        p.blocks = ceil_div64(p.groups, PREACT_THREADS);
        if (p.blocks > 0x7fffffffLL) return p;
        p.kernel = PREACT_FAST;
    } else {
        p.vec = PREACT_PLAIN_VEC;
        p.groups = ceil_div64(n, PREACT_PLAIN_VEC);
        const int64_t want = ceil_div64(p.groups, PREACT_THREADS);
        p.blocks = want < PREACT_MAX_BLOCKS ? want : PREACT_MAX_BLOCKS;
        p.kernel = PREACT_PLAIN;
    }
    p.rc = QE_OK;
    return p;
}

// ---- launcher (qe_preact.hip) ------------------------------------------------------------------------------------------------
int launch_preact(const PreactPlan &p, const float *x, const float *identity, int N, int C, int P, const float *alpha, const float *shift,
                  int n_out, const qe_requant *rq, uint8_t *const *codes, float *sum_out, float *act_out, int32_t *status, hipStream_t s);

}  // namespace qe
