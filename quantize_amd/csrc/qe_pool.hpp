// qe_pool.hpp -- host side of the quantised pooling and ReLU kernels (qe_pool.hip): the window arithmetic, and the one plan
// that qe_avgpool2d_codes_path and qe_avgpool2d_codes both read.  Host-only and header-only apart from the launchers.
#pragma once
#include "qe_common.h"

namespace qe {

// ---- adaptive windows (torch's rule): output o of `out` over an axis of `in` elements covers [lo, hi) ----------------------
__host__ __device__ inline int pool_win_lo(int o, int in, int out) { return (int)(((int64_t)o * in) / out); }
__host__ __device__ inline int pool_win_hi(int o, int in, int out) { return (int)((((int64_t)o + 1) * in + out - 1) / out); }

// the widest adaptive window of an axis
inline int pool_win_max(int in, int out)
{
    int m = 0;
    for (int o = 0; o < out; ++o) {
        const int n = pool_win_hi(o, in, out) - pool_win_lo(o, in, out);
        m = n > m ? n : m;
    }
    return m;
}

// ---- the plan of a codes-domain average pool -------------------------------------------------------------------------------
enum PoolKernel { POOL_NONE = -1, POOL_PLAIN = 0, POOL_PAIR = 1, POOL_PLANE = 2, POOL_KERNELS = 3 };
constexpr int POOL_THREADS = 256;
constexpr int POOL_PAIR_VEC = 16;          // adjacent outputs of a pair thread
constexpr int POOL_SUB8_VEC = 8;           // consecutive outputs of a plain thread that packs sub-8-bit codes: whole bytes

struct PoolRequest {
    int N, C, H, W, kernel, stride, OH, OW;
    int x_bits;                            // the stream's width (8, or the call is refused)
    int rq_bits;                           // 0: no consumer
    bool has_out;
};

struct PoolPlan {
    int kernel = POOL_NONE;
    int rc = QE_ERR_ARG;                   // what the call answers when kernel == POOL_NONE
    int OH = 0, OW = 0;
    int vec = 1;                           // consecutive outputs of a thread
    int T = 1, logT = 0;                   // plane: lanes per plane (a power of two <= 64)
    int ncx = 0;                           // pair: 16-output chunks per output row
    int max_cnt = 0;                       // the largest window
    int64_t blocks = 0;
};

inline PoolPlan plan_pool(const PoolRequest &r)
{
    PoolPlan p;
    if (r.N < 0 || r.C < 0 || r.H <= 0 || r.W <= 0 || r.kernel < 0 || r.OH <= 0 || r.OW <= 0) return p;
    if (r.kernel > 0) {
        if (r.stride <= 0 || r.H < r.kernel || r.W < r.kernel) return p;
        if (r.OH != (r.H - r.kernel) / r.stride + 1 || r.OW != (r.W - r.kernel) / r.stride + 1) return p;
    }
    if (!r.has_out && r.rq_bits == 0) return p;
    p.rc = QE_ERR_UNSUPPORTED;
    if (r.x_bits != 8) return p;
    if ((int64_t)r.H * r.W > 0x7fffffffLL) return p;                      // in-plane offsets are 32-bit
    p.OH = r.OH; p.OW = r.OW;
    const int64_t cnt = r.kernel > 0 ? (int64_t)r.kernel * r.kernel
                                     : (int64_t)pool_win_max(r.H, r.OH) * pool_win_max(r.W, r.OW);
    if (cnt * 255 >= (1LL << 24)) return p;                               // (float)S must be exact
    p.max_cnt = (int)cnt;
    const int64_t NP = (int64_t)r.N * r.C, n = NP * r.OH * r.OW;
    const bool sub8 = r.rq_bits > 0 && r.rq_bits < 8;
    int64_t threads;
    int kernel;
    if (!sub8 && r.kernel == 2 && r.stride == 2) {
        kernel = POOL_PAIR;
        p.vec = POOL_PAIR_VEC;
        p.ncx = ceil_div(r.OW, POOL_PAIR_VEC);
        threads = NP * r.OH * p.ncx;
    } else if (!sub8 && r.OH == 1 && r.OW == 1 && (r.kernel == 0 || (r.kernel == r.H && r.kernel == r.W))) {
        kernel = POOL_PLANE;
        const int chunks = ceil_div(r.H * r.W + 15, 16);                  // aligned 16-byte pieces a plane can touch
        while (p.T < 64 && p.T < chunks) { p.T *= 2; ++p.logT; }
        threads = ceil_div64(NP, POOL_THREADS / p.T) * POOL_THREADS;
    } else {
        kernel = POOL_PLAIN;
        p.vec = sub8 ? POOL_SUB8_VEC : 1;
        threads = ceil_div64(n, p.vec);
    }
    p.blocks = ceil_div64(threads, POOL_THREADS);
    if (p.blocks > 0x7fffffffLL) return p;
    p.kernel = kernel;
    p.rc = QE_OK;
    return p;
}

// ---- launchers (qe_pool.hip) -------------------------------------------------------------------------------------------------
int launch_pool_codes(const PoolPlan &p, const qe_qparam *x, int N, int C, int H, int W, int kernel, int stride, int relu, float *out,
                      const qe_requant *rq, uint8_t *codes, int32_t *status, hipStream_t s);
int launch_quant_relu(const float *x, int64_t n, int64_t inner, const qe_requant *rq, float *out, hipStream_t s);
int launch_quant_maxpool2d(const float *x, int N, int C, int H, int W, int kernel, int stride, int padding, int OH, int OW,
                           const qe_requant *rq, float *out, hipStream_t s);
int launch_quant_adaptive_avgpool2d(const float *x, int N, int C, int H, int W, int OH, int OW, const qe_requant *rq, float *out,
                                    hipStream_t s);

}  // namespace qe
