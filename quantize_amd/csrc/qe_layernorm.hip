// qe_layernorm.hip -- the ViT's row kernels for gfx950 (MI355X): LayerNorm fused with the codes of its consumers, and the
// image quantiser of the patch embedding fused with the unfold.
//
// qe_layernorm_quantize_pack: one wave per row, the row held in registers (NV float4 per lane, E <= 256 NV), read once.
// Two wave reductions: the sum of x - x0 (x0 the row's first value; mean = x0 + sum / E), then the CENTRED sum of squares
// (var = sum((x - mean)^2) / E: no cancellation of E[x^2] - mean^2), rstd = 1 / sqrtf(var + eps) with the correctly rounded division and square root hipcc
// emits by default.  Each lane then writes its values' fp32 LayerNorm (optional) and 4 codes per float4 for every consumer
// (qe_elementwise.hpp: the arithmetic of qe_quantize_pack on the same fp32 value, so the codes are bit-identical to
// quantize_pack of the fp32 output).  Bytes per row: 4 E in, 3 E of codes out (q / k / v), instead of 4 E + 4 E (torch's LN)
// + 3 x (4 E + E) (three quantize_pack passes).
#include "qe_common.h"
#include "qe_elementwise.hpp"

#include <algorithm>

namespace qe {

constexpr int LN_MAX_OUT = 3;

struct LnArgs {
    const float *x, *gamma, *beta;
    float *ln;                      // may be NULL
    uint8_t *codes[LN_MAX_OUT];
    QeRq rq[LN_MAX_OUT];
    int32_t *status;
    int64_t rows;
    int E, n_out;
    float eps;
};

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

template <int NV>
__global__ __launch_bounds__(256) void layernorm_quant_kernel(const LnArgs a)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.rows) return;                            // wave-uniform
    const int E4 = a.E >> 2;
    const float4 *xr = reinterpret_cast<const float4 *>(a.x + row * a.E);
    float4 v[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int idx = lane + 64 * i;
        v[i] = idx < E4 ? xr[idx] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    // the row is shifted by its first value x0 before it is summed: under a large mean offset the terms x - x0 are small
    // (and exact where x is within a factor of two of x0), so the sum keeps the spread that sum(x) would round away
    const float x0 = __shfl(v[0].x, 0);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if (lane + 64 * i < E4) { v[i].x -= x0; v[i].y -= x0; v[i].z -= x0; v[i].w -= x0; }
    }
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < NV; ++i) s += (v[i].x + v[i].y) + (v[i].z + v[i].w);   // lanes past the row hold zeros
    const float mean = wave_sum(s) / (float)a.E;        // of x - x0
    float ss = 0.0f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if (lane + 64 * i < E4) {
            const float d0 = v[i].x - mean, d1 = v[i].y - mean, d2 = v[i].z - mean, d3 = v[i].w - mean;
            ss += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
        }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(ss) / (float)a.E + a.eps);
    bool bad = false;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int idx = lane + 64 * i;
        if (idx >= E4) continue;
        float4 g = make_float4(1.0f, 1.0f, 1.0f, 1.0f), b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (a.gamma != nullptr) g = reinterpret_cast<const float4 *>(a.gamma)[idx];
        if (a.beta != nullptr) b = reinterpret_cast<const float4 *>(a.beta)[idx];
        float4 o;
        o.x = (v[i].x - mean) * rstd * g.x + b.x;
        o.y = (v[i].y - mean) * rstd * g.y + b.y;
        o.z = (v[i].z - mean) * rstd * g.z + b.z;
        o.w = (v[i].w - mean) * rstd * g.w + b.w;
        if (a.ln != nullptr) reinterpret_cast<float4 *>(a.ln + row * a.E)[idx] = o;
        for (int k = 0; k < a.n_out; ++k) {
            const QeRq &q = a.rq[k];
            const float sc = q.scale[0], zr = q.zero[0];
            const uint32_t w = qe_rq_code(o.x, sc, zr, q, bad) | (qe_rq_code(o.y, sc, zr, q, bad) << 8) |
                               (qe_rq_code(o.z, sc, zr, q, bad) << 16) | (qe_rq_code(o.w, sc, zr, q, bad) << 24);
            reinterpret_cast<uint32_t *>(a.codes[k] + row * a.E)[idx] = w;
        }
    }
    if (__builtin_amdgcn_ballot_w64(bad) != 0ull && lane == 0 && a.status != nullptr) atomicOr(a.status, 1);
}

static bool ln_shape_ok(int64_t rows, int E) { return rows >= 0 && E >= 4 && (E & 3) == 0 && E <= QE_LN_MAX_E; }

static int launch_layernorm(const LnArgs &a, hipStream_t s)
{
    const int64_t blocks = (a.rows + 3) / 4;
    if (blocks > 0x7fffffffLL) return QE_ERR_UNSUPPORTED;
    const int nv = (a.E / 4 + 63) / 64;
    if (nv <= 1) hipLaunchKernelGGL(layernorm_quant_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, s, a);
    else if (nv <= 2) hipLaunchKernelGGL(layernorm_quant_kernel<2>, dim3((unsigned)blocks), dim3(256), 0, s, a);
    else if (nv <= 4) hipLaunchKernelGGL(layernorm_quant_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(layernorm_quant_kernel<8>, dim3((unsigned)blocks), dim3(256), 0, s, a);
    QE_LAUNCH_CHECK();
    return QE_OK;
}

// ---------------------------------------------------------------------------------------------
// qe_quantize_patchify: a thread owns 8 consecutive elements of the patch matrix (b whole bytes of the packed stream).
// With p % 8 == 0 the 8 elements are 8 consecutive pixels of one image row: two 16-byte loads.
// ---------------------------------------------------------------------------------------------
struct PatchArgs {
    const float *x;
    uint8_t *codes;
    int32_t *status;
    int64_t n;                   // N * (H/p) * (W/p) * C * p * p
    int C, H, W, p, PW, PP;      // PW = W / p, PP = (H / p) * (W / p)
    int K;                       // C p p
    int per_ch, vec;
    QeRq q;
    int n_bits;
};

__global__ __launch_bounds__(256) void patchify_quant_kernel(const PatchArgs a)
{
    const int64_t n_groups = (a.n + 7) / 8;
    bool bad = false;
    const int pp = a.p * a.p;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n_groups; g += (int64_t)gridDim.x * 256) {
        const int64_t e0 = 8 * g;
        const int cnt = (a.n - e0) < 8 ? (int)(a.n - e0) : 8;
        float v[8];
        int ch[8];
        auto src = [&](int64_t e, int &c) -> int64_t {
            const int64_t r = e / a.K;
            const int k = (int)(e - r * a.K);
            const int64_t n = r / a.PP;
            const int t = (int)(r - n * a.PP);
            const int ph = t / a.PW, pw = t - ph * a.PW;
            c = k / pp;
            const int rem = k - c * pp;
            const int kh = rem / a.p, kw = rem - kh * a.p;
            return ((n * a.C + c) * a.H + (int64_t)ph * a.p + kh) * a.W + (int64_t)pw * a.p + kw;
        };
        if (a.vec && cnt == 8) {
            int c;
            const int64_t i0 = src(e0, c);
            const float4 x0 = *reinterpret_cast<const float4 *>(a.x + i0), x1 = *reinterpret_cast<const float4 *>(a.x + i0 + 4);
            v[0] = x0.x; v[1] = x0.y; v[2] = x0.z; v[3] = x0.w; v[4] = x1.x; v[5] = x1.y; v[6] = x1.z; v[7] = x1.w;
#pragma unroll
            for (int j = 0; j < 8; ++j) ch[j] = c;
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                ch[j] = 0;
                v[j] = 0.0f;
                if (j < cnt) { int c; v[j] = a.x[src(e0 + j, c)]; ch[j] = c; }
            }
        }
        uint64_t bits = 0;
        for (int j = 0; j < cnt; ++j) {
            const float sc = a.per_ch ? a.q.scale[ch[j]] : a.q.scale[0];
            const float zr = a.per_ch ? a.q.zero[ch[j]] : a.q.zero[0];
            bits |= (uint64_t)qe_rq_code(v[j], sc, zr, a.q, bad) << (j * a.n_bits);
        }
        uint8_t *dst = a.codes + g * a.n_bits;
        const int nb = (cnt * a.n_bits + 7) / 8;
        if (a.n_bits == 8 && cnt == 8 && (reinterpret_cast<uintptr_t>(dst) & 7) == 0) *reinterpret_cast<uint64_t *>(dst) = bits;
        else for (int k = 0; k < nb; ++k) dst[k] = (uint8_t)(bits >> (8 * k));
    }
    if (__builtin_amdgcn_ballot_w64(bad) != 0ull && (threadIdx.x & 63) == 0 && a.status != nullptr) atomicOr(a.status, 1);
}

}  // namespace qe

extern "C" int qe_layernorm_quantize_pack_path(int64_t rows, int32_t E, int32_t n_out, const qe_requant *rq, uint8_t *const *codes)
{
    using namespace qe;
    if (!ln_shape_ok(rows, E) || n_out < 0 || n_out > LN_MAX_OUT || (n_out > 0 && (rq == nullptr || codes == nullptr))) return 0;
    for (int k = 0; k < n_out; ++k)
        if (rq[k].n_bits != 8 || rq[k].n_param != 1 || (reinterpret_cast<uintptr_t>(codes[k]) & 3) != 0) return 0;
    return 1;
}

extern "C" size_t qe_layernorm_quantize_pack_workspace_bytes(int64_t rows, int32_t E, int32_t n_out, const qe_requant *rq,
                                                             uint8_t *const *codes, const float *ln_out)
{
    if (rows <= 0 || E <= 0 || ln_out != nullptr || qe_layernorm_quantize_pack_path(rows, E, n_out, rq, codes)) return 0;
    return (size_t)rows * (size_t)E * sizeof(float);
}

extern "C" int qe_layernorm_quantize_pack(const float *x, int64_t rows, int32_t E, const float *gamma, const float *beta, float eps,
                                          int32_t n_out, const qe_requant *rq, uint8_t *const *codes, float *ln_out,
                                          int32_t *status, void *workspace, size_t workspace_bytes, qe_stream_t stream)
{
    using namespace qe;
    if (rows < 0 || n_out < 0 || n_out > LN_MAX_OUT || (n_out > 0 && (rq == nullptr || codes == nullptr))) return QE_ERR_ARG;
    if (!ln_shape_ok(rows, E)) return QE_ERR_UNSUPPORTED;
    if (rows == 0) return QE_OK;
    if (x == nullptr || (n_out == 0 && ln_out == nullptr)) return QE_ERR_ARG;
    if (((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(gamma) | reinterpret_cast<uintptr_t>(beta) |
          reinterpret_cast<uintptr_t>(ln_out)) & 15) != 0)
        return QE_ERR_ARG;
    for (int k = 0; k < n_out; ++k) {
        if (!bits_ok(rq[k].n_bits)) return QE_ERR_NBITS;
        if (codes[k] == nullptr || rq[k].scale == nullptr || rq[k].zero == nullptr || !one_or_per_channel(rq[k].n_param, E))
            return QE_ERR_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    LnArgs a = {};
    a.x = x; a.gamma = gamma; a.beta = beta; a.ln = ln_out; a.status = status; a.rows = rows; a.E = E; a.eps = eps;
    if (qe_layernorm_quantize_pack_path(rows, E, n_out, rq, codes)) {
        a.n_out = n_out;
        for (int k = 0; k < n_out; ++k) { a.codes[k] = codes[k]; a.rq[k] = make_qe_rq(rq[k]); }
        return launch_layernorm(a, s);
    }
    // path 0: the fp32 LayerNorm, then quantize_pack per consumer (per-column rq: channel of element i = i % E)
    float *ln = ln_out;
    if (ln == nullptr) {
        if (workspace == nullptr || workspace_bytes < (size_t)rows * E * sizeof(float) || (reinterpret_cast<uintptr_t>(workspace) & 15) != 0)
            return QE_ERR_WORKSPACE;
        ln = static_cast<float *>(workspace);
    }
    a.ln = ln;
    a.n_out = 0;
    int rc = launch_layernorm(a, s);
    for (int k = 0; k < n_out && rc == QE_OK; ++k)
        rc = qe_quantize_pack(ln, rows * (int64_t)E, rq[k].scale, rq[k].zero, rq[k].n_param, 1, rq[k].qmin, rq[k].qmax,
                              rq[k].n_bits, rq[k].sign, codes[k], status, stream);
    return rc;
}

extern "C" int qe_quantize_patchify(const float *x, int32_t N, int32_t C, int32_t H, int32_t W, int32_t patch, const float *scale,
                                    const float *zero, int32_t n_param, float qmin, float qmax, int n_bits, int sign, uint8_t *out,
                                    int32_t *status, qe_stream_t stream)
{
    using namespace qe;
    if (!bits_ok(n_bits)) return QE_ERR_NBITS;
    if (N < 0 || C <= 0 || H <= 0 || W <= 0 || patch <= 0 || H % patch != 0 || W % patch != 0) return QE_ERR_ARG;
    if (!one_or_per_channel(n_param, C)) return QE_ERR_ARG;
    if (N == 0) return QE_OK;
    if (x == nullptr || out == nullptr || scale == nullptr || zero == nullptr) return QE_ERR_ARG;
    PatchArgs a = {};
    a.x = x; a.codes = out; a.status = status;
    a.C = C; a.H = H; a.W = W; a.p = patch; a.PW = W / patch; a.PP = (H / patch) * (W / patch);
    if ((int64_t)C * patch * patch >= (1ll << 31)) return QE_ERR_UNSUPPORTED;
    a.K = C * patch * patch;
    a.n = (int64_t)N * a.PP * a.K;
    a.per_ch = n_param > 1;
    a.vec = (patch % 8) == 0 && (W % 4) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
    a.q = make_qe_rq(qe_requant{scale, zero, n_param, qmin, qmax, n_bits, sign});
    a.n_bits = n_bits;
    const int64_t groups = (a.n + 7) / 8;
    const int blocks = (int)std::min<int64_t>((groups + 255) / 256, (int64_t)kNumCU * 32);
    hipLaunchKernelGGL(patchify_quant_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    QE_LAUNCH_CHECK();
    return QE_OK;
}
