// qe_linear_grp_i8.hip -- qe_quantlinear_grouped: packed 8-bit activation codes x group-quantised (AWQ layout) weight codes.
//
//   out[b,o] = bias[o] + sx[b] sum_g sw[o,g] sum_{k in group g} (q_x[b,k] - zx[b]) (q_w[o,k] - zw[o,g])
//
// Group g covers k in [g G, (g + 1) G); sw / zw are fp32 arrays of O (K / G) elements in (o, g) order; sx / zx are indexed by
// the row (1 or B of them).  Two kernels and one host plan in a unit of its own: no other code object moves.  The host
// layer of the family and the device leaves it has in common with qe_conv_awq.hip are qe_grp_common.hpp's.
//
// Both kernels read every stored value u as the CENTRED integer u - 2^(bits-1).  A signed and an unsigned stream then differ
// only in the residual zero z' = zero - (signed ? 0 : 2^(bits-1)), and with x_c, w_c the centred codes
//   sum_{k in g} (x_c - zx') (w_c - zw') = P[b,o,g] - zw' Sx[b,g] - zx' (Sw[o,g] - G zw'),   P = sum x_c w_c, Sx = sum x_c, Sw = sum w_c
// P, Sx and Sw are integers below 2^21 in magnitude for G <= 128: exact in int32 and exact as fp32.  Only the fold rounds.
//
// Fast kernel (8-bit activation codes, 4- or 8-bit weight codes, G in {32, 64, 128}, 16-byte aligned streams):
// v_mfma_i32_32x32x32_i8 into an int32 GROUP accumulator; at each group boundary (every G / 32 MFMA k-steps)
//   acc_out = fma(sw[o,g], float(acc_g) - zw' float(Sx[b,g]), acc_out);   acc_g = 0
// and in the epilogue  out = sx[b] (acc_out - zx'[b] T[o]) + bias[o],   T[o] = sum_g sw[o,g] (Sw[o,g] - G zw'[o,g]).
// The instance WZ = false (w_symmetric: every zw' == 0) has no Sx and no second term, XZ = false (x_symmetric) has no T.
// Workgroup = 2 x 2 waves, tile 128 x 128, wave 64 x 64 = 2 x 2 MFMA tiles, one int32 and one fp32 accumulator set of 64
// registers each.  Stage = 64 k = two k-steps, register staged, TWO stage buffers ([128][64] bytes per operand, 16-byte pieces
// XOR-swizzled as in linear_mfma_kernel) and one barrier per stage, as linear_bf16in_kernel.  K is a multiple of 32 only:
// the last stage of an odd k-step count holds one k-step; its second half is staged from a clamped (valid) address and is
// never multiplied.  8-bit bytes are centred by one XOR with 0x80; a 4-bit staging thread owns 32 codes (16 bytes) of a row
// whose nibbles, low first, become bytes of u - 8 in registers -- no widened copy of the weights exists.  Sx comes from
// v_dot4_i32_i8 against ones on the threads that stage the activation bytes and travels through a small LDS array by stage
// parity and k-step; T accumulates on the threads that stage the column's weight codes (they hold the codes: four dots per 16)
// and is reduced once per tile into LDS.  D has the batch row on the register and the feature on the lane: a lane needs one
// sw and one zw per column tile per group, fetched at the top of the stage the group ends in, under that stage's MFMAs.  Rows
// beyond B and columns beyond O read a clamped, valid address and are dropped at the store: no load sits under a per-lane
// condition.
//
// Plain kernel (everything else): one thread per output, group by group in k order: the three integer sums, then the fold.
//
// Fused forms (qe_quantlinear_grouped_residual, qe_quantlinear_grouped_requant): two more epilogues of the fast kernel, a
// template parameter, all of it behind the barrier that frees the stage buffers.  GQ_RES adds a residual to y in both store
// arms; on the float4 arm a tile's residual pieces are requested before its patch transposition, with the store's own row
// mapping, so out == residual is safe.  GQ_CODES / GQ_CODES_GELU store the consumer's 8-bit codes of y / gelu(y) with
// qe_elementwise.hpp's functions (the ones qe_quantize_pack_act runs): the feature is on the lane, so a per-feature quantiser
// is ONE scale and one zero in a register per column tile, as sw and zw are in the K loop.  The codes skip the fp32 patch:
// the four waves write bytes into one [128][128]-byte image of the workgroup's tile in the free stage buffers -- its 16-byte
// pieces XOR-swizzled by 2 ((row >> 2) & 3), which sends the two half waves of a byte write (rows 4 apart, 32 consecutive
// bytes each) to disjoint banks -- and after one barrier 256 threads store the image as 16-byte pieces, 128 contiguous bytes
// per row.  GELU runs in a loop that is not unrolled (one erf body per 32 x 32 tile): the lane parks its 16 values of the
// tile in a private LDS column behind the image and reads them back by loop index.  Where the fused instance is not
// eligible the entry points run two passes: qe_quantlinear_grouped into the workspace, then qe_quantize_pack_act or the add.
#include "qe_grp_common.hpp"         // the host layer and the device leaves shared with qe_conv_awq.hip and qe_linear_grp.hip
#include "qe_elementwise.hpp"
#include "qe_linear_bf16in.hpp"     // launch_add_residual: the elementwise add of qe_quantlinear_residual's path 0

namespace qe {

namespace {

typedef int v4i_q __attribute__((ext_vector_type(4)));
typedef int v16i_q __attribute__((ext_vector_type(16)));
typedef float v16f_q __attribute__((ext_vector_type(16)));

constexpr int GQ_T = 128, GQ_K = 64, GQ_STEP = 32;
constexpr int GQ_PLANE = GQ_T * GQ_K;                     // bytes of one [128][64] int8 image (8 KB)
constexpr int GQ_BUF = 2 * GQ_PLANE;                      // one stage buffer: the activation image, the weight image
// + Sx[stage parity][k-step][row] (int32), T[column], sx[row], zx'[row] (fp32)
constexpr size_t GQ_LDS = (size_t)2 * GQ_BUF + (4 * GQ_T + 3 * GQ_T) * 4;

struct LinGrpI8Args {
    const uint8_t *x, *w;
    const float *x_scale, *x_zero, *w_scale, *w_zero, *bias;
    float *out;
    int x_bits, x_sign, x_per_row, w_bits, w_sign;
    int G, NG;              // group size, groups per row (K / G)
    int64_t B;
    int K, O;
    // the fused epilogues (unused by GQ_F32)
    const float *res;       // GQ_RES: out = y + res (res == out allowed)
    uint8_t *codes;         // GQ_CODES*: B x O stored 8-bit codes of y / gelu(y)
    int32_t *status;        // GQ_CODES*: bit 0 set when a code fails the range test (NaN included)
    int rq_per_col;         // GQ_CODES*: one scale and zero per output feature (else one of each)
    QeRq rq;
};

// ---------------------------------------------------------------------------------------------
// Plain kernel: thread <-> output (b, o), o fastest.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void linear_grp_i8_plain_kernel(const LinGrpI8Args a)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.B * a.O) return;
    const int64_t b = idx / a.O;
    const int o = (int)(idx - b * a.O);
    const int64_t xp = a.x_per_row ? b : 0;
    const float sx = a.x_scale[xp];
    const float zxr = a.x_zero[xp] - (a.x_sign ? 0.0f : (float)(1 << (a.x_bits - 1)));
    const float woff = a.w_sign ? 0.0f : (float)(1 << (a.w_bits - 1));
    float acc = 0.0f;
    for (int g = 0; g < a.NG; ++g) {
        const float sw = a.w_scale[(int64_t)o * a.NG + g], zwr = a.w_zero[(int64_t)o * a.NG + g] - woff;
        int64_t p = 0, s_x = 0, s_w = 0;
        for (int k = g * a.G; k < (g + 1) * a.G; ++k) {
            const int xc = centred_elem(a.x, b * a.K + k, a.x_bits), wc = centred_elem(a.w, (int64_t)o * a.K + k, a.w_bits);
            p += xc * wc; s_x += xc; s_w += wc;
        }
        float t = fmaf(-zwr, (float)s_x, (float)p);
        t = fmaf(-zxr, fmaf(-(float)a.G, zwr, (float)s_w), t);
        acc = fmaf(sw, t, acc);
    }
    a.out[idx] = fmaf(sx, acc, a.bias != nullptr ? a.bias[o] : 0.0f);
}

// ---------------------------------------------------------------------------------------------
// Fast kernel.  WB: bits of a stored weight code (4 | 8).  WZ: residual weight zeros (Sx and the zw' term).  XZ: residual
// activation zeros (T and the zx' term).
// ---------------------------------------------------------------------------------------------
// Epilogue of the fast kernel, a template parameter and never a runtime branch: y (GQ_F32), y + res (GQ_RES), the consumer's
// 8-bit codes of y / gelu(y) (GQ_CODES, GQ_CODES_GELU).
enum { GQ_F32 = 0, GQ_RES = 1, GQ_CODES = 2, GQ_CODES_GELU = 3 };
template <int EPI> constexpr bool gq_codes() { return EPI == GQ_CODES || EPI == GQ_CODES_GELU; }
// byte (row rl, column cl) of the [128][128] code image; piece pc of row rl is at gq_img(rl, 16 * pc)
__device__ __forceinline__ int gq_img(int rl, int cl)
{
    return rl * GQ_T + 16 * ((cl >> 4) ^ (((rl >> 2) & 3) << 1)) + (cl & 15);
}

template <int WB, bool WZ, bool XZ, int EPI>
__global__ __launch_bounds__(256, 2) void linear_grp_i8_mfma_kernel(const LinGrpI8Args a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lsm[];
    int *sxg = reinterpret_cast<int *>(lsm + 2 * GQ_BUF);            // [2][2][128]: Sx of the tile's rows
    float *tcol = reinterpret_cast<float *>(sxg + 4 * GQ_T);         // [128]: T of the tile's columns
    float *rsx = tcol + GQ_T, *rzx = rsx + GQ_T;                     // [128]: sx, zx' of the tile's rows

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave & 1, wn = wave >> 1;
    const int col = lane & 31, h = lane >> 5;
    const int n_ct = (a.O + GQ_T - 1) / GQ_T;
    const int64_t bid = blockIdx.x;
    const int ct = (int)(bid % n_ct);
    const int64_t m0 = (bid / n_ct) * GQ_T;
    const int n0 = ct * GQ_T;
    const int gmask = a.G / GQ_STEP - 1;                  // k-steps per group - 1 (0, 1 or 3)
    const int gsh = a.G == 32 ? 0 : a.G == 64 ? 1 : 2;    // k-step -> group
    const int n_steps = a.K / GQ_STEP, n_stages = (n_steps + 1) >> 1;
    const float woff = a.w_sign ? 0.0f : (float)(1 << (WB - 1));      // zw' = zw - woff

    if (tid < GQ_T) {
        const int64_t row = (m0 + tid < a.B) ? m0 + tid : a.B - 1;
        const int64_t xp = a.x_per_row ? row : 0;
        rsx[tid] = a.x_scale[xp];
        rzx[tid] = a.x_zero[xp] - (a.x_sign ? 0.0f : 128.0f);
    }

    // activations: thread <-> (row r4 + 64 i, 16-byte piece p4 of the stage's 64 k)
    const int p4 = tid & 3, r4 = tid >> 2;
    const uint8_t *xrow[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int r = r4 + 64 * i;
        xrow[i] = a.x + ((m0 + r < a.B) ? m0 + r : a.B - 1) * a.K;
    }
    // weights, 8-bit: the same map on columns; 4-bit: thread <-> (column wc, k-step whh): 16 bytes = 32 codes
    // (twin: conv_awq_mfma_kernel's weight path, here and in fetch and stage)
    const int wc = tid >> 1, whh = tid & 1;
    const uint8_t *wrow[2];
    int64_t tog[2];                                       // the staged columns in the (o, g) arrays (T)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = WB == 8 ? r4 + 64 * i : wc;
        const int cc = (n0 + c < a.O) ? n0 + c : a.O - 1;
        wrow[i] = a.w + (int64_t)cc * a.K * WB / 8;
        tog[i] = (int64_t)cc * a.NG;
    }
    const int tstep = WB == 8 ? (p4 >> 1) : whh;          // the k-step of the stage this thread's weight codes lie in

    uint4 xv[2], wv[2];
    float tsw[2] = {0.0f, 0.0f}, tzw[2] = {0.0f, 0.0f};
    auto fetch = [&](int st) __attribute__((always_inline)) {
        const int kx = min(st * GQ_K + 16 * p4, a.K - 16);            // (clamped in the half stage of an odd k-step count)
#pragma unroll
        for (int i = 0; i < 2; ++i) xv[i] = *reinterpret_cast<const uint4 *>(xrow[i] + kx);
        if constexpr (WB == 8) {
#pragma unroll
            for (int i = 0; i < 2; ++i) wv[i] = *reinterpret_cast<const uint4 *>(wrow[i] + kx);
        } else {
            wv[0] = *reinterpret_cast<const uint4 *>(wrow[0] + min(st * (GQ_K / 2) + 16 * whh, a.K / 2 - 16));
        }
        if constexpr (XZ) {
            const int g = min(2 * st + tstep, n_steps - 1) >> gsh;
#pragma unroll
            for (int i = 0; i < (WB == 8 ? 2 : 1); ++i) { tsw[i] = a.w_scale[tog[i] + g]; tzw[i] = a.w_zero[tog[i] + g] - woff; }
        }
    };
    int sxa[2] = {0, 0};                                  // this thread's share of Sx[., g] of its two rows
    float tacc[2] = {0.0f, 0.0f};                         // this thread's share of T of its column(s)
    auto stage = [&](int st) __attribute__((always_inline)) {
        uint8_t *base = lsm + (st & 1) * GQ_BUF;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int r = r4 + 64 * i;
            const uint4 v = xor80(xv[i]);
            if constexpr (WZ) sxa[i] += dot_ones(v);
            *reinterpret_cast<uint4 *>(base + r * 64 + 16 * (p4 ^ ((r >> 2) & 3))) = v;
        }
        if constexpr (WZ) {
            if (gmask == 0) {                             // G = 32: every k-step is a group; its two threads of a row
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int s = sxa[i] + __shfl_xor(sxa[i], 1);
                    if ((p4 & 1) == 0) sxg[((st & 1) * 2 + (p4 >> 1)) * GQ_T + r4 + 64 * i] = s;
                    sxa[i] = 0;
                }
            } else if ((st & (gmask >> 1)) == (gmask >> 1)) {   // a group ends with this stage: the four threads of a row
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    int s = sxa[i];
                    s += __shfl_xor(s, 1); s += __shfl_xor(s, 2);
                    if (p4 == 0) sxg[((st & 1) * 2 + 1) * GQ_T + r4 + 64 * i] = s;
                    sxa[i] = 0;
                }
            }
        }
        const bool tvalid = 2 * st + tstep < n_steps;     // (the codes of a clamped half stage count for nothing)
        uint8_t *wbase = base + GQ_PLANE;
        if constexpr (WB == 8) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int r = r4 + 64 * i;
                const uint4 v = xor80(wv[i]);
                if constexpr (XZ) {
                    const float t = fmaf(tsw[i], fmaf(-16.0f, tzw[i], (float)dot_ones(v)), tacc[i]);
                    tacc[i] = tvalid ? t : tacc[i];
                }
                *reinterpret_cast<uint4 *>(wbase + r * 64 + 16 * (p4 ^ ((r >> 2) & 3))) = v;
            }
        } else {
            uint4 lo, hi;                                 // codes 0 .. 15, 16 .. 31 of the k-step
            widen_nibbles(wv[0].x, lo.x, lo.y); widen_nibbles(wv[0].y, lo.z, lo.w);
            widen_nibbles(wv[0].z, hi.x, hi.y); widen_nibbles(wv[0].w, hi.z, hi.w);
            if constexpr (XZ) {
                const float t = fmaf(tsw[0], fmaf(-32.0f, tzw[0], (float)(dot_ones(lo) + dot_ones(hi))), tacc[0]);
                tacc[0] = tvalid ? t : tacc[0];
            }
            uint8_t *wd = wbase + wc * 64;
            const int sw3 = (wc >> 2) & 3;
            *reinterpret_cast<uint4 *>(wd + 16 * ((2 * whh) ^ sw3)) = lo;
            *reinterpret_cast<uint4 *>(wd + 16 * ((2 * whh + 1) ^ sw3)) = hi;
        }
    };

    v16i_q accg[2][2];                                    // the running group
    v16f_q acco[2][2];                                    // the folded total
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) { accg[i][j][r] = 0; acco[i][j][r] = 0.0f; }

    // this lane's two output features (clamped) in the (o, g) arrays
    int64_t og[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) og[j] = (int64_t)min(n0 + wn * 64 + j * 32 + col, a.O - 1) * a.NG;

    const int swz = (col >> 2) & 3;
    const int a_off = (wm * 64 + col) * 64, b_off = GQ_PLANE + (wn * 64 + col) * 64;
    fetch(0);
    stage(0);
    for (int st = 0; st < n_stages; ++st) {
        // buffer st & 1 is complete (and Sx of the groups that end in it); every wave has left buffer (st + 1) & 1
        __syncthreads();
        const bool more = st + 1 < n_stages;
        if (more) fetch(st + 1);                          // in flight under the MFMAs
        bool fold[2];                                     // (uniform)
        float gsw[2][2] = {{0.0f, 0.0f}, {0.0f, 0.0f}}, gdz[2][2] = {{0.0f, 0.0f}, {0.0f, 0.0f}};
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int step = 2 * st + ks;
            fold[ks] = step < n_steps && (step & gmask) == gmask;
            if (fold[ks]) {                               // (twin: conv_awq_mfma_kernel's group-boundary fetch)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    gsw[ks][j] = a.w_scale[og[j] + (step >> gsh)];
                    if constexpr (WZ) gdz[ks][j] = a.w_zero[og[j] + (step >> gsh)] - woff;
                }
            }
        }
        const uint8_t *buf = lsm + (st & 1) * GQ_BUF;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            if (2 * st + ks < n_steps) {                  // (uniform: false in the half stage of an odd k-step count)
                const int po = 16 * ((2 * ks + h) ^ swz);
                v4i_q fa[2], fb[2];
#pragma unroll
                for (int j = 0; j < 2; ++j) fb[j] = *reinterpret_cast<const v4i_q *>(buf + b_off + j * 32 * 64 + po);
#pragma unroll
                for (int i = 0; i < 2; ++i) fa[i] = *reinterpret_cast<const v4i_q *>(buf + a_off + i * 32 * 64 + po);
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) accg[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[i], fb[j], accg[i][j], 0, 0, 0);
            }
            if (fold[ks]) {
                const int *sxr = sxg + ((st & 1) * 2 + ks) * GQ_T + wm * 64 + 4 * h;
                grp_fold<WZ>(accg, acco, gsw[ks], gdz[ks], [&](int i, int r) { return (float)sxr[i * 32 + (r & 3) + 8 * (r >> 2)]; });
            }
        }
        if (more) stage(st + 1);
    }
    if constexpr (XZ) {                                   // T: the threads of a column add their shares (twin: conv_awq_mfma_kernel's)
        if constexpr (WB == 8) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                float t = tacc[i];
                t += __shfl_xor(t, 1); t += __shfl_xor(t, 2);
                if (p4 == 0) tcol[r4 + 64 * i] = t;
            }
        } else {
            const float t = tacc[0] + __shfl_xor(tacc[0], 1);
            if (whh == 0) tcol[wc] = t;
        }
    }
    __syncthreads();                                      // every wave is done with the stage buffers; T is complete
    if constexpr (gq_codes<EPI>()) {
        // The feature is on the lane: the consumer's scale and zero of this lane's column are one register each per column
        // tile (a clamped address beyond O, as the bias).  Bytes into the image, one barrier, 16-byte pieces out.
        uint8_t *img = lsm;
        float *mine = reinterpret_cast<float *>(lsm + GQ_T * GQ_T) + wave * (16 * 64) + lane;      // GELU: [16][64] per wave
        bool bad = false;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int cl = wn * 64 + j * 32 + col, c = n0 + cl, cc = min(c, a.O - 1);
            const float bias = a.bias != nullptr ? a.bias[cc] : 0.0f;
            const float sc = a.rq.scale[a.rq_per_col ? cc : 0], zr = a.rq.zero[a.rq_per_col ? cc : 0];
            const float tj = XZ ? tcol[cl] : 0.0f;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int rl0 = wm * 64 + i * 32 + 4 * h;
                float v[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int rl = rl0 + (r & 3) + 8 * (r >> 2);
                    const float t = XZ ? fmaf(-rzx[rl], tj, acco[i][j][r]) : acco[i][j][r];
                    v[r] = fmaf(rsx[rl], t, bias);
                }
                if constexpr (EPI == GQ_CODES_GELU) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) mine[r * 64] = v[r];
#pragma unroll 1
                    for (int r = 0; r < 16; ++r) {
                        const int rl = rl0 + (r & 3) + 8 * (r >> 2);
                        bool b1 = false;
                        img[gq_img(rl, cl)] = (uint8_t)qe_rq_code(qe_gelu(mine[r * 64]), sc, zr, a.rq, b1);
                        bad |= b1 && m0 + rl < a.B && c < a.O;
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int rl = rl0 + (r & 3) + 8 * (r >> 2);
                        bool b1 = false;
                        img[gq_img(rl, cl)] = (uint8_t)qe_rq_code(v[r], sc, zr, a.rq, b1);
                        bad |= b1 && m0 + rl < a.B && c < a.O;
                    }
                }
            }
        }
        __syncthreads();                                  // the image is complete
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int p = tid + 256 * k, rl = p >> 3, pc = p & 7;
            const uint4 v = *reinterpret_cast<const uint4 *>(img + gq_img(rl, 16 * pc));
            const int64_t row = m0 + rl;
            const int c16 = n0 + 16 * pc;                 // O % 16 == 0: a piece lies wholly below O or wholly beyond it
            if (row < a.B && c16 < a.O) *reinterpret_cast<uint4 *>(a.codes + row * a.O + c16) = v;
        }
        if (__builtin_amdgcn_ballot_w64(bad) != 0ull && lane == 0 && a.status != nullptr) atomicOr(a.status, 1);
        return;
    }
    // D has the batch row on the register and the feature on the lane.  Each wave turns its 32 x 32 tiles through a private
    // LDS patch (the stage buffers are free now) and writes 8 rows x 128 contiguous bytes per store instruction.  (A wave's
    // own LDS operations complete in order: its reads see its writes, a later tile's writes cannot overtake them.)
    // (twin: linear_grp_mfma_kernel's patch store)
    float *patch = reinterpret_cast<float *>(lsm) + wave * (32 * 36);
    const int rrow = lane >> 3, rq = lane & 7;
    const bool vec4 = (a.O & 3) == 0 && (reinterpret_cast<uintptr_t>(a.out) & 15) == 0 &&
                      (EPI != GQ_RES || (reinterpret_cast<uintptr_t>(a.res) & 15) == 0);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int c = n0 + wn * 64 + j * 32 + col;
        const float bias = a.bias != nullptr ? a.bias[min(c, a.O - 1)] : 0.0f;
        const float tj = XZ ? tcol[wn * 64 + j * 32 + col] : 0.0f;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int rl0 = wm * 64 + i * 32 + 4 * h;     // + (r & 3) + 8 (r >> 2): register r's row in the tile
            const int64_t row0 = m0 + wm * 64 + i * 32;
            float v[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int rl = rl0 + (r & 3) + 8 * (r >> 2);
                const float t = XZ ? fmaf(-rzx[rl], tj, acco[i][j][r]) : acco[i][j][r];
                v[r] = fmaf(rsx[rl], t, bias);
            }
            if (vec4) {
                const int c4 = n0 + wn * 64 + j * 32 + 4 * rq;       // O % 4 == 0: a piece lies wholly below O or wholly beyond it
                float4 r4v[4] = {};                       // GQ_RES: the tile's residual pieces, in flight under the transposition
                if constexpr (EPI == GQ_RES) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int64_t row = row0 + 8 * k + rrow;
                        if (row < a.B && c4 < a.O) r4v[k] = *reinterpret_cast<const float4 *>(a.res + row * a.O + c4);
                    }
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) patch[((r & 3) + 8 * (r >> 2) + 4 * h) * 36 + col] = v[r];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int rt = 8 * k + rrow;
                    float4 o4 = *reinterpret_cast<const float4 *>(patch + rt * 36 + 4 * rq);
                    if constexpr (EPI == GQ_RES) { o4.x += r4v[k].x; o4.y += r4v[k].y; o4.z += r4v[k].z; o4.w += r4v[k].w; }
                    const int64_t row = row0 + rt;
                    if (row < a.B && c4 < a.O) *reinterpret_cast<float4 *>(a.out + row * a.O + c4) = o4;
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int64_t row = row0 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    if (row < a.B && c < a.O) a.out[row * a.O + c] = EPI == GQ_RES ? v[r] + a.res[row * a.O + c] : v[r];
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Host side: one plan, read by the path and workspace queries and by the launch.  No HIP call in it.
// ---------------------------------------------------------------------------------------------
struct LinGrpI8Plan {
    int fast;               // 1: linear_grp_i8_mfma_kernel, 0: linear_grp_i8_plain_kernel
    GrpI8Instance inst;     // the fast kernel's instance
    int64_t blocks;
    int epi;                // the epilogue the kernel runs: the request's on a fused plan, GQ_F32 on a two-pass plan
    int two_pass;           // a fused form's request the kernel cannot finish: y into the workspace, then the elementwise pass
    size_t ws;              // workspace bytes (y of a two-pass plan)
};

// a validated request (check_grp_i8; check_grp_rq for the re-quantising form).  epi: the form asked for; rq and codes (its
// address alone; NULL reads as aligned) belong to GQ_CODES*
LinGrpI8Plan plan_grp_i8(const qe_qparam *x, const qe_qparam *w, int G, int x_symmetric, int w_symmetric, int64_t B, int K, int O,
                         int epi = GQ_F32, const qe_requant *rq = nullptr, const void *codes = nullptr)
{
    LinGrpI8Plan p = {};
    p.fast = grp_weights_fast(w, G) && x->n_bits == 8 && K > 0 && aligned16(x->data);
    p.inst = grp_i8_instance(w, x_symmetric, w_symmetric);
    p.blocks = p.fast ? ceil_div64(B, GQ_T) * ceil_div64(O, GQ_T) : ceil_div64(B * O, 256);
    const bool codes_form = epi == GQ_CODES || epi == GQ_CODES_GELU;
    const bool fused = p.fast && (!codes_form || (rq->n_bits == 8 && O % 16 == 0 && aligned16(codes)));
    p.two_pass = epi != GQ_F32 && !fused;
    p.epi = p.two_pass ? (int)GQ_F32 : epi;
    p.ws = p.two_pass ? (size_t)B * (size_t)O * sizeof(float) : 0;
    return p;
}

int check_grp_i8(const qe_qparam *x, const qe_qparam *w, int G, int64_t B, int K, int O)
{
    if (B < 0 || K < 0 || O < 0) return QE_ERR_ARG;
    if (int rc = check_operand(x)) return rc;
    if (int rc = check_grp_weights(w, G, K, O)) return rc;
    return one_or_per_channel(x->n_param, B) ? QE_OK : QE_ERR_ARG;
}

// ... then the consumer's quantiser and the activation of the re-quantising form
int check_grp_rq(const qe_requant *rq, int act, int O)
{
    if (int rc = check_requant(rq)) return rc;
    if (!one_or_per_channel(rq->n_param, O)) return QE_ERR_ARG;
    return act == QE_ACT_NONE || act == QE_ACT_GELU ? QE_OK : QE_ERR_ARG;
}

template <int WB, bool WZ, bool XZ>
void launch_grp_i8(const LinGrpI8Plan &p, const LinGrpI8Args &a, hipStream_t s)
{
    const unsigned blocks = (unsigned)p.blocks;
    switch (p.epi) {
    case GQ_RES: launch_instance<&linear_grp_i8_mfma_kernel<WB, WZ, XZ, GQ_RES>>(blocks, 256, GQ_LDS, 0, s, a); break;
    case GQ_CODES: launch_instance<&linear_grp_i8_mfma_kernel<WB, WZ, XZ, GQ_CODES>>(blocks, 256, GQ_LDS, 0, s, a); break;
    case GQ_CODES_GELU: launch_instance<&linear_grp_i8_mfma_kernel<WB, WZ, XZ, GQ_CODES_GELU>>(blocks, 256, GQ_LDS, 0, s, a); break;
    default: launch_instance<&linear_grp_i8_mfma_kernel<WB, WZ, XZ, GQ_F32>>(blocks, 256, GQ_LDS, 0, s, a); break;
    }
}

// One form's request, validated and planned in one place for its path query, its workspace query and its run.  epi: the form
// (GQ_CODES stands for both code forms in a query); rq, act and codes belong to the code forms.  rc != QE_OK: no plan.
struct LinGrpI8Request {
    const qe_qparam *x, *w;
    int G;
    int64_t B;
    int K, O;
    int rc;
    LinGrpI8Plan plan;
};

LinGrpI8Request request_grp_i8(const qe_qparam *x, const qe_qparam *w, int G, int x_symmetric, int w_symmetric, int64_t B, int K, int O,
                               int epi = GQ_F32, const qe_requant *rq = nullptr, int act = QE_ACT_NONE, const void *codes = nullptr)
{
    LinGrpI8Request r = {x, w, G, B, K, O, check_grp_i8(x, w, G, B, K, O), {}};
    if (r.rc == QE_OK && (epi == GQ_CODES || epi == GQ_CODES_GELU)) r.rc = check_grp_rq(rq, act, O);
    if (r.rc == QE_OK) r.plan = plan_grp_i8(x, w, G, x_symmetric, w_symmetric, B, K, O, epi, rq, codes);
    return r;
}

// The kernel of a request's plan; the request is valid and not empty.  `a` carries the destination of the plan's epilogue.
int run_grp_i8(const LinGrpI8Request &r, LinGrpI8Args a, const float *bias, hipStream_t s)
{
    const LinGrpI8Plan &p = r.plan;
    fill_grp_operands(a, r.x, r.w, bias, r.G, r.K);
    a.x_per_row = r.x->n_param != 1; a.B = r.B; a.K = r.K; a.O = r.O;
    return launch_grp<&linear_grp_i8_plain_kernel>(p.fast, p.blocks, a, s, [&] {
        dispatch_grp_i8(p.inst, [&](auto wb, auto wz, auto xz) {
            launch_grp_i8<decltype(wb)::value, decltype(wz)::value, decltype(xz)::value>(p, a, s);
        });
    });
}

bool workspace_ok(const LinGrpI8Plan &p, const void *workspace, size_t workspace_bytes)
{
    return p.ws == 0 || (workspace != nullptr && workspace_bytes >= p.ws && aligned16(workspace));
}

}  // namespace

}  // namespace qe

extern "C" int qe_quantlinear_grouped_path(const qe_qparam *x, const qe_qparam *w, int32_t group_size, int32_t x_symmetric,
                                           int32_t w_symmetric, int64_t B, int32_t K, int32_t O)
{
    const qe::LinGrpI8Request r = qe::request_grp_i8(x, w, group_size, x_symmetric, w_symmetric, B, K, O);
    return r.rc == QE_OK && r.plan.fast;
}

extern "C" int qe_quantlinear_grouped(const qe_qparam *x, const qe_qparam *w, int32_t group_size, int32_t x_symmetric,
                                      int32_t w_symmetric, const float *bias, int64_t B, int32_t K, int32_t O, float *out,
                                      qe_stream_t stream)
{
    using namespace qe;
    const LinGrpI8Request r = request_grp_i8(x, w, group_size, x_symmetric, w_symmetric, B, K, O);
    if (r.rc != QE_OK) return r.rc;
    if (out == nullptr && B * O > 0) return QE_ERR_ARG;
    if (B == 0 || O == 0) return QE_OK;
    LinGrpI8Args a = {};
    a.out = out;
    return run_grp_i8(r, a, bias, static_cast<hipStream_t>(stream));
}

// Fused forms (include/quant_engine.h): the consumer's codes of y / gelu(y), and y + residual.  Path 1 is the fast kernel with
// the epilogue compiled in, path 0 the plan's two passes: y into the workspace on whichever kernel the plain plan names, then
// qe_quantize_pack_act or the elementwise add.
extern "C" int qe_quantlinear_grouped_requant_path(const qe_qparam *x, const qe_qparam *w, int32_t group_size, int32_t x_symmetric,
                                                   int32_t w_symmetric, int64_t B, int32_t K, int32_t O, const qe_requant *rq,
                                                   const uint8_t *codes)
{
    const qe::LinGrpI8Request r = qe::request_grp_i8(x, w, group_size, x_symmetric, w_symmetric, B, K, O, qe::GQ_CODES, rq, QE_ACT_NONE, codes);
    return r.rc == QE_OK && !r.plan.two_pass;
}

extern "C" size_t qe_quantlinear_grouped_requant_workspace_size(const qe_qparam *x, const qe_qparam *w, int32_t group_size,
                                                                 int32_t x_symmetric, int32_t w_symmetric, int64_t B, int32_t K,
                                                                 int32_t O, const qe_requant *rq, const uint8_t *codes)
{
    const qe::LinGrpI8Request r = qe::request_grp_i8(x, w, group_size, x_symmetric, w_symmetric, B, K, O, qe::GQ_CODES, rq, QE_ACT_NONE, codes);
    return r.rc == QE_OK ? r.plan.ws : 0;
}

extern "C" int qe_quantlinear_grouped_requant(const qe_qparam *x, const qe_qparam *w, int32_t group_size, int32_t x_symmetric,
                                              int32_t w_symmetric, const float *bias, int64_t B, int32_t K, int32_t O, int32_t act,
                                              const qe_requant *rq, uint8_t *codes, int32_t *status, void *workspace,
                                              size_t workspace_bytes, qe_stream_t stream)
{
    using namespace qe;
    const LinGrpI8Request r = request_grp_i8(x, w, group_size, x_symmetric, w_symmetric, B, K, O,
                                             act == QE_ACT_GELU ? GQ_CODES_GELU : GQ_CODES, rq, act, codes);
    if (r.rc != QE_OK) return r.rc;
    if (codes == nullptr && B * O > 0) return QE_ERR_ARG;
    if (B == 0 || O == 0) return QE_OK;
    if (!workspace_ok(r.plan, workspace, workspace_bytes)) return QE_ERR_WORKSPACE;
    LinGrpI8Args a = {};
    a.out = static_cast<float *>(workspace);
    a.codes = codes; a.status = status; a.rq_per_col = rq->n_param != 1; a.rq = make_qe_rq(*rq);
    if (int rc = run_grp_i8(r, a, bias, static_cast<hipStream_t>(stream))) return rc;
    if (!r.plan.two_pass) return QE_OK;
    // per-feature rq: channel = output feature o, element (b, o) -> (i / 1) % O
    return qe_quantize_pack_act(a.out, B * (int64_t)O, act, rq->scale, rq->zero, rq->n_param, 1, rq->qmin, rq->qmax, rq->n_bits,
                                rq->sign, codes, nullptr, status, stream);
}

extern "C" int qe_quantlinear_grouped_residual_path(const qe_qparam *x, const qe_qparam *w, int32_t group_size, int32_t x_symmetric,
                                                    int32_t w_symmetric, int64_t B, int32_t K, int32_t O)
{
    const qe::LinGrpI8Request r = qe::request_grp_i8(x, w, group_size, x_symmetric, w_symmetric, B, K, O, qe::GQ_RES);
    return r.rc == QE_OK && !r.plan.two_pass;
}

extern "C" size_t qe_quantlinear_grouped_residual_workspace_size(const qe_qparam *x, const qe_qparam *w, int32_t group_size,
                                                                  int32_t x_symmetric, int32_t w_symmetric, int64_t B, int32_t K,
                                                                  int32_t O)
{
    const qe::LinGrpI8Request r = qe::request_grp_i8(x, w, group_size, x_symmetric, w_symmetric, B, K, O, qe::GQ_RES);
    return r.rc == QE_OK ? r.plan.ws : 0;
}

extern "C" int qe_quantlinear_grouped_residual(const qe_qparam *x, const qe_qparam *w, int32_t group_size, int32_t x_symmetric,
                                               int32_t w_symmetric, const float *bias, int64_t B, int32_t K, int32_t O,
                                               const float *residual, float *out, void *workspace, size_t workspace_bytes,
                                               qe_stream_t stream)
{
    using namespace qe;
    const LinGrpI8Request r = request_grp_i8(x, w, group_size, x_symmetric, w_symmetric, B, K, O, GQ_RES);
    if (r.rc != QE_OK) return r.rc;
    if ((residual == nullptr || out == nullptr) && B * O > 0) return QE_ERR_ARG;
    if (B == 0 || O == 0) return QE_OK;
    const int64_t n = B * (int64_t)O;
    const Span so = span_of(out, n * 4);
    if (!same_or_disjoint(residual, out, n * 4) || overlaps(so, span_of(x->data, qe_packed_nbytes(B * (int64_t)K, x->n_bits))) ||
        overlaps(so, span_of(w->data, qe_packed_nbytes((int64_t)O * K, w->n_bits))))
        return QE_ERR_ARG;
    const LinGrpI8Plan &p = r.plan;
    if (!workspace_ok(p, workspace, workspace_bytes)) return QE_ERR_WORKSPACE;
    LinGrpI8Args a = {};
    a.out = p.two_pass ? static_cast<float *>(workspace) : out;
    a.res = residual;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = run_grp_i8(r, a, bias, s)) return rc;
    return p.two_pass ? launch_add_residual(a.out, residual, out, n, s) : QE_OK;
}

