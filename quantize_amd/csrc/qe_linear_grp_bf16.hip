// qe_linear_grp_bf16.hip -- qe_quantlinear_grouped_bf16_input: bf16 rows x group-quantised (AWQ layout) weight codes, "W4A16".
//
//   out[b,o] = bias[o] + sum_g sw[o,g] * sum_{k in group g} x'[b,k] (q_w[o,k] - zw[o,g])   (+ residual[b,o])
//   x'[b,k]  = x[b,k]  |  bf16_rne(float(x[b,k]) * x_mul[k])  with an x_mul: one fp32 multiply, rounded once to bf16
//
// qe_quantlinear_grouped_float_input's contract (qe_linear_grp.hip) on rows that are bf16 in memory, as the bf16 attention
// cores write them.  A unit of its own, so that no other code object moves; the weight operand's check, its side of fast
// eligibility, the fold of a group and the launch tail are qe_grp_common.hpp's.
//
// Fast kernel (4- and 8-bit codes, G in {32, 64, 128}, K % 32 == 0, 16-byte aligned x, x_mul and weight stream).  A lane's A
// fragment of v_mfma_f32_32x32x16_bf16 is 8 consecutive k of a stored row, 16 bytes as loaded: one MFMA per product where
// linear_grp_mfma_kernel's exact three-way split issues three, no conversion, half the activation bytes.  The codes are
// centred per (row, group) on c = linf_centre(zw[o,g]), so |q - c| <= 255 is bf16-exact and every product is exact in fp32;
// the fp32 accumulation and the fp32 group sum S_x round.  At each group boundary
//   acc_out += sw[o,g] (acc_g - (zw[o,g] - c) S_x[b,g]),   S_x[b,g] = sum_{k in g} x'[b,k],   acc_g = 0
// and the symmetric instance (declared by the caller) has no S_x and no second term.
// Workgroup = 2 x 2 waves, tile 128 x 128, wave 64 x 64 = 2 x 2 MFMA tiles, two accumulator sets of 64 registers.
// Stage = 64 k = two HALVES of 32 k: with one activation image where the fp32-row kernel holds three, a stage buffer of the
// same 32 KB holds twice the depth, and a barrier is paid once per 64 k.  TWO stage buffers ([128][64] bf16 activation and
// weight images, 128-byte rows, the 16-byte piece p of row r at p ^ (r & 7)) and one barrier per stage: behind the barrier
// of stage s the loads of stage s + 1 are issued, the MFMAs of stage s run, and the loaded registers go into the other
// buffer, which every wave left before it reached that barrier (as linear_bf16in_kernel).  A group ends with a half
// ((half & (G / 32 - 1)) == G / 32 - 1), so a stage folds twice (G = 32), once (G = 64) or every other time (G = 128).
// K % 64 == 32 ends in a half stage: its second half is fetched from the first half's (valid) addresses, staged, kept out
// of S_x and never multiplied (as conv_awq_mfma_kernel's).
// A weight staging thread owns the 32 codes of one half of a row: 32 bytes of an 8-bit stream, 16 of a 4-bit one, which
// become bf16 of u - wshift in registers -- no widened copy of the weights exists.  An activation staging thread owns one
// 16-byte piece of two rows in each half; its shares of S_x go through shuffles into sxg[group & 3][row] (a stage of G = 32
// holds two groups, and a fast wave stages the next stage while a slow one still folds this one: four slots, not two).
// With an x_mul (a wave-uniform branch) the staging thread unpacks its bf16 pairs, multiplies in fp32 and rounds back with
// v_cvt_pk_bf16_f32; S_x sums the rounded values, the ones the matrix cores multiply.
// Rows beyond B and columns beyond O read a clamped, valid address (the residual included) and are dropped at the store:
// no load sits under a per-lane condition.  The result leaves through the wave's LDS patch as 16-byte row pieces (O % 4 == 0
// and aligned out / residual; element stores otherwise).  The residual form is a template instance: (acc + bias) + residual,
// the non-residual result plus one fp32 add, bit for bit.
// A NaN or inf in a row of x makes that row's outputs non-finite and no other row's (as qe_quantlinear_bf16_input).
//
// Plain kernel (everything else): one thread per output, the bf16 rows read directly, group by group in k order.
#include "qe_grp_common.hpp"
#include "qe_linear_bf16in.hpp"      // linf_centre

namespace qe {

namespace {

typedef __bf16 v8bf_h __attribute__((ext_vector_type(8)));
typedef __bf16 v2bf_h __attribute__((ext_vector_type(2)));
typedef float v2f_h __attribute__((ext_vector_type(2)));
typedef float v16f_h __attribute__((ext_vector_type(16)));

constexpr int LH_T = 128, LH_K = 64, LH_HALF = 32;
constexpr int LH_PLANE = LH_T * LH_K * 2;                 // bytes of one [128][64] bf16 image (16 KB)
constexpr int LH_BUF = 2 * LH_PLANE;                      // one stage buffer: the activation image, the weight image
constexpr size_t LH_LDS = (size_t)2 * LH_BUF + 4 * LH_T * sizeof(float);   // + S_x[group & 3][row]

struct LinGrpBf16Args {
    const uint16_t *x;      // B x K bf16 bit patterns
    const float *x_mul;
    const uint8_t *w;
    const float *w_scale, *w_zero, *bias;
    const float *res;       // residual form: out = y + res (res == out allowed)
    float *out;
    int w_bits, w_sign;
    int G, NG;              // group size, groups per row (K / G)
    int64_t B;
    int K, O;
};

// the two bf16 of a register as fp32 (exact: a bf16 is the upper half of an fp32)  (twin: qe_linear_bf16in.hip)
__device__ __forceinline__ float bf_lo(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf_hi(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }
// two fp32 -> two bf16, round to nearest even (v_cvt_pk_bf16_f32), `lo` in the low half
__device__ __forceinline__ uint32_t pack_bf16_rne(float lo, float hi)
{
    const v2f_h f = {lo, hi};
    const v2bf_h b = __builtin_convertvector(f, v2bf_h);
    return __builtin_bit_cast(uint32_t, b);
}
// two integers of magnitude <= 255 as fp32 -> two bf16 (exact: the upper halves)
__device__ __forceinline__ uint32_t pack_bf16_exact(float lo, float hi)
{
    return __builtin_amdgcn_perm(__float_as_uint(hi), __float_as_uint(lo), 0x07060302u);
}
// x' of a register's bf16 pair
__device__ __forceinline__ uint32_t mul_pair(uint32_t w, float m0, float m1) { return pack_bf16_rne(bf_lo(w) * m0, bf_hi(w) * m1); }
__device__ __forceinline__ float sum8(uint4 x)
{
    return ((bf_lo(x.x) + bf_hi(x.x)) + (bf_lo(x.y) + bf_hi(x.y))) + ((bf_lo(x.z) + bf_hi(x.z)) + (bf_lo(x.w) + bf_hi(x.w)));
}

// ---------------------------------------------------------------------------------------------
// Plain kernel: thread <-> output (b, o), o fastest.  (twin: linear_grp_plain_kernel)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void linear_grp_bf16_plain_kernel(const LinGrpBf16Args a)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.B * a.O) return;
    const int64_t b = idx / a.O;
    const int o = (int)(idx - b * a.O);
    const uint16_t *xr = a.x + b * a.K;
    float acc = 0.0f;
    for (int g = 0; g < a.NG; ++g) {
        const float sw = a.w_scale[(int64_t)o * a.NG + g], zw = a.w_zero[(int64_t)o * a.NG + g];
        float t = 0.0f;
        for (int k = g * a.G; k < (g + 1) * a.G; ++k) {
            float xv = __uint_as_float((uint32_t)xr[k] << 16);
            if (a.x_mul != nullptr) xv = bf_lo(pack_bf16_rne(xv * a.x_mul[k], 0.0f));
            t = fmaf(xv, (float)unpack_elem(a.w, (int64_t)o * a.K + k, a.w_bits, a.w_sign) - zw, t);
        }
        acc = fmaf(sw, t, acc);
    }
    float y = acc + (a.bias != nullptr ? a.bias[o] : 0.0f);
    if (a.res != nullptr) y += a.res[idx];
    a.out[idx] = y;
}

// ---------------------------------------------------------------------------------------------
// Fast kernel.  WB: bits of a stored code (4 | 8).  SX: the asymmetric form (S_x and the (zw - c) term).  RES: + residual.
// ---------------------------------------------------------------------------------------------
template <int WB, bool SX, bool RES>
__global__ __launch_bounds__(256, 2) void linear_grp_bf16_mfma_kernel(const LinGrpBf16Args a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lsm[];
    float *sxg = reinterpret_cast<float *>(lsm + 2 * LH_BUF);        // [4][128]: S_x of the tile's rows, by group & 3

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave & 1, wn = wave >> 1;
    const int col = lane & 31, h = lane >> 5;
    const int n_ct = (a.O + LH_T - 1) / LH_T;
    const int64_t bid = blockIdx.x;
    const int ct = (int)(bid % n_ct);
    const int64_t m0 = (bid / n_ct) * LH_T;
    const int n0 = ct * LH_T;
    const int gmask = a.G / LH_HALF - 1;                  // halves per group - 1 (0, 1 or 3)
    const int gsh = a.G == 32 ? 0 : a.G == 64 ? 1 : 2;    // half -> group
    const int n_halves = a.K / LH_HALF, n_stages = (n_halves + 1) >> 1;
    const int k_last = a.K - LH_HALF;                     // where the last half starts: the clamp of a half stage

    // activations: thread <-> (row r = (tid >> 2) + 64 i, 16-byte piece ap = tid & 3 of each half's 64 bytes of that row)
    const int ap = tid & 3;
    const uint16_t *xrow[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int r = (tid >> 2) + 64 * i;
        const int64_t row = (m0 + r < a.B) ? m0 + r : a.B - 1;
        xrow[i] = a.x + row * a.K + 8 * ap;
    }
    const float *xmp = a.x_mul != nullptr ? a.x_mul + 8 * ap : nullptr;
    // weights: thread <-> (column c = tid >> 1, half whh = tid & 1): 32 bytes of an 8-bit row, 16 of a 4-bit one
    const int wc = tid >> 1, whh = tid & 1;
    const int wcc = (n0 + wc < a.O) ? n0 + wc : a.O - 1;
    const uint8_t *wrow = a.w + (int64_t)wcc * a.K * WB / 8;
    const float *zrow = a.w_zero + (int64_t)wcc * a.NG;
    const float woff = a.w_sign ? (float)(1 << (WB - 1)) : 0.0f;     // stored u -> q = u - woff

    uint4 xv[2][2], wv[2] = {make_uint4(0u, 0u, 0u, 0u), make_uint4(0u, 0u, 0u, 0u)};
    float4 xm[2][2];
    float zwv = 0.0f;
    auto fetch = [&](int st) __attribute__((always_inline)) {
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            const int k0 = min(st * LH_K + hf * LH_HALF, k_last);
#pragma unroll
            for (int i = 0; i < 2; ++i) xv[hf][i] = *reinterpret_cast<const uint4 *>(xrow[i] + k0);
            if (xmp != nullptr) {                         // (uniform)
                xm[hf][0] = *reinterpret_cast<const float4 *>(xmp + k0);
                xm[hf][1] = *reinterpret_cast<const float4 *>(xmp + k0 + 4);
            }
        }
        const int kw = min(st * LH_K + whh * LH_HALF, k_last);
        if constexpr (WB == 8) {
            wv[0] = *reinterpret_cast<const uint4 *>(wrow + kw);
            wv[1] = *reinterpret_cast<const uint4 *>(wrow + kw + 16);
        } else {
            wv[0] = *reinterpret_cast<const uint4 *>(wrow + kw / 2);
        }
        zwv = zrow[(kw >> 5) >> gsh];
    };
    float sx[2] = {0.0f, 0.0f};                          // this thread's share of S_x[., g] of its two rows
    auto stage = [&](int st) __attribute__((always_inline)) {
        uint8_t *base = lsm + (st & 1) * LH_BUF;
        const int sr = (tid >> 2) & 7;                    // r & 7 of both rows
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            const int hs = 2 * st + hf;
            const bool live = hs < n_halves;              // (uniform) false: the clamped half of a half stage
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int r = (tid >> 2) + 64 * i;
                uint4 x = xv[hf][i];
                if (xmp != nullptr) {                     // (uniform) x' = bf16_rne(x * x_mul)
                    x.x = mul_pair(x.x, xm[hf][0].x, xm[hf][0].y); x.y = mul_pair(x.y, xm[hf][0].z, xm[hf][0].w);
                    x.z = mul_pair(x.z, xm[hf][1].x, xm[hf][1].y); x.w = mul_pair(x.w, xm[hf][1].z, xm[hf][1].w);
                }
                if constexpr (SX) { if (live) sx[i] += sum8(x); }
                *reinterpret_cast<uint4 *>(base + r * 128 + 16 * ((4 * hf + ap) ^ sr)) = x;   // x_mul == NULL: the operand as loaded
            }
            if constexpr (SX) {
                if (live && (hs & gmask) == gmask) {      // the group's last half: the 4 threads of a row add their shares
                    float *dst = sxg + ((hs >> gsh) & 3) * LH_T;
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        float v = sx[i];
                        v += __shfl_xor(v, 1); v += __shfl_xor(v, 2);
                        if (ap == 0) dst[(tid >> 2) + 64 * i] = v;
                        sx[i] = 0.0f;
                    }
                }
            }
        }
        // 32 codes -> 32 bf16 of u - wshift = q - c: the four 16-byte pieces of half whh of the row
        // (twin: linear_grp_mfma_kernel's decode; here a nibble word is split into its even and odd codes first, so that
        // every code is a byte of a register and converts with one v_cvt_f32_ubyte)
        const float wshift = woff + linf_centre(zwv, a.w_sign);
        const uint32_t ww[8] = {wv[0].x, wv[0].y, wv[0].z, wv[0].w, wv[1].x, wv[1].y, wv[1].z, wv[1].w};
        uint8_t *wd = base + LH_PLANE + wc * 128;
        const int sw7 = wc & 7;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            uint32_t pk[4];
            if constexpr (WB == 8) {                      // words 2 t, 2 t + 1: codes 8 t .. 8 t + 7, one per byte
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t w = ww[2 * t + (j >> 1)];
                    const int s = 16 * (j & 1);
                    pk[j] = pack_bf16_exact((float)((w >> s) & 0xffu) - wshift, (float)((w >> (s + 8)) & 0xffu) - wshift);
                }
            } else {                                      // word t: byte j holds code 2 j in its low nibble, 2 j + 1 in its high one
                const uint32_t e = ww[t] & 0x0f0f0f0fu, o = (ww[t] >> 4) & 0x0f0f0f0fu;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    pk[j] = pack_bf16_exact((float)((e >> (8 * j)) & 0xffu) - wshift, (float)((o >> (8 * j)) & 0xffu) - wshift);
            }
            *reinterpret_cast<uint4 *>(wd + 16 * ((4 * whh + t) ^ sw7)) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
        }
    };

    v16f_h accg[2][2], acco[2][2];                        // the running group, the folded total
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) { accg[i][j][r] = 0.0f; acco[i][j][r] = 0.0f; }

    // this lane's two output features (clamped) in the (o, g) arrays
    int64_t og[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) og[j] = (int64_t)min(n0 + wn * 64 + j * 32 + col, a.O - 1) * a.NG;

    const int swz = col & 7;                              // r & 7 of this lane's rows of either image
    const int a_off = (wm * 64 + col) * 128, b_off = LH_PLANE + (wn * 64 + col) * 128;
    fetch(0);
    stage(0);
    for (int st = 0; st < n_stages; ++st) {
        // buffer st & 1 is complete (and S_x of the groups that end in it); every wave has left buffer (st + 1) & 1
        __syncthreads();
        const bool more = st + 1 < n_stages;
        if (more) fetch(st + 1);                          // in flight under the MFMAs
        const uint8_t *buf = lsm + (st & 1) * LH_BUF;
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            const int hs = 2 * st + hf;
            if (hs < n_halves) {                          // (uniform) false: the clamped half of a half stage, never multiplied
                const bool fold = (hs & gmask) == gmask;  // (uniform)
                float gsw[2] = {0.0f, 0.0f}, gdz[2] = {0.0f, 0.0f};
                if (fold) {
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        gsw[j] = a.w_scale[og[j] + (hs >> gsh)];
                        if constexpr (SX) { const float zw = a.w_zero[og[j] + (hs >> gsh)]; gdz[j] = zw - linf_centre(zw, a.w_sign); }
                    }
                }
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const int po = 16 * ((4 * hf + 2 * ks + h) ^ swz);
                    v8bf_h fa[2], fb[2];
#pragma unroll
                    for (int i = 0; i < 2; ++i) fa[i] = *reinterpret_cast<const v8bf_h *>(buf + a_off + i * 32 * 128 + po);
#pragma unroll
                    for (int j = 0; j < 2; ++j) fb[j] = *reinterpret_cast<const v8bf_h *>(buf + b_off + j * 32 * 128 + po);
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < 2; ++j) accg[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], accg[i][j], 0, 0, 0);
                }
                if (fold) {
                    const float *sxr = sxg + ((hs >> gsh) & 3) * LH_T + wm * 64 + 4 * h;
                    grp_fold<SX>(accg, acco, gsw, gdz, [&](int i, int r) { return sxr[i * 32 + (r & 3) + 8 * (r >> 2)]; });
                }
            }
        }
        if (more) stage(st + 1);
    }
    __syncthreads();                                      // every wave is done with the stage buffers
    // D has the batch row on the register and the feature on the lane.  Each wave turns its 32 x 32 tiles through a private
    // LDS patch (the stage buffers are free now) and writes 8 rows x 128 contiguous bytes per store instruction.  (A wave's
    // own LDS operations complete in order: its reads see its writes, a later tile's writes cannot overtake them.)
    // (twin: linear_bf16in_kernel's patch store)
    float *patch = reinterpret_cast<float *>(lsm) + wave * (32 * 36);
    const int rrow = lane >> 3, rq = lane & 7;
    const bool vec4 = (a.O & 3) == 0 && ((reinterpret_cast<uintptr_t>(a.out) | reinterpret_cast<uintptr_t>(a.res)) & 15) == 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int c = n0 + wn * 64 + j * 32 + col;
        const int ccl = min(c, a.O - 1);
        const float bias = a.bias != nullptr ? a.bias[ccl] : 0.0f;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int64_t row0 = m0 + wm * 64 + i * 32;
            if (vec4) {
#pragma unroll
                for (int r = 0; r < 16; ++r) patch[((r & 3) + 8 * (r >> 2) + 4 * h) * 36 + col] = acco[i][j][r] + bias;
                const int c4 = n0 + wn * 64 + j * 32 + 4 * rq;
                const int c4c = min(c4, a.O - 4);         // O % 4 == 0: a piece lies wholly below O or wholly beyond it
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int rt = 8 * k + rrow;
                    float4 o4 = *reinterpret_cast<const float4 *>(patch + rt * 36 + 4 * rq);
                    const int64_t row = row0 + rt;
                    if constexpr (RES) {
                        // from a clamped, valid address whatever the lane's row and column: the value is dropped with the store
                        const float4 r4 = *reinterpret_cast<const float4 *>(a.res + min(row, a.B - 1) * a.O + c4c);
                        o4.x += r4.x; o4.y += r4.y; o4.z += r4.z; o4.w += r4.w;
                    }
                    if (row < a.B && c4 < a.O) *reinterpret_cast<float4 *>(a.out + row * a.O + c4) = o4;
                    if constexpr (RES) __builtin_amdgcn_sched_barrier(0);   // one residual piece in flight (else scratch)
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int64_t row = row0 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    float o = acco[i][j][r] + bias;
                    if constexpr (RES) o += a.res[min(row, a.B - 1) * a.O + ccl];
                    if (row < a.B && c < a.O) a.out[row * a.O + c] = o;
                    if constexpr (RES) __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Host side: one plan, read by the path query and by the launch.  No HIP call in it.
// ---------------------------------------------------------------------------------------------
struct LinGrpBf16Plan {
    int fast;               // 1: linear_grp_bf16_mfma_kernel, 0: linear_grp_bf16_plain_kernel
    int w4, sx;             // the fast kernel's instance (the residual form follows the call)
    int64_t blocks;
};

// a validated request (check_grp_bf16); a query leaves the pointers it does not know null, which reads as aligned
LinGrpBf16Plan plan_grp_bf16(const uint16_t *x, const float *x_mul, const qe_qparam *w, int G, int symmetric, int64_t B, int K, int O)
{
    LinGrpBf16Plan p = {};
    p.fast = grp_weights_fast(w, G) && K > 0 && K % LH_HALF == 0 && aligned16(x) && aligned16(x_mul);
    p.w4 = w->n_bits == 4;
    p.sx = symmetric == 0;
    p.blocks = p.fast ? ceil_div64(B, LH_T) * ceil_div64(O, LH_T) : ceil_div64(B * O, 256);
    return p;
}

// (twin: qe_linear_grp.hip's check_grp)
int check_grp_bf16(const qe_qparam *w, int G, int64_t B, int K, int O)
{
    if (B < 0 || K < 0 || O < 0) return QE_ERR_ARG;
    return check_grp_weights(w, G, K, O);
}
inline bool odd_address(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 1) != 0; }

template <bool RES>
void launch_grp_bf16_fast(const LinGrpBf16Plan &p, const LinGrpBf16Args &a, hipStream_t s)
{
    dispatch_flag(p.w4, [&](auto w4) { dispatch_flag(p.sx, [&](auto sx) {
        launch_instance<&linear_grp_bf16_mfma_kernel<decltype(w4)::value ? 4 : 8, decltype(sx)::value, RES>>((unsigned)p.blocks, 256, LH_LDS, LH_LDS, s, a);
    }); });
}

}  // namespace

}  // namespace qe

extern "C" int qe_quantlinear_grouped_bf16_input_path(const uint16_t *x, const float *x_mul, const qe_qparam *w, int32_t group_size,
                                                      int32_t symmetric, int64_t B, int32_t K, int32_t O)
{
    using namespace qe;
    if (check_grp_bf16(w, group_size, B, K, O) != QE_OK || odd_address(x)) return 0;
    return plan_grp_bf16(x, x_mul, w, group_size, symmetric, B, K, O).fast;
}

extern "C" int qe_quantlinear_grouped_bf16_input(const uint16_t *x, const float *x_mul, const qe_qparam *w, int32_t group_size,
                                                 int32_t symmetric, const float *bias, int64_t B, int32_t K, int32_t O,
                                                 const float *residual, float *out, qe_stream_t stream)
{
    using namespace qe;
    if (int rc = check_grp_bf16(w, group_size, B, K, O)) return rc;
    if ((x == nullptr && B * K > 0) || (out == nullptr && B * O > 0)) return QE_ERR_ARG;
    if (B == 0 || O == 0) return QE_OK;
    if (odd_address(x) || (reinterpret_cast<uintptr_t>(out) & 3) != 0 || (reinterpret_cast<uintptr_t>(residual) & 3) != 0) return QE_ERR_ARG;
    if (overlaps(span_of(x, B * (int64_t)K * 2), span_of(out, B * (int64_t)O * 4))) return QE_ERR_ARG;
    if (residual != nullptr && !same_or_disjoint(residual, out, B * (int64_t)O * 4)) return QE_ERR_ARG;
    const LinGrpBf16Plan p = plan_grp_bf16(x, x_mul, w, group_size, symmetric, B, K, O);
    LinGrpBf16Args a = {};
    a.x = x; a.x_mul = x_mul; a.w = w->data; a.w_scale = w->scale; a.w_zero = w->zero; a.bias = bias; a.res = residual; a.out = out;
    a.w_bits = w->n_bits; a.w_sign = w->sign; a.G = group_size; a.NG = K / group_size; a.B = B; a.K = K; a.O = O;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return launch_grp<&linear_grp_bf16_plain_kernel>(p.fast, p.blocks, a, s, [&] {
        if (residual != nullptr) launch_grp_bf16_fast<true>(p, a, s);
        else launch_grp_bf16_fast<false>(p, a, s);
    });
}
