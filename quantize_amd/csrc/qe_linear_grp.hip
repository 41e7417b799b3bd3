// qe_linear_grp.hip -- qe_quantlinear_grouped_float_input: fp32 activations x group-quantised (AWQ layout) weight codes.
//
//   out[b,o] = bias[o] + sum_g sw[o,g] * sum_{k in group g} x'[b,k] (q_w[o,k] - zw[o,g]),   x'[b,k] = x[b,k] x_mul[k]
//
// Group g covers k in [g G, (g + 1) G); sw / zw are fp32 arrays of O (K / G) elements in (o, g) order.  Two kernels and one
// host plan in a unit of its own, so that no other code object moves; the weight operand's check, its side of fast
// eligibility and the launch tail are qe_grp_common.hpp's, shared with the two int8 units.
//
// Fast kernel (4- and 8-bit codes, G in {32, 64, 128}, K % 32 == 0, 16-byte aligned streams): linear_f32_mfma_kernel's
// arithmetic per GROUP.  x' is split exactly into three bf16 parts, the codes are centred on c = linf_centre(zw[o,g]) per (row,
// group) so that |q - c| <= 255 is bf16-exact, and v_mfma_f32_32x32x16_bf16 sums x' (q - c) into a GROUP accumulator: every
// product is exact in fp32, only the accumulation rounds.  At each group boundary (once per G / 32 stages)
//   acc_out += sw[o,g] (acc_g - (zw[o,g] - c) S_x[b,g]),   S_x[b,g] = sum_{k in g} x'[b,k],   acc_g = 0
// with S_x from the staging threads' shares (the 8 threads of a row add theirs) through a small LDS array, two copies by
// group parity.  The symmetric instance (every zw == c, declared by the caller) has no S_x and no second term.
// Workgroup = 2 x 2 waves, tile 128 x 128, wave 64 x 64 = 2 x 2 MFMA tiles x 3 splits, two accumulator sets of 64 registers.
// Stage = 32 k, register staged, TWO stage buffers (3 activation images + 1 weight image each, [128][32] bf16, 16-byte
// pieces XOR-swizzled as in linear_mfma_kernel) and one barrier per stage, as linear_bf16in_kernel.  A weight staging thread
// owns 16 codes of a row per stage: 16 bytes of an 8-bit stream, 8 bytes of a 4-bit one, whose nibbles (low nibble first)
// become bf16 of u - wshift in registers -- no widened copy of the weights exists.  D has the batch row on the register and
// the feature on the lane: a lane needs one sw and one zw per column tile per group, fetched from global memory at the top
// of the group's last stage.  Rows beyond B and columns beyond O read a clamped, valid address and are dropped at the store:
// no load sits under a per-lane condition.
//
// Plain kernel (everything else): one thread per output, fp32, group by group in k order.
#include "qe_grp_common.hpp"
#include "qe_linear_bf16in.hpp"      // linf_centre

namespace qe {

namespace {

typedef __bf16 v8bf_g __attribute__((ext_vector_type(8)));
typedef float v16f_g __attribute__((ext_vector_type(16)));

constexpr int LG_T = 128, LG_K = 32;
constexpr int LG_PLANE = LG_T * LG_K * 2;                 // bytes of one [128][32] bf16 image (8 KB)
constexpr int LG_BUF = 4 * LG_PLANE;                      // one stage buffer: 3 activation split images, 1 weight image
constexpr size_t LG_LDS = (size_t)2 * LG_BUF + 2 * LG_T * sizeof(float);   // + S_x[group parity][row]

struct LinGrpArgs {
    const float *x, *x_mul;
    const uint8_t *w;
    const float *w_scale, *w_zero, *bias;
    float *out;
    int w_bits, w_sign;
    int G, NG;              // group size, groups per row (K / G)
    int64_t B;
    int K, O;
};

// ---------------------------------------------------------------------------------------------
// Plain kernel: thread <-> output (b, o), o fastest.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void linear_grp_plain_kernel(const LinGrpArgs a)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.B * a.O) return;
    const int64_t b = idx / a.O;
    const int o = (int)(idx - b * a.O);
    const float *xr = a.x + b * a.K;
    float acc = 0.0f;
    for (int g = 0; g < a.NG; ++g) {
        const float sw = a.w_scale[(int64_t)o * a.NG + g], zw = a.w_zero[(int64_t)o * a.NG + g];
        float t = 0.0f;
        for (int k = g * a.G; k < (g + 1) * a.G; ++k) {
            const float xv = a.x_mul != nullptr ? xr[k] * a.x_mul[k] : xr[k];
            t = fmaf(xv, (float)unpack_elem(a.w, (int64_t)o * a.K + k, a.w_bits, a.w_sign) - zw, t);
        }
        acc = fmaf(sw, t, acc);
    }
    a.out[idx] = acc + (a.bias != nullptr ? a.bias[o] : 0.0f);
}

// ---------------------------------------------------------------------------------------------
// Fast kernel.  WB: bits of a stored code (4 | 8).  SX: the asymmetric form (S_x and the (zw - c) term).
// ---------------------------------------------------------------------------------------------
template <int WB, bool SX>
__global__ __launch_bounds__(256, 2) void linear_grp_mfma_kernel(const LinGrpArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lsm[];
    float *sxg = reinterpret_cast<float *>(lsm + 2 * LG_BUF);        // [2][128]: S_x of the tile's rows, by group parity

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave & 1, wn = wave >> 1;
    const int col = lane & 31, h = lane >> 5;
    const int n_ct = (a.O + LG_T - 1) / LG_T;
    const int64_t bid = blockIdx.x;
    const int ct = (int)(bid % n_ct);
    const int64_t m0 = (bid / n_ct) * LG_T;
    const int n0 = ct * LG_T;
    const int gmask = a.G / LG_K - 1;                     // stages per group - 1 (0, 1 or 3)
    const int gsh = a.G == 32 ? 0 : a.G == 64 ? 1 : 2;    // stage -> group

    // activations: thread <-> (row r = (tid >> 3) + 32 i, k quad q8 = tid & 7): one float4 per pass i
    const int q8 = tid & 7;
    const float *xrow[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = (tid >> 3) + 32 * i;
        const int64_t row = (m0 + r < a.B) ? m0 + r : a.B - 1;
        xrow[i] = a.x + row * a.K + 4 * q8;
    }
    const float *xmp = a.x_mul != nullptr ? a.x_mul + 4 * q8 : nullptr;
    // weights: thread <-> (column c = tid >> 1, 16-code half hh = tid & 1): 16 bytes of an 8-bit row, 8 of a 4-bit one
    const int wc = tid >> 1, whh = tid & 1;
    const int wcc = (n0 + wc < a.O) ? n0 + wc : a.O - 1;
    const uint8_t *wrow = a.w + ((int64_t)wcc * a.K + 16 * whh) * WB / 8;
    const float *zrow = a.w_zero + (int64_t)wcc * a.NG;
    const float woff = a.w_sign ? (float)(1 << (WB - 1)) : 0.0f;     // stored u -> q = u - woff

    float4 xv[4], xm = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
    uint4 wv = make_uint4(0u, 0u, 0u, 0u);
    float zwv = 0.0f;
    auto fetch = [&](int st) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 4; ++i) xv[i] = *reinterpret_cast<const float4 *>(xrow[i] + st * LG_K);
        if (xmp != nullptr) xm = *reinterpret_cast<const float4 *>(xmp + st * LG_K);      // (uniform)
        if constexpr (WB == 8) wv = *reinterpret_cast<const uint4 *>(wrow + st * LG_K);
        else {
            const uint2 w2 = *reinterpret_cast<const uint2 *>(wrow + st * (LG_K / 2));
            wv.x = w2.x; wv.y = w2.y;
        }
        zwv = zrow[st >> gsh];
    };
    float sx[4] = {0.0f, 0.0f, 0.0f, 0.0f};              // this thread's share of S_x[., g] of its four rows
    auto stage = [&](int st) __attribute__((always_inline)) {
        uint8_t *base = lsm + (st & 1) * LG_BUF;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = (tid >> 3) + 32 * i;
            float x[4] = {xv[i].x * xm.x, xv[i].y * xm.y, xv[i].z * xm.z, xv[i].w * xm.w};   // x' (x_mul == NULL: x * 1)
            if constexpr (SX) sx[i] += (x[0] + x[1]) + (x[2] + x[3]);
            // piece (16 bytes = 8 k) q8 >> 1 of the row, its half q8 & 1
            uint8_t *dst = base + r * 64 + 16 * ((q8 >> 1) ^ ((r >> 2) & 3)) + 8 * (q8 & 1);
#pragma unroll
            for (int sp = 0; sp < 3; ++sp) {
                uint32_t u[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    u[j] = __float_as_uint(x[j]) & 0xffff0000u;           // sp == 2: the remainder has <= 8 significant bits
                    x[j] -= __uint_as_float(u[j]);
                }
                *reinterpret_cast<uint2 *>(dst + sp * LG_PLANE) =
                    make_uint2(__builtin_amdgcn_perm(u[1], u[0], 0x07060302u), __builtin_amdgcn_perm(u[3], u[2], 0x07060302u));
            }
        }
        if constexpr (SX) {
            if ((st & gmask) == gmask) {                  // the group's last stage: the 8 threads of a row add their shares
                float *dst = sxg + ((st >> gsh) & 1) * LG_T;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float v = sx[i];
                    v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4);
                    if (q8 == 0) dst[(tid >> 3) + 32 * i] = v;
                    sx[i] = 0.0f;
                }
            }
        }
        // 16 codes -> 16 bf16 of u - wshift = q - c (two 16-byte pieces: k 16 hh .. 16 hh + 7, + 8 .. + 15)
        const float wshift = woff + linf_centre(zwv, a.w_sign);
        const uint32_t ww[4] = {wv.x, wv.y, wv.z, wv.w};
        uint32_t pk[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            uint32_t b0, b1;
            if constexpr (WB == 8) {
                b0 = (ww[j >> 1] >> (16 * (j & 1))) & 0xffu; b1 = (ww[j >> 1] >> (16 * (j & 1) + 8)) & 0xffu;
            } else {                                      // byte j of the 8: code 2 j in its low nibble, 2 j + 1 in its high one
                b0 = (ww[j >> 2] >> (8 * (j & 3))) & 0xfu; b1 = (ww[j >> 2] >> (8 * (j & 3) + 4)) & 0xfu;
            }
            const float f0 = (float)b0 - wshift, f1 = (float)b1 - wshift;   // |q - c| <= 255: exact in bf16
            pk[j] = __builtin_amdgcn_perm(__float_as_uint(f1), __float_as_uint(f0), 0x07060302u);
        }
        uint8_t *wd = base + 3 * LG_PLANE + wc * 64;
        const int sw3 = (wc >> 2) & 3;
        *reinterpret_cast<uint4 *>(wd + 16 * ((2 * whh) ^ sw3)) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
        *reinterpret_cast<uint4 *>(wd + 16 * ((2 * whh + 1) ^ sw3)) = make_uint4(pk[4], pk[5], pk[6], pk[7]);
    };

    v16f_g accg[2][2], acco[2][2];                        // the running group, the folded total
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

    const int n_stages = a.K / LG_K;
    const int swz = (col >> 2) & 3;
    const int a_off = (wm * 64 + col) * 64, b_off = 3 * LG_PLANE + (wn * 64 + col) * 64;
    fetch(0);
    stage(0);
    for (int st = 0; st < n_stages; ++st) {
        // buffer st & 1 is complete (and S_x of a group that ends here); every wave has left buffer (st + 1) & 1
        __syncthreads();
        const bool more = st + 1 < n_stages;
        if (more) fetch(st + 1);                          // in flight under the MFMAs
        const bool fold = (st & gmask) == gmask;          // (uniform)
        float gsw[2] = {0.0f, 0.0f}, gdz[2] = {0.0f, 0.0f};
        if (fold) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                gsw[j] = a.w_scale[og[j] + (st >> gsh)];
                if constexpr (SX) { const float zw = a.w_zero[og[j] + (st >> gsh)]; gdz[j] = zw - linf_centre(zw, a.w_sign); }
            }
        }
        const uint8_t *buf = lsm + (st & 1) * LG_BUF;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int po = 16 * ((2 * ks + h) ^ swz);
            v8bf_g fb[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) fb[j] = *reinterpret_cast<const v8bf_g *>(buf + b_off + j * 32 * 64 + po);
#pragma unroll
            for (int sp = 0; sp < 3; ++sp) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const v8bf_g fa = *reinterpret_cast<const v8bf_g *>(buf + sp * LG_PLANE + a_off + i * 32 * 64 + po);
#pragma unroll
                    for (int j = 0; j < 2; ++j) accg[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb[j], accg[i][j], 0, 0, 0);
                }
            }
        }
        if (fold) {
            const float *sxr = sxg + ((st >> gsh) & 1) * LG_T + wm * 64 + 4 * h;
            grp_fold<SX>(accg, acco, gsw, gdz, [&](int i, int r) { return sxr[i * 32 + (r & 3) + 8 * (r >> 2)]; });
        }
        if (more) stage(st + 1);
    }
    __syncthreads();                                      // every wave is done with the stage buffers
    // D has the batch row on the register and the feature on the lane.  Each wave turns its 32 x 32 tiles through a private
    // LDS patch (the stage buffers are free now) and writes 8 rows x 128 contiguous bytes per store instruction.  (A wave's
    // own LDS operations complete in order: its reads see its writes, a later tile's writes cannot overtake them.)
    // (twin: linear_grp_i8_mfma_kernel's patch store)
    float *patch = reinterpret_cast<float *>(lsm) + wave * (32 * 36);
    const int rrow = lane >> 3, rq = lane & 7;
    const bool vec4 = (a.O & 3) == 0 && (reinterpret_cast<uintptr_t>(a.out) & 15) == 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int c = n0 + wn * 64 + j * 32 + col;
        const float bias = a.bias != nullptr ? a.bias[min(c, a.O - 1)] : 0.0f;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int64_t row0 = m0 + wm * 64 + i * 32;
            if (vec4) {
#pragma unroll
                for (int r = 0; r < 16; ++r) patch[((r & 3) + 8 * (r >> 2) + 4 * h) * 36 + col] = acco[i][j][r] + bias;
                const int c4 = n0 + wn * 64 + j * 32 + 4 * rq;       // O % 4 == 0: a piece lies wholly below O or wholly beyond it
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int rt = 8 * k + rrow;
                    const float4 o4 = *reinterpret_cast<const float4 *>(patch + rt * 36 + 4 * rq);
                    const int64_t row = row0 + rt;
                    if (row < a.B && c4 < a.O) *reinterpret_cast<float4 *>(a.out + row * a.O + c4) = o4;
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int64_t row = row0 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    if (row < a.B && c < a.O) a.out[row * a.O + c] = acco[i][j][r] + bias;
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Host side: one plan, read by the path query and by the launch.  No HIP call in it.
// ---------------------------------------------------------------------------------------------
struct LinGrpPlan {
    int fast;               // 1: linear_grp_mfma_kernel, 0: linear_grp_plain_kernel
    int w4, sx;             // the fast kernel's instance
    int64_t blocks;
};

// a validated request (check_grp); a query leaves the pointers it does not know null, which reads as aligned
LinGrpPlan plan_grp(const float *x, const float *x_mul, const qe_qparam *w, int G, int symmetric, int64_t B, int K, int O)
{
    LinGrpPlan p = {};
    p.fast = grp_weights_fast(w, G) && K > 0 && K % LG_K == 0 && aligned16(x) && aligned16(x_mul);
    p.w4 = w->n_bits == 4;
    p.sx = symmetric == 0;
    p.blocks = p.fast ? ceil_div64(B, LG_T) * ceil_div64(O, LG_T) : ceil_div64(B * O, 256);
    return p;
}

int check_grp(const qe_qparam *w, int G, int64_t B, int K, int O)
{
    if (B < 0 || K < 0 || O < 0) return QE_ERR_ARG;
    return check_grp_weights(w, G, K, O);
}

}  // namespace

}  // namespace qe

extern "C" int qe_quantlinear_grouped_float_input_path(const float *x, const float *x_mul, const qe_qparam *w, int32_t group_size,
                                                       int32_t symmetric, int64_t B, int32_t K, int32_t O)
{
    using namespace qe;
    if (check_grp(w, group_size, B, K, O) != QE_OK) return 0;
    return plan_grp(x, x_mul, w, group_size, symmetric, B, K, O).fast;
}

extern "C" int qe_quantlinear_grouped_float_input(const float *x, const float *x_mul, const qe_qparam *w, int32_t group_size,
                                                  int32_t symmetric, const float *bias, int64_t B, int32_t K, int32_t O, float *out,
                                                  qe_stream_t stream)
{
    using namespace qe;
    if (int rc = check_grp(w, group_size, B, K, O)) return rc;
    if ((x == nullptr && B * K > 0) || (out == nullptr && B * O > 0)) return QE_ERR_ARG;
    if (B == 0 || O == 0) return QE_OK;
    const LinGrpPlan p = plan_grp(x, x_mul, w, group_size, symmetric, B, K, O);
    LinGrpArgs a = {};
    a.x = x; a.x_mul = x_mul; a.w = w->data; a.w_scale = w->scale; a.w_zero = w->zero; a.bias = bias; a.out = out;
    a.w_bits = w->n_bits; a.w_sign = w->sign; a.G = group_size; a.NG = K / group_size; a.B = B; a.K = K; a.O = O;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return launch_grp<&linear_grp_plain_kernel>(p.fast, p.blocks, a, s, [&] {
        dispatch_flag(p.w4, [&](auto w4) { dispatch_flag(p.sx, [&](auto sx) {
            launch_instance<&linear_grp_mfma_kernel<decltype(w4)::value ? 4 : 8, decltype(sx)::value>>((unsigned)p.blocks, 256, LG_LDS, LG_LDS, s, a);
        }); });
    });
}
