// qe_linear_bf16in.hip -- the kernels of qe_quantlinear_bf16_input: bf16 activations x 8-bit weight codes, K % 32 == 0.
//
//   out[b,o] = bias[o] + sw[o] ( S_xq[b,o] - (zw[o] - c[o]) S_x[b] ),   S_xq = sum_k x (q_w - c),   S_x = sum_k x
//
// linear_f32_mfma_kernel's formula (qe_linear.hip) with the same centre c = linf_centre(zw), on activations that are bf16
// already: a lane's A fragment of v_mfma_f32_32x32x16_bf16 is 8 consecutive k of a stored row, 16 bytes as loaded -- no
// split into three parts and so one MFMA per product where that kernel issues three, no conversion, half the activation
// bytes.  Every product bf16 x integer code (|q - c| <= 255: bf16-exact) is exact in fp32; only the fp32 accumulation and
// the fp32 row sum S_x round.  (A non-finite x gives NaN where the reference's chain keeps +-inf: the divergence declared
// for the float-input kernels; it stays inside its own row.)
//
// Workgroup = 2 x 2 waves, tile 128 x 128, wave 64 x 64 = 2 x 2 MFMA tiles.  Stage = 32 k of both operands, register
// staged: a thread fetches two 16-byte activation pieces and 16 weight codes, which it turns into 16 bf16 of u - wshift.
// LDS images [row][32 k] bf16 (64-byte rows), 16-byte pieces XOR-swizzled as in linear_mfma_kernel.  TWO stage buffers and
// one barrier per stage: behind the barrier of stage s the loads of stage s + 1 are issued, the MFMAs of stage s run, and
// the loaded registers go into the other buffer, which every wave left before it reached that barrier.
// Rows beyond B and columns beyond O read a clamped, valid address (the residual included) and are dropped at the store:
// no load sits under a per-lane condition.  The result leaves through the wave's LDS patch as 16-byte
// row pieces (O % 4 == 0 and aligned out / residual; element stores otherwise).  The residual form is a template instance.
#include "qe_linear_bf16in.hpp"

namespace qe {

namespace {

typedef __bf16 v8bf_b __attribute__((ext_vector_type(8)));
typedef float v16f_b __attribute__((ext_vector_type(16)));

// the two bf16 of a register as fp32 (exact: a bf16 is the upper half of an fp32)
__device__ __forceinline__ float bf_lo(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf_hi(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }

}  // namespace

template <bool RES>
__global__ __launch_bounds__(256, 2) void linear_bf16in_kernel(const LinBf16Args a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lsm[];   // 2 x (activation image, weight image), row sums, column constants
    float *rowsum = reinterpret_cast<float *>(lsm + 4 * LB_PLANE);
    float4 *colc = reinterpret_cast<float4 *>(rowsum + LB_T);        // sw, zw - c, bias, 0

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave & 1, wn = wave >> 1;
    const int col = lane & 31, h = lane >> 5;
    const int n_ct = (a.O + LB_T - 1) / LB_T;
    const int64_t bid = blockIdx.x;
    const int ct = (int)(bid % n_ct);
    const int64_t m0 = (bid / n_ct) * LB_T;
    const int n0 = ct * LB_T;

    if (tid < LB_T) {
        const int cc = (n0 + tid < a.O) ? n0 + tid : a.O - 1;
        const float zw = a.w_per_tensor ? a.w_zero[0] : a.w_zero[cc];
        colc[tid] = make_float4(a.w_per_tensor ? a.w_scale[0] : a.w_scale[cc], zw - linf_centre(zw, a.w_sign),
                                a.bias ? a.bias[cc] : 0.0f, 0.0f);
    }

    // activations: thread <-> (row r = (tid >> 2) + 64 i, 16-byte piece ap = tid & 3 of the stage's 64 bytes of that row)
    const int ap = tid & 3;
    const uint16_t *xrow[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int r = (tid >> 2) + 64 * i;
        const int64_t row = (m0 + r < a.B) ? m0 + r : a.B - 1;
        xrow[i] = a.x + row * a.K + 8 * ap;
    }
    // weights: thread <-> (column c = tid >> 1, 16-code half hh = tid & 1)
    const int wc = tid >> 1, whh = tid & 1;
    const int wcc = (n0 + wc < a.O) ? n0 + wc : a.O - 1;
    const uint8_t *wrow = a.w + (int64_t)wcc * a.K + 16 * whh;
    // stored u -> q = u - 128 (signed) | u, centred: q - c = u - wshift with wshift an integer in [0, 255]
    const float wshift = (a.w_sign ? 128.0f : 0.0f) + linf_centre(a.w_per_tensor ? a.w_zero[0] : a.w_zero[wcc], a.w_sign);

    uint4 xv[2];
    uint4 wv;
    auto fetch = [&](int st) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 2; ++i) xv[i] = *reinterpret_cast<const uint4 *>(xrow[i] + st * LB_K);
        wv = *reinterpret_cast<const uint4 *>(wrow + st * LB_K);
    };
    float sx[2] = {0.0f, 0.0f};                          // this thread's share of S_x of its two rows
    auto stage = [&](int b) __attribute__((always_inline)) {
        uint8_t *base = lsm + b * 2 * LB_PLANE;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int r = (tid >> 2) + 64 * i;
            const uint4 x = xv[i];
            sx[i] += ((bf_lo(x.x) + bf_hi(x.x)) + (bf_lo(x.y) + bf_hi(x.y))) + ((bf_lo(x.z) + bf_hi(x.z)) + (bf_lo(x.w) + bf_hi(x.w)));
            *reinterpret_cast<uint4 *>(base + r * 64 + 16 * (ap ^ ((r >> 2) & 3))) = x;   // the operand as loaded
        }
        // 16 codes -> 16 bf16 (two 16-byte pieces: k 16 hh .. 16 hh + 7, + 8 .. + 15)
        const uint32_t ww[4] = {wv.x, wv.y, wv.z, wv.w};
        uint32_t pk[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t b0 = (ww[j >> 1] >> (16 * (j & 1))) & 0xffu, b1 = (ww[j >> 1] >> (16 * (j & 1) + 8)) & 0xffu;
            const float f0 = (float)b0 - wshift, f1 = (float)b1 - wshift;   // |q - c| <= 255: exact in bf16
            pk[j] = __builtin_amdgcn_perm(__float_as_uint(f1), __float_as_uint(f0), 0x07060302u);
        }
        uint8_t *wd = base + LB_PLANE + wc * 64;
        const int sw3 = (wc >> 2) & 3;
        *reinterpret_cast<uint4 *>(wd + 16 * ((2 * whh) ^ sw3)) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
        *reinterpret_cast<uint4 *>(wd + 16 * ((2 * whh + 1) ^ sw3)) = make_uint4(pk[4], pk[5], pk[6], pk[7]);
    };

    v16f_b acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    const int n_stages = a.K / LB_K;
    const int swz = (col >> 2) & 3;
    const int a_off = (wm * 64 + col) * 64, b_off = LB_PLANE + (wn * 64 + col) * 64;
    fetch(0);
    stage(0);
    for (int st = 0; st < n_stages; ++st) {
        // buffer st & 1 is complete; and every wave has left buffer (st + 1) & 1, which stage s - 1 ran on
        __syncthreads();
        const bool more = st + 1 < n_stages;
        if (more) fetch(st + 1);                          // in flight under the MFMAs
        const uint8_t *buf = lsm + (st & 1) * 2 * LB_PLANE;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int po = 16 * ((2 * ks + h) ^ swz);
            v8bf_b fa[2], fb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) fa[i] = *reinterpret_cast<const v8bf_b *>(buf + a_off + i * 32 * 64 + po);
#pragma unroll
            for (int j = 0; j < 2; ++j) fb[j] = *reinterpret_cast<const v8bf_b *>(buf + b_off + j * 32 * 64 + po);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        if (more) stage((st + 1) & 1);
    }
    // S_x: the 4 threads of a row (consecutive lanes) add their shares
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        float v = sx[i];
        v += __shfl_xor(v, 1); v += __shfl_xor(v, 2);
        if (ap == 0) rowsum[(tid >> 2) + 64 * i] = v;
    }
    __syncthreads();                                      // the row sums are in place; every wave is done with the stage buffers
    // D has the batch row on the register and the feature on the lane.  Each wave turns its 32 x 32 tiles through a private
    // LDS patch (the stage buffers are free now) and writes 8 rows x 128 contiguous bytes per store instruction.  (A wave's
    // own LDS operations complete in order: its reads see its writes, a later tile's writes cannot overtake them.)
    float *patch = reinterpret_cast<float *>(lsm) + wave * (32 * 36);
    const int rrow = lane >> 3, rq = lane & 7;
    const bool vec4 = (a.O & 3) == 0 && ((reinterpret_cast<uintptr_t>(a.out) | reinterpret_cast<uintptr_t>(a.res)) & 15) == 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int cl = wn * 64 + j * 32 + col;
        const float4 cc = colc[cl];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float v[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int rl = wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                v[r] = fmaf(cc.x, fmaf(-cc.y, rowsum[rl], acc[i][j][r]), cc.z);
            }
            const int64_t row0 = m0 + wm * 64 + i * 32;
            if (vec4) {
#pragma unroll
                for (int r = 0; r < 16; ++r) patch[((r & 3) + 8 * (r >> 2) + 4 * h) * 36 + col] = v[r];
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
                const int c = n0 + cl;
                const int ccl = min(c, a.O - 1);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int64_t row = row0 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    float o = v[r];
                    if constexpr (RES) o += a.res[min(row, a.B - 1) * a.O + ccl];
                    if (row < a.B && c < a.O) a.out[row * a.O + c] = o;
                    if constexpr (RES) __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
    }
}

void launch_linear_bf16in(const LinBf16Args &a, bool residual, int64_t blocks, hipStream_t s)
{
    if (residual) launch_instance<&linear_bf16in_kernel<true>>((unsigned)blocks, 256, linb_lds_bytes(), 0, s, a);
    else launch_instance<&linear_bf16in_kernel<false>>((unsigned)blocks, 256, linb_lds_bytes(), 0, s, a);
}

// out[i] = fp32(x[i]): 8 elements per thread where both rows are 16-byte aligned
__global__ __launch_bounds__(256) void widen_bf16_kernel(const uint16_t *x, float *out, int64_t n, int vec)
{
    const int64_t n8 = vec ? n / 8 : 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
        const uint4 v = reinterpret_cast<const uint4 *>(x)[i];
        reinterpret_cast<float4 *>(out)[2 * i] = make_float4(bf_lo(v.x), bf_hi(v.x), bf_lo(v.y), bf_hi(v.y));
        reinterpret_cast<float4 *>(out)[2 * i + 1] = make_float4(bf_lo(v.z), bf_hi(v.z), bf_lo(v.w), bf_hi(v.w));
    }
    for (int64_t i = 8 * n8 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        out[i] = __uint_as_float((uint32_t)x[i] << 16);
}

void launch_widen_bf16(const uint16_t *x, float *out, int64_t n, hipStream_t s)
{
    if (n <= 0) return;
    const ElementwiseGrid g = elementwise_grid(n, 8, reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out));
    hipLaunchKernelGGL(widen_bf16_kernel, dim3(g.blocks), dim3(256), 0, s, x, out, n, g.vec);
}

}  // namespace qe
