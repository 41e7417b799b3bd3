// qe_conv_mfma.hip -- int8 MFMA implicit-GEMM convolution for gfx950 (MI355X).
//
// Replaces quantconv2d_cuda_kernel (engine/kernels/functions/quantconv2d.cu:49-142) for
// every problem whose activation scale/zero is per tensor (the reference's default
// granularity).  The reference unpacks and dequantises both operands to fp32 inside the
// innermost loop of a one-thread-per-output kernel; here the integer part of the sum is
// done exactly on the matrix cores and the scales are applied once per output:
//
//   out[n,oc,p] = bias[oc] + sum_inb ((qx - zx) sx) ((qw - zw[oc]) sw[oc])
//               = bias[oc] + sx sw[oc] * ( S_aw - zw' S_x - zx' S_w + N_inb zx' zw' )
//   a_x = qx - d_x, a_w = qw - d_w   (d = 128 for unsigned 8-bit, else 0: fits int8)
//   zx' = zx - d_x, zw' = zw - d_w   (floats, may be non-integer: minmax.py:143)
//   S_aw = sum_inb a_x a_w           v_mfma_i32_32x32x32_i8, exact int32; padded taps hold a_x = 0
//   S_x  = sum_inb a_x               v_dot4 on the same B fragments (only if some zw' != 0)
//   S_w  = sum_inb a_w               per-(oc,tap) table from the prep pass, border aware
//                                    (only if zx' != 0); N_inb = IC * #in-bounds taps
//   "inb" = taps inside the image: the reference SKIPS padded taps (quantconv2d.cu:101).
//
// Two kernels per call:
//   prep  : packed OIHW weights (any 1..8 bits) -> int8 a_w in MFMA A-fragment order
//           Wt[tap][ic/16][oc][16], per-oc epilogue constants, per-(oc,tap) sums.
//   main  : GEMM view  D[oc, pixel] = sum_k Wt[oc,k] X[k,pixel],  k = (ic-chunk, tap, ic%32).
//           Workgroup = 256 threads = 4 waves; tile = MT output channels x (TH output rows x
//           full width) pixels of ONE image (<= 256 pixels = 8 MFMA column tiles).  D has the
//           pixel on the lane (32x32 C/D map: col = lane&31), so every accumulator register
//           stores as two 128-byte row segments of the fp32 NCHW output: no epilogue transpose.
//           Activations: NCHW bytes have K strided by H*W, MFMA wants 16 K-contiguous bytes per
//           lane.  Each staging thread loads 16 channels x 4 pixels (16 dwords, coalesced along
//           the row), transposes 4x4 byte blocks with v_perm_b32 and writes one 16-byte
//           [pixel][16 ch] vector per pixel into LDS.  The LDS image is the input halo tile in
//           pixel-major order with zeroed borders: a tap is just a constant LDS offset, so there
//           is no im2col expansion and no per-tap bounds test in the inner loop.
//           Weights: A fragments go L2 -> VGPR directly (each wave owns a distinct 32-row strip,
//           LDS would add a copy without any sharing); all taps of a chunk are requested before
//           the next chunk's activation loads so the in-order vmcnt never parks a fast L2 hit
//           behind an HBM miss.
//           Pipeline per 32-channel chunk: request A(c) -> transpose X(c) regs into LDS -> barrier
//           -> request X(c+1) into registers -> MFMA over all taps -> barrier.
#include "qe_conv_mfma_kernel.hpp"
#include "qe_conv_plan.hpp"

namespace qe {

struct PrepArgs {
    const uint8_t *w;
    const float *w_scale, *w_zero;
    const float *bias;
    int w_bits, w_sign, w_per_tensor;
    int OC, IC, KK, OCP, NG;
    int KH, KW;
    int8_t *wt;
    float *ep;
    int *ws;
};

__device__ __forceinline__ int unpack_code(const uint8_t *__restrict__ p, int64_t ele_idx, int n_bits)
{
    const int64_t bit = ele_idx * n_bits;
    const int64_t byte_idx = bit >> 3;
    const int bit_idx = (int)(bit & 7);
    unsigned v = ((unsigned)p[byte_idx] >> bit_idx);
    if (bit_idx + n_bits > 8) v |= ((unsigned)p[byte_idx + 1] << (8 - bit_idx));
    return (int)(v & ((1u << n_bits) - 1u));
}

// ---------------------------------------------------------------------------------------------
// prep: one workgroup per (padded) output channel.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void conv_mfma_prep_kernel(const PrepArgs a)
{
    __shared__ int s_ws[64];
    const int oc = blockIdx.x;
    const int tid = threadIdx.x;
    if (tid < 64) s_ws[tid] = 0;
    __syncthreads();
    const int cb = code_bias(a.w_bits, a.w_sign);
    const bool live = oc < a.OC;
    for (int idx = tid; idx < a.KK * a.NG; idx += 256) {
        const int tap = idx / a.NG, icg = idx - tap * a.NG;
        uint32_t v[4] = {0, 0, 0, 0};
        int sum = 0;
        if (live) {
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int ic = icg * 16 + j;
                int aw = 0;
                if (ic < a.IC) {
                    const int64_t e = ((int64_t)oc * a.IC + ic) * a.KK + tap;  // quantconv2d.cu:118
                    aw = unpack_code(a.w, e, a.w_bits) - cb;
                }
                sum += aw;
                v[j >> 2] |= ((uint32_t)aw & 0xffu) << ((j & 3) * 8);
            }
        }
        *reinterpret_cast<uint4 *>(a.wt + (((int64_t)tap * a.NG + icg) * a.OCP + oc) * 16) =
            make_uint4(v[0], v[1], v[2], v[3]);
        if (sum != 0) atomicAdd(&s_ws[tap], sum);
    }
    __syncthreads();
    // 2-D prefix table of the per-tap sums: P[i][j] = sum over kh < i, kw < j (border-aware S_w in O(1), epilogue)
    {
        const int PW1 = a.KW + 1, PS = (a.KH + 1) * PW1;
        if (tid < PS) {
            const int i = tid / PW1, j = tid - i * PW1;
            int sum = 0;
            for (int kh = 0; kh < i; ++kh)
                for (int kw = 0; kw < j; ++kw) sum += s_ws[kh * a.KW + kw];
            a.ws[(int64_t)oc * PS + tid] = sum;
        }
    }
    if (tid == 128) {
        float alpha = 0.0f, zwp = 0.0f, b = 0.0f;
        if (live) {
            const float sw = a.w_per_tensor ? a.w_scale[0] : a.w_scale[oc];
            const float zw = a.w_per_tensor ? a.w_zero[0] : a.w_zero[oc];
            alpha = sw;                                   // the epilogue multiplies by the activation scale
            zwp = zw - zero_shift(a.w_bits, a.w_sign);
            b = a.bias ? a.bias[oc] : 0.0f;
        }
        a.ep[oc] = alpha;
        a.ep[a.OCP + oc] = zwp;
        a.ep[2 * a.OCP + oc] = b;
    }
}

// prep for the small-IC kernel: Wt[kh][h][oc][16], byte (kw - 4h)*4 + ic; same ep / ws tables.
__global__ __launch_bounds__(64) void conv_mfma_prep_smallic_kernel(const PrepArgs a, int KH, int KW)
{
    __shared__ int s_ws[64];
    const int oc = blockIdx.x;
    const int tid = threadIdx.x;
    s_ws[tid] = 0;
    __syncthreads();
    const int cb = code_bias(a.w_bits, a.w_sign);
    const bool live = oc < a.OC;
    if (tid < KH * 2) {
        const int kh = tid >> 1, h = tid & 1;
        uint32_t v[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int kw = 4 * h + (j >> 2), ic = j & 3;
            int aw = 0;
            if (live && kw < KW && ic < a.IC) {
                const int64_t e = ((int64_t)oc * a.IC + ic) * a.KK + kh * KW + kw;  // quantconv2d.cu:118
                aw = unpack_code(a.w, e, a.w_bits) - cb;
                atomicAdd(&s_ws[kh * KW + kw], aw);
            }
            v[j >> 2] |= ((uint32_t)aw & 0xffu) << ((j & 3) * 8);
        }
        *reinterpret_cast<uint4 *>(a.wt + (((int64_t)kh * 2 + h) * a.OCP + oc) * 16) = make_uint4(v[0], v[1], v[2], v[3]);
    }
    __syncthreads();
    {
        const int PW1 = KW + 1, PS = (KH + 1) * PW1;
        for (int e = tid; e < PS; e += 64) {
            const int i = e / PW1, j = e - i * PW1;
            int sum = 0;
            for (int kh = 0; kh < i; ++kh)
                for (int kw = 0; kw < j; ++kw) sum += s_ws[kh * KW + kw];
            a.ws[(int64_t)oc * PS + e] = sum;
        }
    }
    if (tid == 0) {
        float alpha = 0.0f, zwp = 0.0f, b = 0.0f;
        if (live) {
            const float sw = a.w_per_tensor ? a.w_scale[0] : a.w_scale[oc];
            const float zw = a.w_per_tensor ? a.w_zero[0] : a.w_zero[oc];
            alpha = sw;                                   // the epilogue multiplies by the activation scale
            zwp = zw - zero_shift(a.w_bits, a.w_sign);
            b = a.bias ? a.bias[oc] : 0.0f;
        }
        a.ep[oc] = alpha;
        a.ep[a.OCP + oc] = zwp;
        a.ep[2 * a.OCP + oc] = b;
    }
}

// Stride-2 gather without index divisions: a plane's OH x nq units (nq = 16-byte pieces per even input row, a power of two)
// sit in UP = 2^LOG_UP consecutive threads, thread u -> row u / nq, piece u % nq by shifts; a block takes 256 / UP planes per
// round and 4 rounds, all 4 loads of a thread issued before its stores.  One unaligned 16-byte load (it may run into the
// following odd row, never past the tensor: 16 nq <= 2 W, H even), two v_perm keep the even bytes, one 8-byte store (the last
// piece of a row in 4 / 2 / 1-byte steps).  The round-1 kernel spent ~3 integer divisions per unit and took byte gathers
// on 14-wide rows: 2.5 TB/s over the two ResNet-50 gathers.
template <int LOG_UP>
__global__ __launch_bounds__(256) void subsample2_kernel(const uint8_t *__restrict__ x, uint8_t *__restrict__ y, int64_t n_planes,
                                                         int H, int W, int OH, int OW, int log_nq)
{
    constexpr int UP = 1 << LOG_UP, PPR = 256 / UP, ROUNDS = 4;
    const int u = threadIdx.x & (UP - 1);
    const int oh = u >> log_nq, q = u & ((1 << log_nq) - 1);
    const bool unit_ok = oh < OH && 8 * q < OW;
    const int64_t plane0 = (int64_t)blockIdx.x * (PPR * ROUNDS) + (threadIdx.x >> LOG_UP);
    uint4 d[ROUNDS];
#pragma unroll
    for (int k = 0; k < ROUNDS; ++k) {
        const int64_t pl = plane0 + k * PPR;
        const bool ok = unit_ok && pl < n_planes;
        const uint8_t *src = x + (ok ? (pl * H + 2 * oh) * (int64_t)W + 16 * q : 0);
        __builtin_memcpy(&d[k], src, 16);
    }
#pragma unroll
    for (int k = 0; k < ROUNDS; ++k) {
        const int64_t pl = plane0 + k * PPR;
        if (!(unit_ok && pl < n_planes)) continue;
        const uint32_t lo = __builtin_amdgcn_perm(d[k].y, d[k].x, 0x06040200u);   // even bytes of dwords 0, 1
        const uint32_t hi = __builtin_amdgcn_perm(d[k].w, d[k].z, 0x06040200u);
        uint8_t *dst = y + (pl * OH + oh) * (int64_t)OW + 8 * q;
        const int left = OW - 8 * q;
        if (left >= 8) {
            const uint2 o = make_uint2(lo, hi);
            __builtin_memcpy(dst, &o, 8);
        } else {
            uint32_t v = lo;
            int done = 0;
            if (left >= 4) { __builtin_memcpy(dst, &lo, 4); done = 4; v = hi; }
            if (left - done >= 2) { const uint16_t h2 = (uint16_t)v; __builtin_memcpy(dst + done, &h2, 2); done += 2; v >>= 16; }
            if (left - done >= 1) dst[done] = (uint8_t)v;
        }
    }
}

// 4-bit activations of a stride-2 1x1 layer: out[r][ow] = 8-bit stored code (q + 128) of in[r_in][2 ow], r = (plane, oh),
// r_in = plane H + 2 oh.  One thread per 8 output bytes = 8 input bytes (16 elements, the even ones are the low nibbles):
// one byte-aligned 8-byte load, a mask and an add, one 8-byte store; the last unit of a row goes byte by byte.
// Replaces expand_codes_s8 over the WHOLE tensor followed by subsample_kernel / the in-kernel stride-2 staging.
__global__ __launch_bounds__(256) void subsample_x4_kernel(const uint8_t *__restrict__ x, uint8_t *__restrict__ y, int64_t n_rows,
                                                           int H, int W, int OH, int OW, int sign)
{
    const int nq = (OW + 7) >> 3;
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= n_rows * nq) return;
    const int64_t r = u / nq;
    const int q = (int)(u - r * nq);
    const int64_t plane = r / OH;
    const int oh = (int)(r - plane * OH);
    const uint8_t *src = x + ((plane * H + 2 * oh) * (int64_t)W >> 1) + 8 * q;      // 2 elements per byte: input column 16 q
    uint8_t *dst = y + r * OW + 8 * q;
    const uint64_t add = sign ? 0x7878787878787878ull : 0x8080808080808080ull;     // q + 128 = nibble - 8 + 128 | nibble + 128
    if (8 * q + 8 <= OW) {
        uint64_t v;
        __builtin_memcpy(&v, src, 8);
        v = (v & 0x0f0f0f0f0f0f0f0full) + add;
        __builtin_memcpy(dst, &v, 8);
    } else {
        for (int j = 0; 8 * q + j < OW; ++j) dst[j] = (uint8_t)((src[j] & 0x0f) + (uint8_t)add);
    }
}

// out[r][ow] = in[r_in][ow * s] for the rows r = (n*IC + c)*OH + oh.
// WIDE (stride 2, W % 4 == 0, W >= 16): one thread per 8 output bytes = one 16-byte load (clamped to end at the row's
// end and rotated back by whole dwords, so nothing is read past a row), two v_perm, one 8-byte store.
// otherwise: one thread per 4 output bytes, byte gathers.
template <bool WIDE>
__global__ __launch_bounds__(256) void subsample_kernel(const uint8_t *__restrict__ x, uint8_t *__restrict__ y, int64_t n_planes,
                                                        int H, int W, int OH, int OW, int s)
{
    constexpr int OPT = WIDE ? 8 : 4;            // output bytes per unit
    constexpr int UPT = 4;                       // units per thread, all loads issued before the first store
    const int nq = (OW + OPT - 1) / OPT;
    const int U = OH * nq;                       // units of one plane
    const int ppb = U >= 256 * UPT ? 1 : (256 * UPT) / U;   // planes per workgroup (32-bit index math only)
    for (int t0 = threadIdx.x; t0 < ppb * U; t0 += 256 * UPT) {
        uint4 d[UPT];
        uint32_t g[UPT];
        uint8_t *dst[UPT];
        int ow0[UPT], rot[UPT];
        bool live[UPT];
#pragma unroll
        for (int k = 0; k < UPT; ++k) {
            const int t = t0 + 256 * k;
            const int pl = t / U, u = t - pl * U;
            const int64_t plane = (int64_t)blockIdx.x * ppb + pl;
            live[k] = t < ppb * U && plane < n_planes;
            const int64_t pc = live[k] ? plane : 0;
            const int oh = u / nq, q = u - oh * nq;
            const uint8_t *src = x + (pc * H + (int64_t)oh * s) * W;
            ow0[k] = OPT * q;
            dst[k] = y + (pc * OH + oh) * OW + ow0[k];
            if constexpr (WIDE) {
                const int iw = 2 * ow0[k];                                // first input column of this unit
                const int iwc = iw < W - 16 ? iw : W - 16;                // 16 bytes that end inside the row
                __builtin_memcpy(&d[k], src + iwc, 16);
                rot[k] = (iw - iwc) >> 2;                                 // whole dwords (W % 4 == 0)
            } else {
                uint32_t v = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c = ow0[k] + j < OW ? ow0[k] + j : OW - 1;  // clamped: always a valid byte of the row
                    v |= (uint32_t)src[(int64_t)c * s] << (8 * j);
                }
                g[k] = v;
            }
        }
#pragma unroll
        for (int k = 0; k < UPT; ++k) {
            if (!live[k]) continue;
            if constexpr (WIDE) {
                const uint4 dd = d[k];
                const int r = rot[k];
                const uint32_t d0 = r == 0 ? dd.x : (r == 1 ? dd.y : (r == 2 ? dd.z : dd.w));
                const uint32_t d1 = r == 0 ? dd.y : (r == 1 ? dd.z : (r == 2 ? dd.w : 0u));
                const uint32_t d2 = r == 0 ? dd.z : (r == 1 ? dd.w : 0u);
                const uint32_t d3 = r == 0 ? dd.w : 0u;
                const uint32_t lo = __builtin_amdgcn_perm(d1, d0, 0x06040200u);   // even bytes of d0, d1
                const uint32_t hi = __builtin_amdgcn_perm(d3, d2, 0x06040200u);
                if (ow0[k] + 8 <= OW && (reinterpret_cast<uintptr_t>(dst[k]) & 3) == 0) {
                    const uint2 o = make_uint2(lo, hi);
                    __builtin_memcpy(dst[k], &o, 8);
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (ow0[k] + j < OW) dst[k][j] = (uint8_t)((j < 4 ? lo : hi) >> (8 * (j & 3)));
                }
            } else {
                if (ow0[k] + 4 <= OW && (reinterpret_cast<uintptr_t>(dst[k]) & 3) == 0) {
                    *reinterpret_cast<uint32_t *>(dst[k]) = g[k];
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (ow0[k] + j < OW) dst[k][j] = (uint8_t)(g[k] >> (8 * j));
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// host side: the launches of a plan (plan_conv, qe_conv_plan.hip, made every decision)
// ---------------------------------------------------------------------------------------------

// diagnostic (-DQE_STAMP) builds: where the kernels drop their per-wave phase sums
unsigned long long *g_mfma_dbg = nullptr;   // also read by qe_linear.hip (diagnostic builds)

int expand_codes_s8(const uint8_t *packed, int64_t n, int n_bits, int sign, uint8_t *out, hipStream_t s);   // qe_tpack.hip

static PrepArgs prep_args(const MfmaPlan &p, const qe_qparam *w, const float *bias, const qe_conv_shape *sh, uint8_t *base)
{
    PrepArgs pa;
    pa.w = w->data; pa.w_scale = w->scale; pa.w_zero = w->zero; pa.bias = bias;
    pa.w_bits = w->n_bits; pa.w_sign = w->sign; pa.w_per_tensor = (w->n_param == 1);
    pa.OC = sh->OC; pa.IC = sh->IC; pa.KK = p.KK; pa.OCP = p.OCP; pa.NG = p.NG; pa.KH = sh->KH; pa.KW = sh->KW;
    pa.wt = reinterpret_cast<int8_t *>(base);
    pa.ep = reinterpret_cast<float *>(base + p.ep_off);
    pa.ws = reinterpret_cast<int *>(base + p.ws_off);
    return pa;
}

static void launch_prep(const MfmaPlan &p, const PrepArgs &pa, hipStream_t s)
{
    if (p.family == MfmaFamily::Stem)
        hipLaunchKernelGGL(conv_mfma_prep_smallic_kernel, dim3(p.OCP), dim3(64), 0, s, pa, pa.KH, pa.KW);
    else
        hipLaunchKernelGGL(conv_mfma_prep_kernel, dim3(p.OCP), dim3(256), 0, s, pa);
}

// the x-independent tables (re-laid-out weights, per-channel constants, tap-sum tables) of plan_prepared into `prepared`
int prepare_conv_tables(const MfmaPlan &p, const qe_qparam *w, const float *bias, const qe_conv_shape *sh, void *prepared,
                        size_t prepared_bytes, hipStream_t s)
{
    if (p.prep_total == 0) return QE_OK;
    if (prepared == nullptr || prepared_bytes < p.prep_total) return QE_ERR_WORKSPACE;
    if ((reinterpret_cast<uintptr_t>(prepared) & 15) != 0) return QE_ERR_ARG;
    launch_prep(p, prep_args(p, w, bias, sh, static_cast<uint8_t *>(prepared)), s);
    QE_LAUNCH_CHECK();
    return QE_OK;
}

// The instance a plan selects: the one switch over the families.  Each family's unit names its instances (case by case,
// null for a parameter combination it does not compile), so a plan value outside the instantiated set cannot run a
// kernel compiled for another tile.
MfmaLaunch mfma_instance(const MfmaPlan &m, int KW, int split, bool rq, bool patch)
{
    switch (m.family) {
        case MfmaFamily::None: return nullptr;
        case MfmaFamily::Halo: {
            const int kkt = mfma_kkt(m.KK, KW);
            switch (m.cfg) {
                case 0: return mfma_halo_cfg0(m.niw, kkt, m.NS, rq, patch);
                case 1: return mfma_halo_cfg1(m.niw, kkt, m.NS, rq, patch);
                case 2: return mfma_halo_cfg2(m.niw, kkt, m.NS, rq, patch);
            }
            return nullptr;
        }
        case MfmaFamily::Ws: return (m.cfg == 0 && !patch) ? mfma_ws(m.niw, split, rq) : nullptr;
        case MfmaFamily::Sm2: return m.cfg <= 1 ? mfma_sm2(m.cfg == 0 ? 2 : 1, split, rq, patch) : nullptr;
        case MfmaFamily::Stem: return mfma_stem(m.cfg, m.niw, rq, patch);
        // the flat kernels test rq.out themselves (one instance for both epilogues, no PATCH form)
        case MfmaFamily::Flat: return patch ? nullptr : mfma_flat(m.cfg, m.niw, m.NS, m.wraw, false);
        case MfmaFamily::FlatS2: return patch ? nullptr : mfma_flat(m.cfg, m.niw, m.NS, m.wraw, true);
        case MfmaFamily::FlatX4: return (m.cfg == 0 && !m.wraw && !patch) ? mfma_flat_x4(m.niw, m.NS) : nullptr;
        case MfmaFamily::Flatg: return (m.cfg == 0 && !patch) ? mfma_flatg(m.niw, m.NS, m.wraw) : nullptr;
    }
    return nullptr;
}

// use_prepared = false: workspace = [prepared part | scratch], the tables are rebuilt on every call; true: the tables are
// in `prepared` (qe_conv_prepare) and the workspace holds the scratch only.  rq != nullptr: the plan's fused
// re-quantisation (codes into `codes`, the range flag into `status`, instead of fp32 into `out`); res != nullptr: its fused residual block end.
int launch_conv_mfma(const ConvPlan &p, const qe_qparam *x, const qe_qparam *w, const float *bias, const qe_conv_shape *sh,
                     float *out, void *workspace, size_t workspace_bytes, const void *prepared, size_t prepared_bytes,
                     bool use_prepared, hipStream_t s, const qe_requant *rq, uint8_t *codes, int32_t *status, const float *res)
{
    const MfmaPlan &m = p.m;
    uint8_t *wsp = static_cast<uint8_t *>(workspace);
    uint8_t *tables = wsp;
    size_t sub_off = m.sub_off, xe_off = m.xe_off;          // the plan's offsets count from [prepared part | scratch]
    if (!use_prepared) {
        if (m.total > 0) {
            if (workspace == nullptr || workspace_bytes < m.total) return QE_ERR_WORKSPACE;
            if ((reinterpret_cast<uintptr_t>(workspace) & 15) != 0) return QE_ERR_ARG;
        }
    } else {
        if (m.prep_total > 0) {
            if (prepared == nullptr || prepared_bytes < m.prep_total) return QE_ERR_WORKSPACE;
            if ((reinterpret_cast<uintptr_t>(prepared) & 15) != 0) return QE_ERR_ARG;
        }
        tables = static_cast<uint8_t *>(const_cast<void *>(prepared));
        if (m.total > m.prep_total) {
            if (workspace == nullptr || workspace_bytes < m.total - m.prep_total) return QE_ERR_WORKSPACE;
            if ((reinterpret_cast<uintptr_t>(workspace) & 15) != 0) return QE_ERR_ARG;
            if (m.sub) sub_off -= m.prep_total;                 // the workspace holds the scratch only
            if (m.expand) xe_off -= m.prep_total;
        }
    }
    const qe_conv_shape *rs = &p.run;

    // pre-passes: the activations the conv kernel reads become 8-bit codes in the workspace
    qe_qparam xr = *x;
    const uint8_t *xsrc = static_cast<const uint8_t *>(x->data);
    if (p.pre == PrePass::SubX4) {
        hipLaunchKernelGGL(subsample_x4_kernel, dim3((unsigned)p.pre_blocks), dim3(256), 0, s, xsrc, wsp + sub_off,
                           (int64_t)sh->N * sh->IC * rs->H, (int)sh->H, (int)sh->W, (int)rs->H, (int)rs->W, (int)x->sign);
        QE_LAUNCH_CHECK();
    } else {
        if (m.expand) {
            const int rc = expand_codes_s8(xsrc, (int64_t)sh->N * sh->IC * sh->H * sh->W, x->n_bits, x->sign, wsp + xe_off, s);
            if (rc != QE_OK) return rc;
            xsrc = wsp + xe_off;
            xr.data = xsrc;
        }
        const int64_t n_planes = (int64_t)sh->N * sh->IC;
        const dim3 grid((unsigned)p.pre_blocks);
        uint8_t *dst = wsp + sub_off;
#define QE_SUB2(L) hipLaunchKernelGGL(subsample2_kernel<L>, grid, dim3(256), 0, s, xsrc, dst, n_planes, (int)sh->H, (int)sh->W, \
                                      (int)rs->H, (int)rs->W, p.sub2_log_nq)
        switch (p.pre) {
            case PrePass::Sub2:
                switch (p.sub2_log_up) {
                    case 3: QE_SUB2(3); break; case 4: QE_SUB2(4); break; case 5: QE_SUB2(5); break;
                    case 6: QE_SUB2(6); break; case 7: QE_SUB2(7); break; default: QE_SUB2(8); break;
                }
                break;
            case PrePass::SubWide:
                hipLaunchKernelGGL(subsample_kernel<true>, grid, dim3(256), 0, s, xsrc, dst, n_planes, (int)sh->H, (int)sh->W,
                                   (int)rs->H, (int)rs->W, (int)sh->stride);
                break;
            case PrePass::SubNarrow:
                hipLaunchKernelGGL(subsample_kernel<false>, grid, dim3(256), 0, s, xsrc, dst, n_planes, (int)sh->H, (int)sh->W,
                                   (int)rs->H, (int)rs->W, (int)sh->stride);
                break;
            default: break;
        }
#undef QE_SUB2
        if (p.pre != PrePass::None) QE_LAUNCH_CHECK();
    }
    if (m.sub) xr.data = wsp + sub_off;
    if (m.sub_x4 || m.expand) { xr.n_bits = 8; xr.sign = 1; }

    if (p.route == ConvRoute::Pwr || p.route == ConvRoute::Pwr7) return launch_pwr(p, &xr, w, bias, out, s, rq, codes, status, res);
    if (p.route == ConvRoute::Flatd) return launch_flatd(p, &xr, w, bias, out, s, rq, codes, status);

    // the MFMA families; without a prepared buffer the tables are rebuilt in the workspace first (the flat kernels with
    // 8-bit weights read the packed tensor and build their constants themselves: no tables)
    const PrepArgs pa = prep_args(m, w, bias, rs, tables);
    if (!use_prepared && m.prep_total > 0) {
        launch_prep(m, pa, s);
        QE_LAUNCH_CHECK();
    }
    MfmaArgs a;
    a.x = static_cast<const uint8_t *>(xr.data);
    a.x_bytes = qe_packed_nbytes((int64_t)rs->N * rs->IC * rs->H * rs->W, xr.n_bits);
    a.x_zero = xr.zero; a.x_bits = xr.n_bits; a.x_sign = xr.sign;
    a.wt = pa.wt; a.ep = pa.ep; a.ws = pa.ws; a.out = out;
    a.N = rs->N; a.IC = rs->IC; a.H = rs->H; a.W = rs->W; a.OC = rs->OC; a.KH = rs->KH; a.KW = rs->KW;
    a.stride = rs->stride; a.pad = rs->padding; a.OH = m.OH; a.OW = m.OW;
    a.OCP = m.OCP; a.NG = m.NG; a.NCH = m.NCH;
    a.TH = m.TH; a.tiles_h = p.tiles_h; a.n_pix_tiles = p.n_pix_tiles; a.n_oc_tiles = p.n_oc_tiles;
    a.IHT = m.IHT; a.IWP = m.IWP; a.ROWMUL = m.ROWMUL; a.COLMUL = m.COLMUL; a.ni = m.ni;
    a.GI = m.GI;
    a.PADW = rs->padding;
    a.chunk = p.chunk;
    a.ptab_off = p.ptab_off; a.ctab = p.ctab ? 1 : 0;
    a.n_top = p.n_top; a.n_bot = p.n_bot; a.n_lft = p.n_lft; a.n_rgt = p.n_rgt;
    a.dbg = g_mfma_dbg;
    a.w_raw = w->data; a.w_scale = w->scale; a.w_zero = w->zero; a.x_scale = xr.scale; a.bias = bias;
    a.w_bits = w->n_bits; a.w_sign = w->sign; a.w_per_tensor = (w->n_param == 1);
    a.rq = make_rq_args(rq, codes, status);
    a.rq_patch = p.rq_patch ? 1 : 0;
    const MfmaLaunch launch = mfma_instance(m, rs->KW, p.split, rq != nullptr, p.rq_patch);
    if (launch == nullptr) return QE_ERR_UNSUPPORTED;       // never for a plan of plan_conv
    launch(a, (unsigned)p.blocks, p.lds, s);
    QE_LAUNCH_CHECK();
    return QE_OK;
}

}  // namespace qe

// Not part of the public ABI (absent from include/quant_engine.h): set the stamp buffer of a
// -DQE_STAMP diagnostic build.
extern "C" void qe_debug_set_stamp_buffer(unsigned long long *p) { qe::g_mfma_dbg = p; }
