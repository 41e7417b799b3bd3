// qe_conv_grp.hip -- grouped packed convolutions (1 < groups < C) for gfx950: codes in, fp32 and / or codes out.
//
// A grouped 3x3 layer reduces over 9 * Cg products per output (Cg = channels of a group), so it belongs on the int8 matrix
// cores.  Two kernels:
//
//   grp_fast_kernel<CG, STRIDE, OUT, CODES>   3x3, padding 1, stride 1 | 2, 8-bit x 8-bit codes of any sign pair, per-tensor
//     activation parameters, IC / groups == OC / groups == CG in {4, 8, 16, 32}.
//     A workgroup owns a SLAB of 32 consecutive channels (32 / CG whole groups; the last slab of a layer may be partial) and
//     walks tiles of it -- a band of TH whole output rows of one image each -- that the slab's workgroups share: a slab's
//     outputs depend only on the same slab's input planes.  At its start a wave builds the nine weight fragments from the raw
//     packed weights (off-group entries are zero: the slab is block diagonal for CG < 32; there are no prepared tables), and
//     the per-channel constants come from those fragments (v_dot4 against ones, the two lane halves added).  Per tile: the rows
//     the band reads are contiguous bytes per channel (NCHW); they are copied to LDS with 16-byte loads on 16-byte aligned
//     ADDRESSES (the LDS copy keeps each channel's address residue mod 16; edge chunks are completed bytewise and never read
//     outside the tensor), then transposed inside LDS into a [row][column -1 .. W][32 channels] tile of re-centred bytes
//     (stored ^ 0x80) whose out-of-image rows, columns and channels are zero.  The products run on v_mfma_i32_32x32x32_i8:
//     A = the slab's weights [output channel][K], B = the tile [K][pixel], K ordered (tap, channel in slab), one K-block of 32
//     per tap.  The window sum A of the arithmetic below comes from a second MFMA against a fragment of ones over the output
//     channel's group, skipped for a slab in which every zw' == 0.  The MFMA lanes (a pixel, 16 channels each) leave f in an
//     fp32 stage in LDS; a second pass with 8 threads per channel, that channel's constants in registers, turns f into y in
//     place and / or into the codes.  The stage leaves with 16-byte stores on aligned addresses per channel (edge chunks:
//     4-byte stores, single bytes only where a channel's span begins or ends inside a word).
//   grp_plain_kernel   one thread per output with unpack_elem: any groups dividing IC and OC, IC / groups != OC / groups, any
//     kernel up to 7x7, stride, padding and operand width, per-input-channel activation parameters.
//
// Arithmetic, per-tensor activation parameters (both kernels, the same fp32 operations in the same order, so they agree bit
// for bit); the scheme of the depthwise kernels extended over the group's channels:
//   z = zi + dz, zi = rint(z) (less 128 for an unsigned operand of the fast kernel: its bytes are re-centred), |dz| <= 1/2 exact
//   a = qx - zxi, b = qw - zwi                                   integers
//   I = sum a b, A = sum a, B = sum b, n = count   over the in-bounds taps and the group's IC / groups channels   int32, exact
//   f = (float)I + fma((float)n dzx, dzw, -dzx (float)B);  f = fma(-dzw, (float)A, f)  (second step only when dzw != 0)
//   y = fma(sx sw, f, bias);  relu: max(y, 0) with NaN passing;  codes: rq_value (qe_conv_common.hpp), as every fused epilogue
// I can exceed 2^24 (288 products of up to 255 * 255), so (float)I is a ROUNDING step (round to nearest even), the same one
// in both kernels; with integer zeros it is the only one before the final fma.
// Per-input-channel activation parameters (plain kernel only: the scale does not factor out of the channel sum): the same
// f_c per channel c of the group from that channel's I_c, A_c, B_c, n_c, then y = bias; y = fma(sx[c] sw, f_c, y) in channel
// order.
// The fast kernel gets I and A from S = sum qx' qw' (MFMA) and the group's box sum Bx = sum qx' (MFMA against ones), and B, n
// and the constants from a 16-entry table per output channel (top / bottom / left / right taps out of bounds) that the
// workgroup computes from the weights in LDS.
// The zero split, the float half, the border classes, the ReLU and the bodies of the 16-byte chunk copies are the depthwise
// kernels' too: qe_conv_span.hpp.
#include "qe_conv_grp.hpp"
#include "qe_conv_span.hpp"

#include <algorithm>

namespace qe {

struct GrpArgs : SpanOperands {
    int IC, OC, H, W, OH, OW, KH, KW, stride, pad, relu;
    int groups, icg, ocg;
    int TH, bands, nslabs, wps, ntiles;   // wps: workgroups of a slab; ntiles: N * bands, the tiles they share
    int in_rows, raw_stride, codes_stride, out_stride;
    int tile_off, stage_off, ostage_off;
};

struct GrpCls { int cI; float cF; };
struct GrpChanTab {
    int zwi, flags;            // flags: 1 zw' != 0 (the box sum enters), 2 dzw != 0 (the second fma)
    float ndzw, alpha, bias;
    RqConst rq;
    GrpCls c[16];              // per border class (bit 0 top, 1 bottom, 2 left, 3 right taps out of bounds)
    int nzx[16];
};

template <int CG, int S, bool HAS_OUT, bool HAS_CODES>
__global__ __launch_bounds__(GRP_THREADS) void grp_fast_kernel(const GrpArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t grp_lds[];
    GrpChanTab *tab = reinterpret_cast<GrpChanTab *>(grp_lds);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int C = a.IC;
    const int HW = a.H * a.W, OHW = a.OH * a.OW;
    const int TC = a.W + 2;

    // ---- the workgroup's slab: blockIdx.x = slab * wps + j, and the workgroup walks the tiles j, j + wps, .. of its slab ----------
    const int slab = (int)(blockIdx.x / (unsigned)a.wps);
    const int j0 = (int)(blockIdx.x - (unsigned)slab * a.wps);
    const int c0 = slab * GRP_SLAB;
    const int cs = min(GRP_SLAB, C - c0);                     // channels of this slab: a multiple of CG

    int zxi;
    float dzx;
    span_split_zero(a.xz[0], a.x_sign ? 0 : 128, zxi, dzx);

    // ---- the wave's weight fragments: lane (row r = output channel in slab, half h) holds K = 16 h + j of each tap ---------------
    v4i wf[9], ones;
    {
        unsigned od[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if ((16 * h + j) / CG == r / CG) od[j >> 2] |= 1u << (8 * (j & 3));
        ones = v4i{(int)od[0], (int)od[1], (int)od[2], (int)od[3]};
        const int64_t wrow = (int64_t)(c0 + r) * CG * 9;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            unsigned d[4] = {0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int ci = 16 * h + j;
                if (r < cs && ci / CG == r / CG) d[j >> 2] |= ((unsigned)a.w[wrow + (ci % CG) * 9 + t] ^ 0x80u) << (8 * (j & 3));
            }
            wf[t] = v4i{(int)d[0], (int)d[1], (int)d[2], (int)d[3]};
        }
    }

    // ---- per-output-channel constants, from the fragments: the off-group entries are zero, so a row's bytes sum to its group's ----
    {
        int swt[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            int sw = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) sw = __builtin_amdgcn_sdot4(wf[t][q], 0x01010101, sw, false);
            swt[t] = sw + __shfl_xor(sw, 32);
        }
        if (wave == 0 && h == 0) {
            GrpChanTab &T = tab[r];
            if (r < cs) {
                const int oc = c0 + r;
                int zwi;
                float dzw;
                span_split_zero(a.wz[a.w_pt ? 0 : oc], a.w_sign ? 0 : 128, zwi, dzw);
                T.zwi = zwi; T.ndzw = -dzw;
                T.flags = ((zwi != 0 || dzw != 0.0f) ? 1 : 0) | (dzw != 0.0f ? 2 : 0);
                T.alpha = a.xs[0] * a.ws[a.w_pt ? 0 : oc];
                T.bias = a.bias != nullptr ? a.bias[oc] : 0.0f;
                if constexpr (HAS_CODES) T.rq = span_rq_setup(a.rq, a.rq_pt ? 0 : oc);
                for (int cls = 0; cls < 16; ++cls) {
                    int taps = 0, sw = 0;
#pragma unroll
                    for (int t = 0; t < 9; ++t) {
                        if (!span_tap_off(cls, t / 3, t % 3)) { ++taps; sw += swt[t]; }
                    }
                    const int nn = taps * CG;
                    const int B = sw - nn * zwi;
                    T.c[cls].cI = -zxi * B;                // sum a b = S - zwi Bx - zxi (Sw - n zwi)
                    T.c[cls].cF = span_cf(nn, B, dzx, dzw);
                    T.nzx[cls] = nn * zxi;
                }
            } else {
                T.zwi = 0; T.flags = 0;
            }
        }
    }
    __syncthreads();
    // the 16 rows of a lane's accumulator: zwi and flags packed, and whether any row of the slab needs the box sum
    int zpk[16];
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const GrpChanTab &T = tab[(reg & 3) + 8 * (reg >> 2) + 4 * h];
        zpk[reg] = (T.zwi << 2) | T.flags;
    }
    const bool box = __builtin_amdgcn_ballot_w64((tab[r].flags & 1) != 0) != 0;
    // the channel a thread finishes in the second pass (8 threads per channel), its constants in registers
    const int ech = tid >> 3, esub = tid & 7;
    float e_alpha = 0.0f, e_bias = 0.0f;
    RqConst e_rq = {};
    if (ech < cs) {
        e_alpha = tab[ech].alpha; e_bias = tab[ech].bias;
        if constexpr (HAS_CODES) e_rq = tab[ech].rq;
    }

    uint8_t *raw = grp_lds + a.stage_off;
    uint8_t *tile = grp_lds + a.tile_off;
    uint8_t *cstage = grp_lds + a.stage_off;
    uint8_t *fstage = grp_lds + a.ostage_off;
    const uint8_t *x_lo = a.x, *x_hi = a.x + (int64_t)a.N * C * HW;
    bool bad = false;

    for (int tix = j0; tix < a.ntiles; tix += a.wps) {
        const int n = tix / a.bands, band = tix - n * a.bands;
        const int oh0 = band * a.TH;
        const int rows = min(a.TH, a.OH - oh0);
        const int ih_base = oh0 * S - 1;                          // image row of tile row 0
        const int ih_lo = max(0, ih_base);
        const int ih_hi = min(a.H, (oh0 + rows - 1) * S + 2);
        const int in_len = (ih_hi - ih_lo) * a.W;                 // bytes of a channel's span
        const int64_t plane0 = (int64_t)n * C + c0;
        const uint8_t *gin0 = a.x + plane0 * HW + ih_lo * a.W;   // 64-bit plane base, 32-bit in-plane offset
        const uintptr_t gin0_addr = reinterpret_cast<uintptr_t>(gin0);
        const int npx = rows * a.OW;                              // outputs of a channel: contiguous (whole rows)
        const int64_t out0 = plane0 * OHW + oh0 * a.OW;
        uint8_t *gcodes0 = HAS_CODES ? a.rq.out + out0 : nullptr;
        float *gout0 = HAS_OUT ? a.out + out0 : nullptr;
        const uintptr_t gcodes_addr = reinterpret_cast<uintptr_t>(gcodes0), gout_addr = reinterpret_cast<uintptr_t>(gout0);

        // ---- copy the channels' spans in: 16-byte loads on aligned addresses ------------------------------------------------------
        {
            const int maxchunks = a.raw_stride >> 4;
            const int total = cs * maxchunks;
            for (int k = tid; k < total; k += GRP_THREADS) {
                const int ch = k / maxchunks, i = k - ch * maxchunks;
                const uint8_t *g = gin0 + (int64_t)ch * HW;
                const int lead = (int)(reinterpret_cast<uintptr_t>(g) & 15);
                if (i >= ((lead + in_len + 15) >> 4)) continue;
                const uint8_t *src = g - lead + 16 * i;
                *reinterpret_cast<uint4 *>(raw + ch * a.raw_stride + 16 * i) = span_load16(src, x_lo, x_hi);
            }
        }
        __syncthreads();

        // ---- transpose into the channel-interleaved tile: [tile row][column -1 .. W][32 channels], re-centred, zero outside -------
        {
            const int items = a.in_rows * TC * 8;
            for (int it = tid; it < items; it += GRP_THREADS) {
                const int q = it & 7, px = it >> 3;
                const int trow = px / TC, tcol = px - trow * TC;
                const int ih = ih_base + trow, iw = tcol - 1;
                unsigned v = 0;
                if (ih >= ih_lo && ih < ih_hi && iw >= 0 && iw < a.W) {
                    const int o = (ih - ih_lo) * a.W + iw;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int ch = 4 * q + k;
                        if (ch < cs) {
                            const int lead = (int)((gin0_addr + (uintptr_t)ch * (uintptr_t)HW) & 15);
                            v |= ((unsigned)raw[ch * a.raw_stride + lead + o] ^ 0x80u) << (8 * k);
                        }
                    }
                }
                *reinterpret_cast<unsigned *>(tile + px * 32 + 4 * q) = v;
            }
        }
        __syncthreads();

        // ---- first pass: a wave takes 32 consecutive outputs of the band at a time, all 32 channels; f goes to LDS ---------------
        int foff[16];                                             // a row's place in the fp32 stage (aligned as its global span)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int ocl = (reg & 3) + 8 * (reg >> 2) + 4 * h;   // C/D map of the 32x32 shapes: the row
            foff[reg] = ocl * a.out_stride + (HAS_OUT ? (int)((gout_addr + 4 * (uintptr_t)ocl * (uintptr_t)OHW) & 15) : 0);
        }
        for (int p0 = wave * 32; p0 < npx; p0 += (GRP_THREADS / 64) * 32) {
            const bool valid = p0 + r < npx;
            const int pl = valid ? p0 + r : npx - 1;
            const int orow = pl / a.OW, ocol = pl - orow * a.OW;
            const uint8_t *bp = tile + ((orow * S) * TC + ocol * S) * 32 + 16 * h;
            v16i acc = {0}, acc2 = {0};
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const v4i bf = *reinterpret_cast<const v4i *>(bp + ((t / 3) * TC + (t % 3)) * 32);
                acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(wf[t], bf, acc, 0, 0, 0);
                if (box) acc2 = __builtin_amdgcn_mfma_i32_32x32x32_i8(ones, bf, acc2, 0, 0, 0);
            }
            const int oh = oh0 + orow;                            // span_out_cls, written out: see section 4g-bis
            const int cls = (oh * S - 1 < 0 ? 1 : 0) | (oh * S + 1 >= a.H ? 2 : 0) | (ocol == 0 ? 4 : 0) | (ocol * S + 1 >= a.W ? 8 : 0);
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int ocl = (reg & 3) + 8 * (reg >> 2) + 4 * h;
                if (!valid || ocl >= cs) continue;
                const GrpChanTab &T = tab[ocl];
                const GrpCls c = T.c[cls];
                const int pk = zpk[reg];
                float f;
                if (pk & 1) {
                    f = (float)(acc[reg] - (pk >> 2) * acc2[reg] + c.cI) + c.cF;
                    if (pk & 2) f = fmaf(T.ndzw, (float)(acc2[reg] - T.nzx[cls]), f);
                } else {
                    f = (float)(acc[reg] + c.cI) + c.cF;
                }
                *reinterpret_cast<float *>(fstage + foff[reg] + 4 * pl) = f;
            }
        }
        __syncthreads();

        // ---- second pass: 8 threads per channel, its constants in registers: y in place, and / or the codes ------------------------
        if (ech < cs) {
            float *fp = reinterpret_cast<float *>(fstage + ech * a.out_stride +
                                                  (HAS_OUT ? (int)((gout_addr + 4 * (uintptr_t)ech * (uintptr_t)OHW) & 15) : 0));
            uint8_t *cp = cstage + ech * a.codes_stride + (HAS_CODES ? (int)((gcodes_addr + (uintptr_t)ech * (uintptr_t)OHW) & 15) : 0);
            for (int px = esub; px < npx; px += 8) {
                float y = fmaf(e_alpha, fp[px], e_bias);
                if (a.relu) y = span_relu(y);
                if constexpr (HAS_OUT) fp[px] = y;
                if constexpr (HAS_CODES) cp[px] = (uint8_t)(unsigned)rq_value(e_rq, y, bad);
            }
        }
        __syncthreads();

        // ---- copy the results out, channel by channel: 16-byte stores on aligned addresses; edge chunks word by word, byte by byte
        if constexpr (HAS_CODES) {
            const int maxchunks = a.codes_stride >> 4;
            const int total = cs * maxchunks;
            for (int k = tid; k < total; k += GRP_THREADS) {
                const int ch = k / maxchunks, i = k - ch * maxchunks;
                uint8_t *g = gcodes0 + (int64_t)ch * OHW;
                const int lead = (int)(reinterpret_cast<uintptr_t>(g) & 15);
                if (i >= ((lead + npx + 15) >> 4)) continue;
                const uint8_t *lo = g, *hi = g + npx;
                uint8_t *dst = g - lead + 16 * i;
                const uint4 v = *reinterpret_cast<const uint4 *>(cstage + ch * a.codes_stride + 16 * i);
                if (dst >= lo && dst + 16 <= hi) {             // span_store16_bytes, written out: see section 4g-bis
                    *reinterpret_cast<uint4 *>(dst) = v;
                } else {
                    const unsigned d[4] = {v.x, v.y, v.z, v.w};
                    for (int q = 0; q < 4; ++q) {
                        uint8_t *dq = dst + 4 * q;
                        if (dq >= lo && dq + 4 <= hi) {
                            *reinterpret_cast<unsigned *>(dq) = d[q];
                        } else {
                            for (int b = 0; b < 4; ++b)
                                if (dq + b >= lo && dq + b < hi) dq[b] = (uint8_t)(d[q] >> (8 * b));
                        }
                    }
                }
            }
        }
        if constexpr (HAS_OUT) {
            const int maxchunks = a.out_stride >> 4;
            const int total = cs * maxchunks;
            for (int k = tid; k < total; k += GRP_THREADS) {
                const int ch = k / maxchunks, i = k - ch * maxchunks;
                uint8_t *g = reinterpret_cast<uint8_t *>(gout0 + (int64_t)ch * OHW);
                const int lead = (int)(reinterpret_cast<uintptr_t>(g) & 15);
                if (i >= ((lead + 4 * npx + 15) >> 4)) continue;
                const uint8_t *lo = g, *hi = g + 4 * (int64_t)npx;
                uint8_t *dst = g - lead + 16 * i;
                const uint4 v = *reinterpret_cast<const uint4 *>(fstage + ch * a.out_stride + 16 * i);
                span_store16_words(dst, v, lo, hi);
            }
        }
        __syncthreads();                                          // the stage is the next tile's raw span
    }
    if constexpr (HAS_CODES) rq_report(a.rq, bad);
}

// One thread per output: every grouped problem the fast family does not take.
__global__ __launch_bounds__(GRP_THREADS) void grp_plain_kernel(const GrpArgs a)
{
    const int64_t OHW = (int64_t)a.OH * a.OW;
    const int64_t idx = (int64_t)blockIdx.x * GRP_THREADS + threadIdx.x;
    bool bad = false;
    if (idx < (int64_t)a.N * a.OC * OHW) {
        const int64_t p = idx / OHW;                  // n * OC + oc
        const int rem = (int)(idx - p * OHW);
        const int oh = rem / a.OW, ow = rem - oh * a.OW;
        const int oc = (int)(p % a.OC);
        const int64_t n = p / a.OC;
        const int ic0 = (oc / a.ocg) * a.icg;
        int zwi;
        float dzw;
        span_split_zero(a.wz[a.w_pt ? 0 : oc], 0, zwi, dzw);
        const float sw = a.ws[a.w_pt ? 0 : oc];
        const int64_t wb = (int64_t)oc * a.icg * a.KH * a.KW;
        int I = 0, A = 0, B = 0, nn = 0;
        int zxi = 0;
        float dzx = 0.0f;
        if (a.x_pt) span_split_zero(a.xz[0], 0, zxi, dzx);
        float y = a.bias != nullptr ? a.bias[oc] : 0.0f;
        for (int ci = 0; ci < a.icg; ++ci) {
            const int ic = ic0 + ci;
            if (!a.x_pt) {
                span_split_zero(a.xz[ic], 0, zxi, dzx);
                I = A = B = nn = 0;
            }
            const int64_t xb = (n * a.IC + ic) * a.H * a.W;
            for (int kh = 0; kh < a.KH; ++kh) {
                const int ih = oh * a.stride - a.pad + kh;
                if (ih < 0 || ih >= a.H) continue;
                for (int kw = 0; kw < a.KW; ++kw) {
                    const int iw = ow * a.stride - a.pad + kw;
                    if (iw < 0 || iw >= a.W) continue;
                    const int qa = unpack_elem(a.x, xb + (int64_t)ih * a.W + iw, a.x_bits, a.x_sign) - zxi;
                    const int qb = unpack_elem(a.w, wb + ((int64_t)ci * a.KH + kh) * a.KW + kw, a.w_bits, a.w_sign) - zwi;
                    I += qa * qb; A += qa; B += qb; ++nn;
                }
            }
            if (!a.x_pt) {
                float f = (float)I + span_cf(nn, B, dzx, dzw);
                if (dzw != 0.0f) f = fmaf(-dzw, (float)A, f);
                y = fmaf(a.xs[ic] * sw, f, y);
            }
        }
        if (a.x_pt) {
            float f = (float)I + span_cf(nn, B, dzx, dzw);
            if (dzw != 0.0f) f = fmaf(-dzw, (float)A, f);
            y = fmaf(a.xs[0] * sw, f, y);
        }
        if (a.relu) y = span_relu(y);
        if (a.out != nullptr) a.out[idx] = y;
        if (a.rq.out != nullptr) {
            const RqConst rc = span_rq_setup(a.rq, a.rq_pt ? 0 : oc);
            a.rq.out[idx] = (uint8_t)(unsigned)rq_value(rc, y, bad);
        }
    }
    if (a.rq.out != nullptr) rq_report(a.rq, bad);
}

// ---- host: the plan ---------------------------------------------------------------------------------------------------

GrpPlan plan_grp(const GrpRequest &r)
{
    GrpPlan p;
    const qe_conv_shape &s = *r.sh;
    const int g = r.groups;
    if (g <= 1 || s.IC % g != 0 || s.OC % g != 0 || (g == s.IC && g == s.OC)) return p;
    if (s.KH > GRP_MAX_K || s.KW > GRP_MAX_K || 2 * s.padding > std::min(s.KH, s.KW)) return p;
    if (s.H + 2 * s.padding < s.KH || s.W + 2 * s.padding < s.KW) return p;
    p.OH = (s.H + 2 * s.padding - s.KH) / s.stride + 1;
    p.OW = (s.W + 2 * s.padding - s.KW) / s.stride + 1;
    if ((int64_t)s.H * s.W > 0x7fffffffLL) return p;                   // in-plane offsets are 32-bit
    p.two_pass = (r.rq_bits > 0 && r.rq_bits < 8) ? 1 : 0;
    p.out16 = (r.has_out && (r.out & 15) == 0) ? 1 : 0;
    p.codes16 = (r.rq_bits == 8 && (r.codes & 15) == 0) ? 1 : 0;
    const bool k_out = r.has_out, k_codes = r.rq_bits == 8;

    // the plain kernel: one thread per output
    p.kernel = GRP_PLAIN;
    p.slab = 1; p.TH = 1; p.TW = 1; p.tiles = p.OH * p.OW; p.nslabs = s.OC; p.lds = 0;
    p.blocks = ceil_div64((int64_t)s.N * s.OC * p.OH * p.OW, GRP_THREADS);
    if (p.blocks > 0x7fffffffLL) { p.kernel = GRP_NONE; return p; }

    const int cg = s.IC / g;
    const int cgi = cg == 4 ? 0 : cg == 8 ? 1 : cg == 16 ? 2 : cg == 32 ? 3 : -1;
    const bool fast = s.KH == 3 && s.KW == 3 && s.padding == 1 && (s.stride == 1 || s.stride == 2) && r.x_bits == 8 &&
                      r.w_bits == 8 && r.x_n_param == 1 && s.IC == s.OC && cgi >= 0 && (k_out || k_codes);
    if (!fast) return p;
    const int S = s.stride;
    GrpPlan f = p;
    auto lds_of = [&](int TH, GrpPlan &q) {
        const int in_rows = (TH - 1) * S + 3;
        const int npx = TH * p.OW;
        q.in_rows = in_rows;
        q.raw_stride = round16(std::min(s.H, in_rows) * s.W + 30);
        q.codes_stride = k_codes ? round16(npx + 30) : 0;
        q.out_stride = round16(4 * npx + 27);             // the fp32 stage: always (the first pass leaves f there)
        q.tile_off = round16(GRP_SLAB * (int)sizeof(GrpChanTab));
        q.stage_off = q.tile_off + in_rows * (s.W + 2) * 32;
        q.ostage_off = q.stage_off + GRP_SLAB * q.codes_stride;
        const int64_t stage = std::max<int64_t>((int64_t)GRP_SLAB * q.raw_stride, (int64_t)GRP_SLAB * (q.codes_stride + q.out_stride));
        return (int64_t)q.stage_off + stage;
    };
    if ((int64_t)s.W * 3 * 32 > GRP_LDS_BUDGET) return p;             // a row too wide for the LDS: the plain kernel
    int TH = std::max(1, std::min(p.OH, GRP_MAX_PIXELS / std::max(1, p.OW)));
    while (TH >= 1 && lds_of(TH, f) > GRP_LDS_BUDGET) --TH;
    if (TH < 1) return p;
    f.tiles = ceil_div(p.OH, TH);
    f.TH = ceil_div(p.OH, f.tiles);                                     // bands of equal height (the last may be shorter)
    f.tiles = ceil_div(p.OH, f.TH);
    f.TW = p.OW;
    f.lds = lds_of(f.TH, f);
    f.slab = GRP_SLAB;
    f.nslabs = ceil_div(s.IC, GRP_SLAB);
    // a workgroup builds its slab's weight fragments once and walks the tiles of its slab: two workgroups per CU in all
    const int64_t ntiles = (int64_t)s.N * f.tiles;
    if (ntiles > 0x7fffffffLL) return p;
    f.wps = (int)std::min<int64_t>(ntiles, std::max(1, 2 * kNumCU / f.nslabs));
    f.blocks = (int64_t)f.nslabs * f.wps;
    f.kernel = GRP_FAST_FIRST + 6 * cgi + 3 * (S - 1) + (k_out && k_codes ? 2 : k_codes ? 1 : 0);
    return f;
}

// the instances by number: the plain kernel, then the fast family as plan_grp numbers it (Cg, then stride, then out | codes | both)
template <int CG, int S, bool HAS_OUT, bool HAS_CODES>
constexpr SpanLaunch<GrpArgs> grp_fast = &launch_instance<&grp_fast_kernel<CG, S, HAS_OUT, HAS_CODES>, GrpArgs>;
#define GRP_CG(CG) grp_fast<CG, 1, true, false>, grp_fast<CG, 1, false, true>, grp_fast<CG, 1, true, true>, \
                   grp_fast<CG, 2, true, false>, grp_fast<CG, 2, false, true>, grp_fast<CG, 2, true, true>
static constexpr SpanLaunch<GrpArgs> kGrpInstances[] = {&launch_instance<&grp_plain_kernel, GrpArgs>, GRP_CG(4), GRP_CG(8), GRP_CG(16),
                                                        GRP_CG(32)};
#undef GRP_CG
static_assert(sizeof(kGrpInstances) / sizeof(kGrpInstances[0]) == GRP_KERNELS, "one launcher per instance number");

int launch_grp(const GrpPlan &p, const qe_qparam *x, const qe_qparam *w, const float *bias, const qe_conv_shape *sh, int groups,
               int relu, float *out, const qe_requant *rq, uint8_t *codes, int32_t *status, hipStream_t s)
{
    if (p.kernel < 0 || p.kernel >= GRP_KERNELS) return QE_ERR_UNSUPPORTED;
    GrpArgs a;
    static_cast<SpanOperands &>(a) = span_operands(x, w, bias, sh->N, out, rq, codes, status);
    a.IC = sh->IC; a.OC = sh->OC; a.H = sh->H; a.W = sh->W; a.OH = p.OH; a.OW = p.OW; a.KH = sh->KH; a.KW = sh->KW;
    a.stride = sh->stride; a.pad = sh->padding; a.relu = relu ? 1 : 0;
    a.groups = groups; a.icg = sh->IC / groups; a.ocg = sh->OC / groups;
    a.TH = p.TH; a.bands = p.tiles; a.nslabs = p.nslabs; a.wps = p.wps; a.ntiles = sh->N * p.tiles;
    a.in_rows = p.in_rows; a.raw_stride = p.raw_stride; a.codes_stride = p.codes_stride; a.out_stride = p.out_stride;
    a.tile_off = p.tile_off; a.stage_off = p.stage_off; a.ostage_off = p.ostage_off;
    kGrpInstances[p.kernel]((unsigned)p.blocks, GRP_THREADS, (size_t)p.lds, 0, s, a);
    QE_LAUNCH_CHECK();
    return QE_OK;
}

}  // namespace qe
