// qe_conv_dw.hip -- depthwise packed convolutions (groups == IC == OC) for gfx950: codes in, fp32 and / or codes out.
//
// A depthwise layer has no reduction over channels, so there is nothing for the matrix cores: it is 9 multiply-adds per output
// and memory bound.  Two kernels:
//
//   dw_fast_kernel<STRIDE, OUT, CODES>   3x3, padding 1, stride 1 | 2, 8-bit x 8-bit codes of any sign pair.
//     A workgroup takes ONE CONTIGUOUS SPAN of the NCHW byte planes: G whole consecutive planes (small planes), or the rows
//     that a band of TH output rows of one plane reads (one-row halo).  The span is copied to LDS with 16-byte loads on
//     16-byte aligned ADDRESSES (the LDS copy keeps the address residue mod 16, so 49- and 196-byte planes on any base cost
//     nothing; the two edge chunks are completed bytewise and never read outside the tensor), each byte re-centred to a signed
//     code (stored ^ 0x80 == stored - 128) on the way.  A thread computes 4 consecutive outputs of one row: per input row three
//     aligned LDS words are funnel-shifted to the 6 (stride 1) or 9 (stride 2) bytes it needs, and each three-byte window goes
//     through one v_dot4_i32_i8 against (w0, w1, w2, 0).  Padding is a zero weight row (rows) or a cleared byte (columns -1 and
//     W), so the int32 sums run over in-bounds taps only.  Results go to LDS as well and leave with 16-byte stores on aligned
//     addresses (edge chunks: 4-byte stores, single bytes only where a span begins or ends inside a word).
//   dw_plain_kernel   one thread per output, any kernel up to 7x7, stride, padding and operand width (unpack_elem).
//
// Arithmetic (both kernels, the same fp32 operations in the same order, so they agree bit for bit):
//   z = zi + dz, zi = rint(z) (less 128 for an unsigned operand of the fast kernel: its bytes are re-centred), |dz| <= 1/2 exact
//   a = qx - zxi, b = qw - zwi                                   integers
//   I = sum a b, A = sum a, B = sum b, n = taps  over the in-bounds taps       int32, exact
//   f = (float)I + fma(n dzx, dzw, -dzx (float)B);  f = fma(-dzw, (float)A, f)  (second step only when zw != 0)
//   y = fma(sx sw, f, bias);  relu: max(y, 0) with NaN passing;  codes: rq_value (qe_conv_common.hpp), as every fused epilogue
// The fast kernel gets I, A from S = sum qx qw and the box sum Bx = sum qx (three more dot4 against (1, 1, 1, 0), skipped for a
// plane with zw == 0), and B, n and the constants from a 16-entry table per plane (top / bottom / left / right tap out of
// bounds) that the workgroup computes in LDS: there are no prepared tables.  With integer zeros everything is exact integers,
// and non-integer zeros only add terms of the size of |dz| * sum, so nothing cancels at the size of the uncentred sums.
// The zero split, the float half, the border classes, the ReLU and the bodies of the 16-byte chunk copies are the grouped
// kernels' too: qe_conv_span.hpp.
#include "qe_conv_dw.hpp"
#include "qe_conv_span.hpp"

namespace qe {

struct DwArgs : SpanOperands {
    int C, H, W, OH, OW, KH, KW, stride, pad, relu;
    int G, TH, bands, ncg;
    unsigned m_ncg, m_oh;
    int in_off, codes_off, out_off;
    int64_t NP;                // planes: N * C
};

struct DwPlaneTab {
    int w[3];            // weight rows as signed bytes (w0, w1, w2, 0)
    int zxi, zwi, need_box;
    float ndzw, alpha, bias;
    int pad_;
    RqConst rq;
    int cI[16], nzx[16]; // per border class (bit 0 top, 1 bottom, 2 left, 3 right tap out of bounds)
    float cF[16];
};

template <int S, bool HAS_OUT, bool HAS_CODES>
__global__ __launch_bounds__(DW_THREADS) void dw_fast_kernel(const DwArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t dw_lds[];
    DwPlaneTab *tab = reinterpret_cast<DwPlaneTab *>(dw_lds);
    const int tid = threadIdx.x;
    const int HW = a.H * a.W, OHW = a.OH * a.OW;

    // ---- the workgroup's span -----------------------------------------------------------------------------------------
    int64_t p0;
    int g, oh0, rows, ih_lo, in_len;
    if (a.bands == 1) {
        p0 = (int64_t)blockIdx.x * a.G;
        g = (int)min((int64_t)a.G, a.NP - p0);
        oh0 = 0; rows = a.OH; ih_lo = 0; in_len = g * HW;
    } else {
        p0 = blockIdx.x / (unsigned)a.bands;
        const int t = blockIdx.x - (unsigned)p0 * a.bands;
        g = 1;
        oh0 = t * a.TH;
        rows = min(a.TH, a.OH - oh0);
        ih_lo = max(0, oh0 * S - 1);
        const int ih_hi = min(a.H, (oh0 + rows - 1) * S + 2);
        in_len = (ih_hi - ih_lo) * a.W;
    }
    const uint8_t *gin = a.x + p0 * HW + ih_lo * a.W;       // 64-bit plane base, 32-bit in-plane offset
    const int lead = (int)(reinterpret_cast<uintptr_t>(gin) & 15);
    const int out_len = g * rows * a.OW;                     // whole planes, or rows of one plane: contiguous either way
    const int64_t out0 = p0 * OHW + oh0 * a.OW;

    // ---- per-plane constants --------------------------------------------------------------------------------------------
    if (tid < g) {
        DwPlaneTab &T = tab[tid];
        const int c = (int)((p0 + tid) % a.C);
        int wv[3][3];
        for (int r = 0; r < 3; ++r) {
            unsigned pk = 0;
            for (int k = 0; k < 3; ++k) {
                const unsigned b = a.w[(int64_t)c * 9 + r * 3 + k] ^ 0x80u;
                wv[r][k] = (int)(int8_t)b;
                pk |= b << (8 * k);
            }
            T.w[r] = (int)pk;
        }
        int zxi, zwi;
        float dzx, dzw;
        span_split_zero(a.xz[a.x_pt ? 0 : c], a.x_sign ? 0 : 128, zxi, dzx);
        span_split_zero(a.wz[a.w_pt ? 0 : c], a.w_sign ? 0 : 128, zwi, dzw);
        T.zxi = zxi; T.zwi = zwi; T.ndzw = -dzw;
        T.need_box = (zwi != 0 || dzw != 0.0f) ? 1 : 0;
        T.alpha = a.xs[a.x_pt ? 0 : c] * a.ws[a.w_pt ? 0 : c];
        T.bias = a.bias != nullptr ? a.bias[c] : 0.0f;
        if constexpr (HAS_CODES) T.rq = span_rq_setup(a.rq, a.rq_pt ? 0 : c);
        for (int cls = 0; cls < 16; ++cls) {
            int n = 0, sw = 0;
            for (int r = 0; r < 3; ++r)
                for (int k = 0; k < 3; ++k)
                    if (!span_tap_off(cls, r, k)) { ++n; sw += wv[r][k]; }
            const int B = sw - n * zwi;
            T.cI[cls] = -zxi * B;                  // sum a b = S - zwi Bx - zxi (Sw - n zwi)
            T.nzx[cls] = n * zxi;
            T.cF[cls] = span_cf(n, B, dzx, dzw);
        }
    }

    // ---- copy the span in: 16-byte loads on aligned addresses, bytes re-centred ----------------------------------------------
    {
        const uint8_t *x_lo = a.x, *x_hi = a.x + a.NP * HW;
        const uint8_t *A0 = gin - lead;
        const int chunks = (lead + in_len + 15) >> 4;
        for (int i = tid; i < chunks; i += DW_THREADS) {
            const uint8_t *src = A0 + 16 * i;
            uint4 v = span_load16(src, x_lo, x_hi);
            v.x ^= 0x80808080u; v.y ^= 0x80808080u; v.z ^= 0x80808080u; v.w ^= 0x80808080u;
            *reinterpret_cast<uint4 *>(dw_lds + a.in_off + 16 * i) = v;
        }
    }
    __syncthreads();

    // ---- compute: a unit is 4 consecutive outputs of one row --------------------------------------------------------------
    uint8_t *gcodes = HAS_CODES ? a.rq.out + out0 : nullptr;
    float *gout = HAS_OUT ? a.out + out0 : nullptr;
    const int lead_c = (int)(reinterpret_cast<uintptr_t>(gcodes) & 15);
    const int lead_o = (int)(reinterpret_cast<uintptr_t>(gout) & 15);
    uint8_t *lcodes = dw_lds + a.codes_off + lead_c;
    uint8_t *lout = dw_lds + a.out_off + lead_o;
    const int in_base = a.in_off + lead;
    bool bad = false;
    const int units = g * rows * a.ncg;
    for (int u = tid; u < units; u += DW_THREADS) {
        const int q1 = (int)__umulhi(2u * (unsigned)u, a.m_ncg);
        const int cg = u - q1 * a.ncg;
        int gi = 0, r = q1;
        if (a.bands == 1) {
            gi = (int)__umulhi(2u * (unsigned)q1, a.m_oh);
            r = q1 - gi * a.OH;
        }
        const DwPlaneTab &T = tab[gi];
        const int oh = oh0 + r, ow0 = cg * DW_VEC;
        const int ih0 = oh * S - 1, col0 = ow0 * S - 1;
        const int rb = span_row_cls(oh, S, a.H);
        const bool top = rb & 1, bot = rb & 2;
        const int mid = in_base + gi * HW + (ih0 + 1 - ih_lo) * a.W + col0;
        // byte masks: column -1 (byte 0 of the first unit of a row) and column W (byte ir)
        const int ir = a.W - col0;
        unsigned m0 = ow0 == 0 ? 0xffffff00u : 0xffffffffu;
        if (ir < 4) m0 &= ~(0xffu << (8 * ir));
        const unsigned m1 = (unsigned)(ir - 4) < 4u ? ~(0xffu << (8 * (ir - 4))) : 0xffffffffu;
        const unsigned m2 = ir == 8 ? 0u : 0xffffffffu;
        const bool box = T.need_box != 0;

        int acc[DW_VEC] = {0, 0, 0, 0}, bx[DW_VEC] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const bool valid = k == 1 || (k == 0 ? !top : !bot);
            const int o = valid ? mid + (k - 1) * a.W : mid;
            const unsigned *p = reinterpret_cast<const unsigned *>(dw_lds + (o & ~3));
            const unsigned sh = (unsigned)o & 3u;
            const unsigned d0 = p[0], d1 = p[1], d2 = p[2];
            const unsigned b0 = __builtin_amdgcn_alignbyte(d1, d0, sh) & m0;
            const unsigned b1 = __builtin_amdgcn_alignbyte(d2, d1, sh) & m1;
            const int wk = valid ? T.w[k] : 0;
            const int ok = valid ? 0x00010101 : 0;
            unsigned win[DW_VEC];
            if constexpr (S == 1) {
                win[0] = b0;
                win[1] = __builtin_amdgcn_alignbyte(b1, b0, 1);
                win[2] = __builtin_amdgcn_alignbyte(b1, b0, 2);
                win[3] = __builtin_amdgcn_alignbyte(b1, b0, 3);
            } else {
                const unsigned b2 = (d2 >> (8 * sh)) & m2;
                win[0] = b0;
                win[1] = __builtin_amdgcn_alignbyte(b1, b0, 2);
                win[2] = b1;
                win[3] = __builtin_amdgcn_alignbyte(b2, b1, 2);
            }
#pragma unroll
            for (int j = 0; j < DW_VEC; ++j) acc[j] = __builtin_amdgcn_sdot4((int)win[j], wk, acc[j], false);
            if (box) {
#pragma unroll
                for (int j = 0; j < DW_VEC; ++j) bx[j] = __builtin_amdgcn_sdot4((int)win[j], ok, bx[j], false);
            }
        }

        const int orow = (gi * rows + r) * a.OW + ow0;       // offset in the workgroup's output span
#pragma unroll
        for (int j = 0; j < DW_VEC; ++j) {
            const int ow = ow0 + j;
            if (ow >= a.OW) break;
            const int cls = span_out_cls(rb, ow, S, a.W);
            float f;
            if (box) {
                f = (float)(acc[j] - T.zwi * bx[j] + T.cI[cls]) + T.cF[cls];
                f = fmaf(T.ndzw, (float)(bx[j] - T.nzx[cls]), f);
            } else {
                f = (float)(acc[j] + T.cI[cls]) + T.cF[cls];
            }
            float y = fmaf(T.alpha, f, T.bias);
            if (a.relu) y = span_relu(y);
            if constexpr (HAS_OUT) *reinterpret_cast<float *>(lout + 4 * (orow + j)) = y;
            if constexpr (HAS_CODES) lcodes[orow + j] = (uint8_t)(unsigned)rq_value(T.rq, y, bad);
        }
    }
    if constexpr (HAS_CODES) rq_report(a.rq, bad);
    __syncthreads();

    // ---- copy the results out: 16-byte stores on aligned addresses; the edge chunks word by word, byte by byte ----------------
    if constexpr (HAS_CODES) {
        const uint8_t *lo = gcodes, *hi = gcodes + out_len;
        uint8_t *A0 = gcodes - lead_c;
        const int chunks = (lead_c + out_len + 15) >> 4;
        for (int i = tid; i < chunks; i += DW_THREADS) {
            uint8_t *dst = A0 + 16 * i;
            const uint4 v = *reinterpret_cast<const uint4 *>(dw_lds + a.codes_off + 16 * i);
            span_store16_bytes(dst, v, lo, hi);
        }
    }
    if constexpr (HAS_OUT) {
        const uint8_t *lo = reinterpret_cast<uint8_t *>(gout), *hi = lo + 4 * (int64_t)out_len;
        uint8_t *A0 = reinterpret_cast<uint8_t *>(gout) - lead_o;
        const int chunks = (lead_o + 4 * out_len + 15) >> 4;
        for (int i = tid; i < chunks; i += DW_THREADS) {
            uint8_t *dst = A0 + 16 * i;
            const uint4 v = *reinterpret_cast<const uint4 *>(dw_lds + a.out_off + 16 * i);
            span_store16_words(dst, v, lo, hi);
        }
    }
}

// One thread per output: every depthwise problem the fast kernel does not take.
__global__ __launch_bounds__(DW_THREADS) void dw_plain_kernel(const DwArgs a)
{
    const int64_t OHW = (int64_t)a.OH * a.OW;
    const int64_t idx = (int64_t)blockIdx.x * DW_THREADS + threadIdx.x;
    bool bad = false;
    if (idx < a.NP * OHW) {
        const int64_t p = idx / OHW;
        const int rem = (int)(idx - p * OHW);
        const int oh = rem / a.OW, ow = rem - oh * a.OW;
        const int c = (int)(p % a.C);
        int zxi, zwi;
        float dzx, dzw;
        span_split_zero(a.xz[a.x_pt ? 0 : c], 0, zxi, dzx);
        span_split_zero(a.wz[a.w_pt ? 0 : c], 0, zwi, dzw);
        const int64_t xb = p * a.H * a.W, wb = (int64_t)c * a.KH * a.KW;
        int I = 0, A = 0, B = 0, n = 0;
        for (int kh = 0; kh < a.KH; ++kh) {
            const int ih = oh * a.stride - a.pad + kh;
            if (ih < 0 || ih >= a.H) continue;
            for (int kw = 0; kw < a.KW; ++kw) {
                const int iw = ow * a.stride - a.pad + kw;
                if (iw < 0 || iw >= a.W) continue;
                const int qa = unpack_elem(a.x, xb + (int64_t)ih * a.W + iw, a.x_bits, a.x_sign) - zxi;
                const int qb = unpack_elem(a.w, wb + kh * a.KW + kw, a.w_bits, a.w_sign) - zwi;
                I += qa * qb; A += qa; B += qb; ++n;
            }
        }
        float f = (float)I + span_cf(n, B, dzx, dzw);
        if (zwi != 0 || dzw != 0.0f) f = fmaf(-dzw, (float)A, f);
        const float alpha = a.xs[a.x_pt ? 0 : c] * a.ws[a.w_pt ? 0 : c];
        float y = fmaf(alpha, f, a.bias != nullptr ? a.bias[c] : 0.0f);
        if (a.relu) y = span_relu(y);
        if (a.out != nullptr) a.out[idx] = y;
        if (a.rq.out != nullptr) {
            const RqConst rc = span_rq_setup(a.rq, a.rq_pt ? 0 : c);
            a.rq.out[idx] = (uint8_t)(unsigned)rq_value(rc, y, bad);
        }
    }
    if (a.rq.out != nullptr) rq_report(a.rq, bad);
}

// ---- host: the plan ---------------------------------------------------------------------------------------------------
static unsigned dw_magic(int d) { return (unsigned)((1ull << 31) / (unsigned)d) + 1u; }

DwPlan plan_dw(const DwRequest &r)
{
    DwPlan p;
    const qe_conv_shape &s = *r.sh;
    if (s.IC != s.OC || s.KH > DW_MAX_K || s.KW > DW_MAX_K || 2 * s.padding > std::min(s.KH, s.KW)) return p;
    p.OH = (s.H + 2 * s.padding - s.KH) / s.stride + 1;
    p.OW = (s.W + 2 * s.padding - s.KW) / s.stride + 1;
    if (s.H + 2 * s.padding < s.KH || s.W + 2 * s.padding < s.KW) return p;
    const int64_t NP = (int64_t)s.N * s.IC;
    if ((int64_t)s.H * s.W > 0x7fffffffLL) return p;                   // in-plane offsets are 32-bit
    p.symmetric = (r.x_sign && r.w_sign) ? 1 : 0;
    p.two_pass = (r.rq_bits > 0 && r.rq_bits < 8) ? 1 : 0;
    p.store16 = (r.has_out && (r.out & 15) == 0) ? 1 : 0;
    p.codes4 = (r.rq_bits == 8 && (r.codes & 3) == 0) ? 1 : 0;
    const bool k_out = r.has_out, k_codes = r.rq_bits == 8;

    // the plain kernel: one thread per output
    p.kernel = DW_PLAIN;
    p.G = 1; p.TH = 1; p.vec = 1; p.bands = p.OH; p.ncg = p.OW; p.lds = 0;
    p.blocks = ceil_div64(NP * p.OH * p.OW, DW_THREADS);
    if (p.blocks > 0x7fffffffLL) { p.kernel = DW_NONE; return p; }

    const bool fast = s.KH == 3 && s.KW == 3 && s.padding == 1 && (s.stride == 1 || s.stride == 2) && r.x_bits == 8 &&
                      r.w_bits == 8 && (k_out || k_codes);
    if (!fast) return p;
    const int S = s.stride;
    const int HW = s.H * s.W, OHW = p.OH * p.OW;
    const int tab = (int)sizeof(DwPlaneTab);
    auto lds_of = [&](int G, int in_len, int out_len, DwPlan &q) {
        q.in_off = round16(G * tab) + 16;
        q.codes_off = q.in_off + round16(in_len + 15) + 16;
        q.out_off = q.codes_off + (k_codes ? round16(out_len + 15) : 0);
        return (int64_t)q.out_off + (k_out ? round16(4 * out_len + 12) : 0);
    };
    DwPlan f = p;
    f.vec = DW_VEC;
    f.ncg = ceil_div(p.OW, DW_VEC);
    // whole planes: as many as fit the LDS budget and the output cap
    int G = (int)std::min<int64_t>(std::min<int64_t>(DW_MAX_G, NP), DW_MAX_OUTPUTS / std::max(1, OHW));
    while (G >= 1 && lds_of(G, G * HW, G * OHW, f) > DW_LDS_BUDGET) --G;
    if (G >= 1 && (int64_t)G * HW + 64 <= DW_LDS_BUDGET) {
        f.G = G; f.TH = p.OH; f.bands = 1;
        f.lds = lds_of(G, G * HW, G * OHW, f);
        f.blocks = ceil_div64(NP, G);
    } else {
        int TH = std::min(p.OH, DW_MAX_OUTPUTS / std::max(1, p.OW));
        auto in_rows = [&](int th) { return std::min(s.H, (th - 1) * S + 3); };
        while (TH >= 1 && lds_of(1, in_rows(TH) * s.W, TH * p.OW, f) > DW_LDS_BUDGET) --TH;
        if (TH < 1) return p;                                           // a row too wide for the LDS: the plain kernel
        f.G = 1; f.bands = ceil_div(p.OH, TH);
        f.TH = ceil_div(p.OH, f.bands);                                 // bands of equal height (the last may be shorter)
        f.bands = ceil_div(p.OH, f.TH);
        f.lds = lds_of(1, in_rows(f.TH) * s.W, f.TH * p.OW, f);
        f.blocks = NP * f.bands;
    }
    if (f.blocks > 0x7fffffffLL) return p;
    f.m_ncg = dw_magic(f.ncg);
    f.m_oh = dw_magic(p.OH);
    f.kernel = DW_FAST_FIRST + 3 * (S - 1) + (k_out && k_codes ? 2 : k_codes ? 1 : 0);
    return f;
}

// the instances by number: the plain kernel, then the fast kernel as plan_dw numbers it (stride, then out | codes | both)
template <int S, bool HAS_OUT, bool HAS_CODES>
constexpr SpanLaunch<DwArgs> dw_fast = &launch_instance<&dw_fast_kernel<S, HAS_OUT, HAS_CODES>, DwArgs>;
static constexpr SpanLaunch<DwArgs> kDwInstances[] = {
    &launch_instance<&dw_plain_kernel, DwArgs>,
    dw_fast<1, true, false>, dw_fast<1, false, true>, dw_fast<1, true, true>,
    dw_fast<2, true, false>, dw_fast<2, false, true>, dw_fast<2, true, true>};
static_assert(sizeof(kDwInstances) / sizeof(kDwInstances[0]) == DW_KERNELS, "one launcher per instance number");

int launch_dw(const DwPlan &p, const qe_qparam *x, const qe_qparam *w, const float *bias, const qe_conv_shape *sh, int relu,
              float *out, const qe_requant *rq, uint8_t *codes, int32_t *status, hipStream_t s)
{
    if (p.kernel < 0 || p.kernel >= DW_KERNELS) return QE_ERR_UNSUPPORTED;
    DwArgs a;
    static_cast<SpanOperands &>(a) = span_operands(x, w, bias, sh->N, out, rq, codes, status);
    a.C = sh->IC; a.H = sh->H; a.W = sh->W; a.OH = p.OH; a.OW = p.OW; a.KH = sh->KH; a.KW = sh->KW;
    a.stride = sh->stride; a.pad = sh->padding; a.relu = relu ? 1 : 0;
    a.G = p.G; a.TH = p.TH; a.bands = p.bands; a.ncg = p.ncg; a.m_ncg = p.m_ncg; a.m_oh = p.m_oh;
    a.in_off = p.in_off; a.codes_off = p.codes_off; a.out_off = p.out_off;
    a.NP = (int64_t)sh->N * sh->IC;
    kDwInstances[p.kernel]((unsigned)p.blocks, DW_THREADS, (size_t)p.lds, 0, s, a);
    QE_LAUNCH_CHECK();
    return QE_OK;
}

}  // namespace qe
