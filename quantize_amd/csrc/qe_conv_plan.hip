// qe_conv_plan.hip -- host-only planner of the packed-activation convolutions (qe_conv_plan.hpp).
#include "qe_conv_plan.hpp"

#include <algorithm>
#include <cstdlib>

namespace qe {

// QE_* knob as an integer, `dflt` when it is not set
static int knob(const char *name, int dflt)
{
    const char *e = env_get(name);
    return e ? atoi(e) : dflt;
}

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// column tiles per wave each layout is instantiated for (descending), and waves along the pixels
static const int kNiw[3][3] = {{7, 4, 2}, {4, 2, 1}, {2, 1, 0}};
static const int kWN[3] = {1, 2, 4};

// ---- the MFMA family of a problem with 8-bit activations (make_plan expands narrower ones first) -----------------------
// plan_front holds what every family starts from; each family function copies it, fills a plan of its own and returns it
// with its family set -- or with MfmaFamily::None when the problem does not fit.  make_plan8 tries them in order.
struct PlanFront {
    MfmaPlan p;                // OH, OW, KK, cfg, MT, OCP
    int max_tiles = 0;         // column tiles of the widest tile of this wave layout
    bool ok = false;
};

static PlanFront plan_front(const qe_conv_shape *sh)
{
    PlanFront f;
    MfmaPlan &p = f.p;
    p.OH = (sh->H + 2 * sh->padding - sh->KH) / sh->stride + 1;
    p.OW = (sh->W + 2 * sh->padding - sh->KW) / sh->stride + 1;
    p.KK = sh->KH * sh->KW;
    if (p.OH <= 0 || p.OW <= 0 || sh->N <= 0 || sh->OC <= 0) return f;
    if ((int64_t)sh->IC * sh->H * sh->W >= (1ll << 31)) return f;
    // int32 accumulators: |a_x a_w| <= 2^14 per product, so a reduction of 2^17 or more terms could overflow silently where
    // the reference (fp32 accumulation, quantconv2d.cu:84) merely rounds -> those problems keep the order-preserving fp32 kernel
    if ((int64_t)sh->IC * sh->KH * sh->KW >= (1ll << 17)) return f;
    if ((int64_t)sh->N * sh->IC * sh->H * sh->W < 64) return f;  // clamped 8-byte reads need a stream >= 8 bytes
    if (sh->W < 4) return f;                                       // rows are fetched in 4-pixel quads
    if ((int64_t)sh->OC * p.OH * p.OW >= (1ll << 29)) return f;      // 32-bit store offsets inside one image
    p.cfg = sh->OC > 64 ? 0 : (sh->OC > 32 ? 1 : 2);
    p.MT = p.cfg == 0 ? 128 : (p.cfg == 1 ? 64 : 32);
    // 4x1 waves: 7 column tiles per wave (112 accumulator registers) keeps the 3x3 variant, which
    // also holds 9 weight fragments, inside 256 VGPRs; 224 pixels = 4 rows of 56 / 8 of 28 / 14x14+.
    f.max_tiles = kNiw[p.cfg][0] * kWN[p.cfg];
    if (p.KK > 64 || p.OW > 32 * f.max_tiles) return f;
    p.OCP = (sh->OC + p.MT - 1) / p.MT * p.MT;
    f.ok = true;
    return f;
}

// 1x1 / stride 1 / no padding: GEMM over the flat pixel index (conv_mfma_flat_kernel).  x4: the instances that read 4-bit
// activations from the packed stream (128-channel workgroups only)
static MfmaPlan plan_flat(const PlanFront &f, const qe_conv_shape *sh, int w_bits, bool x4)
{
    MfmaPlan p = f.p;
    const int P = sh->H * sh->W;
    if (!(p.KK == 1 && sh->stride == 1 && sh->padding == 0 && (P % 4) == 0 && P >= 64 && sh->IC >= 16)) return p;
    if (x4 && p.cfg != 0) return p;
    int tiles = f.max_tiles;
    if (p.cfg == 0) {
        // shallow layers (a single stage) are latency- not MFMA-bound: 128-pixel tiles keep the
        // accumulators small enough for a third workgroup per CU.  Then tile quantisation: a plane of
        // 784 pixels (28x28) wastes 12.5 % of 224- or 128-pixel tiles but only 2 % of 160-pixel ones,
        // so the width with clearly less padding wins.  QE_FLAT_NIW overrides (tuning).
        const int forced = knob("QE_FLAT_NIW", 0);
        if (forced == 4 || forced == 5 || forced == 7) tiles = forced;
        else {
            auto waste = [&](int t) { return (double)((P + 32 * t - 1) / (32 * t)) * (32 * t) / (double)P; };
            tiles = sh->IC <= 128 ? 4 : 7;
            static const int cands[3] = {7, 5, 4};
            for (int c : cands)
                if (waste(c) < waste(tiles) - 0.03) tiles = c;
            // measured exceptions (profiles/r02y_ab_flat_niw.txt, cold per-layer A/B on ResNet-50 at batch 256):
            //   128 -> 512 @28x28: 128-pixel tiles (a fourth workgroup per CU) beat the better-fitting 160-pixel ones by 5 %;
            //   512 -> 128 @28x28: 224-pixel tiles beat 160-pixel ones by 4.5 % (1024 workgroups = two full rounds).
            if (P == 784 && sh->IC <= 128 && sh->OC >= 256) tiles = 4;
            if (P == 784 && sh->IC >= 512 && sh->OC <= 128) tiles = 7;
        }
    }
    const int ntp = 32 * tiles;
    const int rstr = 32 * (tiles | 1);
    const int nch = (sh->IC + 31) / 32;
    p.NS = 1;
    // QE_FLAT_NS: tuning knob.  64 -> 256 @56x56 (write-bound, two chunks in all): one chunk per stage is 3 % faster
    // (r02y_ab_flat_ns.txt)
    const char *ns_env = env_get("QE_FLAT_NS");
    int ns_max = ns_env ? std::max(1, atoi(ns_env)) : 4;
    if (!ns_env && nch == 2 && sh->OC >= 4 * sh->IC && P >= 3136) ns_max = 1;
    for (int cand = 4; cand > 1; cand >>= 1)
        if (cand <= ns_max && cand <= nch && (size_t)(32 * cand) * rstr + (size_t)ntp * 4 <= (size_t)MF_MAX_LDS) { p.NS = cand; break; }
    p.lds = std::max((size_t)(32 * p.NS) * rstr, (size_t)4 * 32 * 36 * 4) + (size_t)ntp * 4;
    p.TH = 1; p.ni = tiles; p.niw = tiles / kWN[p.cfg];
    p.NCH = nch; p.NG = 2 * nch;
    p.wraw = (w_bits == 8) && (sh->IC % 16) == 0 && !x4;   // the 4-bit-activation instances take prepared fragments only
    p.wt_bytes = p.wraw ? 0 : (size_t)p.NG * p.OCP * 16;
    p.IHT = (P + ntp - 1) / ntp;   // pixel tiles per image
    p.family = x4 ? MfmaFamily::FlatX4 : MfmaFamily::Flat;
    return p;
}

// 1x1 / stride 2 / no padding (the downsample branches): same GEMM over the flat OUTPUT pixels, the
// staging keeps the even columns of the even input rows.  224-pixel tiles must hold whole output rows.
static MfmaPlan plan_flat_s2(const PlanFront &f, const qe_conv_shape *sh, int w_bits)
{
    MfmaPlan p = f.p;
    const int POUT = p.OH * p.OW;
    if (!(p.KK == 1 && sh->stride == 2 && sh->padding == 0 && p.cfg == 0 && sh->IC >= 64 &&
          (POUT % 4) == 0 && POUT >= 64 && 224 % p.OW == 0 && sh->W >= 16 && (sh->W % 4) == 0 && knob("QE_FLAT_S2", 1) != 0)) return p;
    const int rt = 224 / p.OW, seg = (sh->W + 15) / 16;
    if (64 * rt * seg > 8 * MF_THREADS) return p;
    const int ntp = 224, rstr = 224;
    p.NS = 2;
    p.lds = std::max((size_t)64 * rstr, (size_t)4 * 32 * 36 * 4) + (size_t)ntp * 4;
    p.TH = 1; p.ni = 7; p.niw = 7;
    p.NCH = (sh->IC + 31) / 32; p.NG = 2 * p.NCH;
    p.wraw = (w_bits == 8) && (sh->IC % 16) == 0;
    p.wt_bytes = p.wraw ? 0 : (size_t)p.NG * p.OCP * 16;
    p.IHT = (POUT + ntp - 1) / ntp;   // pixel tiles per image
    p.family = MfmaFamily::FlatS2;
    return p;
}

// 1x1 / stride 1 / no padding on 49..56-pixel planes (7x7 maps): the flat kernel's small-plane variant
// (conv_mfma_flatg_kernel).  QE_FLATG=0 leaves these layers on the halo kernel.
static MfmaPlan plan_flatg(const PlanFront &f, const qe_conv_shape *sh, int w_bits)
{
    MfmaPlan p = f.p;
    const int P = sh->H * sh->W;
    if (!(p.KK == 1 && sh->stride == 1 && sh->padding == 0 && p.cfg == 0 && sh->IC >= 64 &&
          (P + 7) / 8 == 7 && (int64_t)sh->N * sh->IC * P < (1ll << 32) && knob("QE_FLATG", 1) != 0)) return p;
    const int nch = (sh->IC + 31) / 32;
    p.IWP = 56;                                   // slots per image (P rounded up to 8)
    p.GI = std::max(1, std::min((int)sh->N, 224 / p.IWP));
    p.NS = nch >= 4 ? 4 : 2;
    p.lds = std::max((size_t)(32 * p.NS) * 224, (size_t)4 * 32 * 36 * 4) + (size_t)224 * 4;
    p.TH = 1; p.ni = 7; p.niw = 7;
    p.NCH = nch; p.NG = 2 * nch;
    p.wraw = (w_bits == 8) && (sh->IC % 16) == 0;
    p.wt_bytes = p.wraw ? 0 : (size_t)p.NG * p.OCP * 16;
    p.IHT = 1;
    p.family = MfmaFamily::Flatg;
    return p;
}

// IC <= 4 (the stem): K = (kh) x [kw 0..7][ic 0..3]; the whole (tiny) channel depth is one stage
static bool stem_shape(const qe_conv_shape *sh) { return sh->IC <= 4 && sh->KW <= 8 && sh->KH <= 8; }

static MfmaPlan plan_stem(const PlanFront &f, const qe_conv_shape *sh)
{
    MfmaPlan p = f.p;
    p.NCH = 1;
    p.NG = 2;
    p.niw = kNiw[p.cfg][0];
    int stem_tiles = f.max_tiles;
    // 64-channel workgroups (the ResNet stem): 7 column tiles per wave = 4 output rows per tile instead of 2
    // (fewer, larger workgroups: less halo re-read, prologue amortised)
    if (p.cfg == 1) {
        p.niw = 7;
        stem_tiles = 14;
    }
    int TH = std::min(p.OH, (32 * stem_tiles) / p.OW);
    for (; TH >= 1; --TH) {
        const int IHT = (TH - 1) * sh->stride + sh->KH;
        const int IWP = (p.OW - 1) * sh->stride + 8;
        const size_t lds = ((size_t)IHT * IWP * 2 + MF_TRASH) * 4;
        if (lds <= (size_t)MF_MAX_LDS) { p.TH = TH; p.IHT = IHT; p.IWP = IWP; p.lds = lds; break; }
    }
    if (p.TH == 0) return p;
    p.ni = (p.TH * p.OW + 31) / 32;
    p.wt_bytes = (size_t)sh->KH * 2 * p.OCP * 16;
    p.family = MfmaFamily::Stem;
    return p;
}

// 3x3, 8-bit activations, more than 32 output channels: two strips per wave, weights through LDS
// (conv_mfma_sm2_kernel).  Measured against the halo / warp-specialised kernels on ResNet-50 (tools/ab_env.sh
// QE_SM2 0 1): 56x56 64->64 0.083 -> 0.068 ms, 14x14 256->256 0.050 -> 0.048, 28x28 +4 %, 7x7 maps and the
// stride-2 layers +15 % (the warp-specialised kernel / bigger halo tiles win there).  Default: stride 1 and a
// tile that is either 64 channels wide or a whole image; QE_SM2=1 forces it wherever it fits, QE_SM2=0 never.
static MfmaPlan plan_sm2(const PlanFront &f, const qe_conv_shape *sh)
{
    MfmaPlan p = f.p;
    const int sm2_env = knob("QE_SM2", -1);
    if (!(p.KK == 9 && sh->KW == 3 && sh->KH == 3 && p.cfg <= 1 && sm2_env != 0)) return p;
    const int NQ = (sh->W + 3) / 4;
    const int max_px = 32 * (p.cfg == 0 ? 8 : 16);
    int GI = 1;
    if (p.OH * p.OW <= max_px / 2) GI = std::max(1, std::min((int)sh->N, max_px / (p.OH * p.OW)));
    int TH = (GI > 1) ? p.OH : std::min(p.OH, max_px / p.OW);
    if (GI == 1 && TH >= 1) { const int nt = (p.OH + TH - 1) / TH; TH = (p.OH + nt - 1) / nt; }   // balanced row tiles
    bool fits = false;
    while (TH >= 1) {
        const int IHT = (TH - 1) * sh->stride + 3, IWP = (p.OW - 1) * sh->stride + 3;
        const int units = GI * IHT * NQ;
        const size_t gsz = (size_t)GI * IHT * IWP;
        const size_t wpieces = ((size_t)9 * 2 * p.MT + MF_THREADS - 1) / MF_THREADS * MF_THREADS;   // whole piece rounds
        const size_t lds = align_up((2 * gsz + MF_TRASH) * 16 + gsz * 4, 16) + wpieces * 16;
        if (units <= MF_THREADS && lds <= (size_t)MF_MAX_LDS_SM2) {
            fits = true; p.GI = GI; p.TH = TH; p.IHT = IHT; p.IWP = IWP; p.lds = lds; p.NS = 1;
            break;
        }
        if (GI > 1) { --GI; continue; }
        --TH;
    }
    if (!fits) return p;
    p.NCH = (sh->IC + 31) / 32;
    p.NG = 2 * p.NCH;
    p.ni = (p.GI * p.TH * p.OW + 31) / 32;
    p.niw = 4;
    p.wt_bytes = (size_t)p.KK * p.NG * p.OCP * 16;
    if ((int64_t)p.wt_bytes >= (1ll << 31)) return p;
    if (sm2_env < 0 && !(sh->stride == 1 && p.GI == 1 && (p.cfg == 1 || p.TH == p.OH))) return p;
    p.family = MfmaFamily::Sm2;
    return p;
}

// every other kernel size: the halo tile in LDS (conv_mfma_kernel), or its warp-specialised 3x3 form (conv_mfma_ws_kernel)
static MfmaPlan plan_halo(const PlanFront &f, const qe_conv_shape *sh)
{
    MfmaPlan p = f.p;
    const int NQ = (sh->W + 3) / 4;
    p.NCH = (sh->IC + 31) / 32;
    p.ROWMUL = (sh->KH == 1) ? sh->stride : 1;   // 1xK strided: only every stride-th row is ever read
    p.COLMUL = (sh->KW == 1) ? sh->stride : 1;
    const int max_px = 32 * f.max_tiles;
    // small feature maps (7x7): several whole images per tile, so a weight fragment and a
    // barrier pair are amortised over 7 column tiles instead of 2
    if (p.OH * p.OW <= max_px / 2) p.GI = std::max(1, std::min((int)sh->N, max_px / (p.OH * p.OW)));
    int TH = (p.GI > 1) ? p.OH : std::min(p.OH, max_px / p.OW);
    const bool multi = p.KK == 1;   // 1x1: several chunks per stage
    for (;;) {
        const int IHT = (p.ROWMUL > 1) ? TH : (TH - 1) * sh->stride + sh->KH;
        const int IWP = (p.COLMUL > 1) ? p.OW : (p.OW - 1) * sh->stride + sh->KW;
        const int units = p.GI * IHT * NQ;
        // chunks per stage: as many as the idle staging threads and LDS allow
        int ns = 1;
        if (multi) {
            for (int cand = 4; cand > 1; cand >>= 1) {
                const size_t l = ((size_t)2 * cand * p.GI * IHT * IWP + MF_TRASH) * 16 + (size_t)p.GI * IHT * IWP * 4;
                if (cand <= p.NCH && units * cand <= MF_THREADS && l <= (size_t)MF_MAX_LDS) { ns = cand; break; }
            }
        }
        const size_t lds = ((size_t)2 * ns * p.GI * IHT * IWP + MF_TRASH) * 16 + (size_t)p.GI * IHT * IWP * 4;
        if (lds <= (size_t)MF_MAX_LDS && units <= MF_THREADS) {
            p.TH = TH; p.IHT = IHT; p.IWP = IWP; p.lds = lds; p.NS = ns;
            break;
        }
        if (p.GI > 1) { --p.GI; continue; }
        if (--TH < 1) break;
    }
    if (p.TH == 0) return p;
    // The kernel runs NCH padded to a multiple of NS (the padded chunks carry zero weights).  NS follows the tile,
    // which follows N, so the weight table holds the channel groups of the largest NS this depth allows: its layout
    // (a prepared buffer shared across batch sizes) stays the same for every N.  NG is only the table's stride.
    const int ns_cap = !multi ? 1 : (p.NCH >= 4 ? 4 : (p.NCH >= 2 ? 2 : 1));
    p.NG = 2 * ((p.NCH + ns_cap - 1) / ns_cap * ns_cap);
    p.NCH = (p.NCH + p.NS - 1) / p.NS * p.NS;
    p.ni = (p.GI * p.TH * p.OW + 31) / 32;
    p.niw = kNiw[p.cfg][0];
    for (int i = 0; i < 3; ++i)
        if (kNiw[p.cfg][i] > 0 && kNiw[p.cfg][i] * kWN[p.cfg] >= p.ni) p.niw = kNiw[p.cfg][i];
    p.wt_bytes = (size_t)p.KK * p.NG * p.OCP * 16;
    p.family = MfmaFamily::Halo;
    // 3x3, 8-bit activations, 128-channel tiles: the warp-specialised kernel (producer/consumer
    // waves, double-buffered halo image).
    // Measured on ResNet-50 (A/B, tools/ab_env.sh QE_WS): it wins where a workgroup has little MFMA work
    // per stage to hide its own fetch behind (7x7 maps: 0.068 -> 0.052-0.057 ms) and loses 5-15 % on the
    // 14x14 / 28x28 / 56x56 layers, where two resident single-role workgroups overlap each other better
    // than one specialised one (stamps: the consumer issues one MFMA per ~60 cycles; its weight loads queue
    // behind the producers' HBM misses in the CU's in-order vector-memory path).  QE_WS=1 forces it on.
    const bool ws_default = p.GI > 1 || p.OH * p.OW <= 64;
    if (p.KK == 9 && sh->KW == 3 && p.cfg == 0 && p.NS == 1 && knob("QE_WS", ws_default) != 0) {
        const size_t gsz = (size_t)p.GI * p.IHT * p.IWP;
        const size_t lds = ((size_t)4 * gsz + MF_TRASH) * 16 + gsz * 4;
        if (lds <= (size_t)MF_MAX_LDS) { p.family = MfmaFamily::Ws; p.lds = lds; }
    }
    return p;
}

// table layout of a family's plan: [weights | per-channel constants | tap-sum prefix table]; the flat kernels with raw
// 8-bit weights build their constants themselves and need none
static MfmaPlan plan_tables(MfmaPlan p, const qe_conv_shape *sh)
{
    if (p.wraw) { p.total = 0; return p; }
    p.ep_off = align_up(p.wt_bytes, 256);
    p.ws_off = align_up(p.ep_off + (size_t)3 * p.OCP * sizeof(float), 256);
    p.total = align_up(p.ws_off + (size_t)p.OCP * (sh->KH + 1) * (sh->KW + 1) * sizeof(int), 256);
    return p;
}

// the families in their order of precedence, then the table layout [weights | per-channel constants | tap-sum prefix table]
static MfmaPlan make_plan8(const qe_conv_shape *sh, int w_bits)
{
    const PlanFront f = plan_front(sh);
    if (!f.ok) return f.p;
    MfmaPlan p = plan_flat(f, sh, w_bits, false);
    if (p.family == MfmaFamily::None) p = plan_flat_s2(f, sh, w_bits);
    if (p.family == MfmaFamily::None) p = plan_flatg(f, sh, w_bits);
    if (p.family == MfmaFamily::None) {
        if (stem_shape(sh)) p = plan_stem(f, sh);
        else {
            p = plan_sm2(f, sh);
            if (p.family == MfmaFamily::None) p = plan_halo(f, sh);
        }
    }
    if (p.family == MfmaFamily::None) return f.p;
    return plan_tables(p, sh);
}

// the dense problem a strided 1x1 / pad 0 convolution reduces to: out[n,oc,oh,ow] only ever reads x[n,c,oh*s,ow*s]
static qe_conv_shape dense_shape(const qe_conv_shape *sh)
{
    qe_conv_shape d = *sh;
    d.H = (sh->H - 1) / sh->stride + 1;
    d.W = (sh->W - 1) / sh->stride + 1;
    d.stride = 1;
    return d;
}

// Sub-8-bit activations: the stream is expanded once to signed 8-bit stored codes in the workspace (one pass at HBM rate:
// b/8 + 1 bytes per element) and every fast 8-bit kernel applies.  Decoding them inside the halo kernel was 3-4x slower
// (ResNet-50 W4A4: 16.0 ms vs 4.7 ms per batch-256).
static MfmaPlan make_plan(const qe_conv_shape *sh, int x_bits, int w_bits)
{
    const bool expand = x_bits < 8;
    // Strided 1x1 (the ResNet downsample branches): gather the sampled pixels once (read every other row, write 1/s^2 of
    // the bytes) and run the stride-1 kernels on the dense tensor, instead of staging 2-4x the needed bytes in every
    // one of the OC/128 workgroups that share a pixel tile.  QE_SUBSAMPLE=0 keeps the in-kernel strided staging.
    // Measured (rocprofv3, in the stack): 512->1024 @28->14 187 -> 137 us, 1024->2048 @14->7 143 -> 109 us; on
    // 256->512 @56->28 the gather (93 us) costs more than it saves, so output planes above 256 pixels keep the flat
    // kernel's in-kernel stride-2 staging.  QE_SUBSAMPLE=1 forces the gather, =0 disables it.
    const int sub_env = knob("QE_SUBSAMPLE", -1);
    const int p_out = ((sh->H - 1) / std::max(1, (int)sh->stride) + 1) * ((sh->W - 1) / std::max(1, (int)sh->stride) + 1);
    // 4-bit activations, stride 2: ONE pass reads the even nibbles of the even rows and writes dense 8-bit codes
    // (subsample_x4_kernel) instead of expanding the whole tensor first -- there the gather pays on every plane size
    const bool sub_x4 = x_bits == 4 && sh->stride == 2 && (sh->W % 2) == 0 && ((int64_t)sh->H * sh->W % 2) == 0 &&
                        knob("QE_SUB_X4", 1) != 0;
    const bool sub = sh->KH == 1 && sh->KW == 1 && sh->stride > 1 && sh->padding == 0 && sub_env != 0 &&
                     (sub_env > 0 || p_out <= 256 || sub_x4);
    const qe_conv_shape ds = dense_shape(sh);
    // 4-bit activations on a stride-1 1x1 layer with 128-channel workgroups: the flat kernel unpacks the nibbles in its
    // staging registers (QE_X4=0: expansion pass + 8-bit kernel as for every other sub-8-bit case)
    if (x_bits == 4 && !sub && knob("QE_X4", 1) != 0) {
        const PlanFront f = plan_front(sh);
        MfmaPlan q = f.ok ? plan_flat(f, sh, w_bits, true) : f.p;
        if (q.family == MfmaFamily::FlatX4) {
            q = plan_tables(q, sh);
            q.prep_total = q.total;
            return q;
        }
    }
    MfmaPlan p = make_plan8(sub ? &ds : sh, w_bits);
    p.prep_total = p.total;
    if (p.family != MfmaFamily::None && sub) {
        p.sub = true;
        p.sub_x4 = sub_x4;
        p.sub_off = align_up(p.total, 256);
        p.total = p.sub_off + align_up((size_t)ds.N * ds.IC * ds.H * ds.W, 256);
    } else if (sub) {
        p = make_plan8(sh, w_bits);
        p.prep_total = p.total;
    }
    if (p.family != MfmaFamily::None && expand) {
        p.expand = true;
        p.xe_off = align_up(p.total, 256);
        p.total = p.xe_off + align_up((size_t)sh->N * sh->IC * sh->H * sh->W, 256);
    }
    return p;
}

// The prepared tables are planned at the smallest batch the kernels accept: nothing in their layout depends on N beyond
// that (make_plan8 keeps NG independent of the tile), so one prepared buffer serves every batch size.
MfmaPlan plan_prepared(const qe_conv_shape *sh, int x_bits, int w_bits)
{
    qe_conv_shape s1 = *sh;
    const int64_t img = (int64_t)sh->IC * sh->H * sh->W;
    s1.N = img >= 64 ? 1 : (int)((64 + img - 1) / img);
    return make_plan(&s1, x_bits, w_bits);
}

// What the prepared tables look like: two problems with the same weights and the same signature share one prepared buffer
// whatever their batch size or image size (0: nothing to prepare).  The prep kernels write Wt[tap][NG][OCP][16] (or the
// stem's per-row layout), 3 x OCP constants and the OCP x (KH+1)(KW+1) prefix table.
uint64_t prepared_layout(const MfmaPlan &p, const qe_conv_shape *sh)
{
    if (p.family == MfmaFamily::None || p.prep_total == 0) return 0;
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](uint64_t v) { h = (h ^ v) * 1099511628211ull; };
    mix(p.family == MfmaFamily::Stem ? 1 : 0); mix((uint64_t)p.OCP); mix((uint64_t)p.NG); mix((uint64_t)p.KK); mix((uint64_t)sh->KH); mix((uint64_t)sh->KW);
    mix((uint64_t)sh->IC); mix((uint64_t)sh->OC); mix((uint64_t)p.prep_total); mix((uint64_t)p.ep_off); mix((uint64_t)p.ws_off);
    return h | 1ull;
}

// ---- resident-tile kernels (qe_conv_pwr.hip).  xa: the activation address the kernel reads (alignment only) ----
struct PwrFit {
    int tw = 0, ks = 0, groups = 1;
    bool s2 = false;
};

// QE_PWR=0 disables the kernel, QE_PWR_GROUPS overrides the channel split (tuning).
static bool pwr_plan(const qe_conv_shape *sh, const qe_qparam *x, const qe_qparam *w, uintptr_t xa, PwrFit *pl)
{
    // QE_PWR=0: never; QE_PWR=1: only layers whose planes are ONE tile (14x14: the tile is fetched once instead of OC/128
    // times and every strip leaves as one contiguous run: -20..25 % against the flat kernels, profiles/r03a_ab_pwr.txt) and
    // the stride-2 layers (the strided rows fetched once per tile instead of once per 128 output channels); default (2):
    // every eligible layer -- on stride-1 28x28 / 56x56 planes both kernels sit near the same store rate layer by layer
    // (+-3 %, inside the noise of isolated timings), over the whole step this form is 1.2 % ahead (three alternating pairs of
    // 200-step runs on one box, profiles/r03t_ab_pwr_stack.txt)
    const int mode = knob("QE_PWR", 2);
    if (mode == 0) return false;
    if (sh->KH != 1 || sh->KW != 1 || sh->padding != 0 || (sh->stride != 1 && sh->stride != 2)) return false;
    if (x->n_bits != 8 || w->n_bits != 8 || x->n_param != 1) return false;
    if (sh->IC != 64 && sh->IC != 128 && sh->IC != 256) return false;
    if (sh->OC % 32 != 0 || sh->OC < 128 || sh->N < 1) return false;
    const bool s2 = sh->stride == 2;
    if (s2 && ((sh->H & 1) || (sh->W & 7) || sh->W > 64 || knob("QE_PWR_S2", 1) == 0)) return false;
    const int OH = s2 ? sh->H / 2 : sh->H, OW = s2 ? sh->W / 2 : sh->W;
    const int64_t P = (int64_t)OH * OW;                       // output plane
    // tiles of 224 or 196 pixels that divide the plane (56x56: 14 x 224; 28x28: 4 x 196; 14x14: the plane itself)
    const int tw = (P % 224 == 0) ? 224 : ((P % 196 == 0) ? 196 : 0);
    if (tw == 0) return false;
    if (s2 && (tw % OW != 0 || tw / OW > 8)) return false;    // whole output rows per tile
    if (mode == 1 && !s2 && P != tw) return false;
    if ((int64_t)sh->N * sh->IC * sh->H * sh->W < 16 || (int64_t)sh->OC * P >= (1ll << 29) || (int64_t)sh->IC * sh->H * sh->W >= (1ll << 31)) return false;
    if ((reinterpret_cast<uintptr_t>(w->data) & 15) != 0 || (xa & (s2 ? 7 : 3)) != 0) return false;
    if ((reinterpret_cast<uintptr_t>(w->scale) & 3) != 0) return false;
    const int ks = sh->IC / 32;
    const int waves = ks == 8 ? 8 : 4;                        // IC = 256: 56 KB of tile -> one 8-wave workgroup per CU
    if (sh->OC < 64 * waves) return false;                    // fewer than two strips per wave: the flat kernels' tiling fits better (256 -> 128 @56x56: +19 %)
    const int strips = sh->OC / 32;
    const int g = knob("QE_PWR_GROUPS", 0);
    pl->tw = tw; pl->ks = ks; pl->groups = (g >= 1 && strips % g == 0) ? g : 1; pl->s2 = s2;
    return true;
}

// 7x7 planes: 0 = not eligible, else images per tile
static int pwr7_plan(const qe_conv_shape *sh, const qe_qparam *x, const qe_qparam *w, uintptr_t xa, int *groups)
{
    if (knob("QE_PWR", 2) == 0 || knob("QE_PWR7", 1) == 0) return 0;
    if (sh->KH != 1 || sh->KW != 1 || sh->stride != 1 || sh->padding != 0 || sh->H * sh->W != 49) return 0;
    if (x->n_bits != 8 || w->n_bits != 8 || x->n_param != 1) return 0;
    if (sh->IC != 128 && sh->IC != 256 && sh->IC != 512) return 0;
    const int gi = sh->IC == 512 ? 2 : 4;                     // 64 KB of tile
    if (sh->OC % 32 != 0 || sh->OC < 512 || sh->N < gi || sh->N % gi != 0) return 0;   // >= 2 strips per wave; whole tiles only
    if ((int64_t)sh->N * sh->IC * 49 >= (1ll << 31) || (int64_t)sh->OC * 49 >= (1ll << 29)) return 0;
    if ((reinterpret_cast<uintptr_t>(w->data) & 15) != 0 || (xa & 15) != 0) return 0;
    const int tiles = sh->N / gi, strips = sh->OC / 32;
    int g = 1;
    while (tiles * g < kNumCU && strips % (2 * g) == 0 && strips / (2 * g) >= 8) g *= 2;   // about one workgroup per CU, >= 1 strip per wave
    const int ge = knob("QE_PWR_GROUPS", 0);
    *groups = (ge >= 1 && strips % ge == 0) ? ge : g;
    return gi;
}

// ---- LDS-DMA ring kernel (qe_conv_flatd.hip): 1x1 layers on 7x7 planes ----
static bool flatd_plan(const qe_conv_shape *sh, const qe_qparam *x, const qe_qparam *w, uintptr_t xa)
{
    if (sh->KH != 1 || sh->KW != 1 || sh->stride != 1 || sh->padding != 0) return false;
    if (x->n_bits != 8 || w->n_bits != 8 || x->n_param != 1) return false;
    if (sh->IC % FD_CK != 0 || sh->IC < 2 * FD_CK || sh->OC < 1 || sh->N < 1) return false;
    const int64_t P = (int64_t)sh->H * sh->W;
    if ((int64_t)sh->N * sh->IC * P < 16 || (int64_t)sh->OC * P >= (1ll << 29) || (int64_t)sh->IC * P >= (1ll << 31)) return false;
    if ((reinterpret_cast<uintptr_t>(w->data) & 15) != 0) return false;      // weight rows are fetched as aligned 16-byte pieces
    return P == 49 && sh->OC % 4 == 0 && (xa & 15) == 0;
}

// the LDS byte patch of a re-quantising lane = pixel kernel: one image per tile, dword-aligned rows and codes, and the
// family's unit has a PATCH instance for this plan (mfma_instance: the function the launch calls)
static bool plan_rq_patch(const MfmaPlan &m, const ConvRequest &r, int split)
{
    if (m.GI != 1 || (m.OH * m.OW) % 4 != 0 || (m.TH * m.OW) % 4 != 0) return false;
    if ((r.rq_out & 3) != 0 || knob("QE_RQ_PATCH", 1) == 0) return false;
    return mfma_instance(m, r.sh->KW, split, true, true) != nullptr;
}

// the MFMA-family launch: tiles, grid, epilogue tables and dynamic LDS
static void plan_mfma_launch(ConvPlan &p, const ConvRequest &r, bool rq)
{
    const MfmaPlan &m = p.m;
    const qe_conv_shape *sh = &p.run;
    p.tiles_h = (m.OH + m.TH - 1) / m.TH;
    p.n_pix_tiles = ((sh->N + m.GI - 1) / m.GI) * p.tiles_h;
    p.n_oc_tiles = m.OCP / m.MT;
    const bool flatg = m.family == MfmaFamily::Flatg;
    const bool flat = mfma_is_flat(m.family);
    if (flatg) {
        p.tiles_h = 1;                           // one tile = GI whole images
        p.n_pix_tiles = (sh->N + m.GI - 1) / m.GI;
    } else if (flat) {
        p.tiles_h = m.IHT;                       // pixel tiles per image; one per workgroup: runs of several tiles with
        p.n_pix_tiles = sh->N * p.tiles_h;       // cross-tile prefetch were measured and never paid ('what did not work')
    }
    p.blocks = tile_grid(p.n_pix_tiles, p.tiles_h, p.n_oc_tiles, true, p.chunk);
    // border classes: rows r < n_top have their top taps clipped, the last n_bot rows their bottom taps (columns alike)
    auto clipped_lo = [](int pad, int stride, int O) { return std::min(O, (pad + stride - 1) / stride); };
    auto clipped_hi = [](int I, int pad, int K, int stride, int O) {
        const int full_last = (I + pad - K) >= 0 ? (I + pad - K) / stride : -1;   // last output index with all taps below the edge
        return std::max(0, std::min(O, O - 1 - full_last));
    };
    p.n_top = clipped_lo(sh->padding, sh->stride, m.OH);
    p.n_bot = clipped_hi(sh->H, sh->padding, sh->KH, sh->stride, m.OH);
    p.n_lft = clipped_lo(sh->padding, sh->stride, m.OW);
    p.n_rgt = clipped_hi(sh->W, sh->padding, sh->KW, sh->stride, m.OW);

    if (flat || flatg) {
        // fused re-quantisation: room for the workgroup's byte patch behind the staging image (plan_conv checked the fit)
        p.lds = m.lds;
        if (rq) {
            p.ptab_off = (int)align_up(m.lds, 16);
            p.lds = p.ptab_off + (flatg ? (size_t)m.GI * m.MT * sh->H * sh->W : (size_t)m.MT * 32 * m.ni);
        }
        return;
    }
    // lane = pixel kernels (halo, sm2, stem) with fused re-quantisation, one image per tile: the codes leave through a
    // workgroup byte patch at the START of the dynamic LDS (<= 32 KB: MT x pixel slots; the staging image is dead by then)
    // instead of as byte stores of 32-byte runs; the epilogue's tables sit behind it.  QE_RQ_PATCH=0: byte stores.
    const int units = m.GI * m.IHT * ((sh->W + 3) / 4);
    p.split = units <= 64 ? 4 : (units <= 128 ? 2 : 1);   // channel slices of the staging threads
    p.rq_patch = rq && plan_rq_patch(m, r, p.split);
    const size_t stage_bytes = p.rq_patch ? std::max(m.lds, (size_t)32 * 1024) : m.lds;
    // LDS room for the epilogue's copy of the tile's S_w prefix rows (asymmetric activations; stage_ptab)
    size_t lds_e = stage_bytes;
    const size_t tab = (size_t)m.MT * (sh->KH + 1) * (sh->KW + 1) * sizeof(int);
    const size_t off = align_up(stage_bytes, 16);
    if (off + tab <= (size_t)(m.family == MfmaFamily::Sm2 ? MF_MAX_LDS_SM2 : MF_MAX_LDS)) { p.ptab_off = (int)off; lds_e = off + tab; }
    // The border-class table needs the bands disjoint and (classes) <= (prefix entries per channel) to fit the same LDS slot.
    const int ncls = (1 + p.n_top + p.n_bot) * (1 + p.n_lft + p.n_rgt);
    p.ctab = p.ptab_off != 0 && p.n_top + p.n_bot < m.OH && p.n_lft + p.n_rgt < m.OW && ncls <= (sh->KH + 1) * (sh->KW + 1) &&
             knob("QE_CTAB", 1) != 0;
    // (without the class table the ws epilogue reads the prefix rows from global memory: no LDS slot needed)
    p.lds = (m.family == MfmaFamily::Ws && !p.ctab) ? m.lds : lds_e;
}

ConvPlan plan_conv(const ConvRequest &r)
{
    ConvPlan p;
    const qe_conv_shape *sh = r.sh;
    p.OH = (sh->H + 2 * sh->padding - sh->KH) / sh->stride + 1;
    p.OW = (sh->W + 2 * sh->padding - sh->KW) / sh->stride + 1;
    if (p.OH > 0 && p.OW > 0) p.y_bytes = align_up((size_t)sh->N * sh->OC * p.OH * p.OW * sizeof(float), 256);
    p.m = make_plan(sh, r.x->n_bits, r.w->n_bits);
    const MfmaPlan &m = p.m;
    if (r.x->n_param != 1 || m.family == MfmaFamily::None) return p;   // per-channel activation scales cannot leave the K sum: generic kernel
    p.run = m.sub ? dense_shape(sh) : *sh;
    const qe_conv_shape *rs = &p.run;

    // pre-passes: 4-bit gather, or expansion to 8-bit codes and / or the strided gather (in that order)
    qe_qparam xr = *r.x;                         // the activations the conv kernel reads: 8-bit codes in the workspace
    uintptr_t xa = reinterpret_cast<uintptr_t>(r.x->data);
    if (m.sub_x4 || m.expand) { xr.n_bits = 8; xr.sign = 1; }
    if (m.sub || m.expand) xa = 0;               // workspace offsets are 256-byte aligned
    if (m.sub_x4) {
        p.pre = PrePass::SubX4;
        p.pre_blocks = ((int64_t)sh->N * sh->IC * rs->H * ((rs->W + 7) / 8) + 255) / 256;
    } else if (m.sub) {
        // stride 2, even H, a power-of-two number of 16-byte pieces per row that stays inside two input rows: subsample2_kernel
        const int64_t n_planes = (int64_t)sh->N * sh->IC;
        const int nq = (rs->W + 7) / 8;
        int log_nq = 0;
        while ((1 << log_nq) < nq) ++log_nq;
        const int units2 = rs->H << log_nq;
        if (sh->stride == 2 && (sh->H % 2) == 0 && (1 << log_nq) == nq && 16 * nq <= 2 * sh->W && units2 <= 256 &&
            knob("QE_SUB2", 1) != 0) {
            int log_up = 3;
            while ((1 << log_up) < units2) ++log_up;
            p.pre = PrePass::Sub2;
            p.sub2_log_nq = log_nq;
            p.sub2_log_up = log_up;
            const int ppb = (256 >> log_up) * 4;
            p.pre_blocks = (n_planes + ppb - 1) / ppb;
        } else {
            const bool wide = sh->stride == 2 && (sh->W % 4) == 0 && sh->W >= 16;
            const int units = rs->H * ((rs->W + (wide ? 7 : 3)) / (wide ? 8 : 4));
            const int ppb = units >= 1024 ? 1 : 1024 / units;   // 4 units per thread
            p.pre = wide ? PrePass::SubWide : PrePass::SubNarrow;
            p.pre_blocks = (n_planes + ppb - 1) / ppb;
        }
    }
    if (p.pre_blocks > 0x7fffffffLL) return p;

    // route and epilogue
    PwrFit pf;
    int g7 = 1;
    if (r.residual) {
        // block end (qe_quantconv2d_residual_prepared): stride-1 layers of either resident-tile kernel, 8-bit codes with one
        // scale.  7x7 planes: the 512-channel form only (512 -> 2048, the last stage's block end); the 4-image-tile
        // instances spill with the residual epilogue's registers on top (RQ + RES: 16 bytes of scratch)
        if (r.rq_bits != 0 && (r.rq_bits != 8 || r.rq_n_param != 1)) return p;
        if (m.sub || m.expand || rs->stride != 1) return p;
        if (pwr_plan(rs, &xr, r.w, xa, &pf)) p.route = ConvRoute::Pwr;
        else if (rs->IC == 512 && (p.pwr7_gi = pwr7_plan(rs, &xr, r.w, xa, &g7)) != 0) p.route = ConvRoute::Pwr7;
        else return p;
        p.fused = true;
    } else {
        const bool rq = r.rq_bits > 0;
        if (rq) {
            // the MFMA kernels' fused epilogue (8-bit codes, one output scale); the flat ones need their byte patch to fit
            if (r.rq_bits != 8 || r.rq_n_param != 1) return p;
            if (m.family == MfmaFamily::Flatg || mfma_is_flat(m.family)) {
                const size_t patch = m.family == MfmaFamily::Flatg ? (size_t)m.GI * m.MT * rs->H * rs->W : (size_t)m.MT * 32 * m.ni;
                if (align_up(m.lds, 16) + patch > (size_t)MF_MAX_LDS) return p;
            }
            p.fused = true;
        }
        // 1x1 / stride 1 layers with 8-bit operands whose channel depth fits the LDS (IC = 64 | 128 | 256, OC >= 128; 7x7:
        // 128 | 256 | 512): the resident-tile kernels.  Their re-quantising forms store codes as aligned 16-byte pieces
        // (QE_PWR_RQ=0: off); the plain 7x7 form stores fp32 the same way.  QE_PWR=0 keeps the kernels below.
        const bool pwr_ok = rq ? (r.rq_out & 15) == 0 && knob("QE_PWR_RQ", 1) != 0 : true;
        // 1x1 / stride 1 layers on 7x7 planes with 8-bit operands and IC % 64 == 0: the LDS-DMA ring kernel (-17..-20 % against
        // the register-staged kernels there, profiles/r02b_ab_flatd.txt).  QE_FLATD=0 keeps the register-staged flat kernels.
        // Re-quantising: whole 32-channel strips, codes as aligned 16-byte pieces (QE_FLATD_RQ=0: off).
        const bool fd_ok = flatd_plan(rs, &xr, r.w, xa) && knob("QE_FLATD", 1) != 0 &&
                           (!rq || (rs->OC % 32 == 0 && (r.rq_out & 15) == 0 && knob("QE_FLATD_RQ", 1) != 0));
        if (pwr_ok && pwr_plan(rs, &xr, r.w, xa, &pf)) p.route = ConvRoute::Pwr;
        else if (pwr_ok && (rq || (r.out & 15) == 0) && (p.pwr7_gi = pwr7_plan(rs, &xr, r.w, xa, &g7)) != 0) p.route = ConvRoute::Pwr7;
        else if (fd_ok) p.route = ConvRoute::Flatd;
        else p.route = ConvRoute::Mfma;
    }

    // launch geometry of the route
    if (p.route == ConvRoute::Pwr) {
        p.pwr_tw = pf.tw; p.pwr_ks = pf.ks; p.pwr_groups = pf.groups; p.pwr_s2 = pf.s2;
        const int64_t P = pf.s2 ? (int64_t)(rs->H / 2) * (rs->W / 2) : (int64_t)rs->H * rs->W;
        p.tiles_h = (int)(P / pf.tw);
        p.n_pix_tiles = rs->N * p.tiles_h;
        p.blocks = tile_grid(p.n_pix_tiles, p.tiles_h, pf.groups, true, p.chunk);
    } else if (p.route == ConvRoute::Pwr7) {
        p.pwr_groups = g7;
        p.tiles_h = 1;
        p.n_pix_tiles = rs->N / p.pwr7_gi;
        p.blocks = tile_grid(p.n_pix_tiles, 1, g7, false, p.chunk);
    } else if (p.route == ConvRoute::Flatd) {
        // 8-wave / 256-channel workgroups: measured (profiles/r02l_flatd_w8.txt) -9 % on 512->2048 @7x7, +-3 % on the 14x14
        // layers, +15 % on 2048->512 @7x7 -- halving the activation re-reads does NOT give the -14..-26 % a bytes-through-the-CU
        // model predicts.  On for wide 7x7 layers only; QE_FLATD8=0 | 1 overrides.
        const char *e8 = env_get("QE_FLATD8");
        p.fd_w8 = e8 ? atoi(e8) != 0 && rs->OC > 128 : rs->OC >= 1024;
        const int MT = p.fd_w8 ? 256 : 128;
        p.n_oc_tiles = (rs->OC + MT - 1) / MT;
        p.tiles_h = 1;                           // one tile = 4 whole images
        p.n_pix_tiles = (rs->N + 3) / 4;
        p.blocks = tile_grid(p.n_pix_tiles, p.tiles_h, p.n_oc_tiles, true, p.chunk);
    } else {
        plan_mfma_launch(p, r, p.fused);
    }
    if (p.blocks > 0x7fffffffLL) { p.route = ConvRoute::Generic; p.fused = false; }
    return p;
}

}  // namespace qe
