// qe_conv_plan.hpp -- the host-side plan of one packed-activation (int8 engine) convolution.
//
// plan_conv (qe_conv_plan.hip) decides everything about a request once: the pre-pass (4-bit expansion, strided gather),
// the route (resident-tile pwr / pwr7, LDS-DMA ring flatd, one of the MFMA families, or the generic VALU kernel), the
// epilogue (fused re-quantisation, LDS byte patch, border-class table), every LDS size, the grid and the workspace
// layout.  It is the only reader of the int8-conv QE_* knobs.  The C-ABI queries answer from the plan, and the launchers
// (launch_conv_mfma, launch_pwr, launch_flatd) build kernel arguments from it without re-deciding anything.
//
// The prepared part (re-laid-out weights, per-channel constants, tap-sum tables) comes from plan_prepared: shape without
// the batch size, and bits.  It never depends on a pointer, on N or on the route a run takes.
#pragma once
#include "qe_conv_common.hpp"

namespace qe {

constexpr int FD_CK = 64;   // flatd: input channels per stage

// which MFMA kernel runs (None: no family fits, the generic VALU kernel runs)
enum class MfmaFamily {
    None,
    Halo,      // conv_mfma_kernel: halo tile in LDS, any kernel size
    Ws,        // conv_mfma_ws_kernel: 3x3, warp-specialised producer / consumer waves
    Sm2,       // conv_mfma_sm2_kernel: 3x3, two strips per wave, weights through LDS
    Stem,      // conv_mfma_smallic_kernel: IC <= 4
    Flat,      // conv_mfma_flat_kernel: 1x1 / stride 1 / no padding over the flat pixel index
    FlatS2,    // ... stride 2 (the downsample branches)
    FlatX4,    // ... 4-bit activations read from the packed stream by the kernel itself
    Flatg      // conv_mfma_flatg_kernel: 1x1 on small planes (several whole images per tile)
};

inline bool mfma_is_flat(MfmaFamily f) { return f == MfmaFamily::Flat || f == MfmaFamily::FlatS2 || f == MfmaFamily::FlatX4; }

// MFMA family, pre-pass and workspace [prepared tables | scratch] of one problem
struct MfmaPlan {
    MfmaFamily family = MfmaFamily::None;
    int cfg = 0;       // 0: 4x1 waves (MT 128), 1: 2x2 (MT 64), 2: 1x4 (MT 32)
    int MT = 0, OCP = 0, NCH = 0, NG = 0, KK = 0, OH = 0, OW = 0;
    int TH = 0, ni = 0, niw = 0, IHT = 0, IWP = 0, ROWMUL = 1, COLMUL = 1;
    int GI = 1, NS = 1;
    bool wraw = false;         // the flat kernels read the packed 8-bit weights themselves: no tables
    bool expand = false;       // sub-8-bit activations are expanded to 8-bit codes in the workspace first
    size_t xe_off = 0;
    bool sub = false;          // strided 1x1: the sampled pixels are gathered into a dense tensor first
    bool sub_x4 = false;       // ... straight from the 4-bit stream (subsample_x4_kernel), no expansion pass
    size_t sub_off = 0;
    size_t lds = 0;
    size_t wt_bytes = 0, ep_off = 0, ws_off = 0, total = 0;
    size_t prep_total = 0;     // leading part of the workspace the prep pass fills (x-independent: can be kept across calls)
};

enum class ConvRoute { Generic, Pwr, Pwr7, Flatd, Mfma };
enum class PrePass { None, SubX4, Sub2, SubWide, SubNarrow };   // the strided gathers (m.expand: the 8-bit expansion)

// What is asked.  Pointers only count through their alignment; a query passes 0 for the ones it does not know (out,
// rq_out), which reads as aligned.
struct ConvRequest {
    const qe_conv_shape *sh;
    const qe_qparam *x, *w;    // bits, sign, n_param; the alignment of x->data, w->data and w->scale
    uintptr_t out = 0;         // fp32 output
    uintptr_t rq_out = 0;      // codes of a fused re-quantisation
    int rq_bits = 0;           // > 0: re-quantise the output to rq_bits with rq_n_param parameters
    int rq_n_param = 1;
    bool residual = false;     // block end: relu(conv + identity), with codes when rq_bits > 0
};

struct ConvPlan {
    ConvRoute route = ConvRoute::Generic;
    bool fused = false;        // the requested epilogue (re-quantisation, residual) runs inside the conv kernel
    int OH = 0, OW = 0;        // output plane (<= 0: empty)
    size_t y_bytes = 0;        // the fp32 output, rounded up to 256 bytes (the two-pass epilogues keep it in the workspace)
    MfmaPlan m;
    qe_conv_shape run{};       // the problem the conv kernel sees (the dense one after a strided gather)

    PrePass pre = PrePass::None;
    int64_t pre_blocks = 0;
    int sub2_log_up = 0, sub2_log_nq = 0;

    // XCD-aware block map shared by every route: `chunk` consecutive pixel tiles per XCD run
    int64_t blocks = 0;
    int chunk = 1, n_pix_tiles = 0, n_oc_tiles = 0, tiles_h = 0;
    size_t lds = 0;            // dynamic LDS of the MFMA-family launch (pwr and flatd size theirs at compile time)

    // pwr / pwr7
    int pwr_tw = 0, pwr_ks = 0, pwr_groups = 1, pwr7_gi = 0;
    bool pwr_s2 = false;
    // flatd
    bool fd_w8 = false;        // 8-wave / 256-channel workgroups
    // MFMA families
    bool rq_patch = false;     // re-quantised codes leave through the LDS byte patch (PATCH instances only)
    bool ctab = false;
    int ptab_off = 0;
    int n_top = 0, n_bot = 0, n_lft = 0, n_rgt = 0;
    int split = 1;             // sm2 / ws: channel slices of the staging threads
};

ConvPlan plan_conv(const ConvRequest &rq);
MfmaPlan plan_prepared(const qe_conv_shape *sh, int x_bits, int w_bits);
uint64_t prepared_layout(const MfmaPlan &p, const qe_conv_shape *sh);

// The launch function of the MFMA-family instance a plan selects (split: ConvPlan::split; rq: the re-quantising instance;
// patch: its LDS byte patch form), or null when no such instance is compiled.  The planner asks it whether a PATCH form
// exists, launch_conv_mfma calls what it returns: the two cannot disagree about the instance set (qe_conv_mfma.hip).
MfmaLaunch mfma_instance(const MfmaPlan &m, int KW, int split, bool rq, bool patch);
// tap form of an instance: 1 (1x1), 9 (3x3) or 0 (any other kernel size); only the halo family branches on it
inline int mfma_kkt(int KK, int KW) { return KK == 1 ? 1 : ((KK == 9 && KW == 3) ? 9 : 0); }

// launchers of the routes (the plan was made for these operands).  rq != NULL: the re-quantising instances, which store the
// consumer's 8-bit codes into `codes` and the range flag into `status`
int launch_conv_mfma(const ConvPlan &p, const qe_qparam *x, const qe_qparam *w, const float *bias, const qe_conv_shape *sh,
                     float *out, void *workspace, size_t workspace_bytes, const void *prepared, size_t prepared_bytes,
                     bool use_prepared, hipStream_t s, const qe_requant *rq, uint8_t *codes, int32_t *status, const float *res);
int prepare_conv_tables(const MfmaPlan &p, const qe_qparam *w, const float *bias, const qe_conv_shape *sh, void *prepared,
                        size_t prepared_bytes, hipStream_t s);
int launch_pwr(const ConvPlan &p, const qe_qparam *x, const qe_qparam *w, const float *bias, float *out, hipStream_t s,
               const qe_requant *rq, uint8_t *codes, int32_t *status, const float *res);
int launch_flatd(const ConvPlan &p, const qe_qparam *x, const qe_qparam *w, const float *bias, float *out, hipStream_t s,
                 const qe_requant *rq, uint8_t *codes, int32_t *status);

// ---- float-input convolution (fp32 activations x packed weights, qe_conv_f32.hip) -------------------------------------
// plan_conv_f32 is the only reader of QE_F32_MFMA (0: every shape stays on the VALU kernel) and decides the rest by shape.
// !ok: the generic VALU kernel runs and nothing is prepared.
enum class F32Kernel {         // <WM x WN waves x NIW column tiles per wave>, S2: two 16-channel groups per stage
    Stem4x1x7, Stem2x2x4, Stem2x2x7,
    M4x1x4, M4x1x4S2, M4x1x7, M4x1x7S2, M2x2x2, M2x2x2S2, M2x2x4, M2x2x4S2
};

struct F32Plan {
    bool ok = false;
    F32Kernel kernel = F32Kernel::M4x1x7;
    bool stem = false;         // IC <= 4: K = kh x [kw 0..7][ic 0..3] (conv_f32_stem_kernel and its own table layout)
    int OCP = 0, NG = 0, KK = 0, OH = 0, OW = 0;
    int TH = 0, GI = 1, IHT = 0, IWP = 0, ROWMUL = 1, COLMUL = 1;
    // XCD-aware block map, as ConvPlan's
    int64_t blocks = 0;
    int chunk = 1, n_pix_tiles = 0, n_oc_tiles = 0, tiles_h = 0;
    size_t lds = 0;
    size_t ep_off = 0, total = 0;      // prepared tables: [bf16 weights in fragment order | sw, zw, bias per padded channel]
};

F32Plan plan_conv_f32(const qe_conv_shape *sh);
int prepare_conv_f32(const F32Plan &p, const qe_qparam *w, const float *bias, const qe_conv_shape *sh, void *prepared,
                     size_t prepared_bytes, hipStream_t s);
int launch_conv_f32(const F32Plan &p, const float *x, const qe_conv_shape *sh, const void *prepared, size_t prepared_bytes,
                    float *out, hipStream_t s);

}  // namespace qe
