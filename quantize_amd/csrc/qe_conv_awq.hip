// qe_conv_awq.hip -- qe_quantconv2d_awq: packed NCHW activation codes x group-quantised (AWQ layout) packed OIHW weight codes.
//
//   out[n,o,oh,ow] = act( bias[o] + sx sum_g sw[o,g] sum_{c in g} sum_{kh,kw inside the image}
//                         (q_x[n,c,ih,iw] - zx) (q_w[o,c,kh,kw] - zw[o,g]) )
//
// Group g covers the input channels [g G, (g + 1) G) and all taps; sw / zw are fp32 arrays of OC (IC / G) elements in (o, g)
// order; sx / zx are one element each.  Two kernels and one host plan in a unit of its own: no other code object moves.  The
// host layer of the family and the device leaves it has in common with qe_linear_grp_i8.hip are qe_grp_common.hpp's.
//
// Both kernels read every stored value u as the CENTRED integer u - 2^(bits-1) (qe_linear_grp_i8.hip): with the residual
// zeros z' = zero - (signed ? 0 : 2^(bits-1)) and x_c, w_c the centred codes, over the n taps of a group inside the image
//   sum (x_c - zx') (w_c - zw') = P - zw' Sx - zx' (Sw - n zw'),   P = sum x_c w_c, Sx = sum x_c, Sw = sum w_c
// P, Sx and Sw are integers, exact in int32 and exact as fp32 while G KH KW <= 1024.  Only the fold rounds.
//
// Fast kernel (1x1 / stride 1 / padding 0, 8-bit activation codes, 4- or 8-bit weight codes, G in {32, 64, 128}, w->data
// 16-byte aligned; any N, OC, plane P = H W, any alignment of x->data and out): the grouped linear's arithmetic with the
// activations stored [N][C][P].  A = activations (rows = pixels), B = weights (columns = output channels), so D has the
// output channel on the lane and the pixel on the register: a lane holds ONE sw[o,g] and ONE zw'[o,g] per column tile per
// group, exactly as linear_grp_i8_mfma_kernel, and the fold is
//   acc_out = fma(sw, fma(-zw', float(Sx[p,g]), float(acc_g)), acc_out);   acc_g = 0
// (the opposite roles, qe_conv_pwr.hip's, would put 16 scales per lane per tile into every fold).  Epilogue:
//   out = act(fma(sx, acc_out - zx' T[o], bias[o])),   T[o] = sum_g sw[o,g] (Sw[o,g] - G zw'[o,g]).
// WZ = false (w_symmetric) has no Sx and no second term, XZ = false (x_symmetric) has no T.
//   * Workgroup = 2 x 2 waves, tile = 128 output channels x T pixels of ONE image (T = 128 | 64, a template parameter the
//     plan picks from P alone: a 49-pixel plane wastes 62 % of a 128-pixel tile and 23 % of a 64-pixel one).  Tail pixels
//     and channels are computed on clamped addresses and dropped at the store.
//   * Activations: a stage is 64 channels x T pixels in the native [channel][pixel] byte order, row pitch 32 (T / 32 + 1)
//     bytes -- 160 | 96, 32 x odd, so the 8 rows of a transposed read fall into 8 distinct 32-byte bank groups.  A thread
//     fetches 16-byte row pieces at ANY alignment (planes of 49 or 196 bytes start anywhere); a piece may run into the next
//     channel's plane (those pixels are tail pixels) but never past the tensor: there it is read byte by byte, as
//     span_load16 does.  Recoded once on the way in (^ 0x80); two stage buffers, one barrier per stage.  The A fragments come
//     from ds_read_b64_tr_b8, two per 32 x 32 tile and k-step.
//   * Weights: the grouped linear's path, unchanged: packed [OC][IC] rows, 16-byte pieces XOR-swizzled into a [128][64] image,
//     nibbles widened and centred in registers (v_perm, + 0x78787878, ^ 0x80808080); no widened copy exists.  T accumulates on
//     the threads that stage a column's codes and is reduced once per tile.
//   * Sx: after the transposed read a lane holds 16 k-bytes of its pixel: four v_dot4_i32_i8 against ones, accumulated over
//     the group's k-steps, one exchange with lane ^ 32 at the group's end.  The pixel is on the LANE there and on the
//     REGISTER in D, so the sums cross a small LDS array -- one per WAVE (each wave sums its own rows; the two waves of a
//     pixel half repeat four dots per fragment), written and read by the same wave: no barrier and no stage parity.
//   * IC need only be a multiple of G: with IC % 64 == 32 (G = 32) the last stage holds one k-step; its second half is
//     staged from clamped (valid) addresses and never multiplied.
//   * Store: a register quad is 4 consecutive pixels of one channel.  Each wave turns its 32 x 32 tiles through a private
//     LDS patch and stores 8 channel rows x 128 contiguous bytes per instruction (P % 4 == 0 and a 16-byte aligned out);
//     element stores otherwise.  The PATH never depends on the alignment of x->data or out, only this store arm does.
//
// Plain kernel (everything else: any kernel size, stride, padding, code width, group size, alignment): one thread per
// output, group by group: the three integer sums over the taps inside the image, then the fold.
//
// Fused forms (qe_quantconv2d_awq_fused): two more epilogues of the fast kernel, one more plain kernel, the same K loop.
//   CA_CODES     act(y) as fp32 (optional) and / or as the consumer's 8-bit codes (optional), no identity
//   CA_END       act(y + identity): a residual block's end; out and codes each optional
// The fp32 kernels keep their instruction streams: the fused forms are two more template arguments of the same kernels
// (the form, and the argument block extended by what the epilogue reads), everything they add stands behind an
// `if constexpr` on them, and the defaults instantiate the text that was there before.  (Sharing the K loop as a device
// function moves the fp32 instances' instruction streams, as DESIGN.md records for grp_fold.)
//   * Quantiser: D has the output channel on the LANE, so the consumer's scale and zero (per tensor, or per output channel --
//     what an AWQ consumer's quantiser is once its awq_scale is folded in) are one register each per column tile, loaded
//     from a clamped address as the bias is.  qe_rq_code is qe_quantize_pack's arithmetic: IEEE division, subtraction,
//     rint, clamp, range test.
//   * Code store: a lane holds four dwords of codes of a 32 x 32 tile, at pixels 8 gq + 4 h.  Two v_permlane32_swap
//     between lane and lane ^ 32 leave pixels 0 .. 15 in the h = 0 lane and 16 .. 31 in the h = 1 lane: one 16-byte store per
//     lane (P % 16 == 0, codes 16-byte aligned), four dword stores (P % 4 == 0, codes 4-byte aligned), or sixteen bytes.
//     No LDS pass and no barrier: the patch stays free for the fp32 tile of the same step.
//   * Identity: read with the access pattern out is written with -- 8 channel rows x 128 bytes per instruction into the
//     wave's patch, quads picked up from it (P % 4 == 0, identity and out 16-byte aligned), single elements otherwise.  The
//     loads of a tile are issued before that tile's sx / bias arithmetic.
//   * Flag: the lanes' range flags are ORed over the wave (ballot); at most one atomicOr per wave, only when it is set.
#include "qe_grp_common.hpp"         // the host layer and the device leaves shared with qe_linear_grp_i8.hip
#include "qe_elementwise.hpp"        // qe_rq_code: the quantiser of qe_quantize_pack

namespace qe {

enum { CA_F32 = 0, CA_CODES = 1, CA_END = 2 };            // the epilogue forms

// the kernel argument: both kernels read the same block
struct ConvAwqArgs {
    const uint8_t *x, *w;      // packed NCHW activation codes, packed OIHW weight codes
    const float *x_scale, *x_zero, *w_scale, *w_zero, *bias;
    float *out;                // [N][OC][OH][OW] fp32
    int x_bits, x_sign, w_bits, w_sign;
    int G, NG;                 // input channels per group, groups per output channel (IC / G)
    int N, IC, H, W, OC, KH, KW, stride, padding, OH, OW;
    int P;                     // fast kernel: the plane, H * W
    int tiles;                 // fast kernel: pixel tiles per image
    int relu;
};

// the kernel argument of the fused kernels: the block above (out may be NULL), then what the epilogue adds
struct ConvAwqFusedArgs : ConvAwqArgs {
    const float *identity;     // CA_END: fp32, shaped like out (may be out itself)
    uint8_t *codes;            // [N][OC][OH][OW] stored 8-bit codes, or NULL
    int32_t *status;           // bit 0 set when a code fails the range test (NaN included), or NULL
    int rq_per_col;            // one scale and zero per output channel (else one of each)
    QeRq rq;
};

namespace {

typedef int v2i_a __attribute__((ext_vector_type(2)));
typedef int v4i_a __attribute__((ext_vector_type(4)));
typedef int v16i_a __attribute__((ext_vector_type(16)));
typedef float v16f_a __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float awq_act(float v, int relu) { return (!relu || v > 0.0f || v != v) ? v : 0.0f; }   // NaN passes

// ---------------------------------------------------------------------------------------------
// Plain kernel: thread <-> output (n, o, oh, ow), ow fastest.
// ---------------------------------------------------------------------------------------------
// A = ConvAwqFusedArgs: the fused forms on the plain route: per output the add, the ReLU, the fp32 store, one byte store for
// an 8-bit code and an atomic OR for the flag.  The thread that writes out[idx] has read identity[idx]: in place is safe.
template <class A = ConvAwqArgs>
__global__ __launch_bounds__(256) void conv_awq_plain_kernel(const A a)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)a.N * a.OC * a.OH * a.OW) return;
    const int ow = (int)(idx % a.OW);
    int64_t t = idx / a.OW;
    const int oh = (int)(t % a.OH);
    t /= a.OH;
    const int o = (int)(t % a.OC);
    const int64_t n = t / a.OC;
    const float sx = a.x_scale[0];
    const float zxr = a.x_zero[0] - (a.x_sign ? 0.0f : (float)(1 << (a.x_bits - 1)));
    const float woff = a.w_sign ? 0.0f : (float)(1 << (a.w_bits - 1));
    const int ih0 = oh * a.stride - a.padding, iw0 = ow * a.stride - a.padding;
    float acc = 0.0f;
    for (int g = 0; g < a.NG; ++g) {
        const float sw = a.w_scale[(int64_t)o * a.NG + g], zwr = a.w_zero[(int64_t)o * a.NG + g] - woff;
        int64_t p = 0, s_x = 0, s_w = 0, taps = 0;
        for (int c = g * a.G; c < (g + 1) * a.G; ++c) {
            for (int kh = 0; kh < a.KH; ++kh) {
                const int ih = ih0 + kh;
                if (ih < 0 || ih >= a.H) continue;
                for (int kw = 0; kw < a.KW; ++kw) {
                    const int iw = iw0 + kw;
                    if (iw < 0 || iw >= a.W) continue;
                    const int xc = centred_elem(a.x, ((n * a.IC + c) * a.H + ih) * a.W + iw, a.x_bits);
                    const int wc = centred_elem(a.w, (((int64_t)o * a.IC + c) * a.KH + kh) * a.KW + kw, a.w_bits);
                    p += xc * wc; s_x += xc; s_w += wc; ++taps;
                }
            }
        }
        float f = fmaf(-zwr, (float)s_x, (float)p);
        f = fmaf(-zxr, fmaf(-(float)taps, zwr, (float)s_w), f);
        acc = fmaf(sw, f, acc);
    }
    if constexpr (std::is_same<A, ConvAwqFusedArgs>::value) {
        float v = fmaf(sx, acc, a.bias != nullptr ? a.bias[o] : 0.0f);
        if (a.identity != nullptr) v = v + a.identity[idx];
        v = awq_act(v, a.relu);
        if (a.out != nullptr) a.out[idx] = v;
        if (a.codes != nullptr) {
            bool bad = false;
            const int ci = a.rq_per_col ? o : 0;
            a.codes[idx] = (uint8_t)qe_rq_code(v, a.rq.scale[ci], a.rq.zero[ci], a.rq, bad);
            if (bad && a.status != nullptr) atomicOr(a.status, 1);
        }
        return;
    }
    a.out[idx] = awq_act(fmaf(sx, acc, a.bias != nullptr ? a.bias[o] : 0.0f), a.relu);
}

// ---------------------------------------------------------------------------------------------
// Fast kernel.  WB: bits of a stored weight code (4 | 8).  WZ: residual weight zeros (Sx and the zw' term).  XZ: residual
// activation zeros (T and the zx' term).  T: pixels of a tile (64 | 128).
// ---------------------------------------------------------------------------------------------
// 16 bytes at src, any alignment; the bytes at and beyond x_hi (the tensor's end) are not read and come back 0
__device__ __forceinline__ uint4 load16_any(const uint8_t *src, const uint8_t *x_hi)
{
    uint4 v;
    if (src + 16 <= x_hi) {
        __builtin_memcpy(&v, src, 16);
    } else {
        unsigned d[4] = {0, 0, 0, 0};
        for (int b = 0; b < 16; ++b)
            if (src + b < x_hi) d[b >> 2] |= (unsigned)src[b] << (8 * (b & 3));
        v = make_uint4(d[0], d[1], d[2], d[3]);
    }
    return v;
}

constexpr int CA_OCT = 128, CA_K = 64, CA_STEP = 32;
constexpr int CA_WPLANE = CA_OCT * CA_K;                  // bytes of the [128][64] weight image (8 KB)

template <int T> struct CaGeom {
    static constexpr int MI = T / 64;                     // 32-pixel row tiles of a wave
    static constexpr int PITCH = 32 * (T / 32 + 1);       // bytes of a channel row of the activation image: 32 x odd
    static constexpr int SEGS = T / 16;                   // 16-byte pieces of a channel row
    static constexpr int PPT = CA_K * SEGS / 256;         // ... per thread and stage
    static constexpr int XPLANE = CA_K * PITCH;
    static constexpr int BUF = XPLANE + CA_WPLANE;        // one stage buffer: the activation image, the weight image
    static constexpr int PATCH = 4 * 32 * 36 * 4;         // the four waves' store patches (in the free stage buffers)
    static constexpr int STAGES = 2 * BUF > PATCH ? 2 * BUF : PATCH;
    // + Sx[wave][T / 2] (int32), T[column] (fp32)
    static constexpr size_t LDS = (size_t)STAGES + (4 * (T / 2) + CA_OCT) * 4;
    static_assert(((T / 32 + 1) & 1) == 1 && PPT >= 1, "tile width");
};

// EPI: the epilogue form; A: ConvAwqFusedArgs for a fused form.  (The defaults are the fp32 kernel as it always was.)
template <int WB, bool WZ, bool XZ, int T, int EPI = CA_F32, class A = ConvAwqArgs>
__global__ __launch_bounds__(256, 2) void conv_awq_mfma_kernel(const A a)
{
    using Gm = CaGeom<T>;
    constexpr int MI = Gm::MI, PITCH = Gm::PITCH, SEGS = Gm::SEGS, PPT = Gm::PPT;
    extern __shared__ __attribute__((aligned(16))) uint8_t lsm[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave & 1, wn = wave >> 1;              // pixel half, output-channel half of the tile
    const int col = lane & 31, h = lane >> 5;
    int *sxw = reinterpret_cast<int *>(lsm + Gm::STAGES) + wave * (T / 2);        // [T / 2]: Sx of this wave's rows
    float *tcol = reinterpret_cast<float *>(lsm + Gm::STAGES) + 4 * (T / 2);      // [128]: T of the tile's columns

    const int P = a.P, IC = a.IC, OC = a.OC;
    const int n_ct = (OC + CA_OCT - 1) / CA_OCT;
    const int64_t bid = blockIdx.x;
    const int n0 = (int)(bid % n_ct) * CA_OCT;            // the channel tile runs fastest: neighbours share the pixels
    const int64_t pt = bid / n_ct;
    const int64_t n = pt / a.tiles;
    const int p0 = (int)(pt - n * a.tiles) * T;
    const int gmask = a.G / CA_STEP - 1;                  // k-steps per group - 1 (0, 1 or 3)
    const int gsh = a.G == 32 ? 0 : a.G == 64 ? 1 : 2;    // k-step -> group
    const int n_steps = IC / CA_STEP, n_stages = (n_steps + 1) >> 1;
    const float woff = a.w_sign ? 0.0f : (float)(1 << (WB - 1));      // zw' = zw - woff

    // activations: piece e = tid + 256 i <-> (channel e / SEGS of the stage, 16 pixels from p0 + 16 (e % SEGS)).  A piece
    // that starts beyond the plane holds tail pixels only: it reads the image's first bytes instead.
    const uint8_t *xi = a.x + n * IC * P;
    const uint8_t *x_hi = a.x + (int64_t)a.N * IC * P;
    int pch[PPT], ppx[PPT], plds[PPT];
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
        const int e = tid + 256 * i;
        const int c = e / SEGS, sg = e - c * SEGS;
        pch[i] = c;
        ppx[i] = p0 + 16 * sg < P ? p0 + 16 * sg : -1;
        plds[i] = c * PITCH + 16 * sg;
    }
    // weights, 8-bit: thread <-> (column r4 + 64 i, 16-byte piece p4 of the stage's 64 k); 4-bit: thread <-> (column wc,
    // k-step whh): 16 bytes = 32 codes  (twin: linear_grp_i8_mfma_kernel's weight path, here and in fetch and stage)
    const int p4 = tid & 3, r4 = tid >> 2;
    const int wc = tid >> 1, whh = tid & 1;
    const uint8_t *wrow[2];
    int64_t tog[2];                                       // the staged columns in the (o, g) arrays (T)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = WB == 8 ? r4 + 64 * i : wc;
        const int cc = (n0 + c < OC) ? n0 + c : OC - 1;
        wrow[i] = a.w + (int64_t)cc * IC * WB / 8;
        tog[i] = (int64_t)cc * a.NG;
    }
    const int tstep = WB == 8 ? (p4 >> 1) : whh;          // the k-step of the stage this thread's weight codes lie in

    uint4 xv[PPT], wv[2];
    float tsw[2] = {0.0f, 0.0f}, tzw[2] = {0.0f, 0.0f};
    auto fetch = [&](int st) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < PPT; ++i) {
            const int cg = min(st * CA_K + pch[i], IC - 1);            // (clamped in the half stage of an odd k-step count)
            xv[i] = load16_any(ppx[i] >= 0 ? xi + (int64_t)cg * P + ppx[i] : xi, x_hi);
        }
        if constexpr (WB == 8) {
            const int kx = min(st * CA_K + 16 * p4, IC - 16);
#pragma unroll
            for (int i = 0; i < 2; ++i) wv[i] = *reinterpret_cast<const uint4 *>(wrow[i] + kx);
        } else {
            wv[0] = *reinterpret_cast<const uint4 *>(wrow[0] + min(st * (CA_K / 2) + 16 * whh, IC / 2 - 16));
        }
        if constexpr (XZ) {
            const int g = min(2 * st + tstep, n_steps - 1) >> gsh;
#pragma unroll
            for (int i = 0; i < (WB == 8 ? 2 : 1); ++i) { tsw[i] = a.w_scale[tog[i] + g]; tzw[i] = a.w_zero[tog[i] + g] - woff; }
        }
    };
    float tacc[2] = {0.0f, 0.0f};                         // this thread's share of T of its column(s)
    auto stage = [&](int st) __attribute__((always_inline)) {
        uint8_t *base = lsm + (st & 1) * Gm::BUF;
#pragma unroll
        for (int i = 0; i < PPT; ++i) *reinterpret_cast<uint4 *>(base + plds[i]) = xor80(xv[i]);
        const bool tvalid = 2 * st + tstep < n_steps;     // (the codes of a clamped half stage count for nothing)
        uint8_t *wbase = base + Gm::XPLANE;
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

    v16i_a accg[MI][2];                                   // the running group
    v16f_a acco[MI][2];                                   // the folded total
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) { accg[i][j][r] = 0; acco[i][j][r] = 0.0f; }
    int sxa[MI];                                          // this lane's half of Sx[., g] of its pixel in each row tile
#pragma unroll
    for (int i = 0; i < MI; ++i) sxa[i] = 0;

    // this lane's two output channels (clamped) in the (o, g) arrays
    int64_t og[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) og[j] = (int64_t)min(n0 + wn * 64 + j * 32 + col, OC - 1) * a.NG;

    // transposed read: lane i16 of a 16-lane group gets column i16 of an 8-row x 16-byte block whose row r address comes from
    // lanes 2 r, 2 r + 1: row (i16 >> 1) of the k-half h, byte half (i16 & 1), 16-pixel group (lane >> 4) & 1 of the row tile
    const int i16 = lane & 15;
    const int a_off = (16 * h + (i16 >> 1)) * PITCH + 16 * ((lane >> 4) & 1) + 8 * (i16 & 1) + wm * (T / 2);
    const int swz = (col >> 2) & 3;
    const int b_off = Gm::XPLANE + (wn * 64 + col) * 64;
    fetch(0);
    stage(0);
    for (int st = 0; st < n_stages; ++st) {
        // buffer st & 1 is complete; every wave has left buffer (st + 1) & 1
        __syncthreads();
        const bool more = st + 1 < n_stages;
        if (more) fetch(st + 1);                          // in flight under the MFMAs
        bool fold[2];                                     // (uniform)
        float gsw[2][2] = {{0.0f, 0.0f}, {0.0f, 0.0f}}, gdz[2][2] = {{0.0f, 0.0f}, {0.0f, 0.0f}};
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int step = 2 * st + ks;
            fold[ks] = step < n_steps && (step & gmask) == gmask;
            if (fold[ks]) {                               // (twin: linear_grp_i8_mfma_kernel's group-boundary fetch)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    gsw[ks][j] = a.w_scale[og[j] + (step >> gsh)];
                    if constexpr (WZ) gdz[ks][j] = a.w_zero[og[j] + (step >> gsh)] - woff;
                }
            }
        }
        const uint8_t *buf = lsm + (st & 1) * Gm::BUF;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            if (2 * st + ks < n_steps) {                  // (uniform: false in the half stage of an odd k-step count)
                const int po = 16 * ((2 * ks + h) ^ swz);
                v4i_a fa[MI], fb[2];
#pragma unroll
                for (int j = 0; j < 2; ++j) fb[j] = *reinterpret_cast<const v4i_a *>(buf + b_off + j * 32 * 64 + po);
#pragma unroll
                for (int i = 0; i < MI; ++i) {
                    const uint8_t *src = buf + a_off + ks * 32 * PITCH + i * 32;
                    const v2i_a lo = __builtin_amdgcn_ds_read_tr8_b64_v2i32((v2i_a __attribute__((address_space(3))) *)(src));
                    const v2i_a hi = __builtin_amdgcn_ds_read_tr8_b64_v2i32((v2i_a __attribute__((address_space(3))) *)(src + 8 * PITCH));
                    fa[i] = v4i_a{lo[0], lo[1], hi[0], hi[1]};
                    if constexpr (WZ) sxa[i] += dot_ones(make_uint4((unsigned)lo[0], (unsigned)lo[1], (unsigned)hi[0], (unsigned)hi[1]));
                }
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) accg[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[i], fb[j], accg[i][j], 0, 0, 0);
            }
            if (fold[ks]) {
                if constexpr (WZ) {                       // both k halves of a pixel, from its lane to this wave's array
#pragma unroll
                    for (int i = 0; i < MI; ++i) {
                        const int s = sxa[i] + __shfl_xor(sxa[i], 32);
                        if (h == 0) sxw[i * 32 + col] = s;
                        sxa[i] = 0;
                    }
                    __builtin_amdgcn_wave_barrier();      // (a wave's own LDS operations complete in order)
                }
#pragma unroll
                for (int i = 0; i < MI; ++i) {            // (twin: qe_grp_common.hpp's grp_fold, which the two linear kernels share)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float s = 0.0f;
                        if constexpr (WZ) s = (float)sxw[i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h];
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            const float p = (float)accg[i][j][r];
                            const float t = WZ ? fmaf(-gdz[ks][j], s, p) : p;
                            acco[i][j][r] = fmaf(gsw[ks][j], t, acco[i][j][r]);
                            accg[i][j][r] = 0;
                        }
                    }
                }
                if constexpr (WZ) __builtin_amdgcn_wave_barrier();
            }
        }
        if (more) stage(st + 1);
    }
    if constexpr (XZ) {                                   // T: the threads of a column add their shares (twin: linear_grp_i8_mfma_kernel's)
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

    // D has the pixel on the register and the output channel on the lane; a register quad is 4 consecutive pixels.  Each wave
    // turns its 32 x 32 tiles through a private LDS patch (row = channel, 36 floats) and reads it back with 8 lanes per
    // channel row: 8 rows x 128 contiguous bytes per store instruction.
    const float sx = a.x_scale[0];
    const float zxr = a.x_zero[0] - (a.x_sign ? 0.0f : 128.0f);
    float *patch = reinterpret_cast<float *>(lsm) + wave * (32 * 36);
    const int rrow = lane >> 3, rq = lane & 7;
    if constexpr (EPI != CA_F32) {
        // Every branch on has_out / has_codes / vec4 / cform is wave-uniform.  In place (out == identity): a tile belongs to
        // one wave; in the patch arm the lane that stores the piece (row 8 k + rrow, pixels q0 + 4 rq ..) is the lane that
        // loaded it, and what it stores comes out of the patch, which holds the sums only after every load of the tile has
        // landed in it; in the element arm a lane reads and writes the same elements.  So each element is read before it
        // is written, by the same lane.
        const bool has_out = a.out != nullptr, has_codes = a.codes != nullptr;
        const int64_t img = n * OC * P;
        const bool vec4 = (P & 3) == 0 && (reinterpret_cast<uintptr_t>(a.out) & 15) == 0 &&
                          (EPI != CA_END || (reinterpret_cast<uintptr_t>(a.identity) & 15) == 0);
        const uintptr_t cad = reinterpret_cast<uintptr_t>(a.codes);
        const int cform = ((P & 15) == 0 && (cad & 15) == 0) ? 2 : ((P & 3) == 0 && (cad & 3) == 0) ? 1 : 0;
        bool bad = false;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int c0 = n0 + wn * 64 + j * 32, c = c0 + col, cc = min(c, OC - 1);
            const float bias = a.bias != nullptr ? a.bias[cc] : 0.0f;
            const float tj = XZ ? tcol[wn * 64 + j * 32 + col] : 0.0f;
            float sc = 1.0f, zr = 0.0f;                   // the consumer's quantiser of this lane's channel
            if (has_codes) { sc = a.rq.scale[a.rq_per_col ? cc : 0]; zr = a.rq.zero[a.rq_per_col ? cc : 0]; }
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                const int q0 = p0 + wm * (T / 2) + i * 32;    // + (r & 3) + 8 (r >> 2) + 4 h: register r's pixel
                float v[16];
                if constexpr (EPI == CA_END) {
                    const float *idn = a.identity + img;
                    if (vec4) {
                        float4 ld[4];                     // requested first: in flight under the sx / bias arithmetic
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const int row = 8 * k + rrow, px = q0 + 4 * rq;
                            ld[k] = (c0 + row < OC && px < P) ? *reinterpret_cast<const float4 *>(idn + (int64_t)(c0 + row) * P + px)
                                                              : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                        }
#pragma unroll
                        for (int r = 0; r < 16; ++r) v[r] = fmaf(sx, XZ ? fmaf(-zxr, tj, acco[i][j][r]) : acco[i][j][r], bias);
#pragma unroll
                        for (int k = 0; k < 4; ++k) *reinterpret_cast<float4 *>(patch + (8 * k + rrow) * 36 + 4 * rq) = ld[k];
                        __builtin_amdgcn_wave_barrier();
#pragma unroll
                        for (int gq = 0; gq < 4; ++gq) {
                            const float4 t = *reinterpret_cast<const float4 *>(patch + col * 36 + 8 * gq + 4 * h);
                            v[4 * gq] = v[4 * gq] + t.x; v[4 * gq + 1] = v[4 * gq + 1] + t.y;
                            v[4 * gq + 2] = v[4 * gq + 2] + t.z; v[4 * gq + 3] = v[4 * gq + 3] + t.w;
                        }
                        __builtin_amdgcn_wave_barrier();
                    } else {
                        float id[16];
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int px = q0 + (r & 3) + 8 * (r >> 2) + 4 * h;
                            id[r] = (c < OC && px < P) ? idn[(int64_t)c * P + px] : 0.0f;
                        }
#pragma unroll
                        for (int r = 0; r < 16; ++r) v[r] = fmaf(sx, XZ ? fmaf(-zxr, tj, acco[i][j][r]) : acco[i][j][r], bias) + id[r];
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) v[r] = fmaf(sx, XZ ? fmaf(-zxr, tj, acco[i][j][r]) : acco[i][j][r], bias);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) v[r] = awq_act(v[r], a.relu);
                if (has_out) {                            // (twin: the fp32 form's two store arms below)
                    float *outn = a.out + img;
                    if (vec4) {
#pragma unroll
                        for (int gq = 0; gq < 4; ++gq)
                            *reinterpret_cast<float4 *>(patch + col * 36 + 8 * gq + 4 * h) = make_float4(v[4 * gq], v[4 * gq + 1], v[4 * gq + 2], v[4 * gq + 3]);
                        __builtin_amdgcn_wave_barrier();
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const int row = 8 * k + rrow, px = q0 + 4 * rq;
                            const float4 o4 = *reinterpret_cast<const float4 *>(patch + row * 36 + 4 * rq);
                            if (c0 + row < OC && px < P) *reinterpret_cast<float4 *>(outn + (int64_t)(c0 + row) * P + px) = o4;
                        }
                        __builtin_amdgcn_wave_barrier();
                    } else {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int px = q0 + (r & 3) + 8 * (r >> 2) + 4 * h;
                            if (c < OC && px < P) outn[(int64_t)c * P + px] = v[r];
                        }
                    }
                }
                if (has_codes) {
                    unsigned cw[4];                       // cw[gq]: the codes of pixels q0 + 8 gq + 4 h .. + 3, low byte first
#pragma unroll
                    for (int gq = 0; gq < 4; ++gq) {
                        cw[gq] = 0u;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            bool b1 = false;
                            cw[gq] |= qe_rq_code(v[4 * gq + e], sc, zr, a.rq, b1) << (8 * e);
                            bad |= b1 && c < OC && q0 + 8 * gq + 4 * h + e < P;       // lanes on tile padding never raise the flag
                        }
                    }
                    // lanes [32, 64) of the first operand <-> lanes [0, 32) of the second: afterwards the h = 0 lane holds the
                    // dwords of pixels 0, 4, 8, 12 and the h = 1 lane those of pixels 16, 20, 24, 28
                    const auto s0 = __builtin_amdgcn_permlane32_swap(cw[0], cw[2], false, false);
                    const auto s1 = __builtin_amdgcn_permlane32_swap(cw[1], cw[3], false, false);
                    const unsigned pk[4] = {s0[0], s0[1], s1[0], s1[1]};
                    const int px0 = q0 + 16 * h;
                    uint8_t *dst = a.codes + img + (int64_t)c * P + px0;     // (formed, not touched, beyond OC or P)
                    if (c < OC) {
                        if (cform == 2) {                 // P % 16 == 0: a piece lies wholly inside the plane or beyond it
                            if (px0 < P) *reinterpret_cast<uint4 *>(dst) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
                        } else if (cform == 1) {          // P % 4 == 0: so does a dword
#pragma unroll
                            for (int k = 0; k < 4; ++k)
                                if (px0 + 4 * k < P) *reinterpret_cast<unsigned *>(dst + 4 * k) = pk[k];
                        } else {
#pragma unroll
                            for (int b = 0; b < 16; ++b)
                                if (px0 + b < P) dst[b] = (uint8_t)(pk[b >> 2] >> (8 * (b & 3)));
                        }
                    }
                }
            }
        }
        if (has_codes && __builtin_amdgcn_ballot_w64(bad) != 0ull && lane == 0 && a.status != nullptr) atomicOr(a.status, 1);
        return;
    }
    const bool vec4 = (P & 3) == 0 && (reinterpret_cast<uintptr_t>(a.out) & 15) == 0;
    float *outn = a.out + n * OC * P;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int c0 = n0 + wn * 64 + j * 32, c = c0 + col;
        const float bias = a.bias != nullptr ? a.bias[min(c, OC - 1)] : 0.0f;
        const float tj = XZ ? tcol[wn * 64 + j * 32 + col] : 0.0f;
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            const int q0 = p0 + wm * (T / 2) + i * 32;    // + (r & 3) + 8 (r >> 2) + 4 h: register r's pixel
            float v[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float t = XZ ? fmaf(-zxr, tj, acco[i][j][r]) : acco[i][j][r];
                v[r] = awq_act(fmaf(sx, t, bias), a.relu);
            }
            if (vec4) {
#pragma unroll
                for (int gq = 0; gq < 4; ++gq)
                    *reinterpret_cast<float4 *>(patch + col * 36 + 8 * gq + 4 * h) = make_float4(v[4 * gq], v[4 * gq + 1], v[4 * gq + 2], v[4 * gq + 3]);
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int row = 8 * k + rrow, px = q0 + 4 * rq;      // P % 4 == 0: a piece lies wholly inside the plane or beyond it
                    const float4 o4 = *reinterpret_cast<const float4 *>(patch + row * 36 + 4 * rq);
                    if (c0 + row < OC && px < P) *reinterpret_cast<float4 *>(outn + (int64_t)(c0 + row) * P + px) = o4;
                }
                __builtin_amdgcn_wave_barrier();
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int px = q0 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    if (c < OC && px < P) outn[(int64_t)c * P + px] = v[r];
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Host side: one plan, read by the path queries and by the launches.  No HIP call in it.
// ---------------------------------------------------------------------------------------------
struct ConvAwqPlan {
    int fast;               // 1: conv_awq_mfma_kernel, 0: conv_awq_plain_kernel (a fused form: their fused twins)
    GrpI8Instance inst;     // the fast kernel's instance ...
    int t64;                // ... and its tile width
    int OH, OW, tiles;
    int64_t blocks;
    int epi;                // CA_F32 (qe_quantconv2d_awq) | CA_CODES | CA_END
    int two_pass;           // a fused form with sub-8-bit codes: the kernel writes out, qe_quantize_pack packs it
    int path;               // what the fused path query answers: 1 the fast kernel finishes the work, 0 otherwise
};

// The tile width, from P alone: 64-pixel tiles where they save at least an eighth of the pixels the 128-pixel tiles would
// compute (P = 49: 64 against 128; P = 196, 784, 3136: 128)
bool awq_tile64(int64_t P)
{
    const int64_t pad128 = ceil_div64(P, 128) * 128, pad64 = ceil_div64(P, 64) * 64;
    return (pad128 - pad64) * 8 >= pad128;
}

// a validated request (check_conv_awq; check_conv_awq_fused for a fused form).  epi: the form asked for; rq: its quantiser or
// NULL.  No address enters: alignment selects a store arm inside the kernel.
ConvAwqPlan plan_conv_awq(const qe_qparam *x, const qe_qparam *w, int G, int x_symmetric, int w_symmetric, const qe_conv_shape *sh,
                          int epi = CA_F32, const qe_requant *rq = nullptr)
{
    ConvAwqPlan p = {};
    p.epi = epi;
    p.two_pass = rq != nullptr && rq->n_bits < 8;
    p.OH = (sh->H + 2 * sh->padding - sh->KH) / sh->stride + 1;
    p.OW = (sh->W + 2 * sh->padding - sh->KW) / sh->stride + 1;
    p.fast = grp_weights_fast(w, G) && sh->KH == 1 && sh->KW == 1 && sh->stride == 1 && sh->padding == 0 && x->n_bits == 8 &&
             (int64_t)sh->H * sh->W <= (1 << 30);
    p.inst = grp_i8_instance(w, x_symmetric, w_symmetric);
    const int64_t P = (int64_t)sh->H * sh->W;
    p.t64 = awq_tile64(P);
    p.tiles = (int)ceil_div64(P, p.t64 ? 64 : 128);
    p.blocks = p.fast ? (int64_t)sh->N * p.tiles * ceil_div64(sh->OC, CA_OCT) : ceil_div64((int64_t)sh->N * sh->OC * p.OH * p.OW, 256);
    p.path = p.fast && !p.two_pass;
    return p;
}

int check_conv_awq(const qe_qparam *x, const qe_qparam *w, int G, const qe_conv_shape *sh)
{
    if (sh == nullptr) return QE_ERR_ARG;
    if (sh->N <= 0 || sh->IC <= 0 || sh->H <= 0 || sh->W <= 0 || sh->OC <= 0 || sh->KH <= 0 || sh->KW <= 0 || sh->stride <= 0 ||
        sh->padding < 0 || sh->H + 2 * sh->padding < sh->KH || sh->W + 2 * sh->padding < sh->KW)
        return QE_ERR_ARG;
    if (int rc = check_operand(x)) return rc;
    if (int rc = check_grp_weights(w, G, sh->IC, sh->OC)) return rc;
    return x->n_param == 1 ? QE_OK : QE_ERR_ARG;
}

template <int WB, bool WZ, bool XZ>
void launch_conv_awq(const ConvAwqPlan &p, const ConvAwqArgs &a, hipStream_t s)
{
    const unsigned blocks = (unsigned)p.blocks;
    if (p.t64) launch_instance<&conv_awq_mfma_kernel<WB, WZ, XZ, 64>>(blocks, 256, CaGeom<64>::LDS, 0, s, a);
    else launch_instance<&conv_awq_mfma_kernel<WB, WZ, XZ, 128>>(blocks, 256, CaGeom<128>::LDS, 0, s, a);
}

template <int WB, bool WZ, bool XZ>
void launch_conv_awq_fused(const ConvAwqPlan &p, const ConvAwqFusedArgs &f, hipStream_t s)
{
    const unsigned blocks = (unsigned)p.blocks;
    dispatch_flag(p.epi == CA_END, [&](auto end) {
        constexpr int EPI = decltype(end)::value ? CA_END : CA_CODES;
        if (p.t64) launch_instance<&conv_awq_mfma_kernel<WB, WZ, XZ, 64, EPI, ConvAwqFusedArgs>>(blocks, 256, CaGeom<64>::LDS, 0, s, f);
        else launch_instance<&conv_awq_mfma_kernel<WB, WZ, XZ, 128, EPI, ConvAwqFusedArgs>>(blocks, 256, CaGeom<128>::LDS, 0, s, f);
    });
}

// the kernel argument of either entry point from its plan
void fill_conv_awq(ConvAwqArgs &a, const ConvAwqPlan &p, const qe_qparam *x, const qe_qparam *w, const float *bias, int G,
                   const qe_conv_shape *shape, int relu, float *out)
{
    fill_grp_operands(a, x, w, bias, G, shape->IC);
    a.out = out;
    a.N = shape->N; a.IC = shape->IC; a.H = shape->H; a.W = shape->W; a.OC = shape->OC; a.KH = shape->KH; a.KW = shape->KW;
    a.stride = shape->stride; a.padding = shape->padding; a.OH = p.OH; a.OW = p.OW;
    a.P = p.fast ? shape->H * shape->W : 0; a.tiles = p.tiles; a.relu = relu != 0;
}

// A fused request: the code the call returns for it and, when that is QE_OK, the plan the call and the path query read.
struct ConvAwqFusedRequest {
    int rc;
    ConvAwqPlan plan;
};

// The order decides which code a caller sees: the plain entry point's checks, the destinations and the quantiser's
// pointers, its width, its count, the overlaps; then what no kernel serves.
ConvAwqFusedRequest request_conv_awq_fused(const qe_qparam *x, const qe_qparam *w, int G, int x_symmetric, int w_symmetric,
                                           const float *bias, const qe_conv_shape *sh, const float *identity, const float *out,
                                           const qe_requant *rq, const uint8_t *codes, const int32_t *status)
{
    ConvAwqFusedRequest r = {};
    if ((r.rc = check_conv_awq(x, w, G, sh)) != QE_OK) return r;
    r.rc = QE_ERR_ARG;
    if ((out == nullptr && codes == nullptr) || (codes != nullptr) != (rq != nullptr)) return r;
    if (rq != nullptr) {
        if ((r.rc = check_requant(rq)) != QE_OK) return r;
        r.rc = QE_ERR_ARG;
        if (!one_or_per_channel(rq->n_param, sh->OC)) return r;
    }
    r.plan = plan_conv_awq(x, w, G, x_symmetric, w_symmetric, sh, identity != nullptr ? CA_END : CA_CODES, rq);
    const int64_t n_in = (int64_t)sh->N * sh->IC * sh->H * sh->W, n = (int64_t)sh->N * sh->OC * r.plan.OH * r.plan.OW;
    const Span outs[3] = {span_of(out, n * 4), span_of(codes, rq ? qe_packed_nbytes(n, rq->n_bits) : 0), span_of(status, 4)};
    const Span ins[9] = {span_of(x->data, qe_packed_nbytes(n_in, x->n_bits)),
                         span_of(w->data, qe_packed_nbytes((int64_t)sh->OC * sh->IC * sh->KH * sh->KW, w->n_bits)),
                         span_of(x->scale, 4), span_of(x->zero, 4),
                         span_of(w->scale, 4 * (int64_t)w->n_param), span_of(w->zero, 4 * (int64_t)w->n_param),
                         span_of(bias, 4 * (int64_t)sh->OC), span_of(rq ? rq->scale : nullptr, rq ? 4 * (int64_t)rq->n_param : 0),
                         span_of(rq ? rq->zero : nullptr, rq ? 4 * (int64_t)rq->n_param : 0)};
    if (!outputs_clear(outs, 3, ins, 9)) return r;
    // the identity: an operand to codes and status, and to out unless it IS out
    const Span id = span_of(identity, n * 4);
    if (overlaps(outs[1], id) || overlaps(outs[2], id) || (out != nullptr && !same_or_disjoint(out, identity, n * 4))) return r;
    r.rc = r.plan.two_pass && out == nullptr ? QE_ERR_UNSUPPORTED : QE_OK;
    return r;
}

}  // namespace

}  // namespace qe

extern "C" int qe_quantconv2d_awq_path(const qe_qparam *x, const qe_qparam *w, int32_t group_size, int32_t x_symmetric,
                                       int32_t w_symmetric, const qe_conv_shape *shape)
{
    using namespace qe;
    if (check_conv_awq(x, w, group_size, shape) != QE_OK) return 0;
    return plan_conv_awq(x, w, group_size, x_symmetric, w_symmetric, shape).fast;
}

extern "C" int qe_quantconv2d_awq(const qe_qparam *x, const qe_qparam *w, int32_t group_size, int32_t x_symmetric,
                                  int32_t w_symmetric, const float *bias, const qe_conv_shape *shape, int32_t relu, float *out,
                                  qe_stream_t stream)
{
    using namespace qe;
    if (int rc = check_conv_awq(x, w, group_size, shape)) return rc;
    if (out == nullptr) return QE_ERR_ARG;
    const ConvAwqPlan p = plan_conv_awq(x, w, group_size, x_symmetric, w_symmetric, shape);
    ConvAwqArgs a = {};
    fill_conv_awq(a, p, x, w, bias, group_size, shape, relu, out);
    hipStream_t s = static_cast<hipStream_t>(stream);
    return launch_grp<&conv_awq_plain_kernel<>>(p.fast, p.blocks, a, s, [&] {
        dispatch_grp_i8(p.inst, [&](auto wb, auto wz, auto xz) {
            launch_conv_awq<decltype(wb)::value, decltype(wz)::value, decltype(xz)::value>(p, a, s);
        });
    });
}

extern "C" int qe_quantconv2d_awq_fused_path(const qe_qparam *x, const qe_qparam *w, int32_t group_size, int32_t x_symmetric,
                                             int32_t w_symmetric, const qe_conv_shape *shape, const float *identity, int32_t relu,
                                             const float *out, const qe_requant *rq, const uint8_t *codes, const int32_t *status)
{
    (void)relu;                                           // (the ReLU is a runtime select in every kernel)
    const qe::ConvAwqFusedRequest r = qe::request_conv_awq_fused(x, w, group_size, x_symmetric, w_symmetric, nullptr, shape, identity,
                                                                 out, rq, codes, status);
    return r.rc == QE_OK ? r.plan.path : -1;
}

extern "C" int qe_quantconv2d_awq_fused(const qe_qparam *x, const qe_qparam *w, int32_t group_size, int32_t x_symmetric,
                                        int32_t w_symmetric, const float *bias, const qe_conv_shape *shape, const float *identity,
                                        int32_t relu, float *out, const qe_requant *rq, uint8_t *codes, int32_t *status,
                                        qe_stream_t stream)
{
    using namespace qe;
    const ConvAwqFusedRequest r = request_conv_awq_fused(x, w, group_size, x_symmetric, w_symmetric, bias, shape, identity, out, rq,
                                                         codes, status);
    if (r.rc != QE_OK) return r.rc;
    const ConvAwqPlan &p = r.plan;
    ConvAwqFusedArgs f = {};
    fill_conv_awq(f, p, x, w, bias, group_size, shape, relu, out);
    f.identity = identity;
    if (rq != nullptr && !p.two_pass) {
        f.codes = codes; f.status = status; f.rq_per_col = rq->n_param != 1; f.rq = make_qe_rq(*rq);
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rc = launch_grp<&conv_awq_plain_kernel<ConvAwqFusedArgs>>(p.fast, p.blocks, f, s, [&] {
        dispatch_grp_i8(p.inst, [&](auto wb, auto wz, auto xz) {
            launch_conv_awq_fused<decltype(wb)::value, decltype(wz)::value, decltype(xz)::value>(p, f, s);
        });
    });
    if (rc != QE_OK || !p.two_pass) return rc;
    return qe_quantize_pack(out, (int64_t)shape->N * shape->OC * p.OH * p.OW, rq->scale, rq->zero, rq->n_param, (int64_t)p.OH * p.OW,
                            rq->qmin, rq->qmax, rq->n_bits, rq->sign, codes, status, stream);
}
