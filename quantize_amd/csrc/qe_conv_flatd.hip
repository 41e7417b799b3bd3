// qe_conv_flatd.hip -- 1x1 / stride 1 / pad 0 quantconv2d as a GEMM whose operand stages arrive by LDS-DMA ("flatd").
//
// Replaces the per-element loop of quantconv2d_cuda_kernel (engine/kernels/functions/quantconv2d.cu:78-141) for
// 8-bit x 8-bit 1x1 layers with IC % 64 == 0.  Same arithmetic as conv_mfma_flat_kernel (qe_conv_mfma_kernel.hpp):
//   out[n,oc,p] = bias[oc] + sx sw[oc] ( S_aw - zw' S_x - zx' S_w + IC zx' zw' ),  a = u ^ 0x80, S_aw on
//   v_mfma_i32_32x32x32_i8 with A = activations (rows = pixels, fragments by ds_read_b64_tr_b8 from the native
//   [channel][pixel] order), B = weights (cols = output channel, 16 contiguous bytes of the packed OIHW row).
// What differs is how the operands reach LDS.  The register-staged flat kernel keeps ONE stage of loads in flight per
// workgroup (its staging registers), and a layer with a long K loop and small planes (1024->256 @14x14, 2048->512 @7x7)
// pays one memory round trip per stage: 2.8 TB/s and 1.0 TB/s in the ResNet-50 stack, bound by neither HBM nor MFMA.
// This kernel serves the 7x7 planes (2048->512 and 512->2048 in the last stage); on larger planes it tied or lost against the
// register-staged kernels.
// Here both operands of a 64-channel stage are written into a ring of 3 LDS buffers by global_load_lds_dwordx4 (no
// staging registers, nothing to transpose or convert on the way), two stages ahead of the MFMAs, with one raw
// s_barrier and a counted vmcnt per stage (a __syncthreads() would drain the DMA queue).  The u ^ 0x80 recode moves to
// the fragments.
//
// LDS image of the activations = what ds_read_b64_tr_b8 wants: rows = channels, 16-pixel groups at 8-byte aligned
// addresses, row stride an odd multiple of 32 B (conflict-free).  LDS-DMA writes lane-linear 16-byte slots, but the
// GLOBAL address is per lane, so slot (channel c, j) simply fetches plane bytes [16 j, 16 j + 16) of channel c.  A tile is
// 4 whole images x 2 column tiles: 64-byte rows [image][channel][64], byte-aligned sources (LDS-DMA takes any source
// alignment: tools/probe_dma_align.hip), slot position XOR 2 for channels with bit 2 set so that the 8 rows x 2 pixel
// groups of a transposed read cover all 64 banks once.
// The only bytes such slots could read past the tensor are those behind the LAST plane of the LAST image when the plane
// size is not a multiple of 16: pure-garbage slots fetch the tensor's last 16 bytes instead, and the one slot that is
// partly valid is left out of the DMA (lane masked off) and written by its thread from a register.
#include "qe_conv_common.hpp"
#include "qe_conv_plan.hpp"

#include <utility>

namespace qe {

struct FlatdArgs {
    const uint8_t *x;          // [N][IC][P] stored codes, 8-bit
    const uint8_t *w;          // [OC][IC] stored codes, 8-bit
    const float *x_scale, *x_zero, *w_scale, *w_zero, *bias;
    int x_sign, w_sign, w_per_tensor;
    float *out;                // [N][OC][P] fp32
    int N, IC, OC, P;
    int tiles_per_image;       // unused (a tile is 4 whole images)
    int n_pix_tiles, n_oc_tiles, chunk;
    RqArgs rq;                 // fused re-quantisation (7x7 planes, RQ instances): the 8-bit code of the consumer's quantiser instead of fp32
};

constexpr int FD_RING_DEFAULT = 3;      // slots of the ring (RING - 1 stages in flight); 6 = one workgroup per CU with 5 in flight
// output channels per workgroup = 32 per wave: 4 waves (128 channels, two workgroups per CU) or 8 waves (256 channels, one
// workgroup per CU: the activations of a pixel tile cross the CU's memory path once per 256 output channels instead of
// once per 128 -- the bytes that bound these layers)

template <int RING = FD_RING_DEFAULT, int WAVES = 4> struct FdGeom {
    static constexpr int MT = 32 * WAVES;
    static constexpr int THREADS = 64 * WAVES;
    static constexpr int FD_WBYTES = MT * FD_CK;
    static constexpr int NT = 8;                                     // column tiles: 4 images x 2
    static constexpr int XBYTES = 4 * FD_CK * 64;                    // [image][channel][64 bytes]
    static constexpr int STAGE = XBYTES + FD_WBYTES;
    static constexpr int XINSTR = XBYTES / 1024;                     // wave-level DMA instructions per stage
    static constexpr int NTP = 32 * NT;
    static constexpr int PATCH = WAVES * 32 * 49 * 4;
    static constexpr int RING_BYTES = RING * STAGE > PATCH ? RING * STAGE : PATCH;
    static constexpr int LDS = RING_BYTES + WAVES * NTP * 4 /* S_x, one copy per wave */;
};

// ---------------------------------------------------------------------------------------------
// LDS reads as inline asm.  hipcc (ROCm 7.2) puts `s_waitcnt vmcnt(0)` in front of every transposed-read builtin (and of
// any plain LDS store) that follows an LDS-DMA: their memory operands carry no alias information, so the wait-count
// pass assumes they touch what the DMA writes -- which drained the stages in flight once per stage.  The ring protocol
// (counted vmcnt + barrier) already orders these accesses behind the DMA that fills their slot, so they are written by
// hand.  Rule kept throughout: an asm statement's outputs are VALID when the statement ends (the reads and their
// `s_waitcnt lgkmcnt(0)` live in ONE statement).  Leaving the wait to a later statement is not safe: hipcc may copy an
// output register right behind the statement that declares it, i.e. before the data has arrived (seen: v_mov of
// not-yet-loaded patch rows -> garbage in rows 16-31 of every tile).
// ---------------------------------------------------------------------------------------------
// all fragment reads of one 32-channel chunk: weight fragment + 8 x (8 + 8 channels) transposed reads.  Column tile T =
// image T / 2 (4096 bytes apart), column tile T % 2 (slot position differs by XOR 2: second base)
__device__ __forceinline__ void fd_reads_small(uint32_t tr_addr0, uint32_t tr_addr1, uint32_t wf_addr, v4i &wf, v2i (&lo)[8], v2i (&hi)[8])
{
    asm volatile(
        "ds_read_b128 %0, %19\n\t"
        "ds_read_b64_tr_b8 %1, %17 offset:0\n\t"
        "ds_read_b64_tr_b8 %9, %17 offset:512\n\t"
        "ds_read_b64_tr_b8 %2, %18 offset:0\n\t"
        "ds_read_b64_tr_b8 %10, %18 offset:512\n\t"
        "ds_read_b64_tr_b8 %3, %17 offset:4096\n\t"
        "ds_read_b64_tr_b8 %11, %17 offset:4608\n\t"
        "ds_read_b64_tr_b8 %4, %18 offset:4096\n\t"
        "ds_read_b64_tr_b8 %12, %18 offset:4608\n\t"
        "ds_read_b64_tr_b8 %5, %17 offset:8192\n\t"
        "ds_read_b64_tr_b8 %13, %17 offset:8704\n\t"
        "ds_read_b64_tr_b8 %6, %18 offset:8192\n\t"
        "ds_read_b64_tr_b8 %14, %18 offset:8704\n\t"
        "ds_read_b64_tr_b8 %7, %17 offset:12288\n\t"
        "ds_read_b64_tr_b8 %15, %17 offset:12800\n\t"
        "ds_read_b64_tr_b8 %8, %18 offset:12288\n\t"
        "ds_read_b64_tr_b8 %16, %18 offset:12800\n\t"
        "s_waitcnt lgkmcnt(0)"
        : "=&v"(wf), "=&v"(lo[0]), "=&v"(lo[1]), "=&v"(lo[2]), "=&v"(lo[3]), "=&v"(lo[4]), "=&v"(lo[5]), "=&v"(lo[6]), "=&v"(lo[7]), "=&v"(hi[0]), "=&v"(hi[1]), "=&v"(hi[2]), "=&v"(hi[3]), "=&v"(hi[4]), "=&v"(hi[5]), "=&v"(hi[6]), "=&v"(hi[7])
        : "v"(tr_addr0), "v"(tr_addr1), "v"(wf_addr));
}
// the 4 row groups of a wave's 32 x 36 float store patch (8 rows = 1152 bytes apart)
__device__ __forceinline__ void fd_patch_read4(uint32_t addr, v4i &o0, v4i &o1, v4i &o2, v4i &o3)
{
    asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:1152\n\tds_read_b128 %2, %4 offset:2304\n\t"
                 "ds_read_b128 %3, %4 offset:3456\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(o0), "=&v"(o1), "=&v"(o2), "=&v"(o3) : "v"(addr) : "memory");
}
__device__ __forceinline__ void fd_patch_write(uint32_t lds_addr, float a, float b, float c, float d)
{
    const v4i v = {__float_as_int(a), __float_as_int(b), __float_as_int(c), __float_as_int(d)};
    asm volatile("ds_write_b128 %0, %1" : : "v"(lds_addr), "v"(v) : "memory");
}
__device__ __forceinline__ void fd_lds_drain() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

__device__ __forceinline__ void fd_wait_vmcnt(int n)   // n wave-uniform, 0..31
{
#define QE_VMW(k) case k: __builtin_amdgcn_s_waitcnt(0x0f70 | ((k) & 15) | (((k) >> 4) << 14)); break;
    switch (n) {
        QE_VMW(0) QE_VMW(1) QE_VMW(2) QE_VMW(3) QE_VMW(4) QE_VMW(5) QE_VMW(6) QE_VMW(7) QE_VMW(8) QE_VMW(9) QE_VMW(10)
        QE_VMW(11) QE_VMW(12) QE_VMW(13) QE_VMW(14) QE_VMW(15) QE_VMW(16) QE_VMW(17) QE_VMW(18) QE_VMW(19) QE_VMW(20)
        QE_VMW(21) QE_VMW(22) QE_VMW(23) QE_VMW(24) QE_VMW(25) QE_VMW(26) QE_VMW(27) QE_VMW(28) QE_VMW(29) QE_VMW(30)
        default: __builtin_amdgcn_s_waitcnt(0x0f70); break;
    }
#undef QE_VMW
}

template <int FD_RING, int WAVES, bool RQ = false>
__global__ __launch_bounds__(64 * WAVES, 2) void conv_flatd_kernel(const FlatdArgs a)
{
    using G = FdGeom<FD_RING, WAVES>;
    constexpr int AHEAD = FD_RING - 1;
    constexpr int FD_MT = G::MT, THREADS = G::THREADS;
    constexpr int NT = G::NT;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 31, h = lane >> 5;
    const int P = a.P;

    // ---- tile decode: XCD-aware block map (same scheme as block_to_tile of the register-staged kernels) -------
    int pt, ot;
    {
        const int bid = blockIdx.x;
        const int idx = bid >> 3;
        const int j = idx / a.n_oc_tiles;
        ot = idx - j * a.n_oc_tiles;
        const int c = j / a.chunk;
        pt = (c * 8 + (bid & 7)) * a.chunk + (j - c * a.chunk);
    }
    if (pt >= a.n_pix_tiles) return;
    const int n0 = pt * 4;

    // ---- epilogue constants of this lane's output channel ------------------------------------------------------
    const int oc = ot * FD_MT + wave * 32 + col;
    const int occ = oc < a.OC ? oc : a.OC - 1;
    const float sw = a.w_per_tensor ? a.w_scale[0] : a.w_scale[occ];
    const float zwp = (a.w_per_tensor ? a.w_zero[0] : a.w_zero[occ]) - (a.w_sign ? 0.0f : 128.0f);
    const float alpha = a.x_scale[0] * sw;
    const float bia = a.bias ? a.bias[occ] : 0.0f;
    const float zxp = a.x_zero[0] - (a.x_sign ? 0.0f : 128.0f);

    // ---- DMA sources (stage 0; a stage advances X by 64 planes and W by 64 bytes) ------------------------------
    // X: LDS slot e = 64 * (wave-instruction q) + lane, q = wave, wave + 4, ...
    constexpr int PXW = (G::XINSTR + WAVES - 1) / WAVES;   // X instructions of waves 0 .. (XINSTR % WAVES) - 1 (the others issue one less)
    const int n_xi = (G::XINSTR % WAVES == 0 || wave < G::XINSTR % WAVES) ? PXW : PXW - 1;
    const int64_t x_last16 = (int64_t)a.N * a.IC * P - 16;      // last address a 16-byte read may start at
    const uint8_t *px[PXW];
    int fix_lds = -1, fix_i = -1;                      // this thread writes the tensor's last bytes itself (last stage only)
    uint32_t fix_val = 0;
#pragma unroll
    for (int i = 0; i < PXW; ++i) {
        const int e = 64 * (wave + WAVES * i) + lane;
        const int img = e >> 8, c = (e >> 2) & 63;
        const int j = (e & 3) ^ (2 * ((c >> 2) & 1));
        const int n = n0 + img < a.N ? n0 + img : a.N - 1;
        int64_t src = ((int64_t)n * a.IC + c) * P + 16 * j;
        const bool last_row = (n0 + img == a.N - 1) && c == FD_CK - 1;
        const bool pad = n0 + img >= a.N;                  // an image past the batch in its last tile: computed, never stored
        // stage s adds s * 64 planes: only the last stage of the last image can run past the tensor
        const int64_t lim = x_last16 - (int64_t)(a.IC - FD_CK) * P;
        if (pad) {
            src = lim;      // its slots would repeat the last image's, whose last plane runs up to 15 bytes past the tensor
        } else if (last_row && src > lim) {
            const int pos = 16 * j;                                // first plane byte this slot should hold
            if (pos < P && e < G::XBYTES / 16) {
                // partly valid (P - pos = 4 or 1 bytes): in the last stage this lane is masked out of the DMA (see
                // issue()) and stores the valid bytes itself; in every earlier stage the slot is an ordinary in-bounds
                // read, so its address stays as it is
                fix_lds = e * 16;
                fix_i = i;
                uint32_t v = 0;
                const uint8_t *tail = a.x + (int64_t)a.N * a.IC * P - (P - pos);
                for (int b = 0; b < 4 && b < P - pos; ++b) v |= (uint32_t)tail[b] << (8 * b);
                fix_val = v;
            } else {
                src = lim;                                         // pure garbage slot: any valid 16 bytes will do, in every stage
            }
        }
        px[i] = a.x + src;
    }
    // W: slot e = tid + 256 i <-> row e >> 2 of the tile, position e & 3 holds k-piece (e & 3) ^ ((row >> 2) & 3)
    const uint8_t *pw[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int e = tid + THREADS * i;
        const int r = e >> 2, sl = e & 3;
        const int orow = ot * FD_MT + r < a.OC ? ot * FD_MT + r : a.OC - 1;
        pw[i] = a.w + (int64_t)orow * a.IC + 16 * (sl ^ ((r >> 2) & 3));
    }
    const int64_t x_step = (int64_t)FD_CK * P;
    const int n_stages = a.IC / FD_CK;
    auto issue = [&](int s) __attribute__((always_inline)) {
        uint8_t *buf = smem + (s % FD_RING) * G::STAGE;
        // the one slot that would read past the tensor (last stage of the last plane) is left out of the DMA: its lane is
        // masked off and writes the valid bytes with a plain LDS store before the stage's barrier (a store issued after
        // `s_waitcnt vmcnt(0)` on top of a DMA'd slot was observed to lose against the DMA's own LDS write)
        const int skip = (s == n_stages - 1) ? fix_i : -1;
#pragma unroll
        for (int i = 0; i < PXW; ++i) {
            if (i < n_xi && i != skip)    // first term wave-uniform, second per lane (EXEC mask)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(px[i] + s * x_step),
                                                 (__attribute__((address_space(3))) void *)(buf + 1024 * (wave + WAVES * i)), 16, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(pw[i] + s * FD_CK),
                                             (__attribute__((address_space(3))) void *)(buf + G::XBYTES + (THREADS * i + 64 * wave) * 16), 16, 0, 0);
    };

    for (int s0 = 0; s0 < AHEAD && s0 < n_stages; ++s0) issue(s0);

    // S_x (per-pixel channel sums) is only needed by output channels with zw' != 0: decided per WAVE (its 32 channels),
    // so the prologue needs no workgroup barrier (a __syncthreads() here would drain the two stages just requested)
    const bool need_sx = __builtin_amdgcn_ballot_w64(oc < a.OC && zwp != 0.0f) != 0ull;
    int *sxp = reinterpret_cast<int *>(smem + G::RING_BYTES) + wave * G::NTP;

    v16i acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0;
    int swacc = 0;
    int sxacc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) sxacc[t] = 0;

    // fragment addressing (32-bit LDS byte addresses for the hand-written transposed reads)
    const int i16 = lane & 15;
    const uint32_t smem_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t *)smem;
    // row (16 h + i16/2) of [image][channel][64]; logical slot 2 tt + (lane>>4)&1 sits at position slot ^ 2 for rows 4-7
    const int sm_sl = ((lane >> 4) & 1) ^ (2 * (i16 >> 3));
    const uint32_t rowb = (uint32_t)((16 * h + (i16 >> 1)) * 64 + 8 * (i16 & 1));
    const uint32_t tr_b0 = rowb + 16u * (uint32_t)sm_sl;
    const uint32_t tr_b1 = rowb + 16u * (uint32_t)(sm_sl ^ 2);
    const int wf_base = G::XBYTES + (wave * 32 + col) * FD_CK;
    const int wswz = (col >> 2) & 3;

    auto main_loop = [&](auto sx_tag) __attribute__((always_inline)) {
        constexpr bool SX = decltype(sx_tag)::value;
        for (int s = 0; s < n_stages; ++s) {
            // stage s has landed for this wave once at most the pieces of stage s + 1 are still outstanding
            if (s + 1 < n_stages) {
                const int rem = (AHEAD - 1) < (n_stages - 1 - s) ? (AHEAD - 1) : (n_stages - 1 - s);   // younger stages in flight
                fd_wait_vmcnt(rem * (n_xi + 2));
            } else {
                __builtin_amdgcn_s_waitcnt(0x0f70);
                if (fix_lds >= 0) {
                    uint8_t *dst = smem + (s % FD_RING) * G::STAGE + fix_lds;
                    *dst = (uint8_t)fix_val;
                    __builtin_amdgcn_s_waitcnt(0xc07f);
                }
            }
            __builtin_amdgcn_s_barrier();             // ... for every wave; and ring slot (s + 2) % 3 has no reader left
            if (s + AHEAD < n_stages) issue(s + AHEAD);
            // per 32-channel chunk: one asm statement = weight fragment + every activation fragment + their wait
            const uint32_t xb = smem_lds + (uint32_t)((s % FD_RING) * G::STAGE);
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                v2i lo[NT], hi[NT];
                v4i wf;
                const uint32_t wfa = xb + (uint32_t)(wf_base + 16 * ((2 * k + h) ^ wswz));
                fd_reads_small(xb + tr_b0 + k * 32 * 64, xb + tr_b1 + k * 32 * 64, wfa, wf, lo, hi);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    wf[j] ^= (int)0x80808080;         // u - 128: signed q, or unsigned q - 128
                    swacc = __builtin_amdgcn_sdot4(wf[j], 0x01010101, swacc, false);
                }
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    v4i xf = {lo[t][0], lo[t][1], hi[t][0], hi[t][1]};
#pragma unroll
                    for (int j = 0; j < 4; ++j) xf[j] ^= (int)0x80808080;
                    if constexpr (SX) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) sxacc[t] = __builtin_amdgcn_sdot4(xf[j], 0x01010101, sxacc[t], false);
                    }
                    acc[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(xf, wf, acc[t], 0, 0, 0);
                }
            }
        }
    };
    if (need_sx) main_loop(std::true_type{}); else main_loop(std::false_type{});

    // ---- epilogue ------------------------------------------------------------------------------------------------
    const int sw_sum = swacc + __shfl_xor(swacc, 32);
    const float cst = fmaf((float)a.IC * zxp, zwp, -zxp * (float)sw_sum);
    if (need_sx) {
        // S_x lives on the lane that owns the pixel as an A row; the accumulators have the pixel on the register:
        // through this wave's own LDS copy (written and read by the same wave)
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int v = sxacc[t] + __shfl_xor(sxacc[t], 32);
            if (h == 0) sxp[32 * t + col] = v;
        }
    }
    __syncthreads();          // every wave is done with the ring (it becomes the store patches)
    if constexpr (RQ) {
        // fused re-quantisation: a wave's 32 channels x 49 codes of one image are ONE contiguous 1,568-byte run of the output
        // (16-byte aligned: oc0 % 32 == 0 and OC % 32 == 0, host) -- laid out in the patch as in memory, copied flat.  The
        // fp32 value is computed exactly as below, then quantised as quantize_pack would (rq_value / rq_fast2).
        uint8_t *bp = smem + wave * (32 * 49 * 4);
        const int oc0 = ot * FD_MT + wave * 32;
        RqConst rqc = rq_setup(a.rq);
        rqc.slow = __builtin_amdgcn_readfirstlane(rqc.slow);
        rqc.chk = __builtin_amdgcn_readfirstlane(rqc.chk);
        bool bad = false;
        const bool fast = rq_fast_ok(rqc) && __builtin_amdgcn_ballot_w64(!rq_bounded(alpha, cst, bia, zwp)) == 0ull;
#pragma unroll
        for (int gi = 0; gi < 4; ++gi) {
            const bool img = n0 + gi < a.N;
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
                    const int pxl = 32 * tt + (r & 3) + 8 * (r >> 2) + 4 * h;      // r even: pxl, pxl + 1 are registers r, r + 1
                    float f0 = (float)acc[2 * gi + tt][r] + cst, f1 = (float)acc[2 * gi + tt][r + 1] + cst;
                    if (need_sx) {
                        f0 = fmaf(-zwp, (float)sxp[64 * gi + pxl], f0);
                        f1 = fmaf(-zwp, (float)sxp[64 * gi + pxl + 1], f1);
                    }
                    const float y0 = fmaf(alpha, f0, bia), y1 = fmaf(alpha, f1, bia);
                    float c0, c1;
                    if (fast) {
                        const v2f c2 = rq_fast2(rqc, v2f{y0, y1});
                        c0 = c2.x; c1 = c2.y;
                    } else {
                        bool b0 = false, b1 = false;
                        c0 = rq_value(rqc, y0, b0);
                        c1 = rq_value(rqc, y1, b1);
                        bad |= img && oc < a.OC && ((b0 && pxl < P) || (b1 && pxl + 1 < P));
                    }
                    if (pxl < P) bp[col * P + pxl] = (uint8_t)(unsigned)c0;
                    if (pxl + 1 < P) bp[col * P + pxl + 1] = (uint8_t)(unsigned)c1;
                }
            }
            if (img && oc0 + 32 <= a.OC) {
                uint8_t *dst = a.rq.out + ((int64_t)(n0 + gi) * a.OC + oc0) * P;
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const uint4 d4 = *reinterpret_cast<const uint4 *>(bp + 16 * (64 * k + lane));
                    if (64 * k + lane < 98) *reinterpret_cast<uint4 *>(dst + 16 * (64 * k + lane)) = d4;
                }
            }
        }
        rq_report(a.rq, bad);
    } else {
        // a wave's 32 channels x P pixels of one image are ONE contiguous, 16-byte aligned run of the output
        // ((n OC + oc0) P floats, oc0 % 32 == 0, OC % 4 == 0): the patch is laid out exactly like it and copied flat.
        float *patch = reinterpret_cast<float *>(smem) + wave * (32 * 49);
        const int oc0 = ot * FD_MT + wave * 32;
        const int vrows = min(32, a.OC - oc0);                    // <= 0: nothing to store
        const int nfl = vrows > 0 ? vrows * P : 0;                // floats of the run
        const bool vec_ok = (reinterpret_cast<uintptr_t>(a.out) & 15) == 0;
#pragma unroll
        for (int gi = 0; gi < 4; ++gi) {
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int pxl = 32 * tt + (r & 3) + 8 * (r >> 2) + 4 * h;
                    float f = (float)acc[2 * gi + tt][r] + cst;
                    if (need_sx) f = fmaf(-zwp, (float)sxp[64 * gi + pxl], f);
                    if (pxl < P) patch[col * P + pxl] = fmaf(alpha, f, bia);
                }
            }
            __builtin_amdgcn_s_waitcnt(0xc07f);
            if (n0 + gi < a.N) {
                float *dst = a.out + ((int64_t)(n0 + gi) * a.OC + oc0) * P;
                for (int i = lane; 4 * i < nfl; i += 64) {
                    if (vec_ok && 4 * i + 4 <= nfl) *reinterpret_cast<float4 *>(dst + 4 * i) = *reinterpret_cast<const float4 *>(patch + 4 * i);
                    else for (int b = 4 * i; b < nfl && b < 4 * i + 4; ++b) dst[b] = patch[b];
                }
            }
            __builtin_amdgcn_s_waitcnt(0xc07f);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
template <int WV, bool RQ>
static void launch_fd(const FlatdArgs &a, int64_t blocks, hipStream_t s)
{
    launch_instance<&conv_flatd_kernel<3, WV, RQ>>((unsigned)blocks, 64 * WV, FdGeom<3, WV>::LDS, FdGeom<3, WV>::LDS, s, a);
}

// p.route == Flatd: 8-wave workgroups when p.fd_w8; rq != nullptr: the re-quantising instances
int launch_flatd(const ConvPlan &p, const qe_qparam *x, const qe_qparam *w, const float *bias, float *out, hipStream_t s,
                 const qe_requant *rq, uint8_t *codes, int32_t *status)
{
    const qe_conv_shape *sh = &p.run;
    FlatdArgs a;
    a.rq = make_rq_args(rq, codes, status);
    a.x = static_cast<const uint8_t *>(x->data); a.w = static_cast<const uint8_t *>(w->data);
    a.x_scale = x->scale; a.x_zero = x->zero; a.w_scale = w->scale; a.w_zero = w->zero; a.bias = bias;
    a.x_sign = x->sign; a.w_sign = w->sign; a.w_per_tensor = (w->n_param == 1);
    a.out = out; a.N = sh->N; a.IC = sh->IC; a.OC = sh->OC; a.P = sh->H * sh->W;
    a.n_oc_tiles = p.n_oc_tiles;
    a.tiles_per_image = p.tiles_h;
    a.n_pix_tiles = p.n_pix_tiles;
    a.chunk = p.chunk;
    const int64_t blocks = p.blocks;
    // ring depth 3 = two stages in flight, two workgroups per CU.  A 6-slot ring (one workgroup per CU, five stages in flight)
    // was 25-60 % slower on every layer (profiles/r02i_flatd_ring.txt): the K loop is not bound by prefetch depth.
    if (rq != nullptr) {
        if (p.fd_w8) launch_fd<8, true>(a, blocks, s); else launch_fd<4, true>(a, blocks, s);
    } else {
        if (p.fd_w8) launch_fd<8, false>(a, blocks, s); else launch_fd<4, false>(a, blocks, s);
    }
    QE_LAUNCH_CHECK();
    return QE_OK;
}

}  // namespace qe
