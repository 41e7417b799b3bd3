// qe_conv_common.hpp -- what the packed-activation convolution routes share (the MFMA families of qe_conv_mfma_kernel.hpp,
// the resident-tile kernels of qe_conv_pwr.hip, the LDS-DMA ring of qe_conv_flatd.hip, the float-input kernels of
// qe_conv_f32.hip and the planner): the XCD-aware tile map, the fused output quantiser and the small shared definitions.
#pragma once
#include "qe_common.h"

#include <algorithm>
#include <cstdlib>

namespace qe {

typedef int v2i __attribute__((ext_vector_type(2)));
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

constexpr int MF_THREADS = 256;
constexpr int MF_UNITS = 2;        // staging units (16 ch x 4 px) per thread per chunk
constexpr int MF_TRASH = 64;       // per-lane LDS slots that swallow masked-off staging writes
constexpr int MF_MAX_LDS = 64 * 1024;
constexpr int MF_MAX_LDS_SM2 = 80 * 1024;   // sm2 kernel: 2 workgroups per CU x 80 KB = the CU's 160 KB

struct MfmaArgs;                         // qe_conv_mfma_kernel.hpp
typedef void (*MfmaLaunch)(const MfmaArgs &a, unsigned blocks, size_t lds, hipStream_t s);   // one MFMA-family instance

extern unsigned long long *g_mfma_dbg;   // qe_conv_mfma.hip: stamp buffer of -DQE_STAMP diagnostic builds

// ---- tile map ---------------------------------------------------------------------------------------------------------
// XCD-aware block map shared by every route: blocks b and b+8 share an XCD (and its L2); the workgroups of one pixel tile
// (its oc tiles or channel groups) get ids that differ by multiples of 8 so they read the same activations from one L2.
// XCD x = bid & 7 takes runs of `chunk` consecutive pixel tiles (all their workgroups), run r of the XCD being global run
// 8*r + x.  chunk = 1 interleaves neighbouring tiles over the XCDs; a chunk of one or more whole images keeps the lines an
// L2 has in flight contiguous in memory, which the write-bound layers need (tools/probe_store_pattern2.hip: 4.2 -> 4.9 TB/s
// store-only at 28x28, 5.5 -> 5.8 at 56x56).
//
// tile_grid is the host half: the grid that the kernels' decode assumes.  The device half is
//     idx = bid >> 3; j = idx / per_tile; sub = idx - j * per_tile; c = j / chunk;
//     pt = (c * 8 + (bid & 7)) * chunk + (j - c * chunk);        (pt may lie past the last tile: the kernel tests)
// in block_to_tile (qe_conv_mfma_kernel.hpp) and written out in the pwr, flatd and float-input kernels: routed through one
// shared inline function the compiler orders the same arithmetic differently in those kernels, and their instruction
// streams are kept as measured.  The two halves must agree.
//
// Default: each XCD owns one contiguous eighth of the pixel tiles (sum over the ResNet-50 layers 4.13 -> 4.07 ms against
// single-tile interleaving); with `knob_ok`, QE_CHUNK_IMAGES = k overrides with runs of k images (0: single tiles).
// Returns the grid: whole rounds of 8 runs, times `per_tile` workgroups per pixel tile.
inline int64_t tile_grid(int64_t n_units, int per_image, int64_t per_tile, bool knob_ok, int &chunk)
{
    const int64_t per_xcd = (n_units + 7) / 8;
    const char *e = knob_ok ? env_get("QE_CHUNK_IMAGES") : nullptr;
    const int64_t k = knob_ok ? (int64_t)(e ? atoi(e) : 1 << 20) * per_image : per_xcd;
    chunk = (int)std::max<int64_t>(1, std::min<int64_t>(per_xcd, k));
    const int64_t runs = (n_units + chunk - 1) / chunk;
    return (runs + 7) / 8 * chunk * 8 * per_tile;
}

// ---- fused output quantiser -------------------------------------------------------------------------------------------
// kernel operand (qe_quantconv2d_requant): out != nullptr -> the epilogue stores the 8-bit code of
// round(y / scale - zero).clamp(qmin, qmax) (1 byte per element, NCHW) instead of the fp32 y
struct RqArgs {
    uint8_t *out;
    const float *scale, *zero;         // per tensor (the consumer's activation quantiser; its conv wants one scale anyway)
    float qmin, qmax, lo, hi;          // clamp of the quantiser; representable range of the code (tpack's range test)
    unsigned offset;                   // stored code = (q + offset) & 0xff (tpack.cu:108-111)
    int32_t *status;                   // bit 0 set when a value fails the range test (NaN, or qmin/qmax outside the code range)
};

// from the C ABI's operand: the 8-bit codes of rq into `codes`, the range flag into `status`; rq or codes NULL: no codes
inline RqArgs make_rq_args(const qe_requant *rq, uint8_t *codes, int32_t *status)
{
    RqArgs a;
    a.out = nullptr; a.scale = nullptr; a.zero = nullptr; a.status = nullptr;
    a.qmin = a.qmax = a.lo = a.hi = 0.0f; a.offset = 0;
    if (rq != nullptr && codes != nullptr) {
        const CodeRange cr = code_range(8, rq->sign);          // the epilogues store whole bytes
        a.out = codes; a.scale = rq->scale; a.zero = rq->zero;
        a.qmin = rq->qmin; a.qmax = rq->qmax; a.status = status;
        a.offset = cr.offset; a.lo = cr.lo; a.hi = cr.hi;
    }
    return a;
}

// y -> stored 8-bit code with the arithmetic of the fused quantise+pack kernel (qe_tpack.hip tp_quantize + tp_code):
//   r = rint(y / scale - zero) ; clamp to [qmin, qmax] ; code = (int(r) + offset) & 0xff ; flag when r is NaN or outside the
// code range.  An IEEE division per output element (~10 VALU instructions) made the fused epilogue SLOWER than storing fp32
// (4.84 vs 4.17 ms per step), so the quotient comes from Markstein's sequence on a reciprocal taken once per thread:
//   q0 = y * rcp ; e = fma(-scale, q0, y) ; q = fma(e, rcp, q0)
// which IS the correctly rounded y / scale whenever rcp = RN(1 / scale), the significand of scale is not all ones and
// nothing over- or underflows (Markstein 1990; Cornea et al., "Scientific computing on Itanium", thm. 8.3).  y is first
// clamped to +-B with B / |scale| beyond the clamp bounds, which changes no code and keeps infinities out of the fma;
// tiny quotients (where the sequence could round differently) cannot reach a rounding boundary of q - zero.  Scales
// outside those conditions take the division (`slow`, uniform).  When the status flag comes back set the codes are
// unspecified (the reference raises "out of range" there).
struct RqConst {
    float sc, rcp, nsc, zr, qmin, qmax, offf, B, lo, hi;
    bool slow, chk;
};
__device__ __forceinline__ RqConst rq_setup(const RqArgs &a)
{
    RqConst c;
    c.sc = a.scale[0];
    c.zr = a.zero[0];
    c.rcp = 1.0f / c.sc;
    c.nsc = -c.sc;
    c.qmin = a.qmin; c.qmax = a.qmax; c.lo = a.lo; c.hi = a.hi;
    c.offf = (float)a.offset;
    const float asc = fabsf(c.sc);
    const float span = fmaxf(fabsf(c.qmin), fabsf(c.qmax)) + fabsf(c.zr) + 2.0f;
    c.B = asc * span * 2.0f;
    c.slow = !(asc >= 0x1p-60f && asc <= 0x1p60f) || (__float_as_uint(c.sc) & 0x7fffffu) == 0x7fffffu || !(span <= 0x1p30f) ||
             !(c.qmin <= c.qmax);
    c.chk = !(c.qmin >= c.lo && c.qmax <= c.hi);          // clamp bounds inside the code range: only NaN can fail the range test
    return c;
}
// returns r + offset as a float (0 .. 255 whenever the range test passes)
__device__ __forceinline__ float rq_value(const RqConst &c, float v, bool &bad)
{
    float r;
    if (c.slow) {
        r = rintf(v / c.sc - c.zr);
        r = (r != r) ? r : fminf(fmaxf(r, c.qmin), c.qmax);
        bad |= !(r >= c.lo && r <= c.hi);
    } else {
        bad |= (v != v);
        const float vc = __builtin_amdgcn_fmed3f(v, -c.B, c.B);
        const float q0 = vc * c.rcp;
        const float e = fmaf(c.nsc, q0, vc);
        const float q = fmaf(e, c.rcp, q0);
        r = __builtin_amdgcn_fmed3f(rintf(q - c.zr), c.qmin, c.qmax);
        if (c.chk) bad |= !(r >= c.lo && r <= c.hi);
    }
    return r + c.offf;
}
// Two values per instruction where the ISA has packed fp32 (v_pk_mul_f32, v_pk_fma_f32, v_pk_add_f32: 7.5 instead of 13 VALU
// instructions per output element; the fused epilogue is VALU-bound: 2.8 G elements per batch-256 ResNet-50 step).  Valid
// when rq_fast_ok(c) and the caller has bounded its own constants so that y is finite and |y| <= 2^52 (rq_bounded): then
// no NaN and no overflow can occur anywhere in the sequence, the +-B clamp of rq_value is the identity wherever it matters
// (beyond B the code is the clamp bound either way) and no range flag can be raised -- the same codes as rq_value.
typedef float v2f __attribute__((ext_vector_type(2)));
__device__ __forceinline__ bool rq_fast_ok(const RqConst &c) { return !c.slow && !c.chk; }
// |alpha| <= 2^10, |cst| <= 2^40, |bias| <= 2^50, |zw'| <= 2^20: y = fma(alpha, acc + cst - zw' S_x, bias) stays below 2^52
__device__ __forceinline__ bool rq_bounded(float alpha, float cst, float bias, float zwp)
{
    return fabsf(alpha) <= 0x1p10f && fabsf(cst) <= 0x1p40f && fabsf(bias) <= 0x1p50f && fabsf(zwp) <= 0x1p20f;
}
__device__ __forceinline__ v2f rq_fast2(const RqConst &c, v2f y)
{
#pragma clang fp contract(off)
    const v2f rcp = {c.rcp, c.rcp}, nsc = {c.nsc, c.nsc}, zr = {c.zr, c.zr}, off = {c.offf, c.offf};
    const v2f q0 = y * rcp;
    const v2f e = __builtin_elementwise_fma(nsc, q0, y);
    const v2f q = __builtin_elementwise_fma(e, rcp, q0);
    const v2f d = q - zr;
    v2f r;
    r.x = __builtin_amdgcn_fmed3f(rintf(d.x), c.qmin, c.qmax);
    r.y = __builtin_amdgcn_fmed3f(rintf(d.y), c.qmin, c.qmax);
    return r + off;
}
__device__ __forceinline__ void rq_report(const RqArgs &a, bool bad)
{
    if (__builtin_amdgcn_ballot_w64(bad) != 0 && (threadIdx.x & 63) == 0 && a.status != nullptr) atomicOr(a.status, 1);
}

// stored code u -> MFMA operand a = q - d = u - c, c = off (signed) | 128 (unsigned 8-bit) | 0
__host__ __device__ __forceinline__ int code_bias(int n_bits, int sign)
{
    return sign ? (1 << (n_bits - 1)) : (n_bits == 8 ? 128 : 0);
}
// d: what was subtracted from q on top of the sign offset (added back through the zero point)
__host__ __device__ __forceinline__ float zero_shift(int n_bits, int sign)
{
    return (!sign && n_bits == 8) ? 128.0f : 0.0f;
}

#ifdef QE_STAMP
// In-kernel stamps (guide section 7): one asm statement, fenced, lgkmcnt(0) inside.  Diagnostic build only.
__device__ __forceinline__ unsigned long long qe_stamp()
{
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
#define QE_ST(i) do { const unsigned long long _t = qe_stamp(); st[i] += _t - tprev; tprev = _t; } while (0)
#else
#define QE_ST(i) do { } while (0)
#endif

}  // namespace qe
