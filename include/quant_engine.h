/*
 * quant_engine.h -- C ABI of the MI355X (gfx950) quantized-conv2d engine.
 *
 * This is the drop-in boundary for the reference's `engine.kernels` extension
 * (JingInAI/Quantize, pybind module `quant_engine`, engine/kernels/pybind.cpp:7-17).
 * Every entry point takes plain device pointers, sizes and a HIP stream; no torch
 * types appear here.  The torch-facing `quant_engine` Python module
 * (quantize_amd/csrc/torch_binding.cpp) is a thin layer over these calls that
 * reproduces the reference's argument checks, allocation and error class.
 *
 * Conventions
 *   - all pointers are DEVICE pointers unless stated otherwise;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream);
 *     every call is asynchronous on that stream and performs no host sync,
 *     allocation or free (graph-capturable);
 *   - return value: QE_OK or a QE_ERR_* code; qe_error_string() gives the text,
 *     which for the reference's own checks is the reference's message verbatim;
 *   - packed tensor format (reference: engine/kernels/tpack/tpack.cu:50-81,
 *     tpack.h:14-15): element i of an n_bits-wide tensor occupies bits
 *     [i*n_bits, (i+1)*n_bits) of a little-endian bit stream, stored value =
 *     q + (sign ? 2^(n_bits-1) : 0); the stream is ceil(n*n_bits/8) bytes, no
 *     padding between elements, rows or channels.
 */
#ifndef QUANT_ENGINE_H
#define QUANT_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *qe_stream_t; /* hipStream_t */

enum qe_status {
    QE_OK = 0,
    QE_ERR_NBITS = 1,       /* "n_bits must be in the range (0, 8]"  tpack.cu:13 */
    QE_ERR_RANGE = 2,       /* "The input tensor is out of range."   tpack.cu:14 (reported through `status`, see qe_tpack) */
    QE_ERR_DTYPE = 3,       /* dtype code not in enum qe_dtype */
    QE_ERR_ARG = 4,         /* null pointer / negative size / inconsistent shape */
    QE_ERR_HIP = 5,         /* a HIP runtime call failed; see qe_last_hip_error() */
    QE_ERR_WORKSPACE = 6,   /* workspace too small */
    QE_ERR_UNSUPPORTED = 7  /* shape outside what the kernels index */
};

/* Input element types accepted by qe_tpack: the set the reference dispatches on
 * (AT_DISPATCH_ALL_TYPES_AND(Half), tpack.cu:120). */
enum qe_dtype {
    QE_U8 = 0, QE_I8 = 1, QE_I16 = 2, QE_I32 = 3, QE_I64 = 4,
    QE_F16 = 5, QE_F32 = 6, QE_F64 = 7
};

const char *qe_error_string(int status);
/* hipError_t of the last failing HIP call made by this library on this thread (0 = none). */
int qe_last_hip_error(void);
/* Library version, and the gfx target the device code was built for ("gfx950"). */
const char *qe_version(void);
const char *qe_target_arch(void);

/* ceil(n_elements * n_bits / 8): size of the packed byte stream (tpack.cu:224). */
int64_t qe_packed_nbytes(int64_t n_elements, int n_bits);

/* ---------------------------------------------------------------------------
 * qe_tpack -- replaces tpack()/tpack_cuda()/tpack_cuda_kernel
 *   reference: engine/kernels/tpack/tpack.cu:203-255, :96-128, :30-84.
 * x        n elements of `dtype`, contiguous.
 * out      qe_packed_nbytes(n, n_bits) bytes; EVERY byte is written (no
 *          pre-zeroing needed, unlike tpack.cu:225).
 * status   optional device int32[1], must be zero on entry; bit 0 is set when any
 *          element fails the reference's range check (tpack.cu:211-215: value,
 *          as float, outside [-2^(b-1), 2^(b-1)-1] (sign) or [0, 2^b-1], or NaN).
 *          The caller reads it back to raise "The input tensor is out of
 *          range."; `out` is unspecified in that case (the reference raises
 *          before packing).
 * ------------------------------------------------------------------------- */
int qe_tpack(const void *x, int dtype, int64_t n, int n_bits, int sign,
             uint8_t *out, int32_t *status, qe_stream_t stream);

/* ---------------------------------------------------------------------------
 * qe_tunpack -- replaces tunpack()/tunpack_cuda()/tunpack_cuda_kernel
 *   reference: engine/kernels/tpack/tpack.cu:429-476, :327-359, :267-315.
 * packed   qe_packed_nbytes(n, n_bits) bytes.
 * out      n bytes: int8 when sign, uint8 otherwise (tpack.cu:452-455).
 * ------------------------------------------------------------------------- */
int qe_tunpack(const uint8_t *packed, int64_t n, int n_bits, int sign,
               void *out, qe_stream_t stream);

/* ---------------------------------------------------------------------------
 * qe_quantize_pack -- Quantizer + tpack in one pass
 *   reference: modelzoo/modules/quantizer.py:31,213-226 (q = round(x / scale - zero).clamp(qmin, qmax), returned as an
 *   integer-valued fp32 tensor in packed mode) followed by engine.tpack (tpack.cu:203-255).
 * The packed conv / linear operators have no producer for their activation operand in the reference (the module
 * hands fp32 q to F.conv2d); this is that producer: fp32 activations in, the b-bit stream qe_quantconv2d takes out,
 * without the 4 B/element intermediate.  out is bit-identical to qe_tpack(round(x / scale - zero).clamp(..)).
 * scale/zero  n_param fp32 elements in the MODULE's convention (the value is x / scale - zero; the conv kernels'
 *             (q - zero') dequantisation takes zero' = -zero).  n_param == 1: per tensor; otherwise per channel with
 *             channel(i) = (i / inner) % n_param  (NCHW activations: inner = H*W, n_param = C).
 * status      as qe_tpack: bit 0 set when a clamped value does not fit n_bits/sign (or is NaN).
 * ------------------------------------------------------------------------- */
int qe_quantize_pack(const float *x, int64_t n, const float *scale, const float *zero, int32_t n_param,
                     int64_t inner, float qmin, float qmax, int n_bits, int sign, uint8_t *out,
                     int32_t *status, qe_stream_t stream);

/* ---------------------------------------------------------------------------
 * Convolution problem description shared by the two conv entry points.
 * Shapes follow the reference's host code: square stride/padding, no dilation,
 * no groups (functions/quantconv2d.cu:198-211).  OH/OW are derived:
 * OH = (H + 2*padding - KH)/stride + 1.
 * ------------------------------------------------------------------------- */
typedef struct qe_conv_shape {
    int32_t N, IC, H, W;     /* input  (N, IC, H, W)   NCHW */
    int32_t OC, KH, KW;      /* weight (OC, IC, KH, KW) OIHW */
    int32_t stride, padding;
} qe_conv_shape;

/* Quantisation parameters of one packed operand.
 * scale/zero: device fp32 arrays of `n_param` elements.  n_param == 1 means per
 * tensor (the reference's `numel() == 1` test, quantconv2d.cu:238,244);
 * otherwise activations index by INPUT channel (quantconv2d.cu:115) and weights
 * by OUTPUT channel (quantconv2d.cu:130).  Dequantisation follows the kernel
 * convention (q - zero) * scale (quantconv2d.cu:113-115,128-130). */
typedef struct qe_qparam {
    const uint8_t *data;   /* packed bit stream */
    int32_t n_bits;        /* 1..8  (des[0]) */
    int32_t sign;          /* 0/1   (des[1]) */
    const float *scale;
    const float *zero;
    int32_t n_param;
} qe_qparam;

/* Bytes of scratch qe_quantconv2d needs for this problem (0 is possible).
 * The scratch holds the re-laid-out int8 weights and per-channel epilogue
 * constants of the MFMA path; contents are dead after the call returns to the
 * stream order (i.e. may be reused by the next call on the same stream). */
size_t qe_quantconv2d_workspace_bytes(const qe_conv_shape *shape, int x_bits, int w_bits);

/* ---------------------------------------------------------------------------
 * qe_quantconv2d -- replaces quantconv2d()/quantconv2d_cuda_kernel
 *   reference: engine/kernels/functions/quantconv2d.cu:164-264, :49-142.
 * out[n,oc,oh,ow] = bias[oc] + sum over in-bounds taps (ic,kh,kw) of
 *     ((qx - zx) * sx) * ((qw - zw) * sw)          (fp32 result, NCHW, contiguous)
 * x, w     packed operands (see qe_qparam); x holds N*IC*H*W elements, w holds
 *          OC*IC*KH*KW elements.
 * bias     fp32[OC] or NULL.
 * out      fp32[N*OC*OH*OW]; every element is written.
 * workspace/workspace_bytes  scratch of at least qe_quantconv2d_workspace_bytes().
 * ------------------------------------------------------------------------- */
int qe_quantconv2d(const qe_qparam *x, const qe_qparam *w, const float *bias,
                   const qe_conv_shape *shape, float *out,
                   void *workspace, size_t workspace_bytes, qe_stream_t stream);

/* ---------------------------------------------------------------------------
 * Weights kept prepared across calls.
 *   reference: modelzoo/modules/quantconv2d.py:187-192 (pack() stores the packed weight once) and :230-233 (the
 *   TODO "remove tunpack in loading state_dict, and add support for custom operators"): a packed layer's weights,
 *   scales and bias never change between forward passes, yet the reference op receives them packed on every call.
 * qe_conv_prepare runs the x-independent part of qe_quantconv2d once -- the packed OIHW stream re-laid out as
 * int8 MFMA fragments, per-channel (sw, zw', bias) and the border-aware tap-sum tables -- into a caller-owned
 * device buffer of qe_conv_prepared_bytes() bytes; qe_quantconv2d_prepared then runs only the convolution.
 * Results are bit-identical to qe_quantconv2d.  x_bits selects the kernel plan the tables are laid out for and
 * must match the activations passed later; w / bias must be the same tensors (the 1x1 kernels still read them).
 * qe_conv_prepared_bytes() == 0: nothing to prepare (the kernel consumes the packed weights directly); both
 * calls then accept prepared == NULL.  Scratch for the prepared call: qe_quantconv2d_prepared_workspace_bytes().
 * ------------------------------------------------------------------------- */
size_t qe_conv_prepared_bytes(const qe_conv_shape *shape, int x_bits, int w_bits);
/* Signature of the prepared tables' layout (0: nothing to prepare).  It depends on the weight tensor's geometry and on
 * the kernel family the plan picks, NOT on the batch size, and on the image size only where that changes the family:
 * a caller that keeps prepared buffers per layer keys them on this value, so alternating batch sizes (or image sizes
 * served by the same family) reuse one buffer instead of re-preparing. */
uint64_t qe_conv_prepared_layout(const qe_conv_shape *shape, int x_bits, int w_bits);
size_t qe_quantconv2d_prepared_workspace_bytes(const qe_conv_shape *shape, int x_bits, int w_bits);
int qe_conv_prepare(const qe_qparam *w, const float *bias, const qe_conv_shape *shape, int x_bits,
                    void *prepared, size_t prepared_bytes, qe_stream_t stream);
int qe_quantconv2d_prepared(const qe_qparam *x, const qe_qparam *w, const float *bias,
                            const qe_conv_shape *shape, const void *prepared, size_t prepared_bytes,
                            float *out, void *workspace, size_t workspace_bytes, qe_stream_t stream);

/* ---------------------------------------------------------------------------
 * qe_quantconv2d_requant_prepared -- quantconv2d with the NEXT layer's activation quantiser fused into the epilogue
 *   (conv-epilogue form).  reference: the packed forward of
 *   modelzoo/modules/quantconv2d.py:198-210 followed by the consumer's Quantizer (quantizer.py:31,213-226) and
 *   engine.tpack -- three passes over a 4 B/element tensor there, none here.
 * out  qe_packed_nbytes(N*OC*OH*OW, rq->n_bits) bytes, bit-identical to
 *      qe_quantize_pack(qe_quantconv2d_prepared(x, w, ...), rq->scale, rq->zero, rq->n_param, OH*OW, ...).
 * rq   output quantiser in the MODULE's convention (q = round(y / scale - zero).clamp(qmin, qmax)); n_param = 1 (per
 *      tensor) or OC (per output channel).
 * qe_quantconv2d_requant_path: 1 = the conv kernel stores the codes itself (8-bit codes, per-tensor rq, MFMA-eligible problem);
 *      0 = two passes inside the call (fp32 y in the workspace, then the quantise+pack kernel).
 * workspace  qe_quantconv2d_requant_workspace_bytes(shape, x, w, rq) bytes, 16-byte aligned.
 * prepared   as qe_quantconv2d_prepared (qe_conv_prepare); status as qe_tpack.
 *            The flag is a function of the N*OC*OH*OW values alone, whichever kernel runs and whatever form of the
 *            quantiser it takes: an infinite y clamps to qmin / qmax like any other and raises it only where that clamp
 *            bound lies outside the code range, a NaN always does, and lanes that compute on tile padding never do.
 * ------------------------------------------------------------------------- */
typedef struct qe_requant {
    const float *scale;
    const float *zero;
    int32_t n_param;
    float qmin, qmax;
    int32_t n_bits, sign;
} qe_requant;
int qe_quantconv2d_requant_path(const qe_conv_shape *shape, const qe_qparam *x, const qe_qparam *w, const qe_requant *rq);
size_t qe_quantconv2d_requant_workspace_bytes(const qe_conv_shape *shape, const qe_qparam *x, const qe_qparam *w,
                                              const qe_requant *rq);
int qe_quantconv2d_requant_prepared(const qe_qparam *x, const qe_qparam *w, const float *bias,
                                    const qe_conv_shape *shape, const void *prepared, size_t prepared_bytes,
                                    const qe_requant *rq, uint8_t *out, int32_t *status,
                                    void *workspace, size_t workspace_bytes, qe_stream_t stream);

/* ---------------------------------------------------------------------------
 * qe_quantconv2d_residual_prepared -- a residual block's last convolution with the block end fused into it:
 *   out[n,oc,p] = max(conv(x, w, bias)[n,oc,p] + identity[n,oc,p], 0)          (fp32, NCHW)
 *   codes       = the consumer's quantiser applied to out, packed (as qe_quantize_pack), when rq != NULL.
 *   reference: torchvision's Bottleneck / BasicBlock forward (`out += identity; out = relu(out)`) around the runners'
 *   QuantConv2d (modelzoo/reconstruct.py), followed by the next block's Quantizer + tpack.
 * out       bit-identical to torch.relu(qe_quantconv2d_prepared(...) + identity): one fp32 add, then max with 0, NaN
 *           propagating; codes bit-identical to qe_quantize_pack(out, rq->scale, rq->zero, rq->n_param, OH*OW, ...).
 * identity  fp32, shaped like out.  out == identity (in place) is allowed; any other overlap returns QE_ERR_ARG.
 *           identity / out 16-byte aligned, codes 4-byte aligned.
 * out       may be NULL when rq != NULL (codes only).  status as qe_tpack (bit 0: a code out of range, or NaN).
 * qe_quantconv2d_residual_path: 1 = the conv kernel does it all (1x1 stride-1 resident-tile kernels, 8-bit operands; rq NULL
 *           or 8-bit per tensor); 0 = two passes inside the call (the conv's fp32 y, then one elementwise pass y + identity ->
 *           out + codes), which covers every other problem, sub-8-bit codes and per-channel rq.
 * workspace qe_quantconv2d_residual_workspace_bytes() bytes (0 on path 1), 16-byte aligned.
 * ------------------------------------------------------------------------- */
int qe_quantconv2d_residual_path(const qe_conv_shape *shape, const qe_qparam *x, const qe_qparam *w, const qe_requant *rq);
size_t qe_quantconv2d_residual_workspace_bytes(const qe_conv_shape *shape, const qe_qparam *x, const qe_qparam *w,
                                               const qe_requant *rq);
int qe_quantconv2d_residual_prepared(const qe_qparam *x, const qe_qparam *w, const float *bias,
                                     const qe_conv_shape *shape, const void *prepared, size_t prepared_bytes,
                                     const float *identity, float *out, const qe_requant *rq, uint8_t *codes,
                                     int32_t *status, void *workspace, size_t workspace_bytes, qe_stream_t stream);

/* ---------------------------------------------------------------------------
 * qe_quantconv2d_float_input -- replaces quantconv2d_float_input()/..._cuda
 *   reference: engine/kernels/functions/quantconv2d_float_input.cu:140-220, :45-121.
 * x        fp32[N*IC*H*W], NCHW contiguous.
 * ------------------------------------------------------------------------- */
int qe_quantconv2d_float_input(const float *x, const qe_qparam *w, const float *bias,
                               const qe_conv_shape *shape, float *out, qe_stream_t stream);

/* The same operator on the matrix cores (exact 3-way bf16 split of the fp32 activations x integer weight codes,
 * fp32 accumulation; quantize_amd/csrc/qe_conv_f32.hip).  It needs scratch for the weights in fragment order, which
 * the reference's signature has no place for, hence the _ws form; the plain entry point above keeps the
 * order-preserving VALU kernel (bit-identical to the reference's fmaf chain).  Results of the two differ by fp32
 * accumulation order only (within max(1e-5, |reference chain - exact|), tests/test_conv_f32_gpu.py).
 * qe_quantconv2d_float_input_workspace_bytes() == 0 or path == 0: the problem stays on the VALU kernel.
 * The weight tables are x-independent: qe_conv_f32_prepare once + qe_quantconv2d_float_input_prepared per call keeps
 * them across forward passes (same contract as qe_conv_prepare). */
size_t qe_quantconv2d_float_input_workspace_bytes(const qe_conv_shape *shape, int w_bits);
int qe_quantconv2d_float_input_ws(const float *x, const qe_qparam *w, const float *bias,
                                  const qe_conv_shape *shape, float *out, void *workspace,
                                  size_t workspace_bytes, qe_stream_t stream);
int qe_conv_f32_prepare(const qe_qparam *w, const float *bias, const qe_conv_shape *shape,
                        void *prepared, size_t prepared_bytes, qe_stream_t stream);
int qe_quantconv2d_float_input_prepared(const float *x, const qe_qparam *w, const float *bias,
                                        const qe_conv_shape *shape, const void *prepared,
                                        size_t prepared_bytes, float *out, qe_stream_t stream);
/* 0 = order-preserving VALU kernel, 1 = bf16 MFMA kernel */
int qe_quantconv2d_float_input_path(const qe_conv_shape *shape, const qe_qparam *w);

/* The whole host-side plan of a float-input convolution (for tests, bench and profiles), copied field by field from the one
 * plan that qe_quantconv2d_float_input_path / _workspace_bytes / _ws / _prepared and qe_conv_f32_prepare read (the
 * QE_F32_MFMA knob of the last snapshot included).  The call decides nothing and does no device work.
 *   ok           1: a bf16 MFMA kernel runs; 0: the order-preserving VALU kernel (the other fields then say nothing)
 *   kernel       the instance: 0..2 conv_f32_stem_kernel<4,1,7>, <2,2,4>, <2,2,7> (IC <= 4), 3..10 conv_f32_mfma_kernel
 *                <4,1,4,1>, <4,1,4,2>, <4,1,7,1>, <4,1,7,2>, <2,2,2,1>, <2,2,2,2>, <2,2,4,1>, <2,2,4,2>
 *                (<WM, WN waves, column tiles per wave, 16-channel groups per stage>)
 *   stem         the stem kernel and its table layout
 *   OCP NG KK    padded output channels, 16-channel groups (padded to even on the two-group instances), KH * KW
 *   OH OW TH GI  output plane, output rows and images of a tile (GI > 1: whole images)
 *   IHT IWP ROWMUL COLMUL   rows and columns of the halo image in LDS; a 1-wide kernel side keeps sampled rows / columns only
 *   chunk n_pix_tiles n_oc_tiles tiles_h blocks   the block map and the grid
 *   lds          dynamic LDS bytes of the launch
 *   ep_off total the prepared tables [bf16 weights | sw, zw, bias per padded channel]: offset of the constants, size */
typedef struct qe_conv_f32_plan {
    int32_t ok, kernel, stem;
    int32_t OCP, NG, KK, OH, OW, TH, GI, IHT, IWP, ROWMUL, COLMUL;
    int32_t chunk, n_pix_tiles, n_oc_tiles, tiles_h;
    int64_t blocks, lds, ep_off, total;
} qe_conv_f32_plan;
/* QE_ERR_ARG for a bad shape or a NULL argument. */
int qe_conv_f32_plan_info(const qe_conv_shape *shape, qe_conv_f32_plan *info);

/* Which kernel family qe_quantconv2d will pick for a problem (for tests, bench
 * and profiles): 0 = generic fp32 direct convolution, 1 = int8 MFMA implicit GEMM. */
int qe_quantconv2d_path(const qe_conv_shape *shape, const qe_qparam *x, const qe_qparam *w);

/* The whole host-side plan of a packed-activation convolution request (for tests, bench and profiles): which kernel
 * instance the call launches, with which pre-pass, epilogue, LDS size and grid.  Copied from the one plan every query and
 * launcher reads (the QE_* knobs of the last snapshot included); the call decides nothing and does no device work.
 *   route        0 generic VALU kernel, 1 resident-tile pwr, 2 pwr7, 3 LDS-DMA ring flatd, 4 one of the MFMA families
 *   fused        the requested re-quantisation runs inside the conv kernel
 *   family       0 none, 1 halo, 2 warp-specialised, 3 two-strip, 4 stem, 5 flat, 6 flat stride 2, 7 flat 4-bit
 *                activations, 8 flatg (set whenever an MFMA family fits, also when another route takes the problem)
 *   cfg niw kkt ns split wraw rq patch
 *                the template instance of the family (route 4): wave layout (0: 4x1, 1: 2x2, 2: 1x4), column tiles per
 *                wave, tap form (1: 1x1, 9: 3x3, 0: any other kernel size), chunks per stage, channel slices of the
 *                staging threads, raw 8-bit weights, and whether the re-quantising / LDS byte patch instance is launched
 *   has_instance the library compiles that instance (route 4; a plan without one would fail with QE_ERR_UNSUPPORTED)
 *   pre          strided gather in front of the kernel: 0 none, 1 subsample_x4, 2 subsample2<sub2_log_up>,
 *                3 subsample<wide>, 4 subsample<narrow>; expand: the sub-8-bit expansion pass runs first
 *   lds          dynamic LDS bytes of the MFMA-family launch; blocks: its grid
 *   total / prep_total / y_bytes   workspace [prepared part | scratch], its prepared part, the rounded fp32 output */
typedef struct qe_conv_plan_info {
    int32_t route, fused;
    int32_t family, cfg, niw, kkt, ns, split, wraw, rq, patch, has_instance;
    int32_t ctab, gi, th, ni, mt, nch, oh, ow, rowmul, colmul;
    int32_t pre, sub2_log_up, expand, sub_x4;
    int32_t fd_w8;
    int32_t pwr_tw, pwr_ks, pwr_groups, pwr7_gi, pwr_s2;
    int64_t lds, blocks, total, prep_total, y_bytes;
} qe_conv_plan_info;
/* rq: the consumer's quantiser of a qe_quantconv2d_requant_prepared call, or NULL for the fp32 call; out / codes: the
 * destination addresses (only their alignment counts; NULL reads as aligned).  QE_ERR_ARG for a bad shape or a NULL
 * operand. */
int qe_quantconv2d_plan_info(const qe_conv_shape *shape, const qe_qparam *x, const qe_qparam *w, const qe_requant *rq,
                             const float *out, const uint8_t *codes, qe_conv_plan_info *info);
/* 1 when the library compiles the MFMA-family instance these parameters name (as in qe_conv_plan_info), else 0: what the
 * planner's PATCH question and the launcher ask, answered for any parameter set.  Host-only. */
int qe_conv_mfma_has_instance(int32_t family, int32_t cfg, int32_t niw, int32_t kkt, int32_t ns, int32_t split,
                              int32_t wraw, int32_t rq, int32_t patch);

/* ---------------------------------------------------------------------------
 * qe_quantconv2d_depthwise -- a depthwise convolution (groups == IC == OC == C) on packed codes, fp32 and / or codes out.
 *   reference: the packed forward of modelzoo/modules/quantconv2d.py on a groups = C layer (F.conv2d(..., groups=C) on the
 *   dequantised tensors; pack() leaves w_des [b, s, C, 1, KH, KW]), followed by ReLU and the consumer's Quantizer + tpack.
 *   y[n,c,oh,ow] = bias[c] + sum over in-bounds taps (kh,kw) of ((qx - zx) * sx) * ((qw - zw) * sw);  relu != 0: max(y, 0),
 *   NaN passing, as qe_quantconv2d_residual_prepared.  out (fp32, may be NULL with rq) receives y; codes (with rq) are
 *   bit-identical to qe_quantize_pack(y, rq->scale, rq->zero, rq->n_param, OH*OW, ...).
 * shape    IC == OC == C; a depth multiplier (OC != IC) returns QE_ERR_UNSUPPORTED.  KH, KW <= 7 (need not be equal), any
 *          stride, 2 * padding <= min(KH, KW); anything else returns QE_ERR_UNSUPPORTED.
 * x, w     packed operands: x N*C*H*W elements, w C*KH*KW elements; n_param 1 or C each (x by input channel = the plane).
 * bias     fp32[C] or NULL.   rq   n_param 1 or C.   out 4-byte aligned; status as qe_tpack.
 * QE_ERR_ARG before any device work: a NULL operand, an n_param that is neither 1 nor C, out and codes both NULL, codes
 *          without rq or rq without codes, an output (out, codes, status) overlapping any operand or another output.
 * Integer arithmetic on centred codes: the sums over the in-bounds taps are exact in int32, the zero points enter through their
 * integer parts (exactly) and their remainders (fp32 terms of the size of the remainder), then one fma with sx * sw and bias.
 * Sub-8-bit rq codes: two planes can share a byte of the stream, so the kernels do not pack them: with out != NULL the call
 *          runs the kernel into out and then qe_quantize_pack on it (two_pass); with out == NULL it returns QE_ERR_UNSUPPORTED.
 * No workspace and no prepared tables.  Asynchronous on stream; no host synchronisation, allocation or free.
 * _path (host only): 1 = the fast kernel (3x3, padding 1, stride 1 or 2, 8-bit x 8-bit codes of any sign pair), 0 = the plain
 *          kernel (one thread per output), -1 = none (QE_ERR_UNSUPPORTED or a bad argument).  rq may be NULL.
 * qe_dwconv_plan: the one plan the launcher reads, copied field by field (the call decides nothing, no device work):
 *   kernel     the instance: 0 plain; 1 + 3 * (stride - 1) + e the fast kernel, e = 0 fp32 out, 1 codes, 2 both
 *   symmetric  both operands are signed, so a plane whose zero points are 0 has no zero-point term and the kernel skips them
 *              (an unsigned operand is re-centred by 128 and always has one; the box sum is skipped whenever zw' == 0)
 *   G TH       the fast kernel's span: G whole consecutive planes per workgroup, or (G == 1) bands of TH output rows
 *   vec        consecutive outputs of a thread
 *   store16 codes4  out is 16-byte / codes 4-byte aligned: every store of the body takes that form (otherwise the spans'
 *              aligned chunks are shifted against the tensor and their edges are completed with narrower stores)
 *   two_pass   sub-8-bit codes through out and qe_quantize_pack
 *   OH OW bands     output plane; bands per plane (1: whole planes)
 *   blocks lds the 1-D grid and the dynamic LDS bytes                                                                    */
typedef struct qe_dwconv_plan {
    int32_t kernel, symmetric, G, TH, vec, store16, codes4, two_pass, OH, OW, bands;
    int64_t blocks, lds;
} qe_dwconv_plan;
int qe_quantconv2d_depthwise_path(const qe_conv_shape *shape, const qe_qparam *x, const qe_qparam *w, const qe_requant *rq);
int qe_quantconv2d_depthwise_plan_info(const qe_conv_shape *shape, const qe_qparam *x, const qe_qparam *w, const qe_requant *rq,
                                       const float *out, const uint8_t *codes, qe_dwconv_plan *info);
int qe_quantconv2d_depthwise(const qe_qparam *x, const qe_qparam *w, const float *bias, const qe_conv_shape *shape,
                             int32_t relu, float *out, const qe_requant *rq, uint8_t *codes, int32_t *status,
                             qe_stream_t stream);

/* ---------------------------------------------------------------------------
 * qe_quantconv2d_grouped -- a grouped convolution (1 < groups < channels) on packed codes, fp32 and / or codes out.
 *   reference: the packed forward of modelzoo/modules/quantconv2d.py on a groups = g layer (F.conv2d(..., groups=g) on the
 *   dequantised tensors; pack() leaves w_des [b, s, OC, IC/g, KH, KW]), followed by ReLU and the consumer's Quantizer + tpack.
 *   y[n,oc,oh,ow] = bias[oc] + sum over the IC/g input channels ic of oc's group and the in-bounds taps (kh,kw) of
 *   ((qx - zx) * sx) * ((qw - zw) * sw);  relu != 0: max(y, 0), NaN passing.  out (fp32, may be NULL with rq) receives y; codes
 *   (with rq) are bit-identical to qe_quantize_pack(y, rq->scale, rq->zero, rq->n_param, OH*OW, ...).
 * shape    IC and OC are the totals (qe_conv_shape has no groups); w is (OC, IC/groups, KH, KW).  KH, KW <= 7 (need not be
 *          equal), any stride, 2 * padding <= min(KH, KW); anything else returns QE_ERR_UNSUPPORTED.
 * groups   must divide IC and OC (else QE_ERR_ARG).  groups == 1 and groups == IC == OC return QE_ERR_UNSUPPORTED: the dense and
 *          the depthwise entry points own them and nothing is forwarded.
 * x, w     packed operands: x N*IC*H*W elements, w OC*(IC/groups)*KH*KW elements; x n_param 1 or IC, w n_param 1 or OC.
 * bias     fp32[OC] or NULL.   rq   n_param 1 or OC.   out 4-byte aligned; status as qe_tpack.
 * QE_ERR_ARG before any device work: a NULL operand, a bad n_param or groups, out and codes both NULL, codes without rq or rq
 *          without codes, an output (out, codes, status) overlapping any operand or another output.
 * Arithmetic, per-tensor x parameters: z = zi + dz (zi = rint(z), |dz| <= 1/2), a = qx - zxi, b = qw - zwi; over the in-bounds
 *          taps and the group's input channels I = sum a b, A = sum a, B = sum b and the count n are exact in int32;
 *          f = (float)I + fma((float)n dzx, dzw, -dzx (float)B); when dzw != 0: f = fma(-dzw, (float)A, f); y = fma(sx sw, f, bias).
 *          (float)I is a rounding step once |I| >= 2^24 (288 products of up to 255 * 255).  Both kernels run this sequence.
 *          Per-input-channel x parameters: f_c as above per channel c of the group, y = bias, then y = fma(sx[c] sw, f_c, y) in
 *          channel order (plain kernel only).
 * Sub-8-bit rq codes: two planes can share a byte of the stream, so the kernels do not pack them: with out != NULL the call
 *          runs the kernel into out and then qe_quantize_pack on it (two_pass); with out == NULL it returns QE_ERR_UNSUPPORTED.
 * No workspace and no prepared tables.  Asynchronous on stream; no host synchronisation, allocation or free.
 * _path (host only): 1 = the fast family (3x3, padding 1, stride 1 or 2, 8-bit x 8-bit codes of any sign pair, per-tensor x
 *          parameters, IC/groups == OC/groups in {4, 8, 16, 32}) on v_mfma_i32_32x32x32_i8, 0 = the plain kernel (one thread per
 *          output), -1 = none (QE_ERR_UNSUPPORTED or a bad argument).  rq may be NULL.
 * qe_grpconv_plan: the one plan the launcher reads, copied field by field (the call decides nothing, no device work):
 *   kernel     the instance: 0 plain; 1 + 6 * log2(Cg / 4) + 3 * (stride - 1) + e the fast family, e = 0 fp32 out, 1 codes, 2 both
 *   slab       consecutive channels of a workgroup (fast: 32, i.e. 32 / Cg whole groups; plain: 1)
 *   TH TW      the workgroup's pixel tile in output rows and columns (fast: a band of TH whole rows, TW == OW; plain: 1 x 1)
 *   tiles      tiles per plane
 *   two_pass   sub-8-bit codes through out and qe_quantize_pack
 *   out16 codes16   out / codes are 16-byte aligned (otherwise the per-channel aligned chunks are shifted against the tensor
 *              and their edges are completed with narrower stores)
 *   OH OW      output plane
 *   blocks lds the 1-D grid and the dynamic LDS bytes                                                                    */
typedef struct qe_grpconv_plan {
    int32_t kernel, slab, TH, TW, tiles, two_pass, out16, codes16, OH, OW;
    int64_t blocks, lds;
} qe_grpconv_plan;
int qe_quantconv2d_grouped_path(const qe_conv_shape *shape, int32_t groups, const qe_qparam *x, const qe_qparam *w,
                                const qe_requant *rq);
int qe_quantconv2d_grouped_plan_info(const qe_conv_shape *shape, int32_t groups, const qe_qparam *x, const qe_qparam *w,
                                     const qe_requant *rq, const float *out, const uint8_t *codes, qe_grpconv_plan *info);
int qe_quantconv2d_grouped(const qe_qparam *x, const qe_qparam *w, const float *bias, const qe_conv_shape *shape,
                           int32_t groups, int32_t relu, float *out, const qe_requant *rq, uint8_t *codes, int32_t *status,
                           qe_stream_t stream);

/* ---- quantlinear ------------------------------------------------------------
 * Replaces quantlinear / quantlinear_cuda (functions/quantlinear.cu:233-297, :153-214):
 *   out[b, o] = bias[o] + sum_k (q_x[b,k] + zx[b]) * (q_w[o,k] + zw[o]) * (sx[b] * sw[o])
 * Both operands are packed b-bit streams (x: B*K elements, row major; w: O*K elements, OIHW of a Linear).
 * NOTE the conventions of THIS reference kernel (they differ from quantconv2d): the zero point is ADDED
 * (quantlinear.cu:115,120) and the activation scale/zero are indexed by the batch ROW (:96-99).
 * x->n_param is 1 (broadcast: the reference expands 0-dim tensors, :276-282) or B; w->n_param is 1 or O.
 * bias may be NULL (the reference substitutes zeros, :268).  out: B*O floats, fully written.
 * The reference accumulates stale shared memory when K % 32 != 0 (:76-92 never zero-fills the tail);
 * this entry point computes the sum over k < K for every K.                                            */
int qe_quantlinear(const qe_qparam *x, const qe_qparam *w, const float *bias,
                   int64_t B, int32_t K, int32_t O, float *out, qe_stream_t stream);

/* Replaces quantlinear_float_input (functions/quantlinear_float_input.cu:120-182, kernel :36-104):
 *   out[b, o] = bias[o] + sum_k x[b,k] * ((q_w[o,k] - zw[o]) * sw[o])      ((q - zero): :82-86)
 * x: B*K floats.  w->n_param is 1 (per tensor iff numel()==1, :170) or O.
 * Non-finite activations (this entry point and qe_quantconv2d_float_input, on their MFMA kernels): every output that depends
 * on a +-inf or NaN activation is non-finite -- NaN where the reference's fmaf chain may keep +-inf (the exact bf16 split of
 * an infinity leaves inf - inf in the remainder terms) -- and every other output is unaffected.                          */
int qe_quantlinear_float_input(const float *x, const qe_qparam *w, const float *bias,
                               int64_t B, int32_t K, int32_t O, float *out, qe_stream_t stream);

/* 0 = order-preserving fp32 kernel, 1 = int8 MFMA GEMM (8-bit x 8-bit operands, K % 64 == 0, 16-byte aligned streams). */
int qe_quantlinear_path(const qe_qparam *x, const qe_qparam *w, int64_t B, int32_t K, int32_t O);

/* The kernel qe_quantlinear and its fused forms (qe_quantlinear_requant, qe_quantlinear_residual) run a problem on, from the
 * one plan that every linear query and launch reads (QE_LIN8 and QE_LIN_NJ included): 0 = order-preserving fp32 kernel,
 * 1 = 64-deep int8 MFMA kernel on 128 x 128 tiles, 2 = the same on 128 x 256 tiles, 3 = 128-deep 8-wave kernel on 320 x 256
 * tiles, 4 = 128-deep 4-wave kernel on 160 x 256 tiles.  dst_aligned: the epilogue's destination (out, codes; out and
 * residual) is 16-byte aligned -- the re-quantising form's fused path requires it.  Host-only: no device work. */
int qe_quantlinear_form(const qe_qparam *x, const qe_qparam *w, int64_t B, int32_t K, int32_t O, int32_t dst_aligned);

/* quantlinear_float_input: 0 = order-preserving fp32 kernel (bit-identical to the reference's fused chain), 1 = bf16 MFMA
 * GEMM on an exact three-way split of the activations (8-bit weights, K % 32 == 0, 16-byte aligned operands; results within
 * fp32 accumulation rounding of the exact sum; QE_LIN_F32_MFMA=0 disables it). */
int qe_quantlinear_float_input_path(const float *x, const qe_qparam *w, int64_t B, int32_t K, int32_t O);

/* ---- fused ViT forms ---------------------------------------------------------------------------
 * What runs between the GEMMs of a ViT encoder block (torchvision's EncoderBlock around the reference's QuantLinear /
 * QuantMultiheadAttention: x + attn(ln_1(x)), then y + mlp(ln_2(y)) with mlp = fc1, GELU, fc2) fused into the linears'
 * epilogues or into one pass over a row.  Activation functions applied in front of a consumer's quantiser:          */
enum qe_act { QE_ACT_NONE = 0, QE_ACT_GELU = 1 };   /* GELU: torch's exact form x * 0.5 * (1 + erf(x / sqrt(2))), fp32 */

/* qe_quantize_pack_act -- qe_quantize_pack of act(x).
 * y      optional fp32[n] output of act(x) (NULL: codes only); y == x (in place) or disjoint.
 * out    the codes: bit-identical to qe_quantize_pack(act(x), ...) (same per-element fp32 arithmetic); with
 *        act == QE_ACT_NONE and y == NULL this IS qe_quantize_pack.  Other arguments and `status` as qe_quantize_pack. */
int qe_quantize_pack_act(const float *x, int64_t n, int32_t act, const float *scale, const float *zero, int32_t n_param,
                         int64_t inner, float qmin, float qmax, int n_bits, int sign, uint8_t *out, float *y,
                         int32_t *status, qe_stream_t stream);

/* qe_quantlinear_requant -- qe_quantlinear with the consumer's quantiser (and optionally GELU) fused into the epilogue:
 *   codes = qe_quantize_pack_act(qe_quantlinear(x, w, bias, B, K, O), act, rq)      (bit for bit; B x O row-major elements)
 * rq     module convention (q = round(v / scale - zero).clamp(qmin, qmax)); n_param 1 (per tensor) or O (per output
 *        feature).  codes: qe_packed_nbytes(B * O, rq->n_bits) bytes.  status as qe_tpack.
 * qe_quantlinear_requant_path: 1 = the int8 MFMA kernel stores the codes itself (qe_quantlinear_path == 1, rq 8-bit per
 *        tensor, codes 16-byte aligned, QE_LIN_EPI not 0); 0 = two passes inside the call (qe_quantlinear into the
 *        workspace, then qe_quantize_pack_act).
 * workspace  qe_quantlinear_requant_workspace_bytes() bytes (0 on path 1), 16-byte aligned.                           */
int qe_quantlinear_requant_path(const qe_qparam *x, const qe_qparam *w, int64_t B, int32_t K, int32_t O,
                                const qe_requant *rq, const uint8_t *codes);
size_t qe_quantlinear_requant_workspace_bytes(const qe_qparam *x, const qe_qparam *w, int64_t B, int32_t K, int32_t O,
                                              const qe_requant *rq, const uint8_t *codes);
int qe_quantlinear_requant(const qe_qparam *x, const qe_qparam *w, const float *bias, int64_t B, int32_t K, int32_t O,
                           int32_t act, const qe_requant *rq, uint8_t *codes, int32_t *status,
                           void *workspace, size_t workspace_bytes, qe_stream_t stream);

/* qe_quantlinear_residual / qe_quantlinear_float_input_residual -- a linear with the residual add fused into the epilogue:
 *   out = qe_quantlinear(...) + residual       (resp. qe_quantlinear_float_input; one fp32 add, bit for bit)
 * residual, out  fp32[B * O]; out == residual (in place) is allowed, any other overlap returns QE_ERR_ARG.
 * _path: 1 = the MFMA kernel adds the residual in its epilogue (qe_quantlinear_path == 1, resp.
 *        qe_quantlinear_float_input_path == 1, and QE_LIN_EPI not 0); 0 = the linear into the workspace, then one
 *        elementwise add.  workspace: _workspace_bytes() bytes (0 on path 1), 16-byte aligned.                         */
int qe_quantlinear_residual_path(const qe_qparam *x, const qe_qparam *w, int64_t B, int32_t K, int32_t O);
size_t qe_quantlinear_residual_workspace_bytes(const qe_qparam *x, const qe_qparam *w, int64_t B, int32_t K, int32_t O);
int qe_quantlinear_residual(const qe_qparam *x, const qe_qparam *w, const float *bias, int64_t B, int32_t K, int32_t O,
                            const float *residual, float *out, void *workspace, size_t workspace_bytes, qe_stream_t stream);
int qe_quantlinear_float_input_residual_path(const float *x, const qe_qparam *w, int64_t B, int32_t K, int32_t O);
size_t qe_quantlinear_float_input_residual_workspace_bytes(const float *x, const qe_qparam *w, int64_t B, int32_t K, int32_t O);
int qe_quantlinear_float_input_residual(const float *x, const qe_qparam *w, const float *bias, int64_t B, int32_t K, int32_t O,
                                        const float *residual, float *out, void *workspace, size_t workspace_bytes,
                                        qe_stream_t stream);

/* qe_quantlinear_bf16 -- qe_quantlinear with a bf16 result, for a consumer that would round it anyway (the q / k / v
 * projections in front of qe_attention_bf16_stored):
 *   out[b, o] = bf16( y[b, o] * post_scale ),   y = qe_quantlinear(x, w, bias, B, K, O)      (B x O row-major bf16 bit patterns)
 * y is the fp32 value qe_quantlinear computes for the same problem, bit for bit; the product is one fp32 multiply and the
 * rounding is to nearest even (a NaN stays a NaN, an overflow becomes inf), so post_scale == 1.0f is the plain rounding of
 * y and out equals (qe_quantlinear(...) * post_scale) rounded elementwise.  x, w, bias, B, K, O and their checks as
 * qe_quantlinear_residual; out NULL or not 2-byte aligned is QE_ERR_ARG.
 * _path: 1 = the int8 MFMA kernel rounds and stores the bf16 rows itself (qe_quantlinear_path == 1, O % 8 == 0, out 16-byte
 *        aligned -- so every O % 64 == 0 with an aligned out -- and QE_LIN_EPI not 0); 0 = qe_quantlinear into the
 *        workspace, then one elementwise pass with the same multiply and rounding.  `out` (NULL reads as aligned) is only
 *        looked at for its alignment.  workspace: _workspace_bytes() bytes (0 on path 1), 16-byte aligned.            */
int qe_quantlinear_bf16_path(const qe_qparam *x, const qe_qparam *w, int64_t B, int32_t K, int32_t O, const uint16_t *out);
size_t qe_quantlinear_bf16_workspace_bytes(const qe_qparam *x, const qe_qparam *w, int64_t B, int32_t K, int32_t O,
                                           const uint16_t *out);
int qe_quantlinear_bf16(const qe_qparam *x, const qe_qparam *w, const float *bias, int64_t B, int32_t K, int32_t O,
                        float post_scale, uint16_t *out, void *workspace, size_t workspace_bytes, qe_stream_t stream);

/* qe_quantlinear_bf16_input -- qe_quantlinear_float_input(_residual) on activations that are bf16 in memory (the context
 * qe_attention_bf16_ctx wrote, in front of out_proj):
 *   out = qe_quantlinear_float_input(fp32(x), w, bias, B, K, O)  [+ residual]
 * x  B x K row-major bf16 bit patterns; fp32(x) are the values they denote (exact).  residual NULL: none; given, one fp32 add
 * of residual follows, so the with-residual result is the no-residual result plus residual, bit for bit.  out == residual
 * (in place) is allowed; any other overlap of out with residual or x returns QE_ERR_ARG, as do a NULL x or out, an odd x and
 * an out or residual that is not 4-byte aligned.  w, bias, B, K, O and their checks as qe_quantlinear_float_input_residual.
 * _path: 1 = the bf16-input MFMA kernel (8-bit weights, K % 32 == 0, x 16-byte aligned, QE_LIN_F32_MFMA not 0; the entry
 *        point also wants out 16-byte aligned, which a query cannot see): a row of x is the matrix cores' operand as stored --
 *        one v_mfma_f32_32x32x16_bf16 per product where the float-input kernel's exact three-way split issues three; each
 *        product bf16 x centred integer code is exact in fp32, the fp32 accumulation and the fp32 row sum round, so the
 *        result meets the float-input kernels' parity rule against float64 and is NOT bit-identical to them.  A NaN or inf
 *        in a row of x makes that row's outputs non-finite (NaN where the reference's chain keeps inf) and no other row's.
 *        0 = one elementwise pass widens x to fp32 at the front of the workspace, then the float-input plan runs on the
 *        copy: bit-identical to qe_quantlinear_float_input(_residual) on the widened rows.
 * workspace: _workspace_bytes() bytes, 16-byte aligned: 0 on path 1; on path 0 B * K * 4 (rounded up to 16) plus
 *        qe_quantlinear_float_input_residual_workspace_bytes of the widened problem.                                   */
int qe_quantlinear_bf16_input_path(const uint16_t *x, const qe_qparam *w, int64_t B, int32_t K, int32_t O);
size_t qe_quantlinear_bf16_input_workspace_bytes(const uint16_t *x, const qe_qparam *w, int64_t B, int32_t K, int32_t O);
int qe_quantlinear_bf16_input(const uint16_t *x, const qe_qparam *w, const float *bias, int64_t B, int32_t K, int32_t O,
                              const float *residual, float *out, void *workspace, size_t workspace_bytes, qe_stream_t stream);

/* qe_layernorm_quantize_pack -- torch's F.layer_norm over the last dimension of fp32 rows (rows x E, contiguous) and the
 * codes of up to 3 consumer quantisers of the result (q / k / v projections: each its own), reading each row once.
 *   ln = (x - mean) * rstd * gamma + beta, mean = sum(x) / E, var = sum((x - mean)^2) / E (centred: not E[x^2] - mean^2),
 *   rstd = 1 / sqrtf(var + eps) (correctly rounded division and square root).
 * gamma, beta   fp32[E] (NULL: 1 and 0).
 * n_out, rq[], codes[]  n_out in 0..3 host arrays: rq[i] (module convention, per tensor or n_param == E) and codes[i]
 *        (device, qe_packed_nbytes(rows * E, rq[i].n_bits) bytes).  codes[i] is bit-identical to
 *        qe_quantize_pack(ln, rq[i]) of the fp32 ln this call computes.
 * ln_out optional fp32[rows * E] (NULL: codes only).  status as qe_tpack.
 * Supported: E % 4 == 0, 4 <= E <= QE_LN_MAX_E; other shapes return QE_ERR_UNSUPPORTED.
 * _path: 1 = one pass (every rq 8-bit per tensor, codes 4-byte aligned); 0 = the fp32 ln (into ln_out, or the workspace
 *        when ln_out is NULL) and then qe_quantize_pack per consumer.  workspace: _workspace_bytes() bytes, 16-byte aligned. */
#define QE_LN_MAX_E 2048
int qe_layernorm_quantize_pack_path(int64_t rows, int32_t E, int32_t n_out, const qe_requant *rq, uint8_t *const *codes);
size_t qe_layernorm_quantize_pack_workspace_bytes(int64_t rows, int32_t E, int32_t n_out, const qe_requant *rq,
                                                  uint8_t *const *codes, const float *ln_out);
int qe_layernorm_quantize_pack(const float *x, int64_t rows, int32_t E, const float *gamma, const float *beta, float eps,
                               int32_t n_out, const qe_requant *rq, uint8_t *const *codes, float *ln_out, int32_t *status,
                               void *workspace, size_t workspace_bytes, qe_stream_t stream);

/* qe_quantize_patchify -- the image quantiser of a ViT's patch embedding (conv_proj: kernel = stride = p, no padding) and
 * the unfold, in one pass: fp32 NCHW images (N, C, H, W; H % p == W % p == 0) -> packed codes of the (N*(H/p)*(W/p)) x
 * (C*p*p) patch matrix, row n*(H/p)*(W/p) + ph*(W/p) + pw, column c*p*p + kh*p + kw -- the OIHW K order of the conv's
 * packed weights, so qe_quantlinear(codes, conv weights) is conv_proj with its output already in token order.
 * Bit-identical to qe_quantize_pack of the unfolded fp32 matrix.  scale/zero: n_param 1 (per tensor) or C (per input
 * channel); any n_bits.  status as qe_tpack.                                                                            */
int qe_quantize_patchify(const float *x, int32_t N, int32_t C, int32_t H, int32_t W, int32_t patch, const float *scale,
                         const float *zero, int32_t n_param, float qmin, float qmax, int n_bits, int sign, uint8_t *out,
                         int32_t *status, qe_stream_t stream);

/* qe_attention -- the fp32 attention core of a ViT encoder block / nn.MultiheadAttention (need_weights=False, no mask;
 * qe_attention_masked below takes the masks):
 *   out[n, t, h] = sum_s softmax_s(scale * q[n, t, h] . k[n, s, h]) v[n, s, h]      per image n < N, head h < H
 * for query tokens t < L and key tokens s < S (S != L allowed).  Every tensor is rows of H*d floats; the row of
 * (image n, token t) is n*rn + t*rt, and head h is columns h*d .. h*d + d - 1 of it: token-major (N L, E) rows are
 * rn = L, rt = 1 (the ViT), sequence-major (L N, E) rows are rn = 1, rt = N (nn.MultiheadAttention, batch_first=False).
 * Both are read and written in place: no transposes, no workspace, and the score matrix is never stored.
 * q, k, v, out   device pointers, 16-byte aligned; k and v share kv_rn / kv_rt; out must not overlap q, k or v
 *                (QE_ERR_ARG, as are non-positive sizes and negative strides -- answered before any device work).
 * scale          multiplies q once as it is loaded (fp32); 1 / sqrt(d) gives torch's default.
 * Numerics: scores are fp32 products and sums (fmaf chains); the softmax is online over key tiles with a running row max
 * m, p = exp2f((score - m) * log2(e)) (the max-subtracted score scaled by log2(e), then exp2f); P.V products, their
 * sums and the row sum in fp32; one division by the row sum at the end.
 * Non-finite inputs: a NaN in a query row poisons only that row of that head; a NaN in a key or value row poisons only
 * that (image, head).
 * qe_attention_path (host only): 1 = the fp32 MFMA kernel (v_mfma_f32_32x32x2_f32: d % 16 == 0, d <= 128),
 * 0 = the fp32 VALU kernel (every other d <= 256, and every shape under QE_ATTN=0), -1 = no kernel (d > 256, where
 * qe_attention returns QE_ERR_UNSUPPORTED, or a non-positive size).                                                  */
int qe_attention_path(int32_t L, int32_t S, int32_t H, int32_t d);
int qe_attention(const float *q, const float *k, const float *v, float *out,
                 int32_t N, int32_t L, int32_t S, int32_t H, int32_t d,
                 int64_t q_rn, int64_t q_rt, int64_t kv_rn, int64_t kv_rt, int64_t o_rn, int64_t o_rt,
                 float scale, qe_stream_t stream);

/* qe_attention_masked -- qe_attention with up to three optional operands on the score:
 *   score[n, h, t, s] = scale * q[n, t, h] . k[n, s, h] + mask[n, h, t, s] + key_bias[n, s],   s <= t only when causal
 * and everything after it (online softmax, P.V, one division) as qe_attention.  q .. scale as there.
 * mask           fp32 device pointer or NULL: rows of S contiguous floats, row t of (image n, head h) at
 *                mask + n*mask_sn + h*mask_sh + t*S (element strides, >= 0; 0 broadcasts).  torch's 2-D (L, S) mask is
 *                (0, 0), nn.MultiheadAttention's 3-D (N*H, L, S) is (H*L*S, L*S), a per-image (N, L, S) is (L*S, 0).
 *                Values are finite or -inf; they are added to the scaled score, not multiplied by scale (torch's convention).
 * key_bias       fp32 (N, S) device pointer or NULL: the key-padding mask as an additive row (-inf = padded key), kept
 *                apart from mask so that padding never needs an N*H*L*S tensor.
 * causal         non-zero: key s is visible to query t iff s <= t -- top-left aligned for S != L, torch.ones(L, S).tril(),
 *                the is_causal convention of F.scaled_dot_product_attention.  Key tiles wholly above the diagonal of a
 *                wave's queries are not visited (no K / V load); the diagonal tile is masked by index, no memory read.
 * mask == NULL && key_bias == NULL && !causal is qe_attention: the same kernel instance.  Each combination of operands is
 * its own instance of the two kernels (a template parameter, no branch in the tile loop); 16-byte mask loads where
 * S % 4 == 0 and both strides % 4 == 0, 4-byte loads otherwise: any S works.  No workspace, no host synchronisation.
 * QE_ERR_ARG (before any device work) additionally for: a negative mask stride; mask or key_bias not 16-byte aligned;
 * out overlapping mask or key_bias; a non-zero mask_sn / mask_sh with mask == NULL.
 * Declared behaviours:
 *  - a key tile in which every key of a row is masked, followed by visible keys (padding at the front, a window, holes),
 *    is exact: while the row's running max is -inf the rescale factor is 1 and p = 0.
 *  - a row with NO visible key is NaN in that row of that head (0 / 0 of the final division) and affects nothing else:
 *    what torch.softmax over an all -inf row gives (nn.MultiheadAttention's math path; torch's fused SDPA returns 0).
 *  - non-finite q / k / v at masked positions are unspecified: an additive -inf does not hide a NaN score, a key tile
 *    skipped under causal does.
 * qe_attention_masked_path (host only): the kernel a call with these operands takes, 1 MFMA / 0 VALU / -1 none; the
 * operands select an instance of the kernel qe_attention_path names, never another kernel.                           */
int qe_attention_masked_path(int32_t L, int32_t S, int32_t H, int32_t d, int has_mask, int has_key_bias, int causal);
int qe_attention_masked(const float *q, const float *k, const float *v, float *out,
                        int32_t N, int32_t L, int32_t S, int32_t H, int32_t d,
                        int64_t q_rn, int64_t q_rt, int64_t kv_rn, int64_t kv_rt, int64_t o_rn, int64_t o_rt,
                        float scale, const float *mask, int64_t mask_sn, int64_t mask_sh, const float *key_bias,
                        int causal, qe_stream_t stream);

/* qe_attention_bf16 -- qe_attention_masked with both products on the bf16 matrix cores (v_mfma_f32_32x32x16_bf16): an
 * opt-in trade of the core's fp32 exactness for matrix-core rate.  Same parameters, same layouts, same operands and the
 * same argument checks (QE_ERR_ARG before any device work); mask == NULL && key_bias == NULL && !causal is the unmasked
 * instance.  q, k, v and out stay fp32 in memory and are read in place: no workspace, no host synchronisation.
 * Numerics contract:
 *  - q^ = bf16(fp32(q * scale)), k^ = bf16(k), v^ = bf16(v), each rounded to nearest even;
 *  - scores are fp32 sums of exact bf16 products, plus the fp32 mask / key_bias (summed with each other first);
 *  - the online softmax is qe_attention's, in fp32; p is rounded to bf16 only as the operand of P.V;
 *  - the row sum l is the fp32 sum of the unrounded p; O is accumulated in fp32, one fp32 division by l at the end.
 * Hence, against exact attention on q^, k^, v^ (scale 1), |out - ref| <= 2^-8 max|v^| (the rounding of p) plus qe_attention's
 * own 1e-5 max|v|.  The distance to attention on the unrounded inputs grows with the scores: a score of size s moves by up
 * to ~2^-8 s through the rounding of q and k.
 * NaN and all-masked rows: as qe_attention_masked declares (a row with no visible key is NaN in that row of that head).
 * Shapes: d % 16 == 0 and d <= 128 only.  Every other d returns QE_ERR_UNSUPPORTED: this entry point never runs the fp32
 * kernels instead, and QE_ATTN does not affect it.
 * qe_attention_bf16_path (host only): 2 = the bf16 MFMA kernel, -1 = no kernel (d % 16 != 0, d > 128 or a non-positive
 * size), whatever the operands.                                                                                       */
int qe_attention_bf16_path(int32_t L, int32_t S, int32_t H, int32_t d, int has_mask, int has_key_bias, int causal);
int qe_attention_bf16(const float *q, const float *k, const float *v, float *out,
                      int32_t N, int32_t L, int32_t S, int32_t H, int32_t d,
                      int64_t q_rn, int64_t q_rt, int64_t kv_rn, int64_t kv_rt, int64_t o_rn, int64_t o_rt,
                      float scale, const float *mask, int64_t mask_sn, int64_t mask_sh, const float *key_bias,
                      int causal, qe_stream_t stream);

/* qe_attention_bf16_stored -- qe_attention_bf16 on q, k, v that are bf16 in memory: rows of H*d bf16 elements (bit
 * patterns, 2 bytes each) with the same row strides q_rn, q_rt, kv_rn, kv_rt (in rows), read in place.  out, mask and
 * key_bias stay fp32, every other parameter and every operand is qe_attention_bf16's; the argument checks are the same ones
 * in the same order, the alignment (16 bytes) and the overlap of q / k / v with out taken on 2-byte elements.
 * Numerics contract: q^ = bf16(fp32(q) * scale) (one fp32 multiply, round to nearest even; scale == 1.0f uses the stored q
 * as it is), k^ = k, v^ = v; everything after that is qe_attention_bf16's contract word for word.  On q, k, v that hold
 * bf16 values, qe_attention_bf16 on them as fp32 and this entry point on them as bf16 give the same bits.
 * K rows reach the matrix cores as loaded (16-byte loads), V elements as 2-byte loads: half the bytes of the fp32 rows and
 * no conversion in the key loop.
 * Shapes: d % 16 == 0 and d <= 128 only; every other d returns QE_ERR_UNSUPPORTED and nothing else runs instead.
 * qe_attention_bf16_stored_path (host only): 2 = the bf16 MFMA kernel, -1 = no kernel, as qe_attention_bf16_path.   */
int qe_attention_bf16_stored_path(int32_t L, int32_t S, int32_t H, int32_t d, int has_mask, int has_key_bias, int causal);
int qe_attention_bf16_stored(const uint16_t *q, const uint16_t *k, const uint16_t *v, float *out,
                             int32_t N, int32_t L, int32_t S, int32_t H, int32_t d,
                             int64_t q_rn, int64_t q_rt, int64_t kv_rn, int64_t kv_rt, int64_t o_rn, int64_t o_rt,
                             float scale, const float *mask, int64_t mask_sn, int64_t mask_sh, const float *key_bias,
                             int causal, qe_stream_t stream);

/* qe_attention_bf16_ctx -- qe_attention_bf16_stored with a bf16 context: out holds rows of H*d bf16 elements (bit patterns)
 * with the row strides o_rn, o_rt, and each element is qe_attention_bf16_stored's fp32 element rounded once to bf16, to
 * nearest even (a NaN stays a NaN) -- for every head size, operand mode and layout.  Every other parameter, operand and the
 * numerics contract are qe_attention_bf16_stored's word for word; the argument checks are the same ones in the same order,
 * the alignment (16 bytes) and the overlap of q / k / v, mask and key_bias with out taken on 2-byte output elements.
 * For a consumer that reads bf16 rows: qe_quantlinear_bf16_input (out_proj).
 * qe_attention_bf16_ctx_path (host only): 2 = the bf16 MFMA kernel, -1 = no kernel, as qe_attention_bf16_path.       */
int qe_attention_bf16_ctx_path(int32_t L, int32_t S, int32_t H, int32_t d, int has_mask, int has_key_bias, int causal);
int qe_attention_bf16_ctx(const uint16_t *q, const uint16_t *k, const uint16_t *v, uint16_t *out,
                          int32_t N, int32_t L, int32_t S, int32_t H, int32_t d,
                          int64_t q_rn, int64_t q_rt, int64_t kv_rn, int64_t kv_rt, int64_t o_rn, int64_t o_rt,
                          float scale, const float *mask, int64_t mask_sn, int64_t mask_sh, const float *key_bias,
                          int causal, qe_stream_t stream);

/* ---- auxiliary (no counterpart in the reference's extension) ---------------------------------
 * Global average pool of an fp32 NCHW tensor: out[plane] = mean(x[plane][0..P)) for n_planes = N*C planes of P
 * contiguous floats.  The reference's models do this in PyTorch (torchvision ResNet: AdaptiveAvgPool2d); bench.py's
 * top-1 tail uses this entry point because torch's reduction reads the (256,2048,7,7) conv output at 1.5 TB/s.     */
int qe_global_avgpool(const float *x, int64_t n_planes, int32_t P, float *out, qe_stream_t stream);

/* Max pooling of 8-bit stored codes, NCHW, square window / stride / padding (torchvision's stem: 3, 2, 1).  Exact on codes:
 * the stored code (q, or q + 128 when signed) is order-preserving and the quantiser is non-decreasing, so
 * maxpool(q(relu(y))) == q(maxpool(relu(y))).  Padding taps are ignored (torch pads with -inf); 2 * padding <= kernel.
 * x: N*C*H*W bytes, out: N*C*OH*OW bytes.  Sub-8-bit packed streams are not taken (QE_ERR_UNSUPPORTED from the bindings,
 * which know the stream's width; this entry point sees bytes only). */
int qe_maxpool2d_codes(const uint8_t *x, int32_t N, int32_t C, int32_t H, int32_t W, int32_t kernel, int32_t stride,
                       int32_t padding, uint8_t *out, qe_stream_t stream);

/* ---- quantised ReLU and pooling layers: module forms ------------------------------------------------------------------
 * The packed forwards of the reference's QuantReLU, QuantMaxPool2d and QuantAdaptiveAvgPool2d (modelzoo/modules/quantrelu.py:
 * 81-86, quant_pooling.py:90-97, :159-165): `x, s, z = a_quantizer(x)` and then relu | max_pool2d | adaptive_avg_pool2d of
 * (x + z) * s.  fp32 NCHW in, fp32 out, one pass, no workspace, asynchronous on stream.
 * rq     the layer's activation quantiser in the MODULE's convention; n_bits and sign are ignored (nothing is packed).
 *        n_param 1 (per tensor) or C (per channel; a plane is one channel).
 * qdq(v) = (clamp(rint(v / scale - zero), qmin, qmax) + zero) * scale, each step one fp32 operation in this order: IEEE
 *        division, subtraction, round half to even, clamp (a NaN passes the clamp; +-inf clamps to qmax / qmin), addition,
 *        multiplication (quantizer.py:31,215, quant_pooling.py:95), element for element; no step is fused with another.
 * x, out 4-byte aligned (any such alignment takes the same kernel); QE_ERR_ARG for a NULL operand, a negative size, an
 *        n_param that is neither 1 nor the channel count, or out overlapping x, scale or zero (except x == out where stated).
 *
 * qe_quant_relu          out[i] = relu(qdq(x[i])) for i < n, relu(y) = y when y > 0 or y is NaN, else +0.  The channel of element
 *        i is (i / inner) % n_param (NCHW: inner = H*W), as qe_quantize_pack; any n_param >= 1.  x == out (in place) is allowed,
 *        as QuantReLU(inplace=True).
 * qe_quant_maxpool2d     geometry as qe_maxpool2d_codes: square kernel / stride / padding, dilation 1, ceil_mode false,
 *        2 * padding <= kernel, OH = (H + 2 * padding - kernel) / stride + 1, padding taps ignored.  out[n,c,oh,ow] = the maximum
 *        of qdq(tap) over the in-bounds taps of the window; a window that holds a NaN tap gives NaN; +0 and -0 compare equal and
 *        either may come back.  qdq is non-decreasing for scale > 0, so the kernel takes the maximum of the raw taps and applies
 *        qdq once (the same bits); planes whose scale is not > 0 are done tap by tap.  The ABI has no dilation or return_indices
 *        argument: the bindings answer those with QE_ERR_UNSUPPORTED.
 * qe_quant_adaptive_avgpool2d   the window of output (oh, ow) is rows floor(oh * H / OH) .. ceil((oh + 1) * H / OH) - 1 and
 *        columns floor(ow * W / OW) .. ceil((ow + 1) * W / OW) - 1 (torch's rule).  out = sum / (float)cnt, where sum starts at
 *        +0 and adds qdq(tap) in fp32 tap by tap, rows outer, columns inner, both ascending; cnt is the tap count; one fp32
 *        division.  THIS SEQUENCE IS THE CONTRACT: torch's CPU adaptive_avg_pool2d does not add in a fixed sequential order, so
 *        the result is within (cnt + 1) * 2^-24 * max|qdq(tap)| of torch's and of the exact mean, not torch's bit pattern. */
int qe_quant_relu(const float *x, int64_t n, int64_t inner, const qe_requant *rq, float *out, qe_stream_t stream);
int qe_quant_maxpool2d(const float *x, int32_t N, int32_t C, int32_t H, int32_t W, int32_t kernel, int32_t stride,
                       int32_t padding, const qe_requant *rq, float *out, qe_stream_t stream);
int qe_quant_adaptive_avgpool2d(const float *x, int32_t N, int32_t C, int32_t H, int32_t W, int32_t OH, int32_t OW,
                                const qe_requant *rq, float *out, qe_stream_t stream);

/* ---- qe_avgpool2d_codes -- average pooling of 8-bit stored codes, fp32 and / or the consumer's codes out ---------------
 * What stands between two quantised layers in CLIP's ModifiedResNet (AvgPool2d(2) after the stem, AvgPool2d(stride) in
 * front of the strided convs) and at the end of wrn_40_2 (avg_pool2d(out, 8)); AdaptiveAvgPool2d too.
 * x       N*C*H*W stored codes, one byte each (n_bits == 8; sub-8-bit streams return QE_ERR_UNSUPPORTED); q = byte - 128 when
 *         sign, else byte; scale / zero' in the KERNEL convention (q - zero') * scale; n_param 1 or C.
 * kernel  > 0: kernel x kernel windows at `stride`, no padding, floor mode (nn.AvgPool2d(kernel, stride)); OH and OW must equal
 *         (H - kernel) / stride + 1 and (W - kernel) / stride + 1 (else QE_ERR_ARG).
 *         == 0: adaptive windows to (OH, OW) by the rule of qe_quant_adaptive_avgpool2d (stride is ignored); (1, 1) is the
 *         global pool.
 * value   cnt = taps of the window, fc = (float)cnt.  All operations are single fp32 operations, none fused:
 *         relu == 0:  S = the exact integer sum of q over the window;  y = (scale * ((float)S - fc * zero')) / fc.
 *         relu != 0:  t = (float)q - zero';  r = t when t > 0 or t is NaN, else +0;  R = the fp32 sum of r over the window, from +0,
 *                     tap by tap, rows outer, columns inner, both ascending;  y = (scale * R) / fc.
 *                     (The producer's codes are pre-ReLU.  For an integer zero' with |zero'| <= 256 and cnt * 512 < 2^24 every
 *                     partial sum is an exact integer, so R is the exact integer sum in any order; the kernels use that.)
 *         A window with cnt * 255 >= 2^24 returns QE_ERR_UNSUPPORTED ((float)S would round).
 * out     fp32[N*C*OH*OW], 4-byte aligned; may be NULL when rq != NULL.
 * rq, codes  the consumer's quantiser (module convention; n_param 1 or C) and its packed stream: bit-identical to
 *         qe_quantize_pack(y, rq->scale, rq->zero, rq->n_param, OH*OW, ...) for every n_bits.  codes without rq, rq without codes
 *         and out == codes == NULL are QE_ERR_ARG, as is an output (out, codes, status) overlapping an operand or another output.
 * status  as qe_tpack.     No workspace.  Asynchronous on stream; no host synchronisation, allocation or free.
 * qe_avgpool2d_codes_path (host only): the instance the call with these arguments launches, from the one plan the launch reads:
 *         1 pair   kernel == stride == 2 (rq NULL or 8-bit): a thread makes 16 adjacent outputs of a row from 2 x 32 input bytes
 *                  (two 16-byte loads per row at any alignment, horizontal pair sums by byte dot products, 16-byte stores);
 *         2 plane  the one window is the whole plane (adaptive (1, 1), or kernel == H == W; rq NULL or 8-bit): 2^k lanes per
 *                  plane read it in aligned 16-byte pieces, several planes per workgroup, any plane size the value rule admits;
 *         0 plain  one thread per output (8 consecutive outputs per thread for a sub-8-bit rq, whose bytes it then owns);
 *        -1 none   (the call returns QE_ERR_ARG or QE_ERR_UNSUPPORTED).
 *         out / codes are looked at for being NULL only: no instance depends on an alignment. */
int qe_avgpool2d_codes_path(const qe_qparam *x, int32_t N, int32_t C, int32_t H, int32_t W, int32_t kernel, int32_t stride,
                            int32_t OH, int32_t OW, int32_t relu, const float *out, const qe_requant *rq, const uint8_t *codes);
int qe_avgpool2d_codes(const qe_qparam *x, int32_t N, int32_t C, int32_t H, int32_t W, int32_t kernel, int32_t stride,
                       int32_t OH, int32_t OW, int32_t relu, float *out, const qe_requant *rq, uint8_t *codes, int32_t *status,
                       qe_stream_t stream);

/* ---- qe_affine_relu_quantize_pack -- the boundary between two convolutions of a pre-activation network -------------------
 * What stands between conv2 of one WideResNet block and conv1 / convShortcut of the next (modelzoo/cnns/wideresnet.py:29-37):
 * torch.add, an eval-mode BatchNorm2d that no producer can absorb, ReLU, and the Quantizer + tpack of each consumer, in one pass.
 * All operations are single fp32 operations in this order, none fused:
 *   s[n,c,p]  = x[n,c,p] + identity[n,c,p]            (identity NULL: s = x)
 *   a[n,c,p]  = relu(s * alpha[c] + shift[c])         one multiplication, then one addition; relu(t) = t when t > 0 or t is NaN,
 *                                                     else +0 (torch.relu)
 *   codes[i]  = qe_quantize_pack(a, rq[i].scale, rq[i].zero, rq[i].n_param, P, ...)   for i < n_out, bit-identical
 * x, identity   fp32 NCHW (N, C, P = H*W), 4-byte aligned.
 * alpha, shift  device fp32[C]: the BatchNorm as the per-channel affine ATen applies in eval mode, alpha = gamma / sqrt(var + eps)
 *               and shift = beta - mean * alpha, derived by the caller (once, on the host): no square root is part of this contract.
 * n_out, rq[], codes[]  n_out in 0..2 host arrays: rq[i] in the MODULE's convention, n_param 1 or C, any n_bits in 1..8 and either
 *               sign; codes[i] device, qe_packed_nbytes(N*C*P, rq[i].n_bits) bytes, any alignment.
 * sum_out       fp32[N*C*P] or NULL: s, the residual stream the next equal-width block adds to.  It may be x or identity itself
 *               (in place).
 * act_out       fp32[N*C*P] or NULL: a (the network's tail takes it with n_out == 0).
 * status        as qe_tpack; a function of the N*C*P values alone.  When it comes back set the codes of the offending elements
 *               are unspecified.
 * No workspace, no prepared table, one kernel launch in every form.  Asynchronous on stream; no host synchronisation.
 * Refused before any device work, in this order: n_out outside 0..2 or rq NULL with n_out > 0 (QE_ERR_ARG); per rq[i] a NULL
 * scale / zero (QE_ERR_ARG), n_bits outside 1..8 (QE_ERR_NBITS), n_param < 1 (QE_ERR_ARG); N, C or P <= 0; an n_param that is
 * neither 1 nor C; a NULL x, alpha, shift or codes[i]; n_out == 0 with sum_out == act_out == NULL; an fp32 pointer or status that
 * is not 4-byte aligned (all QE_ERR_ARG); then any overlap of an output (sum_out, act_out, codes[i], status) with an operand or
 * another output, except sum_out == x and sum_out == identity (QE_ERR_ARG).
 * qe_affine_relu_quantize_pack_path (host only): the instance the call launches, from the one plan the launch reads:
 *         1 fast   every rq[i] 8-bit (or n_out == 0) and P % 16 == 0: a thread owns 16 consecutive elements of one plane (16-byte
 *                  loads and stores at any alignment, one 16-byte store of codes per consumer, alpha / shift / scales read once);
 *         0 plain  everything else (a sub-8-bit consumer, a ragged P): a thread owns 8 consecutive elements, whose b-bit codes
 *                  are b whole bytes; grid-stride;
 *        -1 none   (the call returns an error).
 *         sum_out / act_out are looked at for being NULL only: no instance depends on an alignment. */
int qe_affine_relu_quantize_pack_path(int32_t N, int32_t C, int32_t P, int32_t n_out, const qe_requant *rq, const float *sum_out,
                                      const float *act_out);
int qe_affine_relu_quantize_pack(const float *x, const float *identity, int32_t N, int32_t C, int32_t P, const float *alpha,
                                 const float *shift, int32_t n_out, const qe_requant *rq, uint8_t *const *codes, float *sum_out,
                                 float *act_out, int32_t *status, qe_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* QUANT_ENGINE_H */
