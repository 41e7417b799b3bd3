// qe_api.hip -- C-ABI entry points that are not tied to one kernel file: error strings, version, the conv dispatch (generic
// fp32 vs int8 MFMA), the depthwise / grouped run path and the pooling module forms.  Host code only: the checks every
// request shares are in qe_request.hpp, every kernel and its launch in the file of its family.
#include "qe_common.h"
#include "qe_conv_plan.hpp"
#include "qe_conv_dw.hpp"
#include "qe_conv_grp.hpp"
#include "qe_pool.hpp"
#include "qe_preact.hpp"

#include <atomic>
#include <cstring>
#include <mutex>
#include <string>
#include <utility>
#include <vector>
#include <unistd.h>

extern char **environ;

namespace qe {

thread_local int g_last_hip_error = 0;

namespace {
struct EnvSnapshot {
    std::vector<std::pair<std::string, std::string>> kv;
};
std::atomic<EnvSnapshot *> g_env{nullptr};
std::mutex g_env_mutex;
EnvSnapshot *take_env_snapshot()
{
    auto *snap = new EnvSnapshot;
    for (char **e = environ; e != nullptr && *e != nullptr; ++e) {
        if (std::strncmp(*e, "QE_", 3) != 0) continue;
        const char *eq = std::strchr(*e, '=');
        if (eq == nullptr) continue;
        snap->kv.emplace_back(std::string(*e, eq - *e), std::string(eq + 1));
    }
    return snap;
}
}  // namespace

const char *env_get(const char *name)
{
    EnvSnapshot *snap = g_env.load(std::memory_order_acquire);
    if (snap == nullptr) {
        std::lock_guard<std::mutex> lock(g_env_mutex);
        snap = g_env.load(std::memory_order_acquire);
        if (snap == nullptr) {
            snap = take_env_snapshot();
            g_env.store(snap, std::memory_order_release);
        }
    }
    for (const auto &kv : snap->kv)
        if (kv.first == name) return kv.second.c_str();
    return nullptr;
}

int launch_conv_generic(bool packed_in, const void *x, const qe_qparam *xq, const qe_qparam *w,
                        const float *bias, const qe_conv_shape *sh, float *out, hipStream_t s);

// qe_tpack.hip: the two-pass form of the residual block end
int launch_residual_relu_quant(const float *y, const float *identity, float *out, int64_t n, int64_t inner, const qe_requant *rq,
                               uint8_t *codes, int32_t *status, hipStream_t s);

static int check_shape(const qe_conv_shape *sh)
{
    if (sh == nullptr) return QE_ERR_ARG;
    if (sh->N < 0 || sh->IC <= 0 || sh->H <= 0 || sh->W <= 0 || sh->OC < 0 || sh->KH <= 0 || sh->KW <= 0 ||
        sh->stride <= 0 || sh->padding < 0)
        return QE_ERR_ARG;
    return QE_OK;
}

// scale / zero arrays: one element, or one per channel (IC for activations, OC for weights) -- anything else would be
// indexed out of bounds by channel (the reference reads scale[ic] / scale[oc] unchecked, quantconv2d.cu:112-127)
static int check_nparam(const qe_qparam *x, const qe_qparam *w, const qe_conv_shape *sh)
{
    if (x != nullptr && !(x->n_param == 1 || x->n_param >= sh->IC)) return QE_ERR_ARG;
    if (!(w->n_param == 1 || w->n_param >= sh->OC)) return QE_ERR_ARG;
    return QE_OK;
}

// what every packed-conv entry point checks first, in this order: the shape, the input operand, the weight operand, the
// scale counts
static int check_packed_conv(const qe_conv_shape *sh, const qe_qparam *x, const qe_qparam *w)
{
    int rc = check_shape(sh);
    if (rc != QE_OK) return rc;
    if ((rc = check_qparam(x)) != QE_OK) return rc;
    if ((rc = check_qparam(w)) != QE_OK) return rc;
    return check_nparam(x, w, sh);
}

}  // namespace qe

extern "C" const char *qe_error_string(int status)
{
    switch (status) {
        case QE_OK: return "ok";
        case QE_ERR_NBITS: return "n_bits must be in the range (0, 8]";          // tpack.cu:13
        case QE_ERR_RANGE: return "The input tensor is out of range.";           // tpack.cu:14
        case QE_ERR_DTYPE: return "unsupported element type";
        case QE_ERR_ARG: return "invalid argument";
        case QE_ERR_HIP: return "HIP runtime error";
        case QE_ERR_WORKSPACE: return "workspace too small";
        case QE_ERR_UNSUPPORTED: return "problem shape not supported by the gfx950 kernels";
        default: return "unknown error";
    }
}

extern "C" int qe_last_hip_error(void) { return qe::g_last_hip_error; }

// Not part of the public ABI (absent from include/quant_engine.h): take a fresh snapshot of the QE_* environment knobs.
// Old snapshots are kept alive (a few hundred bytes each): a concurrent reader may still hold a pointer into one.
extern "C" void qe_debug_reload_env(void)
{
    std::lock_guard<std::mutex> lock(qe::g_env_mutex);
    qe::g_env.store(qe::take_env_snapshot(), std::memory_order_release);
}
extern "C" const char *qe_version(void) { return "quantize_amd 0.1.0"; }
extern "C" const char *qe_target_arch(void) { return "gfx950"; }

// ---- packed-activation convolutions: every entry point plans once (plan_conv, qe_conv_plan.hip) and reads the plan ----
namespace qe {
// The plan of a dense request.  What the entry points differ in: the consumer (rq, NULL: none), the residual block end and
// the destinations (a query passes NULL for the ones it does not know).
static ConvPlan plan_request(const qe_conv_shape *sh, const qe_qparam *x, const qe_qparam *w, const qe_requant *rq = nullptr,
                             bool residual = false, const float *out = nullptr, const uint8_t *codes = nullptr)
{
    ConvRequest r{sh, x, w, reinterpret_cast<uintptr_t>(out), reinterpret_cast<uintptr_t>(codes)};
    if (rq != nullptr) { r.rq_bits = rq->n_bits; r.rq_n_param = rq->n_param; }
    r.residual = residual;
    return plan_conv(r);
}
// a request that names only the operands' bits (workspace queries)
static ConvPlan plan_bits(const qe_conv_shape *sh, int x_bits, int w_bits)
{
    qe_qparam x{}, w{};
    x.n_bits = x_bits; x.n_param = 1;
    w.n_bits = w_bits; w.n_param = 1;
    return plan_request(sh, &x, &w);
}
// scratch of a run on a prepared buffer, rounded up to 256 bytes (the two-pass epilogues put the fp32 y behind it)
static size_t scratch_bytes(const ConvPlan &p) { return (p.m.total - p.m.prep_total + 255) / 256 * 256; }
// the fp32 y of a two-pass epilogue, behind the conv scratch; NULL: the workspace holds less than both (a non-empty output
// has y_bytes > 0, so a NULL workspace never passes)
static float *two_pass_y(const ConvPlan &p, void *workspace, size_t workspace_bytes)
{
    if (workspace == nullptr || workspace_bytes < scratch_bytes(p) + p.y_bytes) return nullptr;
    return reinterpret_cast<float *>(static_cast<uint8_t *>(workspace) + scratch_bytes(p));
}
}  // namespace qe

extern "C" size_t qe_quantconv2d_workspace_bytes(const qe_conv_shape *shape, int x_bits, int w_bits)
{
    if (qe::check_shape(shape) != QE_OK) return 0;
    return qe::plan_bits(shape, x_bits, w_bits).m.total;
}

extern "C" int qe_quantconv2d_path(const qe_conv_shape *shape, const qe_qparam *x, const qe_qparam *w)
{
    if (qe::check_shape(shape) != QE_OK || x == nullptr || w == nullptr) return 0;
    return qe::plan_request(shape, x, w).route != qe::ConvRoute::Generic ? 1 : 0;
}

// the plan of a request, field by field (tests, bench, profiles): decides nothing, reads no knob of its own
extern "C" int qe_quantconv2d_plan_info(const qe_conv_shape *shape, const qe_qparam *x, const qe_qparam *w, const qe_requant *rq,
                                        const float *out, const uint8_t *codes, qe_conv_plan_info *info)
{
    using namespace qe;
    if (check_shape(shape) != QE_OK || x == nullptr || w == nullptr || info == nullptr) return QE_ERR_ARG;
    const ConvPlan p = plan_request(shape, x, w, rq, false, out, codes);
    const MfmaPlan &m = p.m;
    const bool mfma = p.route == ConvRoute::Mfma;
    qe_conv_plan_info i{};
    i.route = (int)p.route; i.fused = p.fused;
    i.family = (int)m.family; i.cfg = m.cfg; i.niw = m.niw; i.kkt = mfma_kkt(m.KK, p.run.KW); i.ns = m.NS; i.split = p.split;
    i.wraw = m.wraw;
    i.rq = mfma && p.fused; i.patch = p.rq_patch;          // what the re-quantising entry point hands launch_conv_mfma
    i.has_instance = mfma && mfma_instance(m, p.run.KW, p.split, i.rq != 0, p.rq_patch) != nullptr;
    i.ctab = p.ctab; i.gi = m.GI; i.th = m.TH; i.ni = m.ni; i.mt = m.MT; i.nch = m.NCH; i.oh = m.OH; i.ow = m.OW;
    i.rowmul = m.ROWMUL; i.colmul = m.COLMUL;
    i.pre = (int)p.pre; i.sub2_log_up = p.sub2_log_up; i.expand = m.expand; i.sub_x4 = m.sub_x4;
    i.fd_w8 = p.fd_w8;
    i.pwr_tw = p.pwr_tw; i.pwr_ks = p.pwr_ks; i.pwr_groups = p.pwr_groups; i.pwr7_gi = p.pwr7_gi; i.pwr_s2 = p.pwr_s2;
    i.lds = (int64_t)p.lds; i.blocks = p.blocks; i.total = (int64_t)m.total; i.prep_total = (int64_t)m.prep_total;
    i.y_bytes = (int64_t)p.y_bytes;
    *info = i;
    return QE_OK;
}

extern "C" int qe_conv_mfma_has_instance(int32_t family, int32_t cfg, int32_t niw, int32_t kkt, int32_t ns, int32_t split,
                                         int32_t wraw, int32_t rq, int32_t patch)
{
    using namespace qe;
    if (family <= (int)MfmaFamily::None || family > (int)MfmaFamily::Flatg) return 0;
    if (kkt != 1 && kkt != 9 && kkt != 0) return 0;
    MfmaPlan m;
    m.family = (MfmaFamily)family; m.cfg = cfg; m.niw = niw; m.NS = ns; m.wraw = wraw != 0;
    const int KW = kkt == 1 ? 1 : (kkt == 9 ? 3 : 5);      // a kernel size with that tap form
    m.KK = KW * KW;
    return mfma_instance(m, KW, split, rq != 0, patch != 0) != nullptr ? 1 : 0;
}

extern "C" int qe_quantconv2d(const qe_qparam *x, const qe_qparam *w, const float *bias,
                              const qe_conv_shape *shape, float *out,
                              void *workspace, size_t workspace_bytes, qe_stream_t stream)
{
    using namespace qe;
    const int rc = check_packed_conv(shape, x, w);
    if (rc != QE_OK) return rc;
    if (out == nullptr) return QE_ERR_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const ConvPlan p = plan_request(shape, x, w, nullptr, false, out);
    if (p.route == ConvRoute::Generic) return launch_conv_generic(true, x->data, x, w, bias, shape, out, s);
    return launch_conv_mfma(p, x, w, bias, shape, out, workspace, workspace_bytes, nullptr, 0, false, s, nullptr, nullptr, nullptr, nullptr);
}

extern "C" size_t qe_conv_prepared_bytes(const qe_conv_shape *shape, int x_bits, int w_bits)
{
    if (qe::check_shape(shape) != QE_OK) return 0;
    return qe::plan_prepared(shape, x_bits, w_bits).prep_total;
}

extern "C" uint64_t qe_conv_prepared_layout(const qe_conv_shape *shape, int x_bits, int w_bits)
{
    if (qe::check_shape(shape) != QE_OK) return 0;
    return qe::prepared_layout(qe::plan_prepared(shape, x_bits, w_bits), shape);
}

extern "C" size_t qe_quantconv2d_prepared_workspace_bytes(const qe_conv_shape *shape, int x_bits, int w_bits)
{
    if (qe::check_shape(shape) != QE_OK) return 0;
    const qe::ConvPlan p = qe::plan_bits(shape, x_bits, w_bits);
    return p.m.total - p.m.prep_total;
}

extern "C" int qe_conv_prepare(const qe_qparam *w, const float *bias, const qe_conv_shape *shape, int x_bits,
                               void *prepared, size_t prepared_bytes, qe_stream_t stream)
{
    using namespace qe;
    int rc = check_shape(shape);
    if (rc != QE_OK) return rc;
    if ((rc = check_qparam(w)) != QE_OK) return rc;
    if ((rc = check_nparam(nullptr, w, shape)) != QE_OK) return rc;
    if (!(x_bits > 0 && x_bits <= 8)) return QE_ERR_NBITS;
    return prepare_conv_tables(plan_prepared(shape, x_bits, w->n_bits), w, bias, shape, prepared, prepared_bytes,
                               static_cast<hipStream_t>(stream));
}

extern "C" int qe_quantconv2d_prepared(const qe_qparam *x, const qe_qparam *w, const float *bias,
                                       const qe_conv_shape *shape, const void *prepared, size_t prepared_bytes,
                                       float *out, void *workspace, size_t workspace_bytes, qe_stream_t stream)
{
    using namespace qe;
    const int rc = check_packed_conv(shape, x, w);
    if (rc != QE_OK) return rc;
    if (out == nullptr) return QE_ERR_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const ConvPlan p = plan_request(shape, x, w, nullptr, false, out);
    if (p.route == ConvRoute::Generic)   // per-channel activation scales: nothing is prepared
        return launch_conv_generic(true, x->data, x, w, bias, shape, out, s);
    return launch_conv_mfma(p, x, w, bias, shape, out, workspace, workspace_bytes, prepared, prepared_bytes, true, s, nullptr,
                            nullptr, nullptr, nullptr);
}

// ---- fused re-quantisation (conv-epilogue form) ----
extern "C" int qe_quantconv2d_requant_path(const qe_conv_shape *shape, const qe_qparam *x, const qe_qparam *w, const qe_requant *rq)
{
    if (qe::check_shape(shape) != QE_OK || x == nullptr || w == nullptr || rq == nullptr) return 0;
    return qe::plan_request(shape, x, w, rq).fused ? 1 : 0;
}

extern "C" size_t qe_quantconv2d_requant_workspace_bytes(const qe_conv_shape *shape, const qe_qparam *x, const qe_qparam *w,
                                                         const qe_requant *rq)
{
    if (qe::check_shape(shape) != QE_OK || x == nullptr || w == nullptr || rq == nullptr) return 0;
    const qe::ConvPlan p = qe::plan_request(shape, x, w, rq);
    return p.fused ? qe::scratch_bytes(p) : qe::scratch_bytes(p) + p.y_bytes;
}

extern "C" int qe_quantconv2d_requant_prepared(const qe_qparam *x, const qe_qparam *w, const float *bias,
                                               const qe_conv_shape *shape, const void *prepared, size_t prepared_bytes,
                                               const qe_requant *rq, uint8_t *out, int32_t *status,
                                               void *workspace, size_t workspace_bytes, qe_stream_t stream)
{
    using namespace qe;
    int rc = check_packed_conv(shape, x, w);
    if (rc != QE_OK) return rc;
    if ((rc = check_requant(rq)) != QE_OK) return rc;
    if (out == nullptr) return QE_ERR_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const ConvPlan p = plan_request(shape, x, w, rq, false, nullptr, out);
    if (p.OH <= 0 || p.OW <= 0) return QE_ERR_ARG;
    if (shape->N == 0 || shape->OC == 0) return QE_OK;
    if (p.fused)
        return launch_conv_mfma(p, x, w, bias, shape, nullptr, workspace, workspace_bytes, prepared, prepared_bytes, true, s, rq,
                                out, status, nullptr);
    // two passes: y in fp32 behind the conv scratch, then the fused quantise + pack kernel (bit-identical by construction)
    float *y = two_pass_y(p, workspace, workspace_bytes);
    if (y == nullptr) return QE_ERR_WORKSPACE;
    rc = qe_quantconv2d_prepared(x, w, bias, shape, prepared, prepared_bytes, y, workspace, scratch_bytes(p), stream);
    if (rc != QE_OK) return rc;
    const int64_t plane = (int64_t)p.OH * p.OW;
    return qe_quantize_pack(y, (int64_t)shape->N * shape->OC * plane, rq->scale, rq->zero, rq->n_param, plane, rq->qmin,
                            rq->qmax, rq->n_bits, rq->sign, out, status, stream);
}

// ---- residual block end: out = relu(conv + identity), optionally with the consumer's codes ----
extern "C" int qe_quantconv2d_residual_path(const qe_conv_shape *shape, const qe_qparam *x, const qe_qparam *w, const qe_requant *rq)
{
    if (qe::check_shape(shape) != QE_OK || x == nullptr || w == nullptr) return 0;
    return qe::plan_request(shape, x, w, rq, true).fused ? 1 : 0;
}

extern "C" size_t qe_quantconv2d_residual_workspace_bytes(const qe_conv_shape *shape, const qe_qparam *x, const qe_qparam *w,
                                                          const qe_requant *rq)
{
    if (qe::check_shape(shape) != QE_OK || x == nullptr || w == nullptr) return 0;
    const qe::ConvPlan p = qe::plan_request(shape, x, w, rq, true);
    return p.fused ? 0 : qe::scratch_bytes(p) + p.y_bytes;   // the fused kernel reads no scratch
}

extern "C" int qe_quantconv2d_residual_prepared(const qe_qparam *x, const qe_qparam *w, const float *bias,
                                                const qe_conv_shape *shape, const void *prepared, size_t prepared_bytes,
                                                const float *identity, float *out, const qe_requant *rq, uint8_t *codes,
                                                int32_t *status, void *workspace, size_t workspace_bytes, qe_stream_t stream)
{
    using namespace qe;
    int rc = check_packed_conv(shape, x, w);
    if (rc != QE_OK) return rc;
    if (rq != nullptr && (rc = check_requant(rq)) != QE_OK) return rc;
    if (rq != nullptr && !(rq->n_param == 1 || rq->n_param >= shape->OC)) return QE_ERR_ARG;
    if (identity == nullptr || (rq != nullptr && codes == nullptr) || (out == nullptr && rq == nullptr)) return QE_ERR_ARG;
    // 16-byte aligned fp32 tensors, 4-byte aligned codes: what every device allocator returns
    if (((reinterpret_cast<uintptr_t>(identity) | reinterpret_cast<uintptr_t>(out)) & 15) != 0 ||
        (reinterpret_cast<uintptr_t>(codes) & 3) != 0)
        return QE_ERR_ARG;
    const ConvPlan p = plan_request(shape, x, w, rq, true, out, codes);
    if (p.OH <= 0 || p.OW <= 0) return QE_ERR_ARG;
    const int64_t n = (int64_t)shape->N * shape->OC * p.OH * p.OW;
    if (!same_or_disjoint(out, identity, n * 4)) return QE_ERR_ARG;   // in place is allowed; any other overlap is not
    if (n == 0) return QE_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (p.fused) return launch_pwr(p, x, w, bias, out, s, rq, codes, status, identity);
    // two passes: the conv's fp32 y (into out, unless out is NULL or IS the identity: then behind the conv scratch), then
    // one elementwise pass y + identity -> out and codes
    float *y = two_pass_y(p, workspace, workspace_bytes);
    if (y == nullptr) return QE_ERR_WORKSPACE;
    if (out != nullptr && out != identity) y = out;
    rc = qe_quantconv2d_prepared(x, w, bias, shape, prepared, prepared_bytes, y, workspace, scratch_bytes(p), stream);
    if (rc != QE_OK) return rc;
    return launch_residual_relu_quant(y, identity, out, n, (int64_t)p.OH * p.OW, rq, codes, status, s);
}

// ---- float-input convolutions: every entry point that can take the MFMA kernels plans once (plan_conv_f32) ----
static int check_float_input(const qe_conv_shape *shape, const qe_qparam *w, bool operands)
{
    int rc = qe::check_shape(shape);
    if (rc != QE_OK) return rc;
    if ((rc = qe::check_qparam(w)) != QE_OK) return rc;
    if ((rc = qe::check_nparam(nullptr, w, shape)) != QE_OK) return rc;
    return operands ? QE_OK : QE_ERR_ARG;
}

// no workspace, so no prepared tables: always the VALU kernel
extern "C" int qe_quantconv2d_float_input(const float *x, const qe_qparam *w, const float *bias,
                                          const qe_conv_shape *shape, float *out, qe_stream_t stream)
{
    const int rc = check_float_input(shape, w, x != nullptr && out != nullptr);
    if (rc != QE_OK) return rc;
    return qe::launch_conv_generic(false, x, nullptr, w, bias, shape, out, static_cast<hipStream_t>(stream));
}

extern "C" int qe_quantconv2d_float_input_path(const qe_conv_shape *shape, const qe_qparam *w)
{
    if (qe::check_shape(shape) != QE_OK || w == nullptr) return 0;
    return qe::plan_conv_f32(shape).ok ? 1 : 0;
}

// the plan of a float-input request, field by field (tests, bench, profiles): decides nothing
extern "C" int qe_conv_f32_plan_info(const qe_conv_shape *shape, qe_conv_f32_plan *info)
{
    if (qe::check_shape(shape) != QE_OK || info == nullptr) return QE_ERR_ARG;
    const qe::F32Plan p = qe::plan_conv_f32(shape);
    qe_conv_f32_plan i{};
    i.ok = p.ok; i.kernel = (int)p.kernel; i.stem = p.stem;
    i.OCP = p.OCP; i.NG = p.NG; i.KK = p.KK; i.OH = p.OH; i.OW = p.OW; i.TH = p.TH; i.GI = p.GI;
    i.IHT = p.IHT; i.IWP = p.IWP; i.ROWMUL = p.ROWMUL; i.COLMUL = p.COLMUL;
    i.chunk = p.chunk; i.n_pix_tiles = p.n_pix_tiles; i.n_oc_tiles = p.n_oc_tiles; i.tiles_h = p.tiles_h;
    i.blocks = p.blocks; i.lds = (int64_t)p.lds; i.ep_off = (int64_t)p.ep_off; i.total = (int64_t)p.total;
    *info = i;
    return QE_OK;
}

extern "C" size_t qe_quantconv2d_float_input_workspace_bytes(const qe_conv_shape *shape, int w_bits)
{
    (void)w_bits;
    if (qe::check_shape(shape) != QE_OK) return 0;
    return qe::plan_conv_f32(shape).total;
}

extern "C" int qe_quantconv2d_float_input_ws(const float *x, const qe_qparam *w, const float *bias,
                                             const qe_conv_shape *shape, float *out, void *workspace,
                                             size_t workspace_bytes, qe_stream_t stream)
{
    int rc = check_float_input(shape, w, x != nullptr && out != nullptr);
    if (rc != QE_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const qe::F32Plan p = qe::plan_conv_f32(shape);
    if (!p.ok) return qe::launch_conv_generic(false, x, nullptr, w, bias, shape, out, s);
    if ((rc = qe::prepare_conv_f32(p, w, bias, shape, workspace, workspace_bytes, s)) != QE_OK) return rc;
    return qe::launch_conv_f32(p, x, shape, workspace, workspace_bytes, out, s);
}

extern "C" int qe_conv_f32_prepare(const qe_qparam *w, const float *bias, const qe_conv_shape *shape,
                                   void *prepared, size_t prepared_bytes, qe_stream_t stream)
{
    const int rc = check_float_input(shape, w, true);
    if (rc != QE_OK) return rc;
    const qe::F32Plan p = qe::plan_conv_f32(shape);
    if (!p.ok) return QE_OK;          // nothing to prepare: the VALU kernel reads the packed weights
    return qe::prepare_conv_f32(p, w, bias, shape, prepared, prepared_bytes, static_cast<hipStream_t>(stream));
}

extern "C" int qe_quantconv2d_float_input_prepared(const float *x, const qe_qparam *w, const float *bias,
                                                   const qe_conv_shape *shape, const void *prepared,
                                                   size_t prepared_bytes, float *out, qe_stream_t stream)
{
    const int rc = check_float_input(shape, w, x != nullptr && out != nullptr);
    if (rc != QE_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const qe::F32Plan p = qe::plan_conv_f32(shape);
    if (!p.ok) return qe::launch_conv_generic(false, x, nullptr, w, bias, shape, out, s);
    return qe::launch_conv_f32(p, x, shape, prepared, prepared_bytes, out, s);
}

// ---- depthwise and grouped packed convolutions (qe_conv_dw.hip, qe_conv_grp.hip) ----
// A depthwise request is a grouped request with groups == IC == OC, so the two entry families share one request check and
// one run path.  A family supplies what differs: its plan (every query and the launch read one plan: plan_dw / plan_grp),
// its launcher and which of the two entries it is.  The depthwise entries carry no groups argument: groups == 0 stands for it.
namespace qe {
struct DwFamily {
    static constexpr bool depthwise = true;
    static DwPlan plan(const qe_conv_shape *shape, int, const qe_qparam *x, const qe_qparam *w, const qe_requant *rq, const float *out,
                       const uint8_t *codes, bool has_out)
    {
        return plan_dw(DwRequest{shape, x->n_bits, x->sign, w->n_bits, w->sign, rq ? rq->n_bits : 0, has_out,
                                 reinterpret_cast<uintptr_t>(out), reinterpret_cast<uintptr_t>(codes)});
    }
    static int launch(const DwPlan &p, const qe_qparam *x, const qe_qparam *w, const float *bias, const qe_conv_shape *sh, int, int relu,
                      float *out, const qe_requant *rq, uint8_t *codes, int32_t *status, hipStream_t s)
    {
        return launch_dw(p, x, w, bias, sh, relu, out, rq, codes, status, s);
    }
};
struct GrpFamily {
    static constexpr bool depthwise = false;
    static GrpPlan plan(const qe_conv_shape *shape, int groups, const qe_qparam *x, const qe_qparam *w, const qe_requant *rq,
                        const float *out, const uint8_t *codes, bool has_out)
    {
        return plan_grp(GrpRequest{shape, groups, x->n_bits, x->sign, x->n_param, w->n_bits, w->sign, rq ? rq->n_bits : 0, has_out,
                                   reinterpret_cast<uintptr_t>(out), reinterpret_cast<uintptr_t>(codes)});
    }
    static constexpr auto launch = &launch_grp;
};
static_assert((int)DW_NONE == (int)GRP_NONE && (int)DW_PLAIN == (int)GRP_PLAIN, "the queries read both plans' kernel numbers alike");

// shape, groups, operand formats and scale counts of a request (pointers are not looked at).  The order decides which code
// wins: on the depthwise entry OC != IC is refused before the scale counts are looked at; on the grouped entry the groups the
// dense and the depthwise entry points own (they are not forwarded) are refused after them.
static int check_span_request(bool depthwise, const qe_conv_shape *shape, int groups, const qe_qparam *x, const qe_qparam *w,
                              const qe_requant *rq)
{
    int rc = check_shape(shape);
    if (rc != QE_OK) return rc;
    if (x == nullptr || w == nullptr) return QE_ERR_ARG;
    if (!bits_ok(x->n_bits) || !bits_ok(w->n_bits) || (rq != nullptr && !bits_ok(rq->n_bits))) return QE_ERR_NBITS;
    if (depthwise) {
        if (shape->OC != shape->IC) return QE_ERR_UNSUPPORTED;
    } else if (groups < 1 || shape->OC < 1 || shape->IC % groups != 0 || shape->OC % groups != 0) {
        return QE_ERR_ARG;
    }
    if (!one_or_per_channel(x->n_param, shape->IC) || !one_or_per_channel(w->n_param, shape->OC)) return QE_ERR_ARG;
    if (rq != nullptr && !one_or_per_channel(rq->n_param, shape->OC)) return QE_ERR_ARG;
    if (!depthwise && (groups == 1 || (groups == shape->IC && groups == shape->OC))) return QE_ERR_UNSUPPORTED;
    return QE_OK;
}

// 1 = the family's fast kernels, 0 = its plain kernel, -1 = none
template <class F>
static int span_conv_path(const qe_conv_shape *shape, int groups, const qe_qparam *x, const qe_qparam *w, const qe_requant *rq)
{
    if (check_span_request(F::depthwise, shape, groups, x, w, rq) != QE_OK) return -1;
    const auto p = F::plan(shape, groups, x, w, rq, nullptr, nullptr, true);
    return p.kernel == DW_NONE ? -1 : p.kernel == DW_PLAIN ? 0 : 1;
}

// the plan of the request as the call with these destinations would read it, into p
template <class F, class Plan>
static int span_conv_plan(const qe_conv_shape *shape, int groups, const qe_qparam *x, const qe_qparam *w, const qe_requant *rq,
                          const float *out, const uint8_t *codes, const void *info, Plan &p)
{
    if (info == nullptr) return QE_ERR_ARG;
    const int rc = check_span_request(F::depthwise, shape, groups, x, w, rq);
    if (rc != QE_OK) return rc;
    const bool sub8 = rq != nullptr && rq->n_bits < 8;
    p = F::plan(shape, groups, x, w, rq, out, codes, out != nullptr || rq == nullptr || sub8);
    return p.kernel == DW_NONE ? QE_ERR_UNSUPPORTED : QE_OK;
}

template <class F>
static int run_span_conv(const qe_qparam *x, const qe_qparam *w, const float *bias, const qe_conv_shape *shape, int groups, int relu,
                         float *out, const qe_requant *rq, uint8_t *codes, int32_t *status, qe_stream_t stream)
{
    int rc = check_shape(shape);
    if (rc != QE_OK) return rc;
    if ((rc = check_qparam(x)) != QE_OK) return rc;
    if ((rc = check_qparam(w)) != QE_OK) return rc;
    if (rq != nullptr && (rc = check_requant(rq)) != QE_OK) return rc;
    if ((rc = check_span_request(F::depthwise, shape, groups, x, w, rq)) != QE_OK) return rc;
    if ((out == nullptr && codes == nullptr) || (codes != nullptr) != (rq != nullptr)) return QE_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(out) & 3) != 0 || (reinterpret_cast<uintptr_t>(status) & 3) != 0) return QE_ERR_ARG;
    const auto p = F::plan(shape, groups, x, w, rq, out, codes, out != nullptr);
    if (p.kernel == DW_NONE) return QE_ERR_UNSUPPORTED;
    if (p.two_pass && out == nullptr) return QE_ERR_UNSUPPORTED;
    const int IC = shape->IC, OC = shape->OC, icg = F::depthwise ? 1 : IC / groups;
    const int64_t n_in = (int64_t)shape->N * IC * shape->H * shape->W, n = (int64_t)shape->N * OC * p.OH * p.OW;
    // an output may overlap neither an operand nor another output
    const Span outs[3] = {span_of(out, n * 4), span_of(codes, rq ? qe_packed_nbytes(n, rq->n_bits) : 0), span_of(status, 4)};
    const Span ins[9] = {span_of(x->data, qe_packed_nbytes(n_in, x->n_bits)),
                         span_of(w->data, qe_packed_nbytes((int64_t)OC * icg * shape->KH * shape->KW, w->n_bits)),
                         span_of(x->scale, 4 * (int64_t)x->n_param), span_of(x->zero, 4 * (int64_t)x->n_param),
                         span_of(w->scale, 4 * (int64_t)w->n_param), span_of(w->zero, 4 * (int64_t)w->n_param),
                         span_of(bias, 4 * (int64_t)OC), span_of(rq ? rq->scale : nullptr, rq ? 4 * (int64_t)rq->n_param : 0),
                         span_of(rq ? rq->zero : nullptr, rq ? 4 * (int64_t)rq->n_param : 0)};
    if (!outputs_clear(outs, 3, ins, 9)) return QE_ERR_ARG;
    if (n == 0) return QE_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (p.two_pass) {
        if ((rc = F::launch(p, x, w, bias, shape, groups, relu, out, nullptr, nullptr, nullptr, s)) != QE_OK) return rc;
        return qe_quantize_pack(out, n, rq->scale, rq->zero, rq->n_param, (int64_t)p.OH * p.OW, rq->qmin, rq->qmax, rq->n_bits,
                                rq->sign, codes, status, stream);
    }
    return F::launch(p, x, w, bias, shape, groups, relu, out, rq, codes, status, s);
}
}  // namespace qe

extern "C" int qe_quantconv2d_depthwise_path(const qe_conv_shape *shape, const qe_qparam *x, const qe_qparam *w, const qe_requant *rq)
{
    return qe::span_conv_path<qe::DwFamily>(shape, 0, x, w, rq);
}

extern "C" int qe_quantconv2d_depthwise_plan_info(const qe_conv_shape *shape, const qe_qparam *x, const qe_qparam *w, const qe_requant *rq,
                                                  const float *out, const uint8_t *codes, qe_dwconv_plan *info)
{
    qe::DwPlan p;
    const int rc = qe::span_conv_plan<qe::DwFamily>(shape, 0, x, w, rq, out, codes, info, p);
    if (rc != QE_OK) return rc;
    *info = qe_dwconv_plan{p.kernel, p.symmetric, p.G, p.TH, p.vec, p.store16, p.codes4, p.two_pass, p.OH, p.OW, p.bands, p.blocks, p.lds};
    return QE_OK;
}

extern "C" int qe_quantconv2d_depthwise(const qe_qparam *x, const qe_qparam *w, const float *bias, const qe_conv_shape *shape,
                                        int32_t relu, float *out, const qe_requant *rq, uint8_t *codes, int32_t *status,
                                        qe_stream_t stream)
{
    return qe::run_span_conv<qe::DwFamily>(x, w, bias, shape, 0, relu, out, rq, codes, status, stream);
}

extern "C" int qe_quantconv2d_grouped_path(const qe_conv_shape *shape, int32_t groups, const qe_qparam *x, const qe_qparam *w,
                                           const qe_requant *rq)
{
    return qe::span_conv_path<qe::GrpFamily>(shape, groups, x, w, rq);
}

extern "C" int qe_quantconv2d_grouped_plan_info(const qe_conv_shape *shape, int32_t groups, const qe_qparam *x, const qe_qparam *w,
                                                const qe_requant *rq, const float *out, const uint8_t *codes, qe_grpconv_plan *info)
{
    qe::GrpPlan p;
    const int rc = qe::span_conv_plan<qe::GrpFamily>(shape, groups, x, w, rq, out, codes, info, p);
    if (rc != QE_OK) return rc;
    *info = qe_grpconv_plan{p.kernel, p.slab, p.TH, p.TW, p.tiles, p.two_pass, p.out16, p.codes16, p.OH, p.OW, p.blocks, p.lds};
    return QE_OK;
}

extern "C" int qe_quantconv2d_grouped(const qe_qparam *x, const qe_qparam *w, const float *bias, const qe_conv_shape *shape,
                                      int32_t groups, int32_t relu, float *out, const qe_requant *rq, uint8_t *codes,
                                      int32_t *status, qe_stream_t stream)
{
    return qe::run_span_conv<qe::GrpFamily>(x, w, bias, shape, groups, relu, out, rq, codes, status, stream);
}

// ---- quantised ReLU and pooling layers (qe_pool.hip) ----
// The module forms check their request here and hand it to one launcher each; the codes-domain average pool plans once
// (plan_pool, qe_pool.hpp) and the path query and the call read that plan.
namespace qe {
// x, out and the layer's quantiser of a module form: n elements in, n_out out, `channels` planes' worth of scales (0: any count);
// in_place_ok (n_in == n_out): out may be x itself
static int check_module_form(const float *x, int64_t n_in, const qe_requant *rq, float *out, int64_t n_out, int channels, bool in_place_ok)
{
    if (rq == nullptr || rq->scale == nullptr || rq->zero == nullptr || rq->n_param < 1) return QE_ERR_ARG;
    if (channels > 0 && !one_or_per_channel(rq->n_param, channels)) return QE_ERR_ARG;
    if (n_out == 0) return QE_OK;
    if (x == nullptr || out == nullptr) return QE_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(x) & 3) != 0 || (reinterpret_cast<uintptr_t>(out) & 3) != 0) return QE_ERR_ARG;
    const Span o = span_of(out, n_out * 4);
    if (in_place_ok ? !same_or_disjoint(x, out, n_out * 4) : overlaps(o, span_of(x, n_in * 4))) return QE_ERR_ARG;
    const Span q[2] = {span_of(rq->scale, 4 * (int64_t)rq->n_param), span_of(rq->zero, 4 * (int64_t)rq->n_param)};
    return outputs_clear(&o, 1, q, 2) ? QE_OK : QE_ERR_ARG;
}

static PoolPlan plan_pool_request(const qe_qparam *x, int N, int C, int H, int W, int kernel, int stride, int OH, int OW, const float *out,
                                  const qe_requant *rq)
{
    return plan_pool(PoolRequest{N, C, H, W, kernel, stride, OH, OW, x->n_bits, rq != nullptr ? rq->n_bits : 0, out != nullptr});
}

// formats and counts of a codes-domain request (pointers are not looked at)
static int check_pool_request(const qe_qparam *x, int C, const qe_requant *rq)
{
    if (x == nullptr) return QE_ERR_ARG;
    if (!bits_ok(x->n_bits) || (rq != nullptr && !bits_ok(rq->n_bits))) return QE_ERR_NBITS;
    if (!one_or_per_channel(x->n_param, C) || (rq != nullptr && !one_or_per_channel(rq->n_param, C))) return QE_ERR_ARG;
    return QE_OK;
}
}  // namespace qe

extern "C" int qe_quant_relu(const float *x, int64_t n, int64_t inner, const qe_requant *rq, float *out, qe_stream_t stream)
{
    using namespace qe;
    if (n < 0 || inner <= 0) return QE_ERR_ARG;
    const int rc = check_module_form(x, n, rq, out, n, 0, true);
    if (rc != QE_OK || n == 0) return rc;
    return launch_quant_relu(x, n, inner, rq, out, static_cast<hipStream_t>(stream));
}

extern "C" int qe_quant_maxpool2d(const float *x, int32_t N, int32_t C, int32_t H, int32_t W, int32_t kernel, int32_t stride,
                                  int32_t padding, const qe_requant *rq, float *out, qe_stream_t stream)
{
    using namespace qe;
    int OH, OW;
    if (check_pool_window(N, C, H, W, kernel, stride, padding, OH, OW) != QE_OK) return QE_ERR_ARG;
    if ((int64_t)H * W > 0x7fffffffLL) return QE_ERR_UNSUPPORTED;
    const int64_t n_in = (int64_t)N * C * H * W, n = (int64_t)N * C * OH * OW;
    const int rc = check_module_form(x, n_in, rq, out, n, C, false);
    if (rc != QE_OK || n == 0) return rc;
    return launch_quant_maxpool2d(x, N, C, H, W, kernel, stride, padding, OH, OW, rq, out, static_cast<hipStream_t>(stream));
}

extern "C" int qe_quant_adaptive_avgpool2d(const float *x, int32_t N, int32_t C, int32_t H, int32_t W, int32_t OH, int32_t OW,
                                           const qe_requant *rq, float *out, qe_stream_t stream)
{
    using namespace qe;
    if (N < 0 || C < 0 || H <= 0 || W <= 0 || OH <= 0 || OW <= 0) return QE_ERR_ARG;
    if ((int64_t)H * W > 0x7fffffffLL) return QE_ERR_UNSUPPORTED;
    const int64_t n_in = (int64_t)N * C * H * W, n = (int64_t)N * C * OH * OW;
    const int rc = check_module_form(x, n_in, rq, out, n, C, false);
    if (rc != QE_OK || n == 0) return rc;
    return launch_quant_adaptive_avgpool2d(x, N, C, H, W, OH, OW, rq, out, static_cast<hipStream_t>(stream));
}

extern "C" int qe_avgpool2d_codes_path(const qe_qparam *x, int32_t N, int32_t C, int32_t H, int32_t W, int32_t kernel, int32_t stride,
                                       int32_t OH, int32_t OW, int32_t relu, const float *out, const qe_requant *rq, const uint8_t *codes)
{
    (void)relu;
    if (qe::check_pool_request(x, C, rq) != QE_OK || (codes != nullptr) != (rq != nullptr)) return -1;
    return qe::plan_pool_request(x, N, C, H, W, kernel, stride, OH, OW, out, rq).kernel;
}

extern "C" int qe_avgpool2d_codes(const qe_qparam *x, int32_t N, int32_t C, int32_t H, int32_t W, int32_t kernel, int32_t stride,
                                  int32_t OH, int32_t OW, int32_t relu, float *out, const qe_requant *rq, uint8_t *codes,
                                  int32_t *status, qe_stream_t stream)
{
    using namespace qe;
    int rc = check_qparam(x);
    if (rc != QE_OK) return rc;
    if (rq != nullptr && (rc = check_requant(rq)) != QE_OK) return rc;
    if ((rc = check_pool_request(x, C, rq)) != QE_OK) return rc;
    if ((out == nullptr && codes == nullptr) || (codes != nullptr) != (rq != nullptr)) return QE_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(out) & 3) != 0 || (reinterpret_cast<uintptr_t>(status) & 3) != 0) return QE_ERR_ARG;
    const PoolPlan p = plan_pool_request(x, N, C, H, W, kernel, stride, OH, OW, out, rq);
    if (p.kernel == POOL_NONE) return p.rc;
    const int64_t n_in = (int64_t)N * C * H * W, n = (int64_t)N * C * OH * OW;
    // an output may overlap neither an operand nor another output
    const Span outs[3] = {span_of(out, n * 4), span_of(codes, rq ? qe_packed_nbytes(n, rq->n_bits) : 0), span_of(status, 4)};
    const Span ins[5] = {span_of(x->data, n_in), span_of(x->scale, 4 * (int64_t)x->n_param), span_of(x->zero, 4 * (int64_t)x->n_param),
                         span_of(rq ? rq->scale : nullptr, rq ? 4 * (int64_t)rq->n_param : 0),
                         span_of(rq ? rq->zero : nullptr, rq ? 4 * (int64_t)rq->n_param : 0)};
    if (!outputs_clear(outs, 3, ins, 5)) return QE_ERR_ARG;
    if (n == 0) return QE_OK;
    return launch_pool_codes(p, x, N, C, H, W, kernel, stride, relu, out, rq, codes, status, static_cast<hipStream_t>(stream));
}

// ---- the pre-activation boundary (qe_preact.hip): one plan (plan_preact, qe_preact.hpp) for the path query and the call ------------
namespace qe {
static PreactPlan plan_preact_request(int N, int C, int P, int n_out, const qe_requant *rq, const float *sum_out, const float *act_out)
{
    PreactRequest r{N, C, P, n_out, {0, 0}, sum_out != nullptr, act_out != nullptr};
    for (int i = 0; i < n_out && i < PREACT_MAX_OUT; ++i) r.rq_bits[i] = rq[i].n_bits;
    return plan_preact(r);
}

// counts and formats of a request (no address but rq's own is looked at): n_out, then each quantiser, then the sizes, then n_param
static int check_preact_request(int N, int C, int P, int n_out, const qe_requant *rq)
{
    if (n_out < 0 || n_out > PREACT_MAX_OUT || (n_out > 0 && rq == nullptr)) return QE_ERR_ARG;
    for (int i = 0; i < n_out; ++i) {
        const int rc = check_requant(&rq[i]);
        if (rc != QE_OK) return rc;
    }
    if (N <= 0 || C <= 0 || P <= 0) return QE_ERR_ARG;
    for (int i = 0; i < n_out; ++i)
        if (!one_or_per_channel(rq[i].n_param, C)) return QE_ERR_ARG;
    return QE_OK;
}
}  // namespace qe

extern "C" int qe_affine_relu_quantize_pack_path(int32_t N, int32_t C, int32_t P, int32_t n_out, const qe_requant *rq,
                                                 const float *sum_out, const float *act_out)
{
    if (qe::check_preact_request(N, C, P, n_out, rq) != QE_OK) return -1;
    return qe::plan_preact_request(N, C, P, n_out, rq, sum_out, act_out).kernel;
}

extern "C" int qe_affine_relu_quantize_pack(const float *x, const float *identity, int32_t N, int32_t C, int32_t P, const float *alpha,
                                            const float *shift, int32_t n_out, const qe_requant *rq, uint8_t *const *codes,
                                            float *sum_out, float *act_out, int32_t *status, qe_stream_t stream)
{
    using namespace qe;
    const int rc = check_preact_request(N, C, P, n_out, rq);
    if (rc != QE_OK) return rc;
    if (x == nullptr || alpha == nullptr || shift == nullptr || (n_out > 0 && codes == nullptr)) return QE_ERR_ARG;
    for (int i = 0; i < n_out; ++i)
        if (codes[i] == nullptr) return QE_ERR_ARG;
    const PreactPlan p = plan_preact_request(N, C, P, n_out, rq, sum_out, act_out);
    if (p.kernel == PREACT_NONE && p.rc == QE_ERR_ARG) return p.rc;                    // no output requested
    for (const void *f : {(const void *)x, (const void *)identity, (const void *)alpha, (const void *)shift, (const void *)sum_out,
                          (const void *)act_out, (const void *)status})
        if ((reinterpret_cast<uintptr_t>(f) & 3) != 0) return QE_ERR_ARG;
    if (p.kernel == PREACT_NONE) return p.rc;
    // sum_out may be x or identity themselves (in place); otherwise no output overlaps an operand or another output
    const int64_t bytes = (int64_t)N * C * P * 4;
    Span small[2 + 2 * PREACT_MAX_OUT] = {span_of(alpha, 4 * (int64_t)C), span_of(shift, 4 * (int64_t)C)};
    Span others[2 + PREACT_MAX_OUT] = {span_of(act_out, bytes), span_of(status, 4)};
    for (int i = 0; i < n_out; ++i) {
        small[2 + 2 * i] = span_of(rq[i].scale, 4 * (int64_t)rq[i].n_param);
        small[3 + 2 * i] = span_of(rq[i].zero, 4 * (int64_t)rq[i].n_param);
        others[2 + i] = span_of(codes[i], qe_packed_nbytes(bytes / 4, rq[i].n_bits));
    }
    const Span big[2] = {span_of(x, bytes), span_of(identity, bytes)};
    const Span sum = span_of(sum_out, bytes);
    if (!outputs_clear(others, 2 + n_out, small, 2 + 2 * n_out) || !outputs_clear(others, 2 + n_out, big, 2)) return QE_ERR_ARG;
    if (!outputs_clear(&sum, 1, small, 2 + 2 * n_out) || !outputs_clear(&sum, 1, others, 2 + n_out)) return QE_ERR_ARG;
    if (!same_or_disjoint(sum_out, x, bytes) || !same_or_disjoint(sum_out, identity, bytes)) return QE_ERR_ARG;
    return launch_preact(p, x, identity, N, C, P, alpha, shift, n_out, rq, codes, sum_out, act_out, status, static_cast<hipStream_t>(stream));
}
