// torch_binding.cpp -- the `quant_engine` Python module for PyTorch-ROCm.
//
// Drop-in for the reference's pybind module of the same name
// (engine/kernels/pybind.cpp:7-17): its 8 exports (plus 4 of this engine's own), positional-only
// signatures, same return types/dtypes, and the reference's TORCH_CHECK messages (-> Python
// RuntimeError).  All device work goes through the C ABI in include/quant_engine.h;
// this file only checks arguments (the operand, bias and conv-geometry checks once each, shared by
// the four quantised operators), allocates outputs from torch's caching allocator, keeps the parsed
// descriptions and ONE cache of prepared weight tables for both conv operators, and picks up torch's
// current device and stream (the reference launches on the legacy default stream with no device
// guard).
//
// tpack/tunpack dispatch on the tensor's device exactly like the reference (tpack.cu:241-251, :458-468):
// device tensors go to the HIP kernels, CPU-resident tensors (a model packed or reloaded before it was
// moved to the GPU, cfg.device='cpu') to the host loops below.  That is the reference's own contract for
// host data, not a fallback: GPU tensors never take it, and a missing HIP build still fails at import.
// The conv / linear operators stay device-only, as in the reference (CHECK_CUDA, quantconv2d.cu:13,178).
//
// Deliberate differences from the reference, all stricter:
//   * extra TORCH_CHECKs where the reference would read out of bounds (packed buffer
//     shorter than the description says, scale arrays that are neither 1 nor C long);
//   * 64-bit indexing (the reference overflows 32-bit beyond 2^31 bits).
#include <torch/extension.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include <hip/hip_runtime_api.h>

#include <cstdlib>
#include <cstring>
#include <mutex>
#include <optional>
#include <unordered_map>
#include <vector>

#include "qe_request.hpp"          // quant_engine.h and the stored-code range the device path packs with

namespace {

// reference macros: tpack.cu:13-18, quantconv2d.cu:13-15, quantconv2d_float_input.cu:13-16
#define CHECK_NBITS(b) TORCH_CHECK(b > 0 && b <= 8, #b " must be in the range (0, 8]")
#define CHECK_LENGTH(x, min) TORCH_CHECK(x.size(0) >= min, "The description is too short, which should be at least " #min ".")
#define CHECK_CUDA(x) TORCH_CHECK(x.device().is_cuda(), #x " must be a CUDA tensor")
#define CHECK_CONTIGUOUS(x) TORCH_CHECK(x.is_contiguous(), #x " must be contiguous")
#define CHECK_FLOAT(x) TORCH_CHECK(x.dtype() == torch::kFloat32, #x " must be a float tensor")
#define CHECK_INPUT(x) CHECK_CUDA(x); CHECK_CONTIGUOUS(x)

void check_status(int rc, const char *what)
{
    if (rc == QE_OK) return;
    if (rc == QE_ERR_HIP) {
        TORCH_CHECK(false, what, ": HIP error ", qe_last_hip_error(), " (", qe_error_string(rc), ")");
    }
    TORCH_CHECK(false, qe_error_string(rc));
}

qe_stream_t current_stream(const torch::Tensor &t)
{
    return static_cast<qe_stream_t>(c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream());
}

int to_qe_dtype(const torch::Tensor &x, const char *name)
{
    switch (x.scalar_type()) {  // AT_DISPATCH_ALL_TYPES_AND(Half), tpack.cu:120
        case torch::kByte: return QE_U8;
        case torch::kChar: return QE_I8;
        case torch::kShort: return QE_I16;
        case torch::kInt: return QE_I32;
        case torch::kLong: return QE_I64;
        case torch::kHalf: return QE_F16;
        case torch::kFloat: return QE_F32;
        case torch::kDouble: return QE_F64;
        default:
            TORCH_CHECK(false, "\"", name, "\" not implemented for '", toString(x.scalar_type()), "'");
    }
    return -1;
}

struct Des {
    int n_bits = 0;
    int sign = 0;
    std::vector<int64_t> shape;
    int64_t numel = 1;
};

// ------------------------------------------------------------------------------------------
// Host-side caches.  A packed layer hands the SAME des / weight / scale tensors to the
// operator on every forward pass (buffers registered by pack(), quantconv2d.py:187-192), so what the host derives from
// them is kept between calls: the parsed description (saves the blocking device->host copy the reference pays ten
// times per call, quantconv2d.cu:191-207) and the prepared weight tables (prepared_tables() below; saves the re-layout
// launch).  A tensor is recognised by its object (TensorImpl), version counter, data pointer and size, and its entry is
// dropped once the object is gone.  `tensor.data = other` swaps storage without bumping the version: the data
// pointer in the key catches that unless the allocator hands the new storage the old address -- after such surgery on
// a packed module call quant_engine.clear_cache() (or run with QE_NO_CACHE=1, which disables both caches).
// ------------------------------------------------------------------------------------------
struct TensorKey {
    std::optional<c10::weak_intrusive_ptr<c10::TensorImpl>> impl;   // weak: the cache never keeps a tensor alive
    const void *ptr = nullptr;
    int64_t numel = 0;
    uint32_t version = 0;
    bool matches(const torch::Tensor &t) const
    {
        return impl.has_value() && !impl->expired() && impl->_unsafe_get_target() == t.unsafeGetTensorImpl() &&
               ptr == t.data_ptr() && numel == t.numel() && version == t._version();
    }
    static TensorKey of(const torch::Tensor &t)
    {
        TensorKey k;
        k.impl.emplace(t.getIntrusivePtr());
        k.ptr = t.data_ptr();
        k.numel = t.numel();
        k.version = (uint32_t)t._version();
        return k;
    }
};
bool cache_enabled()
{
    static const bool on = !(std::getenv("QE_NO_CACHE") && std::atoi(std::getenv("QE_NO_CACHE")) != 0);
    return on;
}
bool cacheable(const torch::Tensor &t) { return cache_enabled() && t.defined() && !t.is_inference(); }
std::mutex g_cache_mutex;
struct DesEntry { TensorKey key; Des des; };
std::unordered_map<const void *, DesEntry> g_des_cache;
int64_t g_des_hits = 0, g_des_misses = 0, g_prep_hits = 0, g_prep_misses = 0;

Des read_des_uncached(const torch::Tensor &des);

// One device->host copy of the whole description (the reference issues one blocking
// .item() per field: quantconv2d.cu:191-207, tpack.cu:435-474), and none at all when this
// des tensor has been parsed before.
Des read_des(const torch::Tensor &des)
{
    if (!cacheable(des) || !des.device().is_cuda()) return read_des_uncached(des);
    std::lock_guard<std::mutex> lock(g_cache_mutex);
    auto it = g_des_cache.find(des.unsafeGetTensorImpl());
    if (it != g_des_cache.end() && it->second.key.matches(des)) { ++g_des_hits; return it->second.des; }
    ++g_des_misses;
    if (g_des_cache.size() > 8192) g_des_cache.clear();
    DesEntry e{TensorKey::of(des), read_des_uncached(des)};
    g_des_cache[des.unsafeGetTensorImpl()] = e;
    return e.des;
}

Des read_des_uncached(const torch::Tensor &des)
{
    auto d = des.to(torch::kCPU, torch::kLong).contiguous();
    const int64_t *p = d.data_ptr<int64_t>();
    Des r;
    r.n_bits = (int)p[0];
    r.sign = p[1] != 0;
    for (int64_t i = 2; i < d.numel(); ++i) {
        r.shape.push_back(p[i]);
        r.numel *= p[i];
    }
    return r;
}

// ------------------------------------------------------------------------------------------
// Host loops for CPU-resident tensors (reference: tpack_cpu tpack.cu:140-190, tunpack_cpu :371-419).
// Same bit stream as the kernels: element i occupies bits [i*b, (i+1)*b) LSB first, stored value
// u = (uchar)(char)x + offset.  The reference walks the tensor with one .item() per element and a byte
// read-modify-write per half; here the elements go through a 64-bit shift register that is flushed a byte
// at a time (no RMW, output need not be pre-zeroed).  The range check (tpack.cu:211-215) runs in the same pass.
// ------------------------------------------------------------------------------------------
// des = [n_bits, sign, *shape], int32 (tpack.cu:228-238), built on the host
torch::Tensor make_des(int n_bits, bool sign, c10::IntArrayRef sizes)
{
    std::vector<int32_t> d{n_bits, sign ? 1 : 0};
    for (auto s : sizes) d.push_back((int32_t)s);
    return torch::tensor(d, torch::dtype(torch::kInt));
}

// the b-bit stream of x's elements (uninitialised) and the zeroed range flag of the pass that fills it, on x's device
std::pair<torch::Tensor, torch::Tensor> packed_and_status(const torch::Tensor &x, int n_bits)
{
    return {torch::empty({qe_packed_nbytes(x.numel(), n_bits)}, torch::dtype(torch::kByte).device(x.device())),
            torch::zeros({1}, torch::dtype(torch::kInt).device(x.device()))};
}

std::vector<torch::Tensor> tpack_host(const torch::Tensor &x, int n_bits, bool sign)
{
    (void)to_qe_dtype(x, "tpack_cpu");                     // same dtype set as the device path
    const int64_t n = x.numel();
    const auto xf = x.reshape({-1}).to(torch::kFloat);      // x[i].item<float>() of the reference, vectorised
    const float *src = xf.data_ptr<float>();
    const qe::CodeRange cr = qe::code_range(n_bits, sign);
    bool in_range = true;
    for (int64_t i = 0; i < n; ++i) in_range = in_range && (src[i] >= cr.lo && src[i] <= cr.hi);   // NaN fails, as in CHECK_RANGE
    TORCH_CHECK(in_range, "The input tensor is out of range.");

    auto x_out = torch::empty({qe_packed_nbytes(n, n_bits)}, torch::dtype(torch::kByte));
    uint8_t *dst = x_out.data_ptr<uint8_t>();
    uint64_t reg = 0;
    int fill = 0;
    int64_t o = 0;
    for (int64_t i = 0; i < n; ++i) {
        const unsigned e = ((unsigned)(unsigned char)(signed char)src[i] + cr.offset) & cr.mask;
        reg |= (uint64_t)e << fill;
        fill += n_bits;
        while (fill >= 8) { dst[o++] = (uint8_t)reg; reg >>= 8; fill -= 8; }
    }
    if (fill > 0) dst[o++] = (uint8_t)reg;
    return {x_out, make_des(n_bits, sign, x.sizes())};
}

torch::Tensor tunpack_host(const torch::Tensor &x, const Des &d)
{
    auto x_out = torch::empty({d.numel}, torch::dtype(d.sign ? torch::kChar : torch::kByte));
    const uint8_t *src = x.data_ptr<uint8_t>();
    uint8_t *dst = static_cast<uint8_t *>(x_out.data_ptr());
    const qe::CodeRange cr = qe::code_range(d.n_bits, d.sign);
    uint64_t reg = 0;
    int fill = 0;
    int64_t in = 0;
    for (int64_t i = 0; i < d.numel; ++i) {
        while (fill < d.n_bits) { reg |= (uint64_t)src[in++] << fill; fill += 8; }
        dst[i] = (uint8_t)(((unsigned)reg & cr.mask) - cr.offset);   // `element -= offset` in unsigned char, then (signed char)
        reg >>= d.n_bits;
        fill -= d.n_bits;
    }
    return x_out.reshape(d.shape);
}

// ------------------------------------------------------------------------------------------
// tpack  (reference: engine/kernels/tpack/tpack.cu:203-255, tpack.h:17-20)
// ------------------------------------------------------------------------------------------
static std::vector<torch::Tensor> tpack_impl(torch::Tensor x, int n_bits, bool sign, bool check_now)
{
    CHECK_NBITS(n_bits);
    CHECK_CONTIGUOUS(x);
    TORCH_CHECK(x.numel() > 0,
                "min(): Expected reduction dim to be specified for input.numel() == 0. Specify the reduction dim with the 'dim' argument.");
    if (!x.device().is_cuda()) {                                        // tpack.cu:241-251
        auto r = tpack_host(x, n_bits, sign);
        if (!check_now) r.push_back(torch::zeros({1}, torch::dtype(torch::kInt)));   // the host loop has already checked the range
        return r;
    }
    const int dtype = to_qe_dtype(x, "tpack_cuda");

    c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
    auto [x_out, status] = packed_and_status(x, n_bits);
    check_status(qe_tpack(x.data_ptr(), dtype, x.numel(), n_bits, sign ? 1 : 0, x_out.data_ptr<uint8_t>(),
                          status.data_ptr<int32_t>(), current_stream(x)),
                 "tpack");
    // CHECK_RANGE (tpack.cu:14,211-215), fused into the pack pass: one 4-byte read-back
    // instead of two full reductions + two syncs.
    if (check_now) TORCH_CHECK(status.item<int>() == 0, "The input tensor is out of range.");

    auto des = make_des(n_bits, sign, x.sizes()).to(x.device());
    if (check_now) return {x_out, des};
    return {x_out, des, status};
}

std::vector<torch::Tensor> tpack(torch::Tensor x, int n_bits, bool sign) { return tpack_impl(x, n_bits, sign, true); }

// Extension beyond the reference's 8 names: tpack without the blocking read-back of the range flag.  The reference's tpack is
// synchronous by construction (two .item() reductions, tpack.cu:211-215); on the 38.5 M-element input batch the one 4-byte
// read-back this module keeps costs 93 us around a 25 us kernel.  A caller that packs on the hot path (activations per
// step) takes [packed, des, status] here and checks `status` (int32[1]: bit 0 = some element failed CHECK_RANGE, `packed`
// is unspecified then) whenever it next synchronises anyway.
std::vector<torch::Tensor> tpack_async(torch::Tensor x, int n_bits, bool sign) { return tpack_impl(x, n_bits, sign, false); }

// ------------------------------------------------------------------------------------------
// tunpack  (reference: tpack.cu:429-476, tpack.h:30-32)
// ------------------------------------------------------------------------------------------
torch::Tensor tunpack(torch::Tensor x, torch::Tensor des)
{
    CHECK_LENGTH(des, 3);
    const Des d = read_des(des);
    const int n_bits = d.n_bits;
    CHECK_NBITS(n_bits);
    CHECK_CONTIGUOUS(x);
    TORCH_CHECK(x.dtype() == torch::kByte, "The input tensor must be torch.uint8.");
    TORCH_CHECK(d.numel >= 0, "The description holds a negative shape.");
    TORCH_CHECK(x.numel() >= qe_packed_nbytes(d.numel, n_bits),
                "The packed tensor is shorter than its description requires.");
    if (!x.device().is_cuda()) return tunpack_host(x, d);            // tpack.cu:458-468

    c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
    auto x_out = torch::empty({d.numel}, torch::dtype(d.sign ? torch::kChar : torch::kByte).device(x.device()));
    check_status(qe_tunpack(x.data_ptr<uint8_t>(), d.numel, n_bits, d.sign, x_out.data_ptr(), current_stream(x)),
                 "tunpack");
    return x_out.reshape(d.shape);
}

// ------------------------------------------------------------------------------------------
// Argument checks shared by the four quantised operators.  The messages and the order in which the checks fire are the
// reference's and part of the contract: every operator runs them in the order it always has.
// ------------------------------------------------------------------------------------------
struct Operand {                     // one packed operand
    const char *name;                // "input" | "weight", as the messages spell it
    const torch::Tensor &data, &scale, &zero;
    const Des &des;
    int64_t numel;                   // elements the bit stream must hold
    int64_t channels;                // scale / zero hold 1 element or one per channel ...
    const char *channels_name;       // ... "input_channel" / "output_channel" (conv), "batch_size" / "output_size" (linear)
    bool exact;                      // linear: exactly `channels` (indexed by row / column); conv: at least
    qe_qparam qparam() const
    {
        return {data.data_ptr<uint8_t>(), des.n_bits, des.sign, scale.data_ptr<float>(), zero.data_ptr<float>(), (int32_t)scale.numel()};
    }
};

// data_ptr<unsigned char>() / data_ptr<float>() of the reference (quantconv2d.cu:235-247) throw on a dtype mismatch; check
// up front, plus the buffer lengths the kernel will index.  x == nullptr: float input.  Each check runs over the input,
// then the weight, before the next check starts.
void check_operands(const Operand *x, const Operand &w)
{
    auto each = [&](auto check) { if (x) check(*x); check(w); };
    auto is = [](const torch::Tensor &t, torch::ScalarType want) {
        TORCH_CHECK(t.scalar_type() == want, "expected scalar type ", toString(want), " but found ", toString(t.scalar_type()));
    };
    each([&](const Operand &o) { is(o.data, torch::kByte); });
    each([&](const Operand &o) { is(o.scale, torch::kFloat); is(o.zero, torch::kFloat); });
    each([](const Operand &o) {
        TORCH_CHECK(o.data.numel() >= qe_packed_nbytes(o.numel, o.des.n_bits), "The packed ", o.name, " is shorter than its description requires.");
    });
    // The reference expands 0-dim scales (quantlinear.cu:276-290) and indexes anything else by channel; a 1-element tensor
    // is accepted as a broadcast too, anything else has to cover every channel.
    each([](const Operand &o) {
        const int64_t n = o.scale.numel();
        TORCH_CHECK(n == o.zero.numel() && (n == 1 || (o.exact ? n == o.channels : n >= o.channels)), o.name, "_scale/", o.name,
                    "_zero must hold 1 or ", o.channels_name, " elements");
    });
}

// The optional fp32 bias of n output channels; returns its pointer.  reference_linear: quantlinear's own form, which
// looks at device and strides only here and checks the length like the reference (quantlinear.cu:267).
const float *check_bias(const c10::optional<torch::Tensor> &bias, int64_t n, const char *channels_name, bool reference_linear)
{
    if (!bias.has_value()) return nullptr;
    if (reference_linear) { CHECK_INPUT(bias.value()); }
    TORCH_CHECK(bias.value().scalar_type() == torch::kFloat, "expected scalar type Float but found ", toString(bias.value().scalar_type()));
    if (reference_linear) {
        TORCH_CHECK(n == bias.value().size(0), "Weight and bias do not match");
    } else {
        TORCH_CHECK(bias.value().numel() >= n, "bias must hold ", channels_name, " elements");
    }
    return bias.value().data_ptr<float>();
}

// The conv problem of an (N, IC, H, W) input and a weight description (quantconv2d.cu:199-211,
// quantconv2d_float_input.cu:168-178; weight_shape[1] is never read)
struct ConvGeometry {
    qe_conv_shape sh;
    int64_t OH, OW;
    int64_t weight_numel() const { return (int64_t)sh.OC * sh.IC * sh.KH * sh.KW; }
};
ConvGeometry conv_geometry(int64_t N, int64_t IC, int64_t H, int64_t W, const Des &wd, int stride, int padding)
{
    TORCH_CHECK(stride > 0 && padding >= 0, "stride must be positive and padding non-negative");
    ConvGeometry g;
    g.sh = {(int32_t)N, (int32_t)IC, (int32_t)H, (int32_t)W, (int32_t)wd.shape[0], (int32_t)wd.shape[2], (int32_t)wd.shape[3], stride, padding};
    g.OH = (g.sh.H + 2 * padding - g.sh.KH) / stride + 1;
    g.OW = (g.sh.W + 2 * padding - g.sh.KW) / stride + 1;
    TORCH_CHECK(g.OH > 0 && g.OW > 0, "Calculated output size is too small: (", g.OH, " x ", g.OW, ")");
    return g;
}

// ------------------------------------------------------------------------------------------
// The prepared-table cache of both conv operators: the x-independent tables of qe_conv_prepare / qe_conv_f32_prepare are
// built once per (weight, scale, zero, bias) tensor set and kept while those tensors live unchanged; later calls run only
// the convolution.  Results are bit-identical.  One entry per weight tensor.
// Stream rule, the same for both operators (the float-input operator used to rebuild its tables when another stream
// called): the tables are filled in stream order and never rewritten, so an entry remembers the stream that filled it, and
// a hit from another stream synchronises that stream once and takes the entry over.
// ------------------------------------------------------------------------------------------
struct PrepKey {               // what the tables depend on besides the tensors; a field an operator does not use stays zero
    int x_bits;                // 32: float input
    int w_bits, w_sign;
    uint64_t layout;           // packed input: qe_conv_prepared_layout, what the tables look like -- NOT the batch or image
                               // size, so alternating batch sizes of one layer share the entry
    qe_conv_shape sh;          // float input: the problem with N = 0 (the tables do not depend on the batch size)
    size_t bytes;
    bool operator==(const PrepKey &o) const
    {
        return x_bits == o.x_bits && w_bits == o.w_bits && w_sign == o.w_sign && layout == o.layout &&
               std::memcmp(&sh, &o.sh, sizeof(sh)) == 0 && bytes == o.bytes;
    }
};
struct PrepEntry {
    TensorKey w, s, z, b;
    bool has_bias = false;
    PrepKey key{};
    torch::Tensor prepared;
    qe_stream_t stream = nullptr;
};
std::unordered_map<const void *, PrepEntry> g_prep_cache;

bool cacheable(const Operand &w, const c10::optional<torch::Tensor> &bias)
{
    return cacheable(w.data) && cacheable(w.scale) && cacheable(w.zero) && (!bias.has_value() || cacheable(bias.value()));
}

// fill(void *tables) runs the operator's prepare function on `stream`
template <class Fill>
torch::Tensor fresh_tables(size_t bytes, const torch::Device &device, Fill fill)
{
    auto prepared = torch::empty({(int64_t)bytes}, torch::dtype(torch::kByte).device(device));
    fill(prepared.data_ptr());
    return prepared;
}

// The tables of a cacheable weight set, valid for work queued on `stream`
template <class Fill>
torch::Tensor prepared_tables(const Operand &w, const c10::optional<torch::Tensor> &bias, const PrepKey &key, qe_stream_t stream,
                              const torch::Device &device, Fill fill)
{
    {
        std::lock_guard<std::mutex> lock(g_cache_mutex);
        auto it = g_prep_cache.find(w.data.unsafeGetTensorImpl());
        if (it != g_prep_cache.end()) {
            PrepEntry &e = it->second;
            if (e.w.matches(w.data) && e.s.matches(w.scale) && e.z.matches(w.zero) && e.has_bias == bias.has_value() &&
                (!e.has_bias || e.b.matches(bias.value())) && e.key == key) {
                ++g_prep_hits;
                if (e.stream != stream) {
                    TORCH_CHECK(hipStreamSynchronize(static_cast<hipStream_t>(e.stream)) == hipSuccess, "hipStreamSynchronize failed");
                    e.stream = stream;
                }
                return e.prepared;
            }
        }
    }
    PrepEntry e{TensorKey::of(w.data), TensorKey::of(w.scale), TensorKey::of(w.zero), bias.has_value() ? TensorKey::of(bias.value()) : TensorKey{},
                bias.has_value(), key, fresh_tables(key.bytes, device, fill), stream};
    std::lock_guard<std::mutex> lock(g_cache_mutex);
    ++g_prep_misses;
    if (g_prep_cache.size() > 4096) g_prep_cache.clear();
    g_prep_cache[w.data.unsafeGetTensorImpl()] = e;
    return e.prepared;
}

void clear_cache()
{
    std::lock_guard<std::mutex> lock(g_cache_mutex);
    g_des_cache.clear();
    g_prep_cache.clear();
}
std::vector<int64_t> cache_stats()
{
    std::lock_guard<std::mutex> lock(g_cache_mutex);
    return {g_des_hits, g_des_misses, g_prep_hits, g_prep_misses, (int64_t)g_des_cache.size(), (int64_t)g_prep_cache.size()};
}

// ------------------------------------------------------------------------------------------
// quantize_pack (extension): Quantizer + tpack in one pass.
//   reference: modelzoo/modules/quantizer.py:31,213-226 then engine.tpack.  scale/zero in the module's convention
//   (q = round(x / scale - zero)); per channel when they hold x.size(1) elements (activations (N, C, ...)) or
//   x.size(0) elements with channel_dim = 0 (weights (C, ...)).  Returns [packed uint8, des int32] like tpack.
// ------------------------------------------------------------------------------------------
std::vector<torch::Tensor> quantize_pack(torch::Tensor x, torch::Tensor scale, torch::Tensor zero, double qmin, double qmax,
                                         int n_bits, bool sign, int channel_dim)
{
    CHECK_NBITS(n_bits);
    CHECK_CONTIGUOUS(x);
    CHECK_FLOAT(x);
    TORCH_CHECK(x.numel() > 0, "quantize_pack: empty input");
    TORCH_CHECK(scale.numel() == zero.numel() && scale.numel() >= 1, "scale and zero must have the same number of elements");
    TORCH_CHECK(scale.scalar_type() == torch::kFloat && zero.scalar_type() == torch::kFloat, "scale/zero must be float tensors");
    int64_t inner = 1;
    if (scale.numel() > 1) {
        TORCH_CHECK(channel_dim >= 0 && channel_dim < x.dim() && x.size(channel_dim) == scale.numel(),
                    "per-channel scale must hold x.size(channel_dim) elements");
        for (int64_t d = channel_dim + 1; d < x.dim(); ++d) inner *= x.size(d);
    }
    if (!x.device().is_cuda()) {   // host tensors: the module's own arithmetic, then the host packer
        std::vector<int64_t> bshape(x.dim(), 1);
        if (scale.numel() > 1) bshape[channel_dim] = scale.numel();
        auto q = (x / scale.reshape(bshape) - zero.reshape(bshape)).round().clamp(qmin, qmax);
        return tpack_host(q.contiguous(), n_bits, sign);
    }
    CHECK_CUDA(scale);
    CHECK_CUDA(zero);
    CHECK_CONTIGUOUS(scale);
    CHECK_CONTIGUOUS(zero);
    c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
    auto [x_out, status] = packed_and_status(x, n_bits);
    check_status(qe_quantize_pack(x.data_ptr<float>(), x.numel(), scale.data_ptr<float>(), zero.data_ptr<float>(), (int32_t)scale.numel(),
                                  inner, (float)qmin, (float)qmax, n_bits, sign ? 1 : 0, x_out.data_ptr<uint8_t>(),
                                  status.data_ptr<int32_t>(), current_stream(x)),
                 "quantize_pack");
    TORCH_CHECK(status.item<int>() == 0, "The input tensor is out of range.");
    return {x_out, make_des(n_bits, sign, x.sizes()).to(x.device())};
}

// ------------------------------------------------------------------------------------------
// quantconv2d  (reference: functions/quantconv2d.cu:164-264, funcs.h:113-124)
// ------------------------------------------------------------------------------------------
torch::Tensor quantconv2d(const torch::Tensor &input, const torch::Tensor &input_des,
                          const torch::Tensor &input_scale, const torch::Tensor &input_zero,
                          const torch::Tensor &weight, const torch::Tensor &weight_des,
                          const torch::Tensor &weight_scale, const torch::Tensor &weight_zero,
                          const c10::optional<torch::Tensor> &bias, const int stride, const int padding)
{
    CHECK_INPUT(input);
    CHECK_INPUT(input_des);
    CHECK_INPUT(input_scale);
    CHECK_INPUT(input_zero);
    CHECK_INPUT(weight);
    CHECK_INPUT(weight_des);
    CHECK_INPUT(weight_scale);
    CHECK_INPUT(weight_zero);
    if (bias.has_value()) { CHECK_INPUT(bias.value()); }

    TORCH_CHECK(input_des.numel() >= 6 && weight_des.numel() >= 6,
                "The description is too short, which should be at least 6.");
    const Des xd = read_des(input_des);   // quantconv2d.cu:191-193
    const Des wd = read_des(weight_des);  // quantconv2d.cu:194-196
    CHECK_NBITS(xd.n_bits);
    CHECK_NBITS(wd.n_bits);
    const ConvGeometry g = conv_geometry(xd.shape[0], xd.shape[1], xd.shape[2], xd.shape[3], wd, stride, padding);
    const qe_conv_shape &sh = g.sh;
    const Operand x{"input", input, input_scale, input_zero, xd, (int64_t)sh.N * sh.IC * sh.H * sh.W, sh.IC, "input_channel", false};
    const Operand w{"weight", weight, weight_scale, weight_zero, wd, g.weight_numel(), sh.OC, "output_channel", false};
    check_operands(&x, w);
    const float *bias_ptr = check_bias(bias, sh.OC, "output_channel", false);

    c10::hip::HIPGuardMasqueradingAsCUDA guard(input.device());
    auto output = torch::empty({sh.N, sh.OC, g.OH, g.OW}, torch::dtype(torch::kFloat32).device(input.device()));
    const qe_qparam xq = x.qparam(), wq = w.qparam();
    const qe_stream_t stream = current_stream(input);
    auto bytes = [&](size_t n) { return torch::empty({(int64_t)n}, torch::dtype(torch::kByte).device(input.device())); };

    const size_t prep_bytes = qe_conv_prepared_bytes(&sh, xd.n_bits, wd.n_bits);
    const PrepKey key{xd.n_bits, wd.n_bits, wd.sign, qe_conv_prepared_layout(&sh, xd.n_bits, wd.n_bits), qe_conv_shape{}, prep_bytes};
    if (prep_bytes > 0 && qe_quantconv2d_path(&sh, &xq, &wq) == 1 && cacheable(w, bias)) {
        const torch::Tensor prepared = prepared_tables(w, bias, key, stream, input.device(), [&](void *tables) {
            check_status(qe_conv_prepare(&wq, bias_ptr, &sh, xd.n_bits, tables, prep_bytes, stream), "quantconv2d (prepare)");
        });
        const size_t sc_bytes = qe_quantconv2d_prepared_workspace_bytes(&sh, xd.n_bits, wd.n_bits);
        auto scratch = bytes(sc_bytes);
        check_status(qe_quantconv2d_prepared(&xq, &wq, bias_ptr, &sh, prepared.data_ptr(), prep_bytes, output.data_ptr<float>(),
                                             sc_bytes ? scratch.data_ptr() : nullptr, sc_bytes, stream),
                     "quantconv2d");
        return output;
    }
    // nothing to keep, or tensors that cannot be recognised again: the per-call route prepares inside the call
    const size_t ws_bytes = qe_quantconv2d_workspace_bytes(&sh, xd.n_bits, wd.n_bits);
    auto workspace = bytes(ws_bytes);
    check_status(qe_quantconv2d(&xq, &wq, bias_ptr, &sh, output.data_ptr<float>(),
                                ws_bytes ? workspace.data_ptr() : nullptr, ws_bytes, stream),
                 "quantconv2d");
    return output;
}

// ------------------------------------------------------------------------------------------
// quantconv2d_float_input  (reference: functions/quantconv2d_float_input.cu:140-220, funcs.h:143-151)
// ------------------------------------------------------------------------------------------
torch::Tensor quantconv2d_float_input(const torch::Tensor &input, const torch::Tensor &weight,
                                      const torch::Tensor &weight_des, const torch::Tensor &weight_scale,
                                      const torch::Tensor &weight_zero, const c10::optional<torch::Tensor> &bias,
                                      const int stride, const int padding)
{
    CHECK_INPUT(input);
    CHECK_FLOAT(input);
    CHECK_INPUT(weight);
    CHECK_INPUT(weight_des);
    CHECK_INPUT(weight_scale);
    CHECK_INPUT(weight_zero);
    if (bias.has_value()) { CHECK_INPUT(bias.value()); }

    TORCH_CHECK(input.dim() == 4, "input must be a 4-D (N, C, H, W) tensor");
    TORCH_CHECK(weight_des.numel() >= 6, "The description is too short, which should be at least 6.");
    const Des wd = read_des(weight_des);  // quantconv2d_float_input.cu:163-165
    CHECK_NBITS(wd.n_bits);
    const ConvGeometry g = conv_geometry(input.size(0), input.size(1), input.size(2), input.size(3), wd, stride, padding);
    const qe_conv_shape &sh = g.sh;
    const Operand w{"weight", weight, weight_scale, weight_zero, wd, g.weight_numel(), sh.OC, "output_channel", false};
    check_operands(nullptr, w);
    const float *bias_ptr = check_bias(bias, sh.OC, "output_channel", false);

    c10::hip::HIPGuardMasqueradingAsCUDA guard(input.device());
    auto output = torch::empty({sh.N, sh.OC, g.OH, g.OW}, input.options());
    const qe_qparam wq = w.qparam();
    const qe_stream_t stream = current_stream(input);
    // bf16 MFMA kernel where the problem is eligible (its weight tables are x-independent: cached like the packed
    // operator's), the order-preserving VALU kernel otherwise
    const size_t prep_bytes = qe_quantconv2d_float_input_path(&sh, &wq) == 1 ? qe_quantconv2d_float_input_workspace_bytes(&sh, wd.n_bits) : 0;
    if (prep_bytes > 0) {
        qe_conv_shape sh_key = sh;
        sh_key.N = 0;
        const PrepKey key{32, wd.n_bits, wd.sign, 0, sh_key, prep_bytes};
        auto fill = [&](void *tables) {
            check_status(qe_conv_f32_prepare(&wq, bias_ptr, &sh, tables, prep_bytes, stream), "quantconv2d_float_input (prepare)");
        };
        // tensors that cannot be recognised again: the kernel still needs its tables, in a buffer of this call
        const torch::Tensor prepared = cacheable(w, bias) ? prepared_tables(w, bias, key, stream, input.device(), fill)
                                                          : fresh_tables(prep_bytes, input.device(), fill);
        check_status(qe_quantconv2d_float_input_prepared(input.data_ptr<float>(), &wq, bias_ptr, &sh, prepared.data_ptr(), prep_bytes,
                                                         output.data_ptr<float>(), stream),
                     "quantconv2d_float_input");
        return output;
    }
    check_status(qe_quantconv2d_float_input(input.data_ptr<float>(), &wq, bias_ptr, &sh, output.data_ptr<float>(), stream),
                 "quantconv2d_float_input");
    return output;
}

// ------------------------------------------------------------------------------------------
// linear / conv2d: the reference's float demo kernels (functions/linear.cu:187-207,
// functions/conv2d.cu:231-309).  No Python caller exists in the reference (SURVEY.md section 2
// row 8: out of scope); exported for API completeness on top of ATen.  `mode` selected
// between two equivalent kernels in the reference and is ignored here.
// ------------------------------------------------------------------------------------------
torch::Tensor linear(const torch::Tensor &input, const torch::Tensor &weight,
                     const c10::optional<torch::Tensor> &bias, const int mode)
{
    (void)mode;
    return at::linear(input, weight, bias);
}

torch::Tensor conv2d(const torch::Tensor &input, const torch::Tensor &weight,
                     const c10::optional<torch::Tensor> &bias, const int stride, const int padding, const int mode)
{
    (void)mode;
    CHECK_INPUT(input);
    CHECK_INPUT(weight);
    if (bias.has_value()) { CHECK_INPUT(bias.value()); }
    return at::conv2d(input, weight, bias, {stride, stride}, {padding, padding});
}

// ------------------------------------------------------------------------------------------
// quantlinear  (reference: functions/quantlinear.cu:233-297, funcs.h:37-46)
// Conventions of THIS reference kernel: (q + zero), activation scale/zero per batch ROW.
// ------------------------------------------------------------------------------------------
torch::Tensor quantlinear(const torch::Tensor &input, const torch::Tensor &input_des,
                          const torch::Tensor &input_scale, const torch::Tensor &input_zero,
                          const torch::Tensor &weight, const torch::Tensor &weight_des,
                          const torch::Tensor &weight_scale, const torch::Tensor &weight_zero,
                          const c10::optional<torch::Tensor> &bias)
{
    CHECK_INPUT(input);          // quantlinear.cu:245-252
    CHECK_INPUT(weight);
    CHECK_INPUT(input_des);
    CHECK_INPUT(input_scale);
    CHECK_INPUT(input_zero);
    CHECK_INPUT(weight_des);
    CHECK_INPUT(weight_scale);
    CHECK_INPUT(weight_zero);
    TORCH_CHECK(input_des.numel() >= 4 && weight_des.numel() >= 4,
                "The description is too short, which should be at least 4.");
    const Des xd = read_des(input_des);    // :255-257
    const Des wd = read_des(weight_des);   // :258-260
    CHECK_NBITS(xd.n_bits);
    CHECK_NBITS(wd.n_bits);
    const int64_t B = xd.shape[0], K = xd.shape[1], O = wd.shape[0];   // :272-274
    TORCH_CHECK(K == wd.shape[1], "Input and weight do not match");    // :261
    TORCH_CHECK(B >= 0 && K >= 0 && O >= 0 && K < (1ll << 31) && O < (1ll << 31), "invalid linear shape");
    const float *bias_ptr = check_bias(bias, O, "output_size", true);   // :267: before the operands, as in the reference
    const Operand x{"input", input, input_scale, input_zero, xd, B * K, B, "batch_size", true};
    const Operand w{"weight", weight, weight_scale, weight_zero, wd, O * K, O, "output_size", true};
    check_operands(&x, w);

    c10::hip::HIPGuardMasqueradingAsCUDA guard(input.device());
    auto output = torch::empty({B, O}, torch::dtype(torch::kFloat32).device(input.device()));   // :166
    const qe_qparam xq = x.qparam(), wq = w.qparam();
    check_status(qe_quantlinear(&xq, &wq, bias_ptr, B, (int32_t)K, (int32_t)O, output.data_ptr<float>(),
                                current_stream(input)), "quantlinear");
    return output;
}

// ------------------------------------------------------------------------------------------
// quantlinear_float_input  (reference: functions/quantlinear_float_input.cu:120-182, funcs.h:62-68)
// ------------------------------------------------------------------------------------------
torch::Tensor quantlinear_float_input(const torch::Tensor &input, const torch::Tensor &weight,
                                      const torch::Tensor &weight_des, const torch::Tensor &weight_scale,
                                      const torch::Tensor &weight_zero, const c10::optional<torch::Tensor> &bias)
{
    CHECK_INPUT(input);          // quantlinear_float_input.cu:129-138
    CHECK_FLOAT(input);
    CHECK_INPUT(weight);
    CHECK_INPUT(weight_des);
    CHECK_INPUT(weight_scale);
    CHECK_INPUT(weight_zero);
    if (bias.has_value()) { CHECK_INPUT(bias.value()); }
    TORCH_CHECK(input.dim() == 2, "input must be a 2-D (batch_size, input_size) tensor");
    TORCH_CHECK(weight_des.numel() >= 4, "The description is too short, which should be at least 4.");
    const Des wd = read_des(weight_des);   // :141-143
    CHECK_NBITS(wd.n_bits);
    const int64_t B = input.size(0), K = input.size(1), O = wd.shape[0];   // :146-150
    TORCH_CHECK(K == wd.shape[1], "Input and weight do not match");        // (the reference never compares them)
    TORCH_CHECK(K < (1ll << 31) && O >= 0 && O < (1ll << 31), "invalid linear shape");
    const Operand w{"weight", weight, weight_scale, weight_zero, wd, O * K, O, "output_size", true};
    check_operands(nullptr, w);
    const float *bias_ptr = check_bias(bias, O, "output_size", false);
    c10::hip::HIPGuardMasqueradingAsCUDA guard(input.device());
    auto output = torch::empty({B, O}, input.options());   // :153
    const qe_qparam wq = w.qparam();
    check_status(qe_quantlinear_float_input(input.data_ptr<float>(), &wq, bias_ptr, B, (int32_t)K, (int32_t)O,
                                            output.data_ptr<float>(), current_stream(input)), "quantlinear_float_input");
    return output;
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m)
{
    // Same names and positional signatures as the reference module (engine/kernels/pybind.cpp:9-16).
    m.def("tpack", &tpack, "tpack(x, n_bits, sign) -> [packed uint8 1-D, des int32]: b-bit LSB-first bit stream.");
    m.def("tpack_async", &tpack_async,
          "tpack_async(x, n_bits, sign) -> [packed, des, status int32[1]]: tpack without the blocking read-back of the range flag "
          "(status != 0: out of range, packed unspecified).");
    m.def("tunpack", &tunpack, "tunpack(packed, des) -> int8/uint8 tensor of shape des[2:].");
    m.def("linear", &linear, "linear(input, weight, bias, mode): float x @ w.T + b (ATen).");
    m.def("quantlinear", &quantlinear,
          "quantlinear(x, x_des, x_scale, x_zero, w, w_des, w_scale, w_zero, bias) -> fp32 (B, O); (q + zero), per-row x scale.");
    m.def("quantlinear_float_input", &quantlinear_float_input,
          "quantlinear_float_input(x_fp32, w, w_des, w_scale, w_zero, bias) -> fp32 (B, O); (q - zero) weights.");
    m.def("conv2d", &conv2d, "conv2d(input, weight, bias, stride, padding, mode): float conv (ATen).");
    m.def("quantconv2d", &quantconv2d,
          "quantconv2d(x, x_des, x_scale, x_zero, w, w_des, w_scale, w_zero, bias, stride, padding) -> fp32 NCHW.");
    m.def("quantconv2d_float_input", &quantconv2d_float_input,
          "quantconv2d_float_input(x_fp32, w, w_des, w_scale, w_zero, bias, stride, padding) -> fp32 NCHW.");
    // extensions (no counterpart in the reference's module)
    m.def("quantize_pack", &quantize_pack,
          "quantize_pack(x_fp32, scale, zero, qmin, qmax, n_bits, sign, channel_dim) -> [packed, des]: "
          "round(x / scale - zero).clamp(qmin, qmax) packed like tpack, in one pass.");
    m.def("clear_cache", &clear_cache, "drop the cached descriptions and prepared weight tables");
    m.def("cache_stats", &cache_stats, "[des hits, des misses, prepared hits, prepared misses, des entries, prepared entries]");
    m.attr("__qe_version__") = qe_version();
    m.attr("__qe_arch__") = qe_target_arch();
}
