"""ctypes view of the C ABI (include/quant_engine.h) -- what a non-torch host would bind.

Tensors are only used here as device-memory handles (data_ptr) and for the current HIP
stream; every compute call goes straight into libqe_hip.so.  Used by bench.py and by the
`-m gpu` parity tests, which must exercise the C ABI itself and not only the torch module.
"""
import contextlib
import ctypes
import os

from . import loader

_lib = None

QE_OK = 0
QE_ERR_UNSUPPORTED = 7
DTYPES = {"uint8": 0, "int8": 1, "int16": 2, "int32": 3, "int64": 4,
          "float16": 5, "float32": 6, "float64": 7}

ACTS = {None: 0, "none": 0, "gelu": 1}


class QeConvShape(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("N", "IC", "H", "W", "OC", "KH", "KW", "stride", "padding")]


class QeQParam(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("n_bits", ctypes.c_int32), ("sign", ctypes.c_int32),
                ("scale", ctypes.c_void_p), ("zero", ctypes.c_void_p), ("n_param", ctypes.c_int32)]


class QeRequant(ctypes.Structure):
    _fields_ = [("scale", ctypes.c_void_p), ("zero", ctypes.c_void_p), ("n_param", ctypes.c_int32),
                ("qmin", ctypes.c_float), ("qmax", ctypes.c_float), ("n_bits", ctypes.c_int32), ("sign", ctypes.c_int32)]


class QeConvPlanInfo(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_int32) for n in (
        "route", "fused", "family", "cfg", "niw", "kkt", "ns", "split", "wraw", "rq", "patch", "has_instance",
        "ctab", "gi", "th", "ni", "mt", "nch", "oh", "ow", "rowmul", "colmul", "pre", "sub2_log_up", "expand", "sub_x4",
        "fd_w8", "pwr_tw", "pwr_ks", "pwr_groups", "pwr7_gi", "pwr_s2")] +
                [(n, ctypes.c_int64) for n in ("lds", "blocks", "total", "prep_total", "y_bytes")])


class QeConvF32Plan(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_int32) for n in (
        "ok", "kernel", "stem", "OCP", "NG", "KK", "OH", "OW", "TH", "GI", "IHT", "IWP", "ROWMUL", "COLMUL",
        "chunk", "n_pix_tiles", "n_oc_tiles", "tiles_h")] +
                [(n, ctypes.c_int64) for n in ("blocks", "lds", "ep_off", "total")])


class QeDwConvPlan(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_int32) for n in (
        "kernel", "symmetric", "G", "TH", "vec", "store16", "codes4", "two_pass", "OH", "OW", "bands")] +
                [(n, ctypes.c_int64) for n in ("blocks", "lds")])


class QeGrpConvPlan(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_int32) for n in (
        "kernel", "slab", "TH", "TW", "tiles", "two_pass", "out16", "codes16", "OH", "OW")] +
                [(n, ctypes.c_int64) for n in ("blocks", "lds")])


class QeError(RuntimeError):
    pass


_vp, _i32, _i64, _sz, _f32, _str = (ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_float,
                                    ctypes.c_char_p)
_pq, _ps, _pr, _ppc = ctypes.POINTER(QeQParam), ctypes.POINTER(QeConvShape), ctypes.POINTER(QeRequant), ctypes.POINTER(_vp)
_pi = ctypes.POINTER(QeConvPlanInfo)
_pf = ctypes.POINTER(QeConvF32Plan)
_pd = ctypes.POINTER(QeDwConvPlan)
_pg = ctypes.POINTER(QeGrpConvPlan)
_attn = [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i64, _i64, _i64, _i64, _i64, _i64, _f32]

# every symbol include/quant_engine.h declares: name -> (restype, argtypes); lib() applies the table
PROTOTYPES = {
    "qe_error_string": (_str, [_i32]),
    "qe_last_hip_error": (_i32, []),
    "qe_version": (_str, []),
    "qe_target_arch": (_str, []),
    "qe_packed_nbytes": (_i64, [_i64, _i32]),
    "qe_tpack": (_i32, [_vp, _i32, _i64, _i32, _i32, _vp, _vp, _vp]),
    "qe_tunpack": (_i32, [_vp, _i64, _i32, _i32, _vp, _vp]),
    "qe_quantize_pack": (_i32, [_vp, _i64, _vp, _vp, _i32, _i64, _f32, _f32, _i32, _i32, _vp, _vp, _vp]),
    "qe_quantize_pack_act": (_i32, [_vp, _i64, _i32, _vp, _vp, _i32, _i64, _f32, _f32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "qe_quantize_patchify": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _f32, _f32, _i32, _i32, _vp, _vp, _vp]),
    "qe_global_avgpool": (_i32, [_vp, _i64, _i32, _vp, _vp]),
    "qe_maxpool2d_codes": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    # quantised ReLU and pooling layers
    "qe_quant_relu": (_i32, [_vp, _i64, _i64, _pr, _vp, _vp]),
    "qe_quant_maxpool2d": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _pr, _vp, _vp]),
    "qe_quant_adaptive_avgpool2d": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32, _i32, _pr, _vp, _vp]),
    "qe_avgpool2d_codes_path": (_i32, [_pq] + [_i32] * 9 + [_vp, _pr, _vp]),
    "qe_avgpool2d_codes": (_i32, [_pq] + [_i32] * 9 + [_vp, _pr, _vp, _vp, _vp]),
    # the pre-activation boundary: add + per-channel affine + ReLU + the consumers' codes
    "qe_affine_relu_quantize_pack_path": (_i32, [_i32, _i32, _i32, _i32, _pr, _vp, _vp]),
    "qe_affine_relu_quantize_pack": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _i32, _pr, _ppc, _vp, _vp, _vp, _vp]),
    # packed-activation convolutions
    "qe_quantconv2d_path": (_i32, [_ps, _pq, _pq]),
    "qe_quantconv2d_plan_info": (_i32, [_ps, _pq, _pq, _pr, _vp, _vp, _pi]),
    "qe_conv_mfma_has_instance": (_i32, [_i32] * 9),
    "qe_quantconv2d_workspace_bytes": (_sz, [_ps, _i32, _i32]),
    "qe_quantconv2d": (_i32, [_pq, _pq, _vp, _ps, _vp, _vp, _sz, _vp]),
    "qe_conv_prepared_bytes": (_sz, [_ps, _i32, _i32]),
    "qe_conv_prepared_layout": (ctypes.c_uint64, [_ps, _i32, _i32]),
    "qe_conv_prepare": (_i32, [_pq, _vp, _ps, _i32, _vp, _sz, _vp]),
    "qe_quantconv2d_prepared_workspace_bytes": (_sz, [_ps, _i32, _i32]),
    "qe_quantconv2d_prepared": (_i32, [_pq, _pq, _vp, _ps, _vp, _sz, _vp, _vp, _sz, _vp]),
    "qe_quantconv2d_requant_path": (_i32, [_ps, _pq, _pq, _pr]),
    "qe_quantconv2d_requant_workspace_bytes": (_sz, [_ps, _pq, _pq, _pr]),
    "qe_quantconv2d_requant_prepared": (_i32, [_pq, _pq, _vp, _ps, _vp, _sz, _pr, _vp, _vp, _vp, _sz, _vp]),
    "qe_quantconv2d_residual_path": (_i32, [_ps, _pq, _pq, _pr]),
    "qe_quantconv2d_residual_workspace_bytes": (_sz, [_ps, _pq, _pq, _pr]),
    "qe_quantconv2d_residual_prepared": (_i32, [_pq, _pq, _vp, _ps, _vp, _sz, _vp, _vp, _pr, _vp, _vp, _vp, _sz, _vp]),
    # depthwise packed convolutions
    "qe_quantconv2d_depthwise_path": (_i32, [_ps, _pq, _pq, _pr]),
    "qe_quantconv2d_depthwise_plan_info": (_i32, [_ps, _pq, _pq, _pr, _vp, _vp, _pd]),
    "qe_quantconv2d_depthwise": (_i32, [_pq, _pq, _vp, _ps, _i32, _vp, _pr, _vp, _vp, _vp]),
    # grouped packed convolutions
    "qe_quantconv2d_grouped_path": (_i32, [_ps, _i32, _pq, _pq, _pr]),
    "qe_quantconv2d_grouped_plan_info": (_i32, [_ps, _i32, _pq, _pq, _pr, _vp, _vp, _pg]),
    "qe_quantconv2d_grouped": (_i32, [_pq, _pq, _vp, _ps, _i32, _i32, _vp, _pr, _vp, _vp, _vp]),
    # float-input convolutions
    "qe_quantconv2d_float_input": (_i32, [_vp, _pq, _vp, _ps, _vp, _vp]),
    "qe_quantconv2d_float_input_path": (_i32, [_ps, _pq]),
    "qe_conv_f32_plan_info": (_i32, [_ps, _pf]),
    "qe_quantconv2d_float_input_workspace_bytes": (_sz, [_ps, _i32]),
    "qe_quantconv2d_float_input_ws": (_i32, [_vp, _pq, _vp, _ps, _vp, _vp, _sz, _vp]),
    "qe_conv_f32_prepare": (_i32, [_pq, _vp, _ps, _vp, _sz, _vp]),
    "qe_quantconv2d_float_input_prepared": (_i32, [_vp, _pq, _vp, _ps, _vp, _sz, _vp, _vp]),
    # linears and their fused ViT forms
    "qe_quantlinear": (_i32, [_pq, _pq, _vp, _i64, _i32, _i32, _vp, _vp]),
    "qe_quantlinear_path": (_i32, [_pq, _pq, _i64, _i32, _i32]),
    "qe_quantlinear_form": (_i32, [_pq, _pq, _i64, _i32, _i32, _i32]),
    "qe_quantlinear_float_input": (_i32, [_vp, _pq, _vp, _i64, _i32, _i32, _vp, _vp]),
    "qe_quantlinear_float_input_path": (_i32, [_vp, _pq, _i64, _i32, _i32]),
    "qe_quantlinear_requant_path": (_i32, [_pq, _pq, _i64, _i32, _i32, _pr, _vp]),
    "qe_quantlinear_requant_workspace_bytes": (_sz, [_pq, _pq, _i64, _i32, _i32, _pr, _vp]),
    "qe_quantlinear_requant": (_i32, [_pq, _pq, _vp, _i64, _i32, _i32, _i32, _pr, _vp, _vp, _vp, _sz, _vp]),
    "qe_quantlinear_residual_path": (_i32, [_pq, _pq, _i64, _i32, _i32]),
    "qe_quantlinear_residual_workspace_bytes": (_sz, [_pq, _pq, _i64, _i32, _i32]),
    "qe_quantlinear_residual": (_i32, [_pq, _pq, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _sz, _vp]),
    "qe_quantlinear_float_input_residual_path": (_i32, [_vp, _pq, _i64, _i32, _i32]),
    "qe_quantlinear_float_input_residual_workspace_bytes": (_sz, [_vp, _pq, _i64, _i32, _i32]),
    "qe_quantlinear_float_input_residual": (_i32, [_vp, _pq, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _sz, _vp]),
    "qe_quantlinear_bf16_path": (_i32, [_pq, _pq, _i64, _i32, _i32, _vp]),
    "qe_quantlinear_bf16_workspace_bytes": (_sz, [_pq, _pq, _i64, _i32, _i32, _vp]),
    "qe_quantlinear_bf16": (_i32, [_pq, _pq, _vp, _i64, _i32, _i32, _f32, _vp, _vp, _sz, _vp]),
    "qe_quantlinear_bf16_input_path": (_i32, [_vp, _pq, _i64, _i32, _i32]),
    "qe_quantlinear_bf16_input_workspace_bytes": (_sz, [_vp, _pq, _i64, _i32, _i32]),
    "qe_quantlinear_bf16_input": (_i32, [_vp, _pq, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _sz, _vp]),
    "qe_layernorm_quantize_pack_path": (_i32, [_i64, _i32, _i32, _pr, _ppc]),
    "qe_layernorm_quantize_pack_workspace_bytes": (_sz, [_i64, _i32, _i32, _pr, _ppc, _vp]),
    "qe_layernorm_quantize_pack": (_i32, [_vp, _i64, _i32, _vp, _vp, _f32, _i32, _pr, _ppc, _vp, _vp, _vp, _sz, _vp]),
    "qe_attention_path": (_i32, [_i32, _i32, _i32, _i32]),
    "qe_attention": (_i32, _attn + [_vp]),
    "qe_attention_masked_path": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32, _i32]),
    "qe_attention_masked": (_i32, _attn + [_vp, _i64, _i64, _vp, _i32, _vp]),
    "qe_attention_bf16_path": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32, _i32]),
    "qe_attention_bf16": (_i32, _attn + [_vp, _i64, _i64, _vp, _i32, _vp]),
    "qe_attention_bf16_stored_path": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32, _i32]),
    "qe_attention_bf16_stored": (_i32, _attn + [_vp, _i64, _i64, _vp, _i32, _vp]),
    "qe_attention_bf16_ctx_path": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32, _i32]),
    "qe_attention_bf16_ctx": (_i32, _attn + [_vp, _i64, _i64, _vp, _i32, _vp]),
}
SYMBOLS = sorted(PROTOTYPES)
# exported by the library but absent from the header (not part of the public ABI): kept out of SYMBOLS
DEBUG_PROTOTYPES = {
    "qe_debug_reload_env": (None, []),
    "qe_debug_set_stamp_buffer": (None, [_vp]),
}


def lib():
    """dlopen libqe_hip.so (no GPU needed to load it) and declare the prototypes."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("QE_LIB") or loader.lib_path()   # QE_LIB: diagnostic builds only (tools/)
    if not os.path.exists(path):
        raise ImportError("libqe_hip.so not built: run `python -m quantize_amd.build`. No fallback exists.")
    L = ctypes.CDLL(path)
    for table in (PROTOTYPES, DEBUG_PROTOTYPES):
        for name, (restype, argtypes) in table.items():
            f = getattr(L, name)
            f.restype, f.argtypes = restype, argtypes
    _lib = L
    return L


def check(rc):
    if rc != QE_OK:
        L = lib()
        msg = L.qe_error_string(rc).decode()
        if rc == 5:
            msg += " (hipError_t %d)" % L.qe_last_hip_error()
        raise QeError(msg)


def _stream(stream=None):
    import torch
    s = torch.cuda.current_stream() if stream is None else stream
    return ctypes.c_void_p(s.cuda_stream)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _ws(need, dev):
    import torch
    return torch.empty(need, dtype=torch.uint8, device=dev) if need else None


def _given_ws(workspace, need, dev):
    """The caller's workspace as it is (the library refuses one that is too small), or a new one of `need` bytes."""
    return _ws(need, dev) if workspace is None else workspace


def _status(status, dev):
    import torch
    return torch.zeros(1, dtype=torch.int32, device=dev) if status is None else status


def _prep(t):
    """(pointer, bytes) of a prepared-table or workspace tensor; (None, 0) when there is none or it is empty."""
    return (t.data_ptr(), t.numel()) if t is not None and t.numel() else (None, 0)


def packed_nbytes(n, n_bits):
    return int(lib().qe_packed_nbytes(int(n), int(n_bits)))


def tpack(x, n_bits, sign, out=None, status=None, stream=None):
    """qe_tpack on a contiguous device tensor. Returns (packed uint8 tensor, status int32[1] tensor)."""
    import torch
    assert x.is_cuda and x.is_contiguous()
    n = x.numel()
    if out is None:
        out = torch.empty(packed_nbytes(n, n_bits), dtype=torch.uint8, device=x.device)
    status = _status(status, x.device)
    check(lib().qe_tpack(x.data_ptr(), DTYPES[str(x.dtype).replace("torch.", "")], n, int(n_bits),
                         1 if sign else 0, out.data_ptr(), status.data_ptr(), _stream(stream)))
    return out, status


def tunpack(packed, n, n_bits, sign, out=None, stream=None):
    import torch
    assert packed.is_cuda and packed.is_contiguous() and packed.dtype == torch.uint8
    if out is None:
        out = torch.empty(n, dtype=torch.int8 if sign else torch.uint8, device=packed.device)
    check(lib().qe_tunpack(packed.data_ptr(), int(n), int(n_bits), 1 if sign else 0, out.data_ptr(),
                           _stream(stream)))
    return out


def conv_shape(N, IC, H, W, OC, KH, KW, stride, padding):
    return QeConvShape(int(N), int(IC), int(H), int(W), int(OC), int(KH), int(KW), int(stride), int(padding))


def out_hw(sh):
    return ((sh.H + 2 * sh.padding - sh.KH) // sh.stride + 1, (sh.W + 2 * sh.padding - sh.KW) // sh.stride + 1)


def qparam(data, n_bits, sign, scale, zero):
    """Packed operand: uint8 stream + fp32 scale/zero tensors (1 element = per tensor)."""
    assert scale.numel() == zero.numel()
    q = QeQParam(data.data_ptr(), int(n_bits), 1 if sign else 0, scale.data_ptr(), zero.data_ptr(),
                 int(scale.numel()))
    q._keep = (data, scale, zero)  # keep the tensors alive as long as the struct
    return q


def workspace_bytes(sh, x_bits, w_bits):
    return int(lib().qe_quantconv2d_workspace_bytes(ctypes.byref(sh), int(x_bits), int(w_bits)))


def reload_env():
    """Re-read the QE_* tuning knobs: the library snapshots them once per process (qe_common.h env_get); call this after
    changing one inside a live process (tests, A/B tools).  Not part of the public C ABI."""
    lib().qe_debug_reload_env()


@contextlib.contextmanager
def knobs(**env):
    """Set QE_* knobs (value None: unset), re-read them; on exit, also on an exception, put the environment back and
    re-read again.  The one way to flip a knob in a live process: `with capi.knobs(QE_PWR="0"): ...`."""
    old = {k: os.environ.get(k) for k in env}

    def put(kv):
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        reload_env()

    try:
        put(env)
        yield
    finally:
        put(old)


def conv_prepared_layout(sh, x_bits, w_bits):
    return int(lib().qe_conv_prepared_layout(ctypes.byref(sh), int(x_bits), int(w_bits)))


def conv_path(sh, xq, wq):
    return int(lib().qe_quantconv2d_path(ctypes.byref(sh), ctypes.byref(xq), ctypes.byref(wq)))


# qe_conv_plan_info: route, MFMA family and pre-pass by number
CONV_ROUTES = {0: "generic", 1: "pwr", 2: "pwr7", 3: "flatd", 4: "mfma"}
CONV_FAMILIES = {0: "none", 1: "halo", 2: "ws", 3: "sm2", 4: "stem", 5: "flat", 6: "flat_s2", 7: "flat_x4", 8: "flatg"}
CONV_PREPASSES = {0: "none", 1: "sub_x4", 2: "sub2", 3: "sub_wide", 4: "sub_narrow"}


def conv_plan_info(sh, xq, wq, rq=None, out=0, codes=0):
    """qe_quantconv2d_plan_info (host-only): the plan of the request as a QeConvPlanInfo, with the QE_* knobs of the last
    reload_env().  rq: a capi.requant for the re-quantising call; out / codes: destination addresses (0: aligned)."""
    info = QeConvPlanInfo()
    check(lib().qe_quantconv2d_plan_info(ctypes.byref(sh), ctypes.byref(xq), ctypes.byref(wq),
                                         None if rq is None else ctypes.byref(rq), int(out) or None, int(codes) or None,
                                         ctypes.byref(info)))
    return info


def conv_mfma_has_instance(family, cfg, niw, kkt, ns, split, wraw, rq, patch):
    """qe_conv_mfma_has_instance (host-only): the library compiles this MFMA-family instance (fields as QeConvPlanInfo)."""
    return bool(lib().qe_conv_mfma_has_instance(int(family), int(cfg), int(niw), int(kkt), int(ns), int(split), int(wraw),
                                                int(rq), int(patch)))


def quantconv2d(xq, wq, bias, sh, out=None, workspace=None, stream=None):
    import torch
    dev = wq._keep[0].device
    OH, OW = out_hw(sh)
    if out is None:
        out = torch.empty((sh.N, sh.OC, OH, OW), dtype=torch.float32, device=dev)
    if workspace is None:
        workspace = _ws(workspace_bytes(sh, xq.n_bits, wq.n_bits), dev)
    check(lib().qe_quantconv2d(ctypes.byref(xq), ctypes.byref(wq), _ptr(bias), ctypes.byref(sh), out.data_ptr(),
                               *_prep(workspace), _stream(stream)))
    return out


def conv_prepare(wq, bias, sh, x_bits, stream=None):
    """qe_conv_prepare: the x-independent tables of a conv layer, once.  Returns a uint8 device tensor (possibly empty)."""
    import torch
    dev = wq._keep[0].device
    need = int(lib().qe_conv_prepared_bytes(ctypes.byref(sh), int(x_bits), wq.n_bits))
    prepared = torch.empty(max(need, 0), dtype=torch.uint8, device=dev)
    check(lib().qe_conv_prepare(ctypes.byref(wq), _ptr(bias), ctypes.byref(sh), int(x_bits), *_prep(prepared), _stream(stream)))
    return prepared


def quantconv2d_prepared(xq, wq, bias, sh, prepared, out=None, workspace=None, stream=None):
    import torch
    dev = wq._keep[0].device
    OH, OW = out_hw(sh)
    if out is None:
        out = torch.empty((sh.N, sh.OC, OH, OW), dtype=torch.float32, device=dev)
    if workspace is None:
        workspace = _ws(int(lib().qe_quantconv2d_prepared_workspace_bytes(ctypes.byref(sh), xq.n_bits, wq.n_bits)), dev)
    check(lib().qe_quantconv2d_prepared(ctypes.byref(xq), ctypes.byref(wq), _ptr(bias), ctypes.byref(sh), *_prep(prepared),
                                        out.data_ptr(), *_prep(workspace), _stream(stream)))
    return out


def requant(scale, zero, qmin, qmax, n_bits, sign):
    """qe_requant: the consumer's activation quantiser (module convention: q = round(y / scale - zero).clamp(qmin, qmax))."""
    r = QeRequant(scale.data_ptr(), zero.data_ptr(), int(scale.numel()), float(qmin), float(qmax), int(n_bits), 1 if sign else 0)
    r._keep = (scale, zero)
    return r


def requant_path(sh, xq, wq, rq):
    return int(lib().qe_quantconv2d_requant_path(ctypes.byref(sh), ctypes.byref(xq), ctypes.byref(wq), ctypes.byref(rq)))


def quantconv2d_requant_prepared(xq, wq, bias, sh, prepared, rq, out=None, status=None, workspace=None, stream=None):
    """qe_quantconv2d_requant_prepared: conv + the consumer's quantiser + tpack in one call; returns (packed uint8, status)."""
    import torch
    dev = wq._keep[0].device
    OH, OW = out_hw(sh)
    if out is None:
        out = torch.empty(packed_nbytes(sh.N * sh.OC * OH * OW, rq.n_bits), dtype=torch.uint8, device=dev)
    status = _status(status, dev)
    if workspace is None:
        workspace = _ws(int(lib().qe_quantconv2d_requant_workspace_bytes(ctypes.byref(sh), ctypes.byref(xq), ctypes.byref(wq),
                                                                         ctypes.byref(rq))), dev)
    check(lib().qe_quantconv2d_requant_prepared(ctypes.byref(xq), ctypes.byref(wq), _ptr(bias), ctypes.byref(sh), *_prep(prepared),
                                                ctypes.byref(rq), out.data_ptr(), status.data_ptr(), *_prep(workspace),
                                                _stream(stream)))
    return out, status


def residual_path(sh, xq, wq, rq=None):
    """1: the conv kernel adds the identity, applies the ReLU and writes out / codes itself; 0: two passes inside the call."""
    return int(lib().qe_quantconv2d_residual_path(ctypes.byref(sh), ctypes.byref(xq), ctypes.byref(wq),
                                                  None if rq is None else ctypes.byref(rq)))


def residual_workspace_bytes(sh, xq, wq, rq=None):
    return int(lib().qe_quantconv2d_residual_workspace_bytes(ctypes.byref(sh), ctypes.byref(xq), ctypes.byref(wq),
                                                             None if rq is None else ctypes.byref(rq)))


def quantconv2d_residual_prepared(xq, wq, bias, sh, prepared, identity, rq=None, out="new", codes=None, status=None,
                                  workspace=None, stream=None):
    """qe_quantconv2d_residual_prepared: out = relu(conv + identity) (fp32) and, with rq, the consumer's codes of out.
    out="new" allocates it, None skips it (rq required), or pass a tensor (identity itself: in place).
    Returns (out or None, codes or None, status int32[1] tensor)."""
    import torch
    dev = wq._keep[0].device
    OH, OW = out_hw(sh)
    assert identity.is_contiguous() and identity.dtype == torch.float32 and identity.numel() == sh.N * sh.OC * OH * OW
    if isinstance(out, str):
        out = torch.empty((sh.N, sh.OC, OH, OW), dtype=torch.float32, device=dev)
    if rq is not None and codes is None:
        codes = torch.empty(packed_nbytes(sh.N * sh.OC * OH * OW, rq.n_bits), dtype=torch.uint8, device=dev)
    status = _status(status, dev)
    if workspace is None:
        workspace = _ws(residual_workspace_bytes(sh, xq, wq, rq), dev)
    check(lib().qe_quantconv2d_residual_prepared(
        ctypes.byref(xq), ctypes.byref(wq), _ptr(bias), ctypes.byref(sh), *_prep(prepared), identity.data_ptr(), _ptr(out),
        None if rq is None else ctypes.byref(rq), _ptr(codes), status.data_ptr(), *_prep(workspace), _stream(stream)))
    return out, codes, status


# qe_dwconv_plan: the kernel instance by number
DW_KERNELS = ("plain", "fast_s1_out", "fast_s1_codes", "fast_s1_both", "fast_s2_out", "fast_s2_codes", "fast_s2_both")


# The depthwise and the grouped entry points differ in their names, in one `groups` argument (head: () | (groups,)) and in
# their plan struct; one helper each stands behind the two path queries, the two plan queries and the two calls.
def _span_path(fn, sh, head, xq, wq, rq):
    return int(fn(ctypes.byref(sh), *head, ctypes.byref(xq), ctypes.byref(wq), None if rq is None else ctypes.byref(rq)))


def _span_plan_info(fn, info, sh, head, xq, wq, rq, out, codes):
    check(fn(ctypes.byref(sh), *head, ctypes.byref(xq), ctypes.byref(wq), None if rq is None else ctypes.byref(rq),
             int(out) or None, int(codes) or None, ctypes.byref(info)))
    return info


def _span_conv(fn, xq, wq, bias, sh, head, relu, rq, out, codes, status, stream):
    import torch
    dev = wq._keep[0].device
    OH, OW = out_hw(sh)
    if isinstance(out, str):
        out = torch.empty((sh.N, sh.OC, OH, OW), dtype=torch.float32, device=dev)
    if rq is not None and codes is None:
        codes = torch.empty(packed_nbytes(sh.N * sh.OC * OH * OW, rq.n_bits), dtype=torch.uint8, device=dev)
    status = _status(status, dev)
    check(fn(ctypes.byref(xq), ctypes.byref(wq), _ptr(bias), ctypes.byref(sh), *head, 1 if relu else 0, _ptr(out),
             None if rq is None else ctypes.byref(rq), _ptr(codes), status.data_ptr(), _stream(stream)))
    return out, codes, status


def depthwise_path(sh, xq, wq, rq=None):
    """qe_quantconv2d_depthwise_path (host-only): 1 = the fast depthwise kernel, 0 = the plain one, -1 = none."""
    return _span_path(lib().qe_quantconv2d_depthwise_path, sh, (), xq, wq, rq)


def depthwise_plan_info(sh, xq, wq, rq=None, out=0, codes=0):
    """qe_quantconv2d_depthwise_plan_info (host-only): the plan of the request as a QeDwConvPlan.  out / codes: destination
    addresses; with rq, out == 0 asks for the codes-only call (pass any aligned non-zero address for both), codes == 0 reads
    as aligned."""
    return _span_plan_info(lib().qe_quantconv2d_depthwise_plan_info, QeDwConvPlan(), sh, (), xq, wq, rq, out, codes)


def quantconv2d_depthwise(xq, wq, bias, sh, relu=False, rq=None, out="new", codes=None, status=None, stream=None):
    """qe_quantconv2d_depthwise: y = [relu](depthwise conv + bias) as fp32 `out` and / or, with rq, the consumer's codes of y.
    out="new" allocates it, None skips it (rq required), or pass a tensor.  Returns (out or None, codes or None, status)."""
    return _span_conv(lib().qe_quantconv2d_depthwise, xq, wq, bias, sh, (), relu, rq, out, codes, status, stream)


# qe_grpconv_plan: the kernel instance by number
GRP_KERNELS = ("plain",) + tuple("fast_cg%d_s%d_%s" % (cg, s, e) for cg in (4, 8, 16, 32) for s in (1, 2)
                                 for e in ("out", "codes", "both"))


def grouped_path(sh, groups, xq, wq, rq=None):
    """qe_quantconv2d_grouped_path (host-only): 1 = the fast grouped family, 0 = the plain kernel, -1 = none."""
    return _span_path(lib().qe_quantconv2d_grouped_path, sh, (int(groups),), xq, wq, rq)


def grouped_plan_info(sh, groups, xq, wq, rq=None, out=0, codes=0):
    """qe_quantconv2d_grouped_plan_info (host-only): the plan of the request as a QeGrpConvPlan.  out / codes: destination
    addresses; with rq, out == 0 asks for the codes-only call (pass any aligned non-zero address for both), codes == 0 reads
    as aligned."""
    return _span_plan_info(lib().qe_quantconv2d_grouped_plan_info, QeGrpConvPlan(), sh, (int(groups),), xq, wq, rq, out, codes)


def quantconv2d_grouped(xq, wq, bias, sh, groups, relu=False, rq=None, out="new", codes=None, status=None, stream=None):
    """qe_quantconv2d_grouped: y = [relu](grouped conv + bias) as fp32 `out` and / or, with rq, the consumer's codes of y.
    out="new" allocates it, None skips it (rq required), or pass a tensor.  Returns (out or None, codes or None, status)."""
    return _span_conv(lib().qe_quantconv2d_grouped, xq, wq, bias, sh, (int(groups),), relu, rq, out, codes, status, stream)


def maxpool2d_codes(x, n_bits, N, C, H, W, kernel=3, stride=2, padding=1, out=None, stream=None):
    """qe_maxpool2d_codes on an 8-bit stored-code stream (N*C*H*W bytes) -> N*C*OH*OW bytes.  Sub-8-bit streams are not
    taken: QeError(QE_ERR_UNSUPPORTED)."""
    import torch
    if int(n_bits) != 8:
        check(QE_ERR_UNSUPPORTED)
    OH, OW = (H + 2 * padding - kernel) // stride + 1, (W + 2 * padding - kernel) // stride + 1
    if out is None:
        out = torch.empty(max(N * C * OH * OW, 0), dtype=torch.uint8, device=x.device)
    check(lib().qe_maxpool2d_codes(x.data_ptr(), int(N), int(C), int(H), int(W), int(kernel), int(stride), int(padding),
                                   out.data_ptr(), _stream(stream)))
    return out


def _fp32_nchw(x):
    import torch
    assert x.is_cuda and x.is_contiguous() and x.dtype == torch.float32 and x.dim() == 4


def quant_relu(x, rq, inner=None, out=None, stream=None):
    """qe_quant_relu: relu(qdq(x)) of a contiguous fp32 tensor under the layer's quantiser rq (a capi.requant; per channel:
    dimension 1, so inner defaults to the product of the later dimensions).  out=None: a new tensor; out=x: in place."""
    import torch
    assert x.is_cuda and x.is_contiguous() and x.dtype == torch.float32
    if inner is None:
        inner = 1
        for v in x.shape[2:]:
            inner *= v
    if out is None:
        out = torch.empty_like(x)
    check(lib().qe_quant_relu(x.data_ptr(), x.numel(), int(inner), ctypes.byref(rq), out.data_ptr(), _stream(stream)))
    return out


def quant_maxpool2d(x, rq, kernel, stride=None, padding=0, dilation=1, return_indices=False, ceil_mode=False, out=None, stream=None):
    """qe_quant_maxpool2d: max_pool2d(qdq(x)) of fp32 NCHW x.  Square geometry, dilation 1, no indices, floor mode: anything else
    raises QeError(QE_ERR_UNSUPPORTED)."""
    import torch
    _fp32_nchw(x)
    stride = kernel if stride is None else stride
    if int(dilation) != 1 or return_indices or ceil_mode:
        check(QE_ERR_UNSUPPORTED)
    N, C, H, W = x.shape
    OH, OW = (H + 2 * padding - kernel) // stride + 1, (W + 2 * padding - kernel) // stride + 1
    if out is None:
        out = torch.empty((N, C, max(OH, 0), max(OW, 0)), dtype=torch.float32, device=x.device)
    check(lib().qe_quant_maxpool2d(x.data_ptr(), N, C, H, W, int(kernel), int(stride), int(padding), ctypes.byref(rq),
                                   out.data_ptr(), _stream(stream)))
    return out


def quant_adaptive_avgpool2d(x, rq, output_size, out=None, stream=None):
    """qe_quant_adaptive_avgpool2d: the mean of qdq(x) over torch's adaptive windows, summed in the header's fixed order."""
    import torch
    _fp32_nchw(x)
    N, C, H, W = x.shape
    OH, OW = (output_size, output_size) if isinstance(output_size, int) else output_size
    OH, OW = (H if OH is None else int(OH)), (W if OW is None else int(OW))
    if out is None:
        out = torch.empty((N, C, OH, OW), dtype=torch.float32, device=x.device)
    check(lib().qe_quant_adaptive_avgpool2d(x.data_ptr(), N, C, H, W, OH, OW, ctypes.byref(rq), out.data_ptr(), _stream(stream)))
    return out


# qe_avgpool2d_codes_path: the instance by number
POOL_KERNELS = ("plain", "pair", "plane")


def avgpool2d_out_hw(H, W, kernel, stride, output_size=None):
    """(OH, OW) of a codes-domain average pool: fixed windows (kernel > 0, floor mode, no padding) or adaptive (kernel == 0)."""
    if kernel:
        return (H - kernel) // stride + 1, (W - kernel) // stride + 1
    return (output_size, output_size) if isinstance(output_size, int) else tuple(output_size)


def avgpool2d_codes_path(xq, N, C, H, W, kernel=0, stride=None, output_size=None, relu=False, rq=None, out=256, codes=256):
    """qe_avgpool2d_codes_path (host-only): 1 pair, 2 plane, 0 plain, -1 none.  out / codes: destination addresses (out == 0 asks
    for the codes-only call; codes is passed only with rq)."""
    stride = (kernel or 1) if stride is None else stride
    OH, OW = avgpool2d_out_hw(H, W, kernel, stride, output_size)
    return int(lib().qe_avgpool2d_codes_path(ctypes.byref(xq), int(N), int(C), int(H), int(W), int(kernel), int(stride), int(OH),
                                             int(OW), 1 if relu else 0, int(out) or None, None if rq is None else ctypes.byref(rq),
                                             (int(codes) or None) if rq is not None else None))


def avgpool2d_codes(xq, N, C, H, W, kernel=0, stride=None, output_size=None, relu=False, rq=None, out="new", codes=None,
                    status=None, stream=None):
    """qe_avgpool2d_codes: the window means of 8-bit stored codes (kernel > 0: nn.AvgPool2d(kernel, stride); kernel == 0: adaptive
    to output_size) as fp32 `out` and / or, with rq, the consumer's codes.  relu: max(q - zero', 0) per tap first.
    out="new" allocates it, None skips it (rq required), or pass a tensor.  Returns (out or None, codes or None, status)."""
    import torch
    dev = xq._keep[0].device
    stride = (kernel or 1) if stride is None else stride
    OH, OW = avgpool2d_out_hw(H, W, kernel, stride, output_size)
    n = max(N * C * OH * OW, 0)
    if isinstance(out, str):
        out = torch.empty((N, C, max(OH, 0), max(OW, 0)), dtype=torch.float32, device=dev)
    if rq is not None and codes is None:
        codes = torch.empty(packed_nbytes(n, rq.n_bits), dtype=torch.uint8, device=dev)
    status = _status(status, dev)
    check(lib().qe_avgpool2d_codes(ctypes.byref(xq), int(N), int(C), int(H), int(W), int(kernel), int(stride), int(OH), int(OW),
                                   1 if relu else 0, _ptr(out), None if rq is None else ctypes.byref(rq), _ptr(codes),
                                   status.data_ptr(), _stream(stream)))
    return out, codes, status


# qe_affine_relu_quantize_pack_path: the instance by number
PREACT_KERNELS = ("plain", "fast")


def affine_relu_quantize_pack_path(N, C, P, rqs=(), sum_out=256, act_out=0):
    """qe_affine_relu_quantize_pack_path (host-only): 1 fast, 0 plain, -1 none.  sum_out / act_out: destination addresses (0:
    not requested)."""
    rqs = list(rqs)
    return int(lib().qe_affine_relu_quantize_pack_path(int(N), int(C), int(P), len(rqs), _rq_array(rqs), int(sum_out) or None,
                                                       int(act_out) or None))


def affine_relu_quantize_pack(x, alpha, shift, identity=None, rqs=(), sum_out=None, act_out=None, codes=None, status=None, stream=None):
    """qe_affine_relu_quantize_pack on fp32 NCHW x: s = x + identity (identity None: x), a = relu(s * alpha[c] + shift[c]), and the
    codes of a under every quantiser in rqs (at most two capi.requant).  sum_out / act_out: None skips the output, "new" allocates
    it, or pass a tensor (sum_out may be x or identity: in place).  Returns (list of codes, sum_out or None, act_out or None,
    status)."""
    import torch
    _fp32_nchw(x)
    N, C, H, W = x.shape
    rqs = list(rqs)
    if isinstance(sum_out, str):
        sum_out = torch.empty_like(x)
    if isinstance(act_out, str):
        act_out = torch.empty_like(x)
    if codes is None:
        codes = [torch.empty(packed_nbytes(x.numel(), r.n_bits), dtype=torch.uint8, device=x.device) for r in rqs]
    status = _status(status, x.device)
    cp = (ctypes.c_void_p * max(1, len(codes)))(*[c.data_ptr() for c in codes])
    check(lib().qe_affine_relu_quantize_pack(x.data_ptr(), _ptr(identity), N, C, H * W, alpha.data_ptr(), shift.data_ptr(), len(rqs),
                                             _rq_array(rqs), cp, _ptr(sum_out), _ptr(act_out), status.data_ptr(), _stream(stream)))
    return codes, sum_out, act_out, status


def quantize_pack(x, scale, zero, qmin, qmax, n_bits, sign, inner=1, out=None, status=None, stream=None):
    """qe_quantize_pack: round(x / scale - zero).clamp(qmin, qmax) packed to n_bits; per channel when scale has > 1
    element (channel(i) = (i / inner) % numel(scale))."""
    import torch
    assert x.is_cuda and x.is_contiguous() and x.dtype == torch.float32 and scale.numel() == zero.numel()
    n = x.numel()
    if out is None:
        out = torch.empty(packed_nbytes(n, n_bits), dtype=torch.uint8, device=x.device)
    status = _status(status, x.device)
    check(lib().qe_quantize_pack(x.data_ptr(), n, scale.data_ptr(), zero.data_ptr(), int(scale.numel()), int(inner),
                                 float(qmin), float(qmax), int(n_bits), 1 if sign else 0, out.data_ptr(), status.data_ptr(),
                                 _stream(stream)))
    return out, status


def quantconv2d_float_input(x, wq, bias, sh, out=None, stream=None, mfma=True):
    """mfma=True: qe_quantconv2d_float_input_ws (bf16 MFMA kernel where eligible); False: the order-preserving VALU kernel."""
    import torch
    assert x.is_cuda and x.is_contiguous() and x.dtype == torch.float32
    OH, OW = out_hw(sh)
    if out is None:
        out = torch.empty((sh.N, sh.OC, OH, OW), dtype=torch.float32, device=x.device)
    bp = _ptr(bias)
    if mfma:
        need = int(lib().qe_quantconv2d_float_input_workspace_bytes(ctypes.byref(sh), wq.n_bits))
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=x.device)
        check(lib().qe_quantconv2d_float_input_ws(x.data_ptr(), ctypes.byref(wq), bp, ctypes.byref(sh), out.data_ptr(),
                                                  ws.data_ptr(), ws.numel(), _stream(stream)))
    else:
        check(lib().qe_quantconv2d_float_input(x.data_ptr(), ctypes.byref(wq), bp, ctypes.byref(sh), out.data_ptr(), _stream(stream)))
    return out


def float_input_path(sh, wq):
    return int(lib().qe_quantconv2d_float_input_path(ctypes.byref(sh), ctypes.byref(wq)))


# qe_conv_f32_plan_info: the kernel instance by number (F32Kernel, qe_conv_plan.hpp)
F32_KERNELS = ("Stem4x1x7", "Stem2x2x4", "Stem2x2x7", "M4x1x4", "M4x1x4S2", "M4x1x7", "M4x1x7S2", "M2x2x2", "M2x2x2S2",
               "M2x2x4", "M2x2x4S2")


def conv_f32_plan_info(sh):
    """qe_conv_f32_plan_info (host-only): the plan of a float-input convolution as a QeConvF32Plan, with the QE_F32_MFMA
    knob of the last reload_env().  ok == 0: the VALU kernel runs and the other fields say nothing."""
    info = QeConvF32Plan()
    check(lib().qe_conv_f32_plan_info(ctypes.byref(sh), ctypes.byref(info)))
    return info


def conv_f32_prepare(wq, bias, sh, stream=None):
    import torch
    need = int(lib().qe_quantconv2d_float_input_workspace_bytes(ctypes.byref(sh), wq.n_bits))
    prepared = torch.empty(need, dtype=torch.uint8, device=wq._keep[0].device)
    check(lib().qe_conv_f32_prepare(ctypes.byref(wq), _ptr(bias), ctypes.byref(sh), *_prep(prepared), _stream(stream)))
    return prepared


def quantconv2d_float_input_prepared(x, wq, bias, sh, prepared, out=None, stream=None):
    import torch
    OH, OW = out_hw(sh)
    if out is None:
        out = torch.empty((sh.N, sh.OC, OH, OW), dtype=torch.float32, device=x.device)
    check(lib().qe_quantconv2d_float_input_prepared(x.data_ptr(), ctypes.byref(wq), _ptr(bias), ctypes.byref(sh), *_prep(prepared),
                                                    out.data_ptr(), _stream(stream)))
    return out


def linear_path(xq, wq, B, K, O):
    return int(lib().qe_quantlinear_path(ctypes.byref(xq), ctypes.byref(wq), int(B), int(K), int(O)))


# qe_quantlinear_form: the kernel an int8 linear problem runs on
LINEAR_FORMS = {0: "fp32 chain", 1: "64-deep 128x128", 2: "64-deep 128x256", 3: "8-wave 320x256", 4: "4-wave 160x256"}


def linear_form(xq, wq, B, K, O, dst_aligned=True):
    """qe_quantlinear_form (host-only): 0 = order-preserving fp32 kernel, 1 = 64-deep 128 x 128, 2 = 64-deep 128 x 256,
    3 = 8-wave 320 x 256, 4 = 4-wave 160 x 256 -- with the QE_LIN8 / QE_LIN_NJ knobs of the last reload_env()."""
    return int(lib().qe_quantlinear_form(ctypes.byref(xq), ctypes.byref(wq), int(B), int(K), int(O), 1 if dst_aligned else 0))


def quantlinear(xq, wq, bias, B, K, O, out=None, stream=None):
    """out[b,o] = bias[o] + sum_k (qx + zx[b]) (qw + zw[o]) sx[b] sw[o]  (the reference kernel's (q + zero) convention)."""
    import torch
    if out is None:
        out = torch.empty((B, O), dtype=torch.float32, device=wq._keep[0].device)
    check(lib().qe_quantlinear(ctypes.byref(xq), ctypes.byref(wq), _ptr(bias), int(B), int(K), int(O), out.data_ptr(),
                               _stream(stream)))
    return out


def linear_float_input_path(x, wq, B, K, O):
    return int(lib().qe_quantlinear_float_input_path(x.data_ptr(), ctypes.byref(wq), int(B), int(K), int(O)))


def quantlinear_float_input(x, wq, bias, O, out=None, stream=None):
    import torch
    assert x.is_cuda and x.is_contiguous() and x.dtype == torch.float32 and x.dim() == 2
    B, K = x.shape
    if out is None:
        out = torch.empty((B, O), dtype=torch.float32, device=x.device)
    check(lib().qe_quantlinear_float_input(x.data_ptr(), ctypes.byref(wq), _ptr(bias), int(B), int(K), int(O), out.data_ptr(),
                                           _stream(stream)))
    return out


def global_avgpool(x, out=None, stream=None):
    """mean over the last two dims of a contiguous fp32 NCHW tensor -> (N, C)."""
    import torch
    assert x.is_cuda and x.is_contiguous() and x.dtype == torch.float32 and x.dim() == 4
    N, C, H, W = x.shape
    if out is None:
        out = torch.empty((N, C), dtype=torch.float32, device=x.device)
    check(lib().qe_global_avgpool(x.data_ptr(), N * C, H * W, out.data_ptr(), _stream(stream)))
    return out


# ---- fused ViT forms ----------------------------------------------------------------------------------------------
def quantize_pack_act(x, scale, zero, qmin, qmax, n_bits, sign, act=None, inner=1, out=None, y=None, status=None, stream=None):
    """qe_quantize_pack_act: codes of act(x) (act None | "gelu"); y: optional fp32 output of act(x) (a tensor, or "new").
    Returns (codes, y or None, status)."""
    import torch
    assert x.is_cuda and x.is_contiguous() and x.dtype == torch.float32 and scale.numel() == zero.numel()
    n = x.numel()
    if out is None:
        out = torch.empty(packed_nbytes(n, n_bits), dtype=torch.uint8, device=x.device)
    if isinstance(y, str):
        y = torch.empty_like(x)
    status = _status(status, x.device)
    check(lib().qe_quantize_pack_act(x.data_ptr(), n, ACTS[act], scale.data_ptr(), zero.data_ptr(), int(scale.numel()), int(inner),
                                     float(qmin), float(qmax), int(n_bits), 1 if sign else 0, out.data_ptr(), _ptr(y),
                                     status.data_ptr(), _stream(stream)))
    return out, y, status


def linear_requant_path(xq, wq, B, K, O, rq, codes=None):
    """1: the MFMA kernel writes the codes itself.  codes=None asks for a 16-byte aligned buffer (torch allocations are)."""
    return int(lib().qe_quantlinear_requant_path(ctypes.byref(xq), ctypes.byref(wq), int(B), int(K), int(O), ctypes.byref(rq),
                                                 codes.data_ptr() if codes is not None else 256))


def quantlinear_requant(xq, wq, bias, B, K, O, rq, act=None, codes=None, status=None, workspace=None, stream=None):
    """qe_quantlinear_requant: the consumer's codes of act(quantlinear(...)) (B x O elements).  Returns (codes, status)."""
    import torch
    dev = wq._keep[0].device
    if codes is None:
        codes = torch.empty(packed_nbytes(B * O, rq.n_bits), dtype=torch.uint8, device=dev)
    status = _status(status, dev)
    need = int(lib().qe_quantlinear_requant_workspace_bytes(ctypes.byref(xq), ctypes.byref(wq), int(B), int(K), int(O),
                                                            ctypes.byref(rq), codes.data_ptr()))
    ws = _given_ws(workspace, need, dev)
    check(lib().qe_quantlinear_requant(ctypes.byref(xq), ctypes.byref(wq), _ptr(bias), int(B), int(K), int(O), ACTS[act],
                                       ctypes.byref(rq), codes.data_ptr(), status.data_ptr(), *_prep(ws), _stream(stream)))
    return codes, status


def linear_residual_path(xq, wq, B, K, O):
    return int(lib().qe_quantlinear_residual_path(ctypes.byref(xq), ctypes.byref(wq), int(B), int(K), int(O)))


def quantlinear_residual(xq, wq, bias, B, K, O, residual, out=None, workspace=None, stream=None):
    """qe_quantlinear_residual: out = quantlinear(...) + residual (out=None: a new tensor; out=residual: in place)."""
    import torch
    assert residual.is_contiguous() and residual.dtype == torch.float32 and residual.numel() == B * O
    dev = residual.device
    if out is None:
        out = torch.empty((B, O), dtype=torch.float32, device=dev)
    need = int(lib().qe_quantlinear_residual_workspace_bytes(ctypes.byref(xq), ctypes.byref(wq), int(B), int(K), int(O)))
    ws = _given_ws(workspace, need, dev)
    check(lib().qe_quantlinear_residual(ctypes.byref(xq), ctypes.byref(wq), _ptr(bias), int(B), int(K), int(O), residual.data_ptr(),
                                        out.data_ptr(), *_prep(ws), _stream(stream)))
    return out


def quantlinear_bf16_path(xq, wq, B, K, O, out=None):
    """qe_quantlinear_bf16_path: 1 = the MFMA kernel rounds and stores the bf16 rows itself, 0 = two passes inside the call.
    out=None asks for a 16-byte aligned buffer (torch allocations are)."""
    return int(lib().qe_quantlinear_bf16_path(ctypes.byref(xq), ctypes.byref(wq), int(B), int(K), int(O), _ptr(out)))


def quantlinear_bf16(xq, wq, bias, B, K, O, post_scale=1.0, out=None, workspace=None, stream=None):
    """qe_quantlinear_bf16: bf16(quantlinear(...) * post_scale) as a torch.bfloat16 tensor (B, O) -- one fp32 multiply, round
    to nearest even: equal to (quantlinear(...) * post_scale).to(torch.bfloat16) element for element."""
    import torch
    dev = wq._keep[0].device
    if out is None:
        out = torch.empty((B, O), dtype=torch.bfloat16, device=dev)
    assert out.is_contiguous() and out.dtype == torch.bfloat16 and out.numel() == B * O
    need = int(lib().qe_quantlinear_bf16_workspace_bytes(ctypes.byref(xq), ctypes.byref(wq), int(B), int(K), int(O), out.data_ptr()))
    ws = _given_ws(workspace, need, dev)
    check(lib().qe_quantlinear_bf16(ctypes.byref(xq), ctypes.byref(wq), _ptr(bias), int(B), int(K), int(O), float(post_scale),
                                    out.data_ptr(), *_prep(ws), _stream(stream)))
    return out


def linear_float_input_residual_path(x, wq, B, K, O):
    return int(lib().qe_quantlinear_float_input_residual_path(x.data_ptr(), ctypes.byref(wq), int(B), int(K), int(O)))


def quantlinear_float_input_residual(x, wq, bias, O, residual, out=None, workspace=None, stream=None):
    """qe_quantlinear_float_input_residual: out = quantlinear_float_input(x, ...) + residual."""
    import torch
    assert x.is_cuda and x.is_contiguous() and x.dtype == torch.float32 and x.dim() == 2
    B, K = x.shape
    assert residual.is_contiguous() and residual.dtype == torch.float32 and residual.numel() == B * O
    if out is None:
        out = torch.empty((B, O), dtype=torch.float32, device=x.device)
    need = int(lib().qe_quantlinear_float_input_residual_workspace_bytes(x.data_ptr(), ctypes.byref(wq), int(B), int(K), int(O)))
    ws = _given_ws(workspace, need, x.device)
    check(lib().qe_quantlinear_float_input_residual(x.data_ptr(), ctypes.byref(wq), _ptr(bias), int(B), int(K), int(O),
                                                    residual.data_ptr(), out.data_ptr(), *_prep(ws), _stream(stream)))
    return out


def _check_bf16_rows(x):
    import torch
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 2 and x.is_contiguous()):
        raise ValueError("x must be a contiguous torch.bfloat16 CUDA tensor of shape (B, K)")


def quantlinear_bf16_input_path(x, wq, B, K, O):
    """qe_quantlinear_bf16_input_path: 1 = the bf16-input MFMA kernel reads the rows of x as they are stored, 0 = one pass
    widens them to fp32 and the float-input plan runs on the copy."""
    return int(lib().qe_quantlinear_bf16_input_path(_ptr(x), ctypes.byref(wq), int(B), int(K), int(O)))


def quantlinear_bf16_input(x, wq, bias, O, residual=None, out=None, workspace=None, stream=None):
    """qe_quantlinear_bf16_input: quantlinear_float_input on a contiguous torch.bfloat16 (B, K) tensor, read in place
    (+ residual when given: one fp32 add; out=residual: in place).  Anything else as x raises ValueError."""
    import torch
    _check_bf16_rows(x)
    B, K = x.shape
    if residual is not None:
        assert residual.is_contiguous() and residual.dtype == torch.float32 and residual.numel() == B * O
    if out is None:
        out = torch.empty((B, O), dtype=torch.float32, device=x.device)
    assert out.is_contiguous() and out.dtype == torch.float32 and out.numel() == B * O
    # the query cannot see `out`: an `out` that is not 16-byte aligned takes path 0 whatever it answers
    need = int(lib().qe_quantlinear_bf16_input_workspace_bytes(x.data_ptr() if out.data_ptr() % 16 == 0 else 2, ctypes.byref(wq),
                                                               int(B), int(K), int(O)))
    ws = _given_ws(workspace, need, x.device)
    check(lib().qe_quantlinear_bf16_input(x.data_ptr(), ctypes.byref(wq), _ptr(bias), int(B), int(K), int(O), _ptr(residual),
                                          out.data_ptr(), *_prep(ws), _stream(stream)))
    return out


def _rq_array(rqs):
    arr = (QeRequant * max(1, len(rqs)))(*rqs) if rqs else None
    return arr


def layernorm_path(rows, E, rqs, codes):
    arr = _rq_array(rqs)
    cp = (ctypes.c_void_p * max(1, len(codes)))(*[c.data_ptr() for c in codes])
    return int(lib().qe_layernorm_quantize_pack_path(int(rows), int(E), len(rqs), arr, cp))


def layernorm_quantize_pack(x, gamma, beta, eps, rqs=(), ln_out=None, codes=None, status=None, workspace=None, stream=None):
    """qe_layernorm_quantize_pack over the last dimension of x: the codes of every quantiser in rqs (a list of capi.requant),
    and the fp32 LayerNorm when ln_out is a tensor or "new".  Returns (list of codes, ln_out or None, status)."""
    import torch
    assert x.is_cuda and x.is_contiguous() and x.dtype == torch.float32
    E = x.shape[-1]
    rows = x.numel() // E
    rqs = list(rqs)
    if isinstance(ln_out, str):
        ln_out = torch.empty_like(x)
    if codes is None:
        codes = [torch.empty(packed_nbytes(rows * E, r.n_bits), dtype=torch.uint8, device=x.device) for r in rqs]
    status = _status(status, x.device)
    arr = _rq_array(rqs)
    cp = (ctypes.c_void_p * max(1, len(codes)))(*[c.data_ptr() for c in codes])
    need = int(lib().qe_layernorm_quantize_pack_workspace_bytes(int(rows), int(E), len(rqs), arr, cp, _ptr(ln_out)))
    ws = _given_ws(workspace, need, x.device)
    check(lib().qe_layernorm_quantize_pack(x.data_ptr(), int(rows), int(E), _ptr(gamma), _ptr(beta), float(eps), len(rqs), arr, cp,
                                           _ptr(ln_out), status.data_ptr(), *_prep(ws), _stream(stream)))
    return codes, ln_out, status


def quantize_patchify(x, patch, scale, zero, qmin, qmax, n_bits, sign, out=None, status=None, stream=None):
    """qe_quantize_patchify: NCHW images -> packed codes of the (N (H/p) (W/p)) x (C p p) patch matrix.  Returns (codes, status)."""
    import torch
    assert x.is_cuda and x.is_contiguous() and x.dtype == torch.float32 and x.dim() == 4 and scale.numel() == zero.numel()
    N, C, H, W = x.shape
    if out is None:
        out = torch.empty(packed_nbytes(x.numel(), n_bits), dtype=torch.uint8, device=x.device)
    status = _status(status, x.device)
    check(lib().qe_quantize_patchify(x.data_ptr(), N, C, H, W, int(patch), scale.data_ptr(), zero.data_ptr(), int(scale.numel()),
                                     float(qmin), float(qmax), int(n_bits), 1 if sign else 0, out.data_ptr(), status.data_ptr(),
                                     _stream(stream)))
    return out, status


def attention_path(L, S, H, d):
    """qe_attention_path: 1 = the fp32 MFMA kernel, 0 = the fp32 VALU kernel, -1 = no kernel for the shape."""
    return int(lib().qe_attention_path(int(L), int(S), int(H), int(d)))


def attention_masked_path(L, S, H, d, has_mask=False, has_key_bias=False, causal=False):
    """qe_attention_masked_path: the kernel a masked call takes (1 MFMA, 0 VALU, -1 none)."""
    return int(lib().qe_attention_masked_path(int(L), int(S), int(H), int(d), int(bool(has_mask)), int(bool(has_key_bias)),
                                              int(bool(causal))))


def attention_bf16_path(L, S, H, d, has_mask=False, has_key_bias=False, causal=False):
    """qe_attention_bf16_path: 2 = the bf16 MFMA kernel, -1 = no kernel (d % 16 != 0, d > 128, a non-positive size)."""
    return int(lib().qe_attention_bf16_path(int(L), int(S), int(H), int(d), int(bool(has_mask)), int(bool(has_key_bias)),
                                            int(bool(causal))))


def attention_bf16_stored_path(L, S, H, d, has_mask=False, has_key_bias=False, causal=False):
    """qe_attention_bf16_stored_path: 2 = the bf16 MFMA kernel on bf16 rows, -1 = no kernel, as attention_bf16_path."""
    return int(lib().qe_attention_bf16_stored_path(int(L), int(S), int(H), int(d), int(bool(has_mask)), int(bool(has_key_bias)),
                                                   int(bool(causal))))


def attention_bf16_ctx_path(L, S, H, d, has_mask=False, has_key_bias=False, causal=False):
    """qe_attention_bf16_ctx_path: 2 = the bf16 MFMA kernel on bf16 rows with a bf16 context, -1 = no kernel."""
    return int(lib().qe_attention_bf16_ctx_path(int(L), int(S), int(H), int(d), int(bool(has_mask)), int(bool(has_key_bias)),
                                                int(bool(causal))))


PRECISIONS = ("fp32", "bf16")


def attention(q, k, v, N, L, H, S=None, layout="token", scale=None, out=None, stream=None, mask=None, key_bias=None,
              causal=False, precision="fp32", out_dtype=None):
    """qe_attention: softmax(scale q k^T) v per (image, head) on fp32 rows of E = H d floats, read in place.
    layout "token": q / out are (N L, E) and k / v (N S, E) rows (a ViT's projections); "seq": (L N, E) and (S N, E)
    (nn.MultiheadAttention with batch_first=False).  S defaults to L, scale to d ** -0.5.  Returns out, shaped like q
    (a new tensor when out is None).  No host synchronisation.
    mask / key_bias / causal (qe_attention_masked): the score becomes scale q.k + mask + key_bias, keys s <= t only under
    causal (top-left aligned).  mask: contiguous fp32, additive (finite or -inf), of shape (L, S), (N, L, S), (N, H, L, S) or
    (N*H, L, S); key_bias: contiguous fp32 (N, S).  A row with no visible key comes out NaN.
    precision "bf16" (qe_attention_bf16): both products on the bf16 matrix cores, fp32 softmax and accumulation, the same
    operands; d % 16 == 0 and d <= 128 only -- any other d raises QeError (unsupported), never the fp32 kernels instead.
    With precision "bf16", q, k and v may be torch.bfloat16 tensors, all three (qe_attention_bf16_stored: the rows are read
    as bf16, q^ = bf16(fp32(q) scale), k and v as stored; out stays fp32).  Mixed dtypes, or bf16 tensors with precision
    "fp32", raise ValueError.
    out_dtype=torch.bfloat16 (qe_attention_bf16_ctx; torch.bfloat16 q / k / v only, ValueError otherwise): the context as a
    bf16 tensor, each element the fp32 context's rounded to nearest even -- out, when given, is that bf16 tensor.  None (or
    torch.float32): the fp32 context."""
    if precision not in PRECISIONS:
        raise ValueError("precision must be 'fp32' or 'bf16'")
    import torch
    if out_dtype not in (None, torch.float32, torch.bfloat16):
        raise ValueError("out_dtype must be None, torch.float32 or torch.bfloat16")
    ctx16 = out_dtype == torch.bfloat16
    if ctx16 and not (q.dtype == k.dtype == v.dtype == torch.bfloat16):
        raise ValueError("out_dtype=torch.bfloat16 is allowed only with torch.bfloat16 q / k / v (precision='bf16'); got %s, %s, %s"
                         % (q.dtype, k.dtype, v.dtype))
    S = L if S is None else int(S)
    N, L, H = int(N), int(L), int(H)
    stored = q.dtype == torch.bfloat16
    if not (q.dtype == k.dtype == v.dtype) or q.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("q, k and v must all be torch.float32 or all torch.bfloat16; got %s, %s, %s" % (q.dtype, k.dtype, v.dtype))
    if stored and precision != "bf16":
        raise ValueError("torch.bfloat16 q / k / v need precision='bf16'")
    for t, rows in ((q, N * L), (k, N * S), (v, N * S)):
        assert t.is_cuda and t.is_contiguous() and t.numel() % rows == 0
    E = q.numel() // (N * L)
    assert k.numel() == N * S * E and v.numel() == N * S * E and E % H == 0
    d = E // H
    if layout == "token":
        q_rn, q_rt, kv_rn, kv_rt = L, 1, S, 1
    elif layout == "seq":
        q_rn, q_rt, kv_rn, kv_rt = 1, N, 1, N
    else:
        raise ValueError("layout must be 'token' or 'seq'")
    if out is None:
        out = torch.empty_like(q, dtype=torch.bfloat16 if ctx16 else torch.float32)
    assert out.is_contiguous() and out.dtype == (torch.bfloat16 if ctx16 else torch.float32) and out.numel() == q.numel()
    scale = float(d ** -0.5 if scale is None else scale)
    if mask is None and key_bias is None and not causal and precision == "fp32":
        check(lib().qe_attention(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), N, L, S, H, d, q_rn, q_rt, kv_rn,
                                 kv_rt, q_rn, q_rt, scale, _stream(stream)))
        return out
    mask_sn = mask_sh = 0
    if mask is not None:
        if not (torch.is_tensor(mask) and mask.is_cuda and mask.is_contiguous() and mask.dtype == torch.float32):
            raise ValueError("mask must be a contiguous fp32 CUDA tensor (additive: finite or -inf)")
        shape = tuple(mask.shape)
        if shape == (L, S):
            pass
        elif shape == (N, H, L, S) or shape == (N * H, L, S):
            mask_sn, mask_sh = H * L * S, L * S
        elif shape == (N, L, S):
            mask_sn = L * S
        else:
            raise ValueError("mask must be (L, S), (N, L, S), (N, H, L, S) or (N*H, L, S); got %s" % (shape,))
    if key_bias is not None:
        if not (torch.is_tensor(key_bias) and key_bias.is_cuda and key_bias.is_contiguous()
                and key_bias.dtype == torch.float32 and tuple(key_bias.shape) == (N, S)):
            raise ValueError("key_bias must be a contiguous fp32 CUDA tensor of shape (N, S)")
    run = lib().qe_attention_bf16_ctx if ctx16 else lib().qe_attention_bf16_stored if stored else lib().qe_attention_bf16 if precision == "bf16" else lib().qe_attention_masked
    check(run(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), N, L, S, H, d, q_rn, q_rt, kv_rn, kv_rt, q_rn, q_rt, scale,
              _ptr(mask), mask_sn, mask_sh, _ptr(key_bias), 1 if causal else 0, _stream(stream)))
    return out
