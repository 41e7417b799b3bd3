#!/usr/bin/env python3
"""Compare the linear plans of two builds, query by query: the host-side twin of tools/kernel_code_diff.py.

  tools/linear_plan_diff.py <old libqe_hip.so> <new libqe_hip.so>

Loads both libraries by path and asks each every host-only linear query of include/quant_engine.h -- qe_quantlinear_path and
_form, qe_quantlinear_float_input_path, and the _path and _workspace_bytes of the requant, residual, bf16, float-input
residual and bf16-input entries -- on a grid that crosses every rule of plan_linear (qe_linear.hip): row counts around the
chip-filling thresholds, reductions that are and are not whole stages (and one past the int32 bound), widths that are and
are not whole column tiles or multiples of 8, 8-bit and 4-bit operands, a per-tensor and a per-channel consumer quantiser,
each address 0, 2 and 4 bytes off a 16-byte boundary, and every QE_LIN_* knob.  No GPU is needed: the queries make no HIP
call.  Prints the answers that differ (the first 20) and the counts; the exit status is 1 on any difference.
"""
import ctypes
import itertools
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from quantize_amd.capi import QeQParam, QeRequant  # noqa: E402  (the structures only: no library is loaded by the import)

BS = (1, 33, 197, 3152, 12608, 50432)
KS = (32, 64, 100, 128, 768, 1056, 3072, 4096, 131072)
OS = (1, 16, 40, 96, 256, 768, 1000, 3072)
BITS = ((8, 8), (4, 8), (8, 4))                      # (activations, weights)
KNOBS = ({}, {"QE_LIN_EPI": "0"}, {"QE_LIN_F32_MFMA": "0"}, {"QE_LIN8": "0"}, {"QE_LIN8": "1"}, {"QE_LIN8": "2"},
         {"QE_LIN_NJ": "2"}, {"QE_LIN_NJ": "4"})
BASE = 1 << 20                                       # a 16-byte aligned stand-in address: the queries read alignment only
# (activations, weights, out / codes) byte offsets: all aligned, then one address at a time 2 and 4 bytes off
OFFSETS = [(0, 0, 0)] + [tuple(o if i == j else 0 for j in range(3)) for i in range(3) for o in (2, 4)]

_i32, _i64, _sz, _vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t, ctypes.c_void_p
_pq, _pr = ctypes.POINTER(QeQParam), ctypes.POINTER(QeRequant)
_dims = [_i64, _i32, _i32]
SIGS = {
    "qe_quantlinear_path": (_i32, [_pq, _pq] + _dims),
    "qe_quantlinear_form": (_i32, [_pq, _pq] + _dims + [_i32]),
    "qe_quantlinear_float_input_path": (_i32, [_vp, _pq] + _dims),
    "qe_quantlinear_requant_path": (_i32, [_pq, _pq] + _dims + [_pr, _vp]),
    "qe_quantlinear_requant_workspace_bytes": (_sz, [_pq, _pq] + _dims + [_pr, _vp]),
    "qe_quantlinear_residual_path": (_i32, [_pq, _pq] + _dims),
    "qe_quantlinear_residual_workspace_bytes": (_sz, [_pq, _pq] + _dims),
    "qe_quantlinear_bf16_path": (_i32, [_pq, _pq] + _dims + [_vp]),
    "qe_quantlinear_bf16_workspace_bytes": (_sz, [_pq, _pq] + _dims + [_vp]),
    "qe_quantlinear_float_input_residual_path": (_i32, [_vp, _pq] + _dims),
    "qe_quantlinear_float_input_residual_workspace_bytes": (_sz, [_vp, _pq] + _dims),
    "qe_quantlinear_bf16_input_path": (_i32, [_vp, _pq] + _dims),
    "qe_quantlinear_bf16_input_workspace_bytes": (_sz, [_vp, _pq] + _dims),
}


def load(path):
    L = ctypes.CDLL(os.path.abspath(path))
    for name, (res, args) in SIGS.items():
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    L.qe_debug_reload_env.restype, L.qe_debug_reload_env.argtypes = None, []
    return L


def answers(L, B, K, O, xb, wb, ox, ow, od):
    """[(query, answer)] of one problem: every query, the requant ones with a per-tensor and a per-channel quantiser."""
    x, w = QeQParam(BASE + ox, xb, 1, BASE, BASE, 1), QeQParam(BASE + ow, wb, 1, BASE, BASE, 1)
    xa, dst, d = BASE + ox, BASE + od, (B, K, O)
    out = [("path", L.qe_quantlinear_path(x, w, *d)),
           ("form", L.qe_quantlinear_form(x, w, *d, 1 if od == 0 else 0)),
           ("float_input_path", L.qe_quantlinear_float_input_path(xa, w, *d)),
           ("residual_path", L.qe_quantlinear_residual_path(x, w, *d)),
           ("residual_ws", L.qe_quantlinear_residual_workspace_bytes(x, w, *d)),
           ("bf16_path", L.qe_quantlinear_bf16_path(x, w, *d, dst)),
           ("bf16_ws", L.qe_quantlinear_bf16_workspace_bytes(x, w, *d, dst)),
           ("float_input_residual_path", L.qe_quantlinear_float_input_residual_path(xa, w, *d)),
           ("float_input_residual_ws", L.qe_quantlinear_float_input_residual_workspace_bytes(xa, w, *d)),
           ("bf16_input_path", L.qe_quantlinear_bf16_input_path(xa, w, *d)),
           ("bf16_input_ws", L.qe_quantlinear_bf16_input_workspace_bytes(xa, w, *d))]
    for n_param in (1, O):
        rq = QeRequant(BASE, BASE, n_param, -128.0, 127.0, 8, 1)
        out += [("requant_path/%d" % n_param, L.qe_quantlinear_requant_path(x, w, *d, rq, dst)),
                ("requant_ws/%d" % n_param, L.qe_quantlinear_requant_workspace_bytes(x, w, *d, rq, dst))]
    return out


def main(argv):
    if len(argv) != 3:
        sys.exit(__doc__)
    old, new = load(argv[1]), load(argv[2])
    keep = {k: os.environ.get(k) for kn in KNOBS for k in kn}
    compared = differ = 0
    for kn in KNOBS:
        for k in keep:
            os.environ.pop(k, None)
        os.environ.update(kn)
        old.qe_debug_reload_env()
        new.qe_debug_reload_env()
        for (B, K, O), (xb, wb), offs in itertools.product(itertools.product(BS, KS, OS), BITS, OFFSETS):
            for (q, a), (_, b) in zip(answers(old, B, K, O, xb, wb, *offs), answers(new, B, K, O, xb, wb, *offs)):
                compared += 1
                if a != b:
                    differ += 1
                    if differ <= 20:
                        print("%s %s bits %s offsets %s knobs %s: %s -> %s" % (q, (B, K, O), (xb, wb), offs, kn, a, b))
    for k, v in keep.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v
    print("answers compared: %d, different: %d" % (compared, differ))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
