"""CPU: the host side of qe_quantlinear_grouped_requant / qe_quantlinear_grouped_residual -- the exports, the path and workspace
queries over an eligibility table, and the refusal codes in the header's order.  Addresses are numbers: no row reaches a launch."""
import ctypes

import pytest

from quantize_amd import capi

OK, NBITS, ARG, WORKSPACE = 0, 1, 4, 6
A = 256      # an aligned stand-in address
B, K = 129, 96
XD, WD, OUT = 1 << 20, 2 << 20, 3 << 20      # refusal rows: 2 x 64 activation bytes, 4 x 64 / 2 weight bytes, 2 x 4 floats


def _q(bits, n_param, data=A, scale=A, zero=A):
    return capi.QeQParam(data, bits, 0, scale, zero, n_param)


def _rq(bits=8, n=1, scale=A, zero=A):
    return capi.QeRequant(scale, zero, n, 0.0, 255.0, bits, 0)


# w bits, group size, O, rq bits, rq n_param, codes address -> (requant path, residual path)
@pytest.mark.parametrize("wb,g,o,rq_bits,rq_n,codes,paths", [
    (4, 32, 144, 8, 1, A, (1, 1)), (8, 32, 144, 8, 144, A, (1, 1)), (4, 32, 144, 8, 1, None, (1, 1)),
    (3, 32, 144, 8, 1, A, (0, 0)), (4, 48, 144, 8, 1, A, (0, 0)),                       # the plain kernel's requests
    (4, 32, 130, 8, 1, A, (0, 1)), (4, 32, 144, 4, 1, A, (0, 1)), (4, 32, 144, 8, 1, A + 1, (0, 1))])
def test_exports_paths_and_workspace(wb, g, o, rq_bits, rq_n, codes, paths):
    L = capi.lib()
    x, w, rq = _q(8, 1), _q(wb, o * (K // g)), _rq(rq_bits, rq_n)
    args = (ctypes.byref(x), ctypes.byref(w), g, 0, 1, B, K, o)
    assert L.qe_quantlinear_grouped_requant_path(*args, ctypes.byref(rq), codes) == paths[0]
    assert L.qe_quantlinear_grouped_requant_workspace_size(*args, ctypes.byref(rq), codes) == (0 if paths[0] else B * o * 4)
    assert L.qe_quantlinear_grouped_residual_path(*args) == paths[1]
    assert L.qe_quantlinear_grouped_residual_workspace_size(*args) == (0 if paths[1] else B * o * 4)
    assert callable(capi.quantlinear_grouped_requant) and callable(capi.quantlinear_grouped_residual)


W = _q(4, 4 * 2)      # O = 4, K = 64, G = 32


@pytest.mark.parametrize("name,x,w,rows,act,rq,codes,code", [
    ("negative B before null rq", _q(8, 1), W, -1, 0, None, A, ARG),
    ("x n_bits 9 before null rq", _q(9, 1), W, 2, 0, None, A, NBITS),
    ("w n_param before rq n_bits", _q(8, 1), _q(4, 4), 2, 0, _rq(9), A, ARG),
    ("null rq", _q(8, 1), W, 2, 0, None, A, ARG),
    ("null rq scale before rq n_bits", _q(8, 1), W, 2, 0, _rq(9, scale=None), A, ARG),
    ("rq n_bits 9 before rq n_param", _q(8, 1), W, 2, 0, _rq(9, n=3), A, NBITS),
    ("rq n_param 3 of O 4", _q(8, 1), W, 2, 0, _rq(n=3), A, ARG),
    ("act 7", _q(8, 1), W, 2, 7, _rq(), A, ARG),
    ("null codes", _q(8, 1), W, 2, 1, _rq(), None, ARG),
    ("no rows, null codes", _q(8, 1), W, 0, 1, _rq(), None, OK),
    ("two passes (O % 16), no workspace", _q(8, 1), W, 2, 0, _rq(n=4), A, WORKSPACE)])
def test_requant_refusal_order(name, x, w, rows, act, rq, codes, code):
    L = capi.lib()
    head, rp = (ctypes.byref(x), ctypes.byref(w), 32, 0, 0), None if rq is None else ctypes.byref(rq)
    assert L.qe_quantlinear_grouped_requant(*head, None, rows, 64, 4, act, rp, codes, None, None, 0, None) == code, name
    if code in (ARG, NBITS) and codes is not None and act in (0, 1):
        assert L.qe_quantlinear_grouped_requant_path(*head, rows, 64, 4, rp, codes) == 0, name
        assert L.qe_quantlinear_grouped_requant_workspace_size(*head, rows, 64, 4, rp, codes) == 0, name


@pytest.mark.parametrize("name,x,w,rows,residual,out,ws_bytes,code", [
    ("w n_bits 0 before null residual", _q(8, 1), _q(0, 8), 2, None, OUT, 0, NBITS),
    ("null residual", _q(8, 1), W, 2, None, OUT, 0, ARG),
    ("null out", _q(8, 1), W, 2, OUT, None, 0, ARG),
    ("no rows, null residual and out", _q(8, 1), W, 0, None, None, 0, OK),
    ("out one element into residual", _q(8, 1), W, 2, OUT, OUT + 4, 0, ARG),
    ("out over the last byte of x", _q(8, 1, data=XD), W, 2, OUT, XD + 127, 0, ARG),
    ("out over the last byte of w", _q(8, 1), _q(4, 8, data=WD), 2, OUT, WD + 127, 0, ARG),
    ("overlap before the workspace", _q(8, 1), _q(3, 8), 2, OUT, OUT + 4, 0, ARG),
    ("two passes (3-bit weights), no workspace", _q(8, 1), _q(3, 8), 2, OUT, OUT, 0, WORKSPACE),
    ("two passes, a workspace one byte short", _q(8, 1), _q(3, 8), 2, OUT, OUT, 31, WORKSPACE)])
def test_residual_refusal_order(name, x, w, rows, residual, out, ws_bytes, code):
    L = capi.lib()
    head = (ctypes.byref(x), ctypes.byref(w), 32, 0, 0)
    assert L.qe_quantlinear_grouped_residual(*head, None, rows, 64, 4, residual, out, A if ws_bytes else None, ws_bytes, None) == code, name
    if code == NBITS:
        assert L.qe_quantlinear_grouped_residual_path(*head, rows, 64, 4) == 0, name
