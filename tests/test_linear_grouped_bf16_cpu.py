"""CPU: qe_quantlinear_grouped_bf16_input's host side -- the symbols, the path query, the refusal codes in the order the header
states, and the weight operand held to the family's one check (csrc/qe_grp_common.hpp) through the fp32-row entry point.
Addresses are numbers: no row reaches a launch."""
import ctypes

import pytest

from quantize_amd import capi

OK, NBITS, ARG = 0, 1, 4
A = 1 << 20      # aligned stand-in addresses, 1 MB apart
X, XMUL, W, OUT, RES = A, 2 * A, 3 * A, 6 * A, 7 * A


def _wq(bits=4, n_param=8, data=W, zero=5 * A):
    return capi.QeQParam(data, bits, 0, 4 * A, zero, n_param)


def test_symbols_are_declared_and_exported():
    for name in ("qe_quantlinear_grouped_bf16_input", "qe_quantlinear_grouped_bf16_input_path"):
        assert name in capi.PROTOTYPES and name in capi.SYMBOLS and hasattr(capi.lib(), name)


# bits, G, K, x address, weight address, x_mul address -> path.  (The query takes neither out nor residual: out + 4 bytes only
# moves the store form inside the fast kernel, which the GPU file runs with path == 1.)
PATHS = ([(b, g, k, X, W, xm, 1) for b in (4, 8) for g in (32, 64, 128) for k in (g, 3 * g, 384) for xm in (None, XMUL)] +
         [(3, 32, 96, X, W, None, 0), (4, 48, 96, X, W, None, 0), (4, 8, 40, X, W, None, 0), (4, 32, 96, X, W + 1, None, 0),
          (8, 32, 96, X, W, XMUL + 4, 0), (4, 32, 96, X + 2, W, None, 0), (4, 32, 96, X + 1, W, None, 0)])


@pytest.mark.parametrize("bits,G,K,x,waddr,xm,path", PATHS)
def test_path(bits, G, K, x, waddr, xm, path):
    for sym in (False, True):
        assert capi.linear_grouped_bf16_input_path(x, _wq(bits, 130 * (K // G), data=waddr), G, 129, K, 130, x_mul=xm, symmetric=sym) == path


@pytest.mark.parametrize("name,w,G,B,x,res,out,code", [
    ("negative B", _wq(), 32, -1, X, None, OUT, ARG),
    ("null w", None, 32, 2, X, None, OUT, ARG),
    ("null data before n_bits", _wq(9, data=None), 32, 2, X, None, OUT, ARG),
    ("null zero", _wq(zero=None), 32, 2, X, None, OUT, ARG),
    ("n_bits 9 before group_size 0", _wq(9), 0, 2, X, None, OUT, NBITS),
    ("n_bits 9 before an odd x", _wq(9), 32, 2, X + 1, None, OUT, NBITS),
    ("group_size 0", _wq(), 0, 2, X, None, OUT, ARG),
    ("K % group_size", _wq(), 48, 2, X, None, OUT, ARG),
    ("n_param per row only", _wq(n_param=4), 32, 2, X, None, OUT, ARG),
    ("null x", _wq(), 32, 2, None, None, OUT, ARG),
    ("null out", _wq(), 32, 2, X, None, None, ARG),
    ("no rows, before an odd x", _wq(), 32, 0, X + 1, None, None, OK),
    ("odd x", _wq(), 32, 2, X + 1, None, OUT, ARG),
    ("out + 2", _wq(), 32, 2, X, None, OUT + 2, ARG),
    ("residual + 2", _wq(), 32, 2, X, RES + 2, OUT, ARG),
    ("out overlaps the last byte of x", _wq(), 32, 2, X, None, X + 2 * 64 * 2 - 4, ARG),
    ("x overlaps the last byte of out", _wq(), 32, 2, OUT + 2 * 4 * 4 - 2, None, OUT, ARG),
    ("residual overlaps out", _wq(), 32, 2, X, OUT + 4, OUT, ARG),
])
def test_refusal_code(name, w, G, B, x, res, out, code, K=64, O=4):
    L = capi.lib()
    wp = None if w is None else ctypes.byref(w)
    assert L.qe_quantlinear_grouped_bf16_input(x, None, wp, G, 0, None, B, K, O, res, out, None) == code, name
    if code != OK and x is not None and res is None and out == OUT:      # what the query can see (a null x reads as aligned)
        assert L.qe_quantlinear_grouped_bf16_input_path(x, None, wp, G, 0, B, K, O) == 0, name


# the weight operand as tests/test_grp_weights_cpu.py holds the other three entry points: the family's eligibility and codes
K, O, B = 384, 8, 2


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("G", [16, 32, 48, 64, 128])
@pytest.mark.parametrize("bits", [3, 4, 8])
def test_the_weight_side_of_the_path_is_the_familys(bits, G, off):
    L, wq = capi.lib(), _wq(bits, O * K // G, data=W + off)
    want = int(bits in (4, 8) and G in (32, 64, 128) and off == 0)
    assert L.qe_quantlinear_grouped_bf16_input_path(X, XMUL, ctypes.byref(wq), G, 0, B, K, O) == want
    assert L.qe_quantlinear_grouped_float_input_path(X, XMUL, ctypes.byref(wq), G, 0, B, K, O) == want


@pytest.mark.parametrize("kw,G", [(dict(data=None), 32), (dict(bits=0), 32), (dict(bits=9), 32), (dict(n_param=O), 0),
                                  (dict(n_param=O * 3), 112), (dict(n_param=O * K // 32 - 1), 32)])
def test_a_faulty_weight_operand_gets_the_familys_code(kw, G):
    L, wq = capi.lib(), _wq(**{"n_param": O * K // 32, **kw})
    code = L.qe_quantlinear_grouped_float_input(X, XMUL, ctypes.byref(wq), G, 0, None, B, K, O, OUT, None)
    assert code != OK
    assert L.qe_quantlinear_grouped_bf16_input(X, XMUL, ctypes.byref(wq), G, 0, None, B, K, O, None, OUT, None) == code
    assert L.qe_quantlinear_grouped_bf16_input_path(X, XMUL, ctypes.byref(wq), G, 0, B, K, O) == 0
