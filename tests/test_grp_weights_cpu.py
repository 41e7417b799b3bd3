"""CPU: the three group-quantised (AWQ layout) entry points read ONE check of the weight operand and ONE weight side of fast
eligibility (csrc/qe_grp_common.hpp).  Over a table of weight operands, with everything else eligible for all three, the path
queries agree; a request whose only fault is in the weight operand gets the same code from all three run entry points.  The
addresses are numbers, not memory: every call here is a host-only query or is refused before a launch."""
import ctypes

import pytest

from quantize_amd import capi

K, O, B = 384, 8, 2                                   # K: a multiple of every G of the table; 1x1 / stride 1 / padding 0 on 7 x 7
OK, NBITS, ARG = 0, 1, 4
X, XMUL, W, OUT = 8192, 12288, 4096, 1 << 20           # 16-byte aligned addresses


def _wq(w_bits=4, G=32, addr=W, n_param=None):
    return capi.QeQParam(addr, w_bits, 0, 256, 512, O * K // G if n_param is None else n_param)


def _paths(wq, G):
    L, xq, sh = capi.lib(), capi.QeQParam(X, 8, 0, 256, 512, 1), capi.conv_shape(B, K, 7, 7, O, 1, 1, 1, 0)
    return (L.qe_quantlinear_grouped_float_input_path(X, XMUL, ctypes.byref(wq), G, 0, B, K, O),
            L.qe_quantlinear_grouped_path(ctypes.byref(xq), ctypes.byref(wq), G, 0, 0, B, K, O),
            L.qe_quantconv2d_awq_path(ctypes.byref(xq), ctypes.byref(wq), G, 0, 0, ctypes.byref(sh)))


def _runs(wq, G):
    L, xq, sh = capi.lib(), capi.QeQParam(X, 8, 0, 256, 512, 1), capi.conv_shape(B, K, 7, 7, O, 1, 1, 1, 0)
    return (L.qe_quantlinear_grouped_float_input(X, XMUL, ctypes.byref(wq), G, 0, None, B, K, O, OUT, None),
            L.qe_quantlinear_grouped(ctypes.byref(xq), ctypes.byref(wq), G, 0, 0, None, B, K, O, OUT, None),
            L.qe_quantconv2d_awq(ctypes.byref(xq), ctypes.byref(wq), G, 0, 0, None, ctypes.byref(sh), 0, OUT, None))


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("G", [16, 32, 48, 64, 128])
@pytest.mark.parametrize("w_bits", [3, 4, 8])
def test_the_three_paths_agree_on_the_weight_side(w_bits, G, off):
    want = int(w_bits in (4, 8) and G in (32, 64, 128) and off == 0)
    assert _paths(_wq(w_bits, G, W + off), G) == (want, want, want)


FAULTS = {"w.data": (dict(addr=0), 32, ARG), "w.n_bits=0": (dict(w_bits=0), 32, NBITS), "w.n_bits=9": (dict(w_bits=9), 32, NBITS),
          "G=0": (dict(n_param=O), 0, ARG), "K%G": (dict(n_param=O * 3), 112, ARG), "w.n_param": (dict(n_param=O * K // 32 - 1), 32, ARG)}


@pytest.mark.parametrize("what", list(FAULTS))
def test_a_faulty_weight_operand_gets_one_code_from_the_three_entry_points(what):
    kw, G, code = FAULTS[what]
    assert _runs(_wq(**kw), G) == (code, code, code)
    assert _paths(_wq(**kw), G) == (0, 0, 0)
