"""CPU: qe_quantlinear_grouped_float_input's host side -- the path query over the shapes the GPU file runs, the refusal codes of
the bad requests, and PackedGroupedLinear.from_awq on the G15 fixture (the reference's AWQ estimator) against the reference's
own codes and simulated output.  Addresses are numbers: no row reaches a launch."""
import ctypes
import os

import numpy as np
import pytest
import torch

from quantize_amd import capi
from quantize_amd.packed import PackedGroupedLinear

import linear_grouped_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g15_awq_linear.npz")
OK, NBITS, ARG = 0, 1, 4
A = 256      # an aligned stand-in address


def _wq(bits, n_param, data=A, scale=A, zero=A):
    return capi.QeQParam(data, bits, 0, scale, zero, n_param)


# bits, G, K, weight address, x_mul address -> path
PATHS = ([(b, g, k, A, xm, 1) for b in (4, 8) for g in (32, 64, 128) for k in (g, 3 * g, 384) for xm in (None, A)] +
         [(3, 32, 96, A, None, 0), (4, 48, 96, A, None, 0), (4, 8, 40, A, None, 0), (4, 32, 96, A + 1, None, 0),
          (8, 32, 96, A, A + 4, 0), (2, 64, 128, A, None, 0)])


@pytest.mark.parametrize("bits,G,K,waddr,xm,path", PATHS)
def test_path(bits, G, K, waddr, xm, path):
    O = 130
    for sym in (False, True):
        assert capi.linear_grouped_float_input_path(A, _wq(bits, O * (K // G), data=waddr), G, 129, K, O, x_mul=xm,
                                                    symmetric=sym) == path


@pytest.mark.parametrize("name,w,G,B,K,O,x,out,code", [
    ("negative B", _wq(4, 8), 32, -1, 64, 4, A, A, ARG),
    ("null w", None, 32, 2, 64, 4, A, A, ARG),
    ("null data before n_bits", _wq(9, 8, data=None), 32, 2, 64, 4, A, A, ARG),
    ("null zero", _wq(4, 8, zero=None), 32, 2, 64, 4, A, A, ARG),
    ("n_bits 9 before group_size 0", _wq(9, 8), 0, 2, 64, 4, A, A, NBITS),
    ("group_size 0", _wq(4, 8), 0, 2, 64, 4, A, A, ARG),
    ("group_size -32", _wq(4, 8), -32, 2, 64, 4, A, A, ARG),
    ("K % group_size", _wq(4, 8), 48, 2, 64, 4, A, A, ARG),
    ("n_param per row only", _wq(4, 4), 32, 2, 64, 4, A, A, ARG),
    ("n_param one group too many", _wq(4, 12), 32, 2, 64, 4, A, A, ARG),
    ("null x", _wq(4, 8), 32, 2, 64, 4, None, A, ARG),
    ("null out", _wq(4, 8), 32, 2, 64, 4, A, None, ARG),
    ("no rows", _wq(4, 8), 32, 0, 64, 4, None, None, OK),
])
def test_refusal_code(name, w, G, B, K, O, x, out, code):
    L = capi.lib()
    wp = None if w is None else ctypes.byref(w)
    assert L.qe_quantlinear_grouped_float_input(x, None, wp, G, 0, None, B, K, O, out, None) == code, name
    if code != OK and x is not None and out is not None:      # (the query reads a null x as an aligned one)
        assert L.qe_quantlinear_grouped_float_input_path(x, None, wp, G, 0, B, K, O) == 0, name


@pytest.mark.parametrize("layer", ["sym", "asym"])
def test_from_awq_reproduces_the_reference(layer):
    g, lin, exact = ref.g15_layer(GOLDEN, layer)
    K, O, G = (int(v) for v in g["config"][:3])
    assert lin.symmetric == (layer == "sym") and lin.w_signed == (layer == "sym")
    codes = ref.decode(lin.weight.numpy(), O * K, lin.w_bits, lin.w_signed).reshape(O, K)
    assert np.array_equal(codes, g[layer + "_codes"].astype(np.int64))
    again = PackedGroupedLinear.from_state_dict(lin.state_dict())      # the state_dict round trip loads the same layer
    assert torch.equal(again.weight, lin.weight) and torch.equal(again.x_mul, lin.x_mul) and again.group_size == G
    x = g[layer + "_pre_act"]
    # the contract's exact value against the reference's fp32 simulation.  They differ by fp32 roundings of the operands -- three
    # in the reference's w_sim = (q + zero) * scale / awq_scale, two in x' = x * fp32(1 / awq_scale) -- and by the reference's
    # fp32 F.linear over K terms, taken as log2(K) roundings (a blocked sum): (3 + log2 K) 2^-23 of sum |term| covers both
    out = g[layer + "_out"]
    mag = np.abs(ref.xprime(x, lin.x_mul.numpy())) @ np.abs(ref.dequantised(lin.weight.numpy(), lin.w_bits, lin.w_signed,
                                                                        lin.w_scale.numpy(), lin._neg_w_zero.numpy(), G, O, K)).T.astype(np.float64)
    assert (np.abs(out - exact) <= (3 + np.log2(K)) * 2.0 ** -23 * mag + 1e-6).all()
