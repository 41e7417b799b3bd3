"""CPU: PackedAwqConv2d on the G16 layers of the reference's AWQ estimator (tests/golden/g16_awq_conv.npz), its state_dict
round trip, and the host side of qe_quantconv2d_awq: the path of a table of requests and the code of every refused one.  The
addresses are numbers, not memory: no request here reaches a launch (each is a host-only query or is refused)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from quantize_amd import capi, packed

from awq_conv_ref import g16_layer
from linear_grouped_ref import decode

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g16_awq_conv.npz")
ARG, NBITS = 4, 1


@pytest.mark.parametrize("name", ["p", "k"])
def test_from_awq_reproduces_the_simulated_weight(name):
    g, conv, _ = g16_layer(GOLDEN, name)
    shape = g["w_sim"].shape
    assert (conv.O, conv.K, conv.KH, conv.KW) == shape and conv.w_scale.numel() == shape[0] * shape[1] // conv.group_size
    codes = decode(conv.weight.numpy(), int(np.prod(shape)), conv.w_bits, conv.w_signed).reshape(shape)
    assert np.array_equal(conv.dequantised_weight(torch.from_numpy(codes)).numpy(), g["w_sim"])
    assert conv.w_centred == (name == "p")              # the symmetric layer's zeros are the centre of its signed stream


def test_state_dict_round_trip():
    _, conv, _ = g16_layer(GOLDEN, "k")
    conv.set_quantizer(torch.tensor(0.05), torch.tensor(-3.0), 0, 255)
    sd = {"m." + k: v for k, v in conv.state_dict().items()}
    back = packed.from_state_dict(sd)["m"]
    assert type(back) is packed.PackedAwqConv2d and (back.stride, back.padding, back.group_size) == (1, 1, 32)
    a, b = conv.state_dict(), back.state_dict()
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def _request(IC=64, OC=8, hw=(7, 7), k=1, stride=1, padding=0, G=32, x_bits=8, w_bits=4, w_addr=4096, x_addr=8192 + 1, n_x=1, n_w=None):
    xq = capi.QeQParam(x_addr, x_bits, 0, 256, 512, n_x)
    wq = capi.QeQParam(w_addr, w_bits, 0, 256, 512, OC * (IC // G if G > 0 and IC % G == 0 else 1) if n_w is None else n_w)
    return xq, wq, G, capi.conv_shape(2, IC, hw[0], hw[1], OC, k, k, stride, padding)


@pytest.mark.parametrize("kw,path", [(dict(), 1), (dict(hw=(1, 1)), 1), (dict(w_bits=8, G=128, IC=384), 1), (dict(G=64, IC=192, OC=130), 1),
                                     (dict(k=3, padding=1), 0), (dict(stride=2), 0), (dict(padding=1), 0), (dict(w_bits=3), 0),
                                     (dict(x_bits=4), 0), (dict(G=48, IC=96), 0), (dict(G=16), 0), (dict(w_addr=4097), 0)])
def test_path_is_answered_on_the_host(kw, path):
    xq, wq, G, sh = _request(**kw)
    for xs in (0, 1):
        assert capi.conv_awq_path(xq, wq, G, sh, x_symmetric=xs, w_symmetric=xs) == path


REFUSED = {"shape": (dict(), ARG), "N": (dict(), ARG), "OW": (dict(k=9), ARG), "stride": (dict(stride=0), ARG),
           "x.data": (dict(x_addr=0), ARG), "x.n_bits": (dict(x_bits=9), NBITS), "w.data": (dict(w_addr=0), ARG),
           "w.n_bits": (dict(w_bits=0), NBITS), "G": (dict(G=0), ARG), "IC%G": (dict(IC=80), ARG), "x.n_param": (dict(n_x=64), ARG),
           "w.n_param": (dict(n_w=8), ARG), "out": (dict(), ARG)}


@pytest.mark.parametrize("what", list(REFUSED))
def test_refused_requests(what):
    kw, code = REFUSED[what]
    xq, wq, G, sh = _request(**kw)
    if what == "N":
        sh.N = 0
    shp = None if what == "shape" else ctypes.byref(sh)
    out = None if what == "out" else ctypes.c_void_p(1 << 20)
    L = capi.lib()
    assert L.qe_quantconv2d_awq(ctypes.byref(xq), ctypes.byref(wq), G, 0, 0, None, shp, 0, out, None) == code
    if what != "out":
        assert L.qe_quantconv2d_awq_path(ctypes.byref(xq), ctypes.byref(wq), G, 0, 0, shp) == 0
