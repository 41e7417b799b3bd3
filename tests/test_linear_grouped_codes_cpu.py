"""CPU: qe_quantlinear_grouped's host side -- the float64 reference against an independent dequantise-then-matmul, the path
query over an eligibility table, the refusal codes in the header's order, and PackedGroupedLinear's optional activation
quantiser (state_dict round trip, the per-channel scale).  Addresses are numbers: no row reaches a launch."""
import ctypes

import numpy as np
import pytest
import torch

from quantize_amd import capi
from quantize_amd.packed import PackedGroupedLinear
from quantize_amd.synthetic import pack_codes

import linear_grouped_codes_ref as ref

OK, NBITS, ARG = 0, 1, 4
A = 256      # an aligned stand-in address


def _q(bits, n_param, data=A, scale=A, zero=A):
    return capi.QeQParam(data, bits, 0, scale, zero, n_param)


def test_reference_against_dequantise_then_matmul():
    rng = np.random.RandomState(0)
    B, K, O, G = 5, 96, 7, 32
    c = dict(B=B, K=K, O=O, G=G, x_bits=8, x_signed=False, w_bits=4, w_signed=True, bias=rng.randn(O),
             x_stream=pack_codes(rng.randint(0, 256, size=(B, K)), 8, False), w_stream=pack_codes(rng.randint(-8, 8, size=(O, K)), 4, True),
             sx=rng.uniform(0.5, 1.5, B), zx=rng.uniform(100, 150, B), sw=rng.uniform(0.5, 1.5, O * K // G), zw=rng.uniform(-1, 1, O * K // G))
    qx, qw, sx, zx, sw, zw = ref._operands(c)
    want = ((qx - zx) * sx) @ ((qw - np.repeat(zw, G, 1)) * np.repeat(sw, G, 1)).T + c["bias"]
    got, mag = ref.forward(c, terms=True)
    assert np.allclose(got, want, rtol=1e-12, atol=1e-12) and (np.abs(got) <= mag).all()


# x bits, w bits, G, K, x address, w address -> path
@pytest.mark.parametrize("xb,wb,G,K,xa,wa,path", [
    (8, 4, 32, 32, A, A, 1), (8, 8, 32, 96, A, A, 1), (8, 4, 64, 192, A, A, 1), (8, 8, 128, 384, A, A, 1),
    (8, 3, 32, 96, A, A, 0), (8, 4, 48, 96, A, A, 0), (8, 4, 32, 96, A + 1, A, 0), (8, 4, 32, 96, A, A + 1, 0), (4, 4, 32, 96, A, A, 0)])
def test_path(xb, wb, G, K, xa, wa, path):
    B, O = 129, 130
    for sym in (False, True):
        for n_param in (1, B):
            assert capi.linear_grouped_path(_q(xb, n_param, data=xa), _q(wb, O * (K // G), data=wa), G, B, K, O,
                                            x_symmetric=sym, w_symmetric=not sym) == path


@pytest.mark.parametrize("name,x,w,G,B,K,O,out,code", [
    ("negative B before null x", None, _q(4, 8), 32, -1, 64, 4, A, ARG),
    ("null x", None, _q(4, 8), 32, 2, 64, 4, A, ARG),
    ("null x data before x n_bits", _q(9, 1, data=None), _q(4, 8), 32, 2, 64, 4, A, ARG),
    ("x n_bits 9 before null w", _q(9, 1), None, 32, 2, 64, 4, A, NBITS),
    ("null w", _q(8, 1), None, 32, 2, 64, 4, A, ARG),
    ("null w zero before w n_bits", _q(8, 1), _q(9, 8, zero=None), 32, 2, 64, 4, A, ARG),
    ("w n_bits 0 before group_size 0", _q(8, 1), _q(0, 8), 0, 2, 64, 4, A, NBITS),
    ("group_size 0", _q(8, 1), _q(4, 8), 0, 2, 64, 4, A, ARG),
    ("K % group_size", _q(8, 1), _q(4, 8), 48, 2, 64, 4, A, ARG),
    ("x n_param 3 of B 2", _q(8, 3), _q(4, 8), 32, 2, 64, 4, A, ARG),
    ("w n_param per row only", _q(8, 2), _q(4, 4), 32, 2, 64, 4, A, ARG),
    ("null out", _q(8, 1), _q(4, 8), 32, 2, 64, 4, None, ARG),
    ("no rows", _q(8, 1), _q(4, 8), 32, 0, 64, 4, None, OK),
])
def test_refusal_code(name, x, w, G, B, K, O, out, code):
    L = capi.lib()
    xp, wp = (None if v is None else ctypes.byref(v) for v in (x, w))
    assert L.qe_quantlinear_grouped(xp, wp, G, 0, 0, None, B, K, O, out, None) == code, name
    if code != OK and out is not None:
        assert L.qe_quantlinear_grouped_path(xp, wp, G, 0, 0, B, K, O) == 0, name


def _layer(**kw):
    rng = np.random.RandomState(3)
    O, K, G = 6, 64, 32
    w = torch.from_numpy(pack_codes(rng.randint(0, 16, size=(O, K)), 4, False))
    des = torch.tensor([4, 0, O, K], dtype=torch.int32)
    scale, zero = torch.rand(O * K // G) + 0.5, torch.full((O * K // G,), -8.0)     # module convention: kernel zero 8 = the centre
    return PackedGroupedLinear(w, des, scale, zero, G, awq_scale=torch.rand(K) + 0.5, **kw)


def test_state_dict_round_trip_with_and_without_the_quantiser():
    plain = _layer()
    assert not any(k.startswith("a_quantizer") for k in plain.state_dict()) and plain.w_centred
    assert PackedGroupedLinear.from_state_dict(plain.state_dict()).a_scale is None
    with pytest.raises(ValueError):
        plain.quantize(torch.zeros(2, 64))
    lin = _layer(a_scale=torch.tensor(0.037), a_zero=torch.tensor(-128.0), a_qmin=0, a_qmax=255)
    sd = lin.state_dict()
    assert {k for k in sd if k.startswith("a_")} == {"a_quantizer." + k for k in ("scale", "zero", "qmin", "qmax")}
    again = PackedGroupedLinear.from_state_dict({"p." + k: v for k, v in sd.items()}, "p.")
    assert torch.equal(again.a_scale, lin.a_scale) and torch.equal(again.a_zero, lin.a_zero) and again.a_centred
    assert (again.a_bits, again.a_signed, again.a_qmin, again.a_qmax) == (8, False, 0.0, 255.0)
    assert torch.equal(again._a_scale_k, lin._a_scale_k) and not _layer(a_scale=torch.tensor(0.1), a_zero=torch.tensor(-127.5), a_qmin=0, a_qmax=255).a_centred


def test_quantiser_scale_is_the_product_formed_in_double():
    lin = _layer(a_scale=torch.tensor(0.037), a_zero=torch.tensor(-3.25), a_qmin=-128, a_qmax=127)
    want = (np.float64(lin.a_scale.numpy()[0]) * lin.awq_scale.numpy().astype(np.float64)).astype(np.float32)
    assert np.array_equal(lin._a_scale_k.numpy(), want) and lin.a_signed
    assert np.array_equal(lin._a_zero_k.numpy(), np.full(64, -3.25, np.float32))
