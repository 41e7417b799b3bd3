"""GPU: qe_quantconv2d_awq (packed NCHW activation codes x group-quantised AWQ-layout OIHW weight codes) against the float64
reference of its contract (tests/awq_conv_ref.py) under the project's parity rule, conftest.conv_tolerance with the fp32 F.conv2d
on the dequantised operands as the chain; one case per group size on a power-of-two grid that must equal float64 bit for bit; the
G16 layers of the reference's AWQ estimator through PackedAwqConv2d; and the memory contract of each kernel."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from quantize_amd import capi
from quantize_amd.synthetic import pack_codes

import awq_conv_ref as ref
from awq_cases import codes as _codes
from arena import FILLS, Arena, same_bytes
from conftest import conv_tolerance

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g16_awq_conv.npz")
PLANES = ((1, 1), (7, 7), (10, 13), (14, 14))          # P = 1, 49, 130, 196


def _case(seed, w_bits, G, IC, N, OC, hw, wsym, xsym, relu=False, x_bits=8, k=1, stride=1, padding=0):
    """Random operands.  Symmetric: zeros at the stream's centre; asymmetric: the centre plus a fraction in (-0.5, 0.5)."""
    rng = np.random.RandomState(seed)
    NG = IC // G
    c = dict(w_bits=w_bits, x_bits=x_bits, G=G, IC=IC, N=N, OC=OC, H=hw[0], W=hw[1], KH=k, KW=k, stride=stride, padding=padding,
             wsym=wsym, xsym=xsym, relu=relu)
    c["x_stream"], c["x_signed"], cx = _codes(rng, (N, IC) + tuple(hw), x_bits, xsym, (1 << x_bits) / 8)
    c["w_stream"], c["w_signed"], cw = _codes(rng, (OC, IC, k, k), w_bits, wsym, 0)
    c["sx"] = (rng.uniform(0.5, 1.5, size=1) * 2.0 ** (5 - x_bits)).astype(np.float32)
    c["zx"] = (cx + (0 if xsym else 1) * rng.uniform(-0.5, 0.5, size=1)).astype(np.float32)
    c["sw"] = (rng.uniform(0.5, 1.5, size=OC * NG) * 2.0 ** (4 - w_bits) / np.sqrt(IC * k * k)).astype(np.float32)
    c["zw"] = (cw + (0 if wsym else 1) * rng.uniform(-0.5, 0.5, size=OC * NG)).astype(np.float32)
    c["bias"] = rng.randn(OC).astype(np.float32)
    return c


def _run(c, out_off=0, x_off=0, w_off=0, place=None):
    """The call on the device.  out_off: elements the output view starts past an aligned address; x_off / w_off: bytes the
    streams do.  place: an Arena's place (operands inside guards) or None.  Returns (path, out)."""
    dev = torch.device("cuda")
    put = (lambda a, **kw: torch.from_numpy(a).to(dev)) if place is None else (lambda a, **kw: place(torch.from_numpy(a).to(dev), **kw))
    xs = put(np.concatenate([np.zeros(x_off, np.uint8), c["x_stream"]]))[x_off:]
    ws = put(np.concatenate([np.zeros(w_off, np.uint8), c["w_stream"]]))[w_off:]
    xq = capi.qparam(xs, c["x_bits"], c["x_signed"], put(c["sx"]), put(c["zx"]))
    wq = capi.qparam(ws, c["w_bits"], c["w_signed"], put(c["sw"]), put(c["zw"]))
    sh = capi.conv_shape(c["N"], c["IC"], c["H"], c["W"], c["OC"], c["KH"], c["KW"], c["stride"], c["padding"])
    shape = (c["N"], c["OC"]) + ref.out_hw(c)
    out = c.get("out")
    if out is None:
        out = torch.empty(int(np.prod(shape)) + out_off, dtype=torch.float32, device=dev)[out_off:].view(shape)
    kw = dict(x_symmetric=c["xsym"], w_symmetric=c["wsym"])
    path = capi.conv_awq_path(xq, wq, c["G"], sh, **kw)
    capi.quantconv2d_awq(xq, wq, c["G"], put(c["bias"]), sh, relu=c["relu"], out=out, **kw)
    torch.cuda.synchronize()
    return path, out


def _assert_parity(c, got):
    xd, wd = ref.dequantised(c)
    chain = F.conv2d(torch.from_numpy(xd), torch.from_numpy(wd), torch.from_numpy(c["bias"]), c["stride"], c["padding"])
    chain = (F.relu(chain) if c["relu"] else chain).numpy()
    err, allowed = conv_tolerance(got.cpu().numpy(), ref.forward(c), chain)
    print("max err %.3g allowed %.3g" % (err.max(), allowed))
    assert got.shape == chain.shape and err.max() <= allowed


# bits x G x (w_symmetric, x_symmetric) x IC in {G, 3G, 384}; the plane, N, OC, relu and the misaligned views rotate
FAST = [(bits, G, wsym, xsym, ki) for bits in (4, 8) for G in (32, 64, 128) for wsym in (0, 1) for xsym in (0, 1) for ki in range(3)]


@pytest.mark.parametrize("n,bits,G,wsym,xsym,ki", [(n,) + f for n, f in enumerate(FAST)])
def test_fast_kernel_parity(n, bits, G, wsym, xsym, ki):
    IC = (G, 3 * G, 384)[ki]
    hw, N, OC = PLANES[(n + n // 4) % 4], (1, 3)[(n + n // 3) % 2], (4, 130)[(n // 2 + ki) % 2]
    c = _case(300 + n, bits, G, IC, N, OC, hw, bool(wsym), bool(xsym), relu=(n // 5) % 2 == 1)
    path, got = _run(c, out_off=(n // 3 + ki) % 2, x_off=(n // 7) % 2)      # out_off 1: a 4-byte aligned view, element stores
    assert path == 1
    _assert_parity(c, got)


PLAIN = {"3x3": dict(k=3, padding=1), "3x3s2": dict(k=3, padding=1, stride=2), "1x1s2": dict(stride=2), "bits3": dict(w_bits=3),
         "G48": dict(G=48, IC=96), "x4": dict(x_bits=4), "stream+1": dict(w_off=1)}


@pytest.mark.parametrize("name", list(PLAIN))
@pytest.mark.parametrize("sym", [False, True])
def test_plain_kernel_parity(name, sym):
    kw = dict(PLAIN[name])
    w_off = kw.pop("w_off", 0)
    c = _case(17 + len(name), kw.pop("w_bits", 4), kw.pop("G", 32), kw.pop("IC", 64), 2, 5, (7, 6), sym, sym, relu=sym, **kw)
    path, got = _run(c, w_off=w_off)
    assert path == 0
    _assert_parity(c, got)


@pytest.mark.parametrize("G,hw", [(32, (7, 7)), (64, (14, 14)), (128, (10, 13))])
def test_fast_kernel_exact_on_a_power_of_two_grid(G, hw):
    """4-bit unsigned weight codes, 8-bit unsigned activation codes, IC = 256: sw in {2^-2, 2^-1, 1}, sx = 2^-4, zeros of both
    operands integer or half-integer around the centre, bias multiples of 2^-8.  Every term is a multiple of 2^-8 and, as
    asserted from the float64 reference, sum |term| < 2^24 units.  The kernel's own partial sums -- the integer group sums,
    sw (P - zw' Sx), zx' T, then one scaling by the power of two sx -- are all fp32 numbers too, so the result equals float64
    bit for bit.  A neighbouring group's scale, a swapped nibble or pixel, a missed Sx or T term or a wrong centre moves it by
    whole units."""
    rng = np.random.RandomState(G)
    N, IC, OC = 2, 256, 130
    c = dict(w_bits=4, x_bits=8, G=G, IC=IC, N=N, OC=OC, H=hw[0], W=hw[1], KH=1, KW=1, stride=1, padding=0, wsym=False, xsym=False,
             w_signed=False, x_signed=False, relu=False)
    c["w_stream"] = pack_codes(rng.randint(0, 16, size=(OC, IC)), 4, False)
    c["x_stream"] = pack_codes(rng.randint(0, 256, size=(N, IC) + hw), 8, False)
    c["sw"] = (2.0 ** rng.randint(-2, 1, size=OC * IC // G)).astype(np.float32)
    c["zw"] = (rng.randint(12, 21, size=OC * IC // G) / 2.0).astype(np.float32)
    c["sx"] = np.array([2.0 ** -4], np.float32)
    c["zx"] = np.array([128 + rng.randint(-4, 5) / 2.0], np.float32)
    c["bias"] = (rng.randint(-512, 513, size=OC) / 256.0).astype(np.float32)
    exact, mag = ref.forward(c, terms=True)
    assert mag.max() < 2.0 ** 24 * 2.0 ** -8
    path, got = _run(c)
    assert path == 1
    assert np.array_equal(got.cpu().numpy().astype(np.float64), exact)


@pytest.mark.parametrize("layer", ["p", "k"])
def test_g16_awq_layers_through_the_packed_class(layer):
    """The reference's AWQ estimator's layers (p: 1x1, IC 64, OC 48, symmetric; k: 3x3 / padding 1, IC 32, OC 16, asymmetric) with
    a min/max 8-bit quantiser of pre_act / awq_scale: quantize() equals numpy's fp32 rint(x / s_c - z).clip bit for bit,
    call_packed meets the float64 contract on those codes."""
    g, conv, x = ref.g16_layer(GOLDEN, layer)
    awq = g["awq_scale"].reshape(1, -1, 1, 1)
    xp = x / awq
    s = np.float32((xp.max() - xp.min()) / 255.0)
    z = np.float32(xp.min() / s)
    conv.set_quantizer(torch.tensor(s), torch.tensor(z), 0, 255)
    s_c = (np.float64(s) * awq.astype(np.float64)).astype(np.float32)
    conv = conv.to("cuda")
    codes, des = conv.quantize(torch.from_numpy(x).cuda())
    assert tuple(des) == (8, 0) + x.shape
    want = np.clip(np.rint(x / s_c - z), 0, 255).astype(np.uint8)
    assert np.array_equal(codes.cpu().numpy().reshape(x.shape), want)
    got = conv.call_packed(codes, des)
    assert capi.conv_awq_path(conv.xq(codes), conv.wq(), conv.group_size, capi.conv_shape(*x.shape, conv.O, conv.KH, conv.KW, 1,
                              conv.padding)) == (layer == "p")
    c = dict(w_bits=conv.w_bits, x_bits=8, G=conv.group_size, IC=conv.K, N=x.shape[0], OC=conv.O, H=x.shape[2], W=x.shape[3],
             KH=conv.KH, KW=conv.KW, stride=1, padding=conv.padding, relu=False, w_signed=conv.w_signed, x_signed=False,
             x_stream=codes.cpu().numpy(), w_stream=conv.weight.cpu().numpy(), sx=np.array([s]), zx=np.array([-z]),
             sw=conv.w_scale.cpu().numpy(), zw=conv._neg_w_zero.cpu().numpy(), bias=conv.bias.cpu().numpy())
    _assert_parity(c, got)


@pytest.mark.parametrize("kernel,bits,G,IC,hw,sym", [("fast-sym", 4, 64, 128, (14, 14), True), ("fast-asym", 4, 32, 96, (7, 7), False),
                                                     ("plain", 3, 48, 96, (7, 7), False)])
def test_memory_contract(kernel, bits, G, IC, hw, sym):
    """Inside guard bands under both fills: guards and inputs unchanged, every output byte written, the output equal to the
    plain call's byte for byte."""
    c = _case(41, bits, G, IC, 3, 132, hw, sym, sym, relu=True)
    path, plain = _run(c)
    assert path == (kernel != "plain")
    outs = []
    for fill in FILLS:
        arena = Arena("cuda", fill)
        c["out"] = arena.blank((c["N"], c["OC"]) + hw, torch.float32, name="out")
        _, out = _run(c, place=arena.place)
        arena.check(kernel)
        outs.append(out.clone())
        del c["out"]
    assert same_bytes(outs[0], plain) and same_bytes(outs[1], plain)
