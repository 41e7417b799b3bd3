"""GPU: qe_quantlinear_grouped (8-bit activation codes x group-quantised AWQ-layout weight codes on the int8 matrix cores) against
the float64 reference of its contract (tests/linear_grouped_codes_ref.py) under the project's parity rule, conftest.conv_tolerance
with the fp32 F.linear on the dequantised operands as the chain; one test per group size on a power-of-two grid that must equal
float64 bit for bit; the G15 layers of the reference's AWQ estimator through PackedGroupedLinear's packed route; and the memory
contract of each kernel."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from quantize_amd import capi
from quantize_amd.synthetic import pack_codes

import linear_grouped_codes_ref as ref
from awq_cases import linear_case as _case
from linear_grouped_ref import g15_layer
from arena import FILLS, Arena, same_bytes
from conftest import conv_tolerance

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g15_awq_linear.npz")


def _run(c, out_off=0, x_off=0, place=None):
    """The call on the device.  out_off / x_off: elements / bytes the output view / activation stream start past an aligned
    address.  place: an Arena's place (operands inside guards) or None.  Returns (path, out view)."""
    dev = torch.device("cuda")
    put = (lambda a, **kw: torch.from_numpy(a).to(dev)) if place is None else (lambda a, **kw: place(torch.from_numpy(a).to(dev), **kw))
    xs = put(np.concatenate([np.zeros(x_off, np.uint8), c["x_stream"]]))[x_off:]
    xq = capi.qparam(xs, c["x_bits"], c["x_signed"], put(c["sx"]), put(c["zx"]))
    wq = capi.qparam(put(c["w_stream"]), c["w_bits"], c["w_signed"], put(c["sw"]), put(c["zw"]))
    bias, B, K, O = put(c["bias"]), c["B"], c["K"], c["O"]
    out = c.get("out")
    if out is None:
        out = torch.empty(B * O + out_off, dtype=torch.float32, device=dev)[out_off:].view(B, O)
    kw = dict(x_symmetric=c["xsym"], w_symmetric=c["wsym"])
    path = capi.linear_grouped_path(xq, wq, c["G"], B, K, O, **kw)
    capi.quantlinear_grouped(xq, wq, c["G"], bias, B, K, O, out=out, **kw)
    torch.cuda.synchronize()
    return path, out


def _assert_parity(c, got):
    xd, wd = ref.dequantised(c)
    chain = F.linear(torch.from_numpy(xd), torch.from_numpy(wd), torch.from_numpy(c["bias"])).numpy()
    err, allowed = conv_tolerance(got.cpu().numpy(), ref.forward(c), chain)
    print("max err %.3g allowed %.3g" % (err.max(), allowed))
    assert err.max() <= allowed


# bits x G x (w_symmetric, x_symmetric) x K in {G, 3G, 384}: B (1, 127, 129), O (4, 130), per-row sx and a misaligned out rotate
FAST = [(bits, G, wsym, xsym, ki) for bits in (4, 8) for G in (32, 64, 128) for wsym in (0, 1) for xsym in (0, 1) for ki in range(3)]


@pytest.mark.parametrize("n,bits,G,wsym,xsym,ki", [(n,) + f for n, f in enumerate(FAST)])
def test_fast_kernel_parity(n, bits, G, wsym, xsym, ki):
    K = (G, 3 * G, 384)[ki]
    B, O = (1, 127, 129)[(n + n // 3) % 3], (4, 130)[(n // 2 + ki) % 2]
    c = _case(200 + n, bits, G, K, B, O, bool(wsym), bool(xsym), per_row=(n + n // 6) % 2 == 0)
    path, got = _run(c, out_off=(n // 3 + ki) % 2)           # out_off 1: a 4-byte aligned view, element stores
    assert path == 1
    _assert_parity(c, got)


@pytest.mark.parametrize("w_bits,x_bits,G,K,x_off", [(3, 8, 32, 96, 0), (4, 8, 48, 96, 0), (4, 8, 8, 40, 0), (4, 8, 32, 96, 1), (4, 4, 32, 96, 0)],
                         ids=["bits3", "G48", "K40", "stream+1", "x4"])
@pytest.mark.parametrize("sym", [False, True])
def test_plain_kernel_parity(w_bits, x_bits, G, K, x_off, sym):
    c = _case(17 + w_bits + G + x_bits, w_bits, G, K, 33, 130, sym, sym, per_row=not sym, x_bits=x_bits)
    path, got = _run(c, x_off=x_off)
    assert path == 0
    _assert_parity(c, got)


@pytest.mark.parametrize("G", [32, 64, 128])
def test_fast_kernel_exact_on_a_power_of_two_grid(G):
    """4-bit unsigned weight codes, 8-bit unsigned activation codes, K = 256: sw in {2^-2, 2^-1, 1}, sx in {2^-4, 2^-3} per row, zeros
    of both operands integer or half-integer around the centre, bias multiples of 2^-8.  Every term is a multiple of 2^-8 and,
    as asserted from the float64 reference, sum |term| < 2^24 units.  The kernel's own partial sums -- the integer group sums,
    sw (P - zw' Sx) in units of 2^-3 below 256 * 128 * 10.5 < 2^19, zx' T, then one scaling by the power of two sx -- are all
    fp32 numbers too, so the result equals float64 bit for bit.  A neighbouring group's scale, a swapped nibble, a missed Sx
    or T term or a wrong centre moves it by whole units."""
    rng = np.random.RandomState(G)
    B, K, O = 129, 256, 130
    NG = K // G
    c = dict(w_bits=4, x_bits=8, G=G, K=K, B=B, O=O, wsym=False, xsym=False, w_signed=False, x_signed=False)
    c["w_stream"] = pack_codes(rng.randint(0, 16, size=(O, K)), 4, False)
    c["x_stream"] = pack_codes(rng.randint(0, 256, size=(B, K)), 8, False)
    c["sw"] = (2.0 ** rng.randint(-2, 1, size=O * NG)).astype(np.float32)
    c["zw"] = (rng.randint(12, 21, size=O * NG) / 2.0).astype(np.float32)
    c["sx"] = (2.0 ** rng.randint(-4, -2, size=B)).astype(np.float32)
    c["zx"] = (128 + rng.randint(-4, 5, size=B) / 2.0).astype(np.float32)
    c["bias"] = (rng.randint(-512, 513, size=O) / 256.0).astype(np.float32)
    exact, mag = ref.forward(c, terms=True)
    assert mag.max() < 2.0 ** 24 * 2.0 ** -8
    path, got = _run(c)
    assert path == 1
    assert np.array_equal(got.cpu().numpy().astype(np.float64), exact)


@pytest.mark.parametrize("layer", ["sym", "asym"])
def test_g15_awq_layers_through_the_packed_route(layer):
    """The reference's AWQ estimator's layers with a min/max 8-bit quantiser of pre_act * x_mul: quantize() equals numpy's fp32
    rint(x / s_k - z).clip bit for bit, call_packed meets the float64 contract on those codes."""
    g, lin, _ = g15_layer(GOLDEN, layer)
    K, O, G = (int(v) for v in g["config"][:3])
    x = g[layer + "_pre_act"]
    xp = x * lin.x_mul.numpy()[None, :]
    s = np.float32((xp.max() - xp.min()) / 255.0)
    z = np.float32(xp.min() / s)
    lin.set_quantizer(torch.tensor(s), torch.tensor(z), 0, 255)
    s_k = (np.float64(s) * lin.awq_scale.numpy().astype(np.float64)).astype(np.float32)
    lin = lin.to("cuda")
    codes, des = lin.quantize(torch.from_numpy(x).cuda())
    assert tuple(des) == (8, 0) + x.shape
    want = np.clip(np.rint(x / s_k[None, :] - z), 0, 255).astype(np.uint8)
    assert np.array_equal(codes.cpu().numpy().reshape(x.shape), want)
    got = lin.call_packed(codes, des)
    c = dict(w_bits=lin.w_bits, x_bits=8, G=G, K=K, B=x.shape[0], O=O, w_signed=lin.w_signed, x_signed=False,
             x_stream=codes.cpu().numpy(), w_stream=lin.weight.cpu().numpy(), sx=np.array([s]), zx=np.array([-z]),
             sw=lin.w_scale.cpu().numpy(), zw=lin._neg_w_zero.cpu().numpy(), bias=lin.bias.cpu().numpy())
    _assert_parity(c, got)


@pytest.mark.parametrize("kernel,bits,G,K,sym", [("fast-sym", 4, 64, 128, True), ("fast-asym", 4, 32, 96, False), ("plain", 3, 48, 96, False)])
def test_memory_contract(kernel, bits, G, K, sym):
    """Inside guard bands under both fills: guards and inputs unchanged, every output byte written, the output equal to the
    plain call's byte for byte."""
    c = _case(41, bits, G, K, 129, 132, sym, sym, per_row=True)
    path, plain = _run(c)
    assert path == (kernel != "plain")
    outs = []
    for fill in FILLS:
        arena = Arena("cuda", fill)
        c["out"] = arena.blank((c["B"], c["O"]), torch.float32, name="out")
        _, out = _run(c, place=arena.place)
        arena.check(kernel)
        outs.append(out.clone())
        del c["out"]
    assert same_bytes(outs[0], plain) and same_bytes(outs[1], plain)
