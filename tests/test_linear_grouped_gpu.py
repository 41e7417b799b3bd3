"""GPU: qe_quantlinear_grouped_float_input (group-quantised AWQ-layout weights on fp32 rows) against the float64 reference of its
contract (tests/linear_grouped_ref.py) under the project's parity rule, conftest.conv_tolerance with the fp32 F.linear on the
dequantised weights and x * x_mul as the chain; one test on a power-of-two grid that must equal float64 bit for bit; the G15
layers of the reference's AWQ estimator through PackedGroupedLinear.from_awq; and the memory contract of each kernel."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from quantize_amd import capi
from quantize_amd.synthetic import pack_codes

import linear_grouped_ref as ref
from arena import FILLS, Arena, same_bytes
from conftest import conv_tolerance

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g15_awq_linear.npz")


def _case(seed, bits, G, K, B, O, asym, mul):
    """Random operands: positive-mean activations; symmetric = signed codes and zeros 0, asymmetric = unsigned codes and a
    kernel-convention zero of 2^(bits-1) plus a fraction (the module's zero ~ -2^(bits-1))."""
    rng = np.random.RandomState(seed)
    NG = K // G
    lo, hi = (0, 1 << bits) if asym else (-(1 << (bits - 1)), 1 << (bits - 1))
    c = dict(bits=bits, G=G, K=K, B=B, O=O, signed=not asym, sym=not asym)
    c["stream"] = pack_codes(rng.randint(lo, hi, size=(O, K)), bits, not asym)
    c["x"] = (rng.randn(B, K) + 1.0).astype(np.float32)
    c["x_mul"] = rng.uniform(0.5, 2.0, size=K).astype(np.float32) if mul else None
    c["scale"] = (rng.uniform(0.5, 1.5, size=O * NG) * 2.0 ** (4 - bits) / np.sqrt(K)).astype(np.float32)
    c["zero"] = ((1 << (bits - 1)) + rng.uniform(-0.5, 0.5, size=O * NG) if asym else np.zeros(O * NG)).astype(np.float32)
    c["bias"] = rng.randn(O).astype(np.float32)
    return c


def _run(c, out_off=0, w_off=0, place=None):
    """The call on the device.  out_off / w_off: elements / bytes the output view / weight stream start past an aligned address.
    place: an Arena's place (operands inside guards) or None.  Returns (path, out view)."""
    dev = torch.device("cuda")
    put = (lambda a, **kw: torch.from_numpy(a).to(dev)) if place is None else (lambda a, **kw: place(torch.from_numpy(a).to(dev), **kw))
    stream = np.concatenate([np.zeros(w_off, np.uint8), c["stream"]])
    w = put(stream)[w_off:]
    x, sc, ze, bias = put(c["x"]), put(c["scale"]), put(c["zero"]), put(c["bias"])
    xm = None if c["x_mul"] is None else put(c["x_mul"])
    wq = capi.qparam(w, c["bits"], c["signed"], sc, ze)
    out = c.get("out")
    if out is None:
        out = torch.empty(c["B"] * c["O"] + out_off, dtype=torch.float32, device=dev)[out_off:].view(c["B"], c["O"])
    path = capi.linear_grouped_float_input_path(x, wq, c["G"], c["B"], c["K"], c["O"], x_mul=xm, symmetric=c["sym"])
    capi.quantlinear_grouped_float_input(x, wq, c["G"], bias, c["O"], x_mul=xm, out=out, symmetric=c["sym"])
    torch.cuda.synchronize()
    return path, out


def _assert_parity(c, got):
    exact = ref.forward(c["x"], c["x_mul"], c["stream"], c["bits"], c["signed"], c["scale"], c["zero"], c["G"], c["bias"], c["O"])
    wd = ref.dequantised(c["stream"], c["bits"], c["signed"], c["scale"], c["zero"], c["G"], c["O"], c["K"])
    xp = c["x"] if c["x_mul"] is None else c["x"] * c["x_mul"][None, :]
    chain = F.linear(torch.from_numpy(xp), torch.from_numpy(wd), torch.from_numpy(c["bias"])).numpy()
    err, allowed = conv_tolerance(got.cpu().numpy(), exact, chain)
    print("max err %.3g allowed %.3g" % (err.max(), allowed))
    assert err.max() <= allowed


# bits x G x symmetry x K in {G, 3G, 384}: B (1, 127, 129), O (4, 130), x_mul and a misaligned out rotate through the cases
FAST = [(bits, G, asym, ki) for bits in (4, 8) for G in (32, 64, 128) for asym in (False, True) for ki in range(3)]


@pytest.mark.parametrize("n,bits,G,asym,ki", [(n,) + f for n, f in enumerate(FAST)])
def test_fast_kernel_parity(n, bits, G, asym, ki):
    K = (G, 3 * G, 384)[ki]
    B, O = (1, 127, 129)[(n + n // 3) % 3], (4, 130)[(n // 2 + ki) % 2]
    c = _case(100 + n, bits, G, K, B, O, asym, mul=(n + n // 6) % 2 == 0)
    path, got = _run(c, out_off=(n // 3 + ki) % 2)           # out_off 1: a 4-byte aligned view, element stores
    assert path == 1
    _assert_parity(c, got)


@pytest.mark.parametrize("bits,G,K,w_off", [(3, 32, 96, 0), (4, 48, 96, 0), (4, 8, 40, 0), (4, 32, 96, 1)],
                         ids=["bits3", "G48", "K40", "stream+1"])
@pytest.mark.parametrize("asym", [False, True])
def test_plain_kernel_parity(bits, G, K, w_off, asym):
    c = _case(7 + bits + G, bits, G, K, 33, 130, asym, mul=asym)
    path, got = _run(c, w_off=w_off)
    assert path == 0
    _assert_parity(c, got)


@pytest.mark.parametrize("G", [32, 64, 128])
def test_fast_kernel_exact_on_a_power_of_two_grid(G):
    """4-bit unsigned codes, K = 256: x multiples of 2^-3, x_mul in {0.5, 1, 2}, scales powers of two in [2^-3, 1], zeros integer
    or half-integer, bias multiples of 2^-8 -> every term is a multiple of 2^-8 and, as asserted from the float64 reference,
    sum |term| < 2^24 units: every partial sum in any order is an fp32 number, so the result equals float64 bit for bit.  A
    scale of the neighbouring group, a swapped nibble or a wrong centre changes it by whole units."""
    rng = np.random.RandomState(G)
    B, K, O = 129, 256, 130
    NG = K // G
    c = dict(bits=4, G=G, K=K, B=B, O=O, signed=False, sym=False)
    c["stream"] = pack_codes(rng.randint(0, 16, size=(O, K)), 4, False)
    c["x"] = (rng.randint(-32, 33, size=(B, K)) / 8.0).astype(np.float32)
    c["x_mul"] = rng.choice([0.5, 1.0, 2.0], size=K).astype(np.float32)
    c["scale"] = (2.0 ** rng.randint(-3, 1, size=O * NG)).astype(np.float32)
    c["zero"] = (rng.randint(12, 20, size=O * NG) / 2.0).astype(np.float32)
    c["bias"] = (rng.randint(-512, 513, size=O) / 256.0).astype(np.float32)
    exact, mag = ref.forward(c["x"], c["x_mul"], c["stream"], 4, False, c["scale"], c["zero"], G, c["bias"], O, terms=True)
    assert mag.max() < 2.0 ** 24 * 2.0 ** -8
    path, got = _run(c)
    assert path == 1
    assert np.array_equal(got.cpu().numpy().astype(np.float64), exact)


@pytest.mark.parametrize("layer", ["sym", "asym"])
def test_g15_awq_layers(layer):
    """The reference's AWQ estimator's layers, packed by from_awq: against the float64 value of the contract, as close as the
    reference's own simulated fp32 output is."""
    g, lin, exact = ref.g15_layer(GOLDEN, layer)
    t = lambda k: torch.from_numpy(g["%s_%s" % (layer, k)])
    got = lin.to("cuda")(t("pre_act").cuda())
    err, allowed = conv_tolerance(got.cpu().numpy(), exact, g[layer + "_out"])
    print("max err %.3g allowed %.3g" % (err.max(), allowed))
    assert err.max() <= allowed


@pytest.mark.parametrize("kernel,bits,G,K,asym", [("fast-sym", 4, 64, 128, False), ("fast-asym", 4, 32, 96, True), ("plain", 3, 48, 96, True)])
def test_memory_contract(kernel, bits, G, K, asym):
    """Inside guard bands under both fills: guards and inputs unchanged, every output byte written, the output equal to the
    plain call's byte for byte."""
    c = _case(41, bits, G, K, 129, 132, asym, mul=True)
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
