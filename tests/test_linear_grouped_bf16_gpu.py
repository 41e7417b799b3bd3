"""GPU: qe_quantlinear_grouped_bf16_input (group-quantised AWQ-layout weights on bf16 rows) against the float64 reference of the
grouped contract (tests/linear_grouped_ref.py) on x' = bf16_rne(x * x_mul), under the project's parity rule,
conftest.conv_tolerance with the fp32 F.linear on the dequantised weights and x' as the chain; the residual form bit for bit
against the two steps; a power-of-two grid that must equal float64 bit for bit; and PackedGroupedLinear on bf16 rows."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from quantize_amd import capi
from quantize_amd.packed import PackedGroupedLinear
from quantize_amd.synthetic import pack_codes

import linear_grouped_ref as ref
from conftest import conv_tolerance

pytestmark = pytest.mark.gpu


def bf16_rne(a):
    """fp32 -> the nearest bf16 (ties to even), as fp32.  Finite values only."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000).astype(np.uint32).view(np.float32)


def _xprime(c):
    """The contract's x': one fp32 multiply, rounded once to bf16."""
    return c["x"] if c["x_mul"] is None else bf16_rne(c["x"] * c["x_mul"][None, :])


def _case(seed, bits, G, K, B, O, asym, mul):
    """Random operands as tests/test_linear_grouped_gpu.py draws them, the activations rounded to bf16."""
    rng = np.random.RandomState(seed)
    NG = K // G
    lo, hi = (0, 1 << bits) if asym else (-(1 << (bits - 1)), 1 << (bits - 1))
    return dict(bits=bits, G=G, K=K, B=B, O=O, signed=not asym, sym=not asym,
                stream=pack_codes(rng.randint(lo, hi, size=(O, K)), bits, not asym),
                x=bf16_rne((rng.randn(B, K) + 1.0).astype(np.float32)),
                x_mul=rng.uniform(0.5, 2.0, size=K).astype(np.float32) if mul else None,
                scale=(rng.uniform(0.5, 1.5, size=O * NG) * 2.0 ** (4 - bits) / np.sqrt(K)).astype(np.float32),
                zero=((1 << (bits - 1)) + rng.uniform(-0.5, 0.5, size=O * NG) if asym else np.zeros(O * NG)).astype(np.float32),
                bias=rng.randn(O).astype(np.float32))


def _offset(a, off, dtype):
    """The array on the device as a view `off` elements past an aligned address."""
    t = torch.empty(a.size + off, dtype=dtype, device="cuda")[off:]
    t.copy_(torch.from_numpy(a.reshape(-1)).to(dtype))
    return t.view(a.shape)


def _run(c, out_off=0, w_off=0, x_off=0, residual=None, out=None):
    """The call on the device.  out_off / x_off / w_off: elements / elements / bytes the output view, the rows and the weight
    stream start past an aligned address.  Returns (path, out view)."""
    dev = torch.device("cuda")
    put = lambda a: torch.from_numpy(a).to(dev)
    w = _offset(c["stream"], w_off, torch.uint8)
    x = _offset(c["x"], x_off, torch.bfloat16)                 # exact: the values are bf16 already
    xm = None if c["x_mul"] is None else put(c["x_mul"])
    wq = capi.qparam(w, c["bits"], c["signed"], put(c["scale"]), put(c["zero"]))
    if out is None:
        out = torch.empty(c["B"] * c["O"] + out_off, dtype=torch.float32, device=dev)[out_off:].view(c["B"], c["O"])
    path = capi.linear_grouped_bf16_input_path(x, wq, c["G"], c["B"], c["K"], c["O"], x_mul=xm, symmetric=c["sym"])
    capi.quantlinear_grouped_bf16_input(x, wq, c["G"], put(c["bias"]), c["O"], x_mul=xm, symmetric=c["sym"], residual=residual, out=out)
    torch.cuda.synchronize()
    return path, out


def _assert_parity(c, got):
    xp = _xprime(c)
    exact = ref.forward(xp, None, c["stream"], c["bits"], c["signed"], c["scale"], c["zero"], c["G"], c["bias"], c["O"])
    wd = ref.dequantised(c["stream"], c["bits"], c["signed"], c["scale"], c["zero"], c["G"], c["O"], c["K"])
    chain = F.linear(torch.from_numpy(xp), torch.from_numpy(wd), torch.from_numpy(c["bias"])).numpy()
    err, allowed = conv_tolerance(got.cpu().numpy(), exact, chain)
    print("max err %.3g allowed %.3g" % (err.max(), allowed))
    assert err.max() <= allowed


def _assert_residual_is_one_add(c, plain_out, **kw):
    """Aligned, misaligned and in place: the residual form equals the plain output plus the residual, added in fp32, bit for bit."""
    res = np.random.RandomState(5).randn(c["B"], c["O"]).astype(np.float32)
    want = plain_out + torch.from_numpy(res).cuda()
    for mode in ("aligned", "misaligned", "in place"):
        r = _offset(res, int(mode == "misaligned"), torch.float32)
        _, got = _run(c, residual=r, out=r if mode == "in place" else None, **kw)
        assert torch.equal(got, want), mode


# bits x G x symmetry x K in {G, 3G, 384}: B (1, 127, 129), O (4, 130), x_mul and a misaligned out rotate through the cases;
# K = 32 and K = 96 end in a half stage, K = 384 at G = 128 runs several stages per group
FAST = [(bits, G, asym, ki) for bits in (4, 8) for G in (32, 64, 128) for asym in (False, True) for ki in range(3)]


def _fast_case(n, bits, G, asym, ki):
    K = (G, 3 * G, 384)[ki]
    B, O = (1, 127, 129)[(n + n // 3) % 3], (4, 130)[(n // 2 + ki) % 2]
    return _case(100 + n, bits, G, K, B, O, asym, mul=(n + n // 6) % 2 == 0)


@pytest.mark.parametrize("n,bits,G,asym,ki", [(n,) + f for n, f in enumerate(FAST)])
def test_fast_kernel_parity(n, bits, G, asym, ki):
    c = _fast_case(n, bits, G, asym, ki)
    path, got = _run(c, out_off=(n // 3 + ki) % 2)           # out_off 1: a 4-byte aligned view, element stores
    assert path == 1
    _assert_parity(c, got)


@pytest.mark.parametrize("n", [1, 4, 20, 23], ids=["w4-sym", "w4-asym", "w8-sym", "w8-asym"])      # every <WB, SX> once
def test_fast_kernel_residual(n):
    c = _fast_case(n, *FAST[n])
    path, plain_out = _run(c)
    assert path == 1
    _assert_residual_is_one_add(c, plain_out)


@pytest.mark.parametrize("bits,G,K,w_off,x_off", [(3, 32, 96, 0, 0), (4, 48, 96, 0, 0), (4, 8, 40, 0, 0), (4, 32, 96, 1, 0), (4, 32, 96, 0, 1)],
                         ids=["bits3", "G48", "K40", "stream+1", "x+1"])
@pytest.mark.parametrize("asym", [False, True])
def test_plain_kernel_parity(bits, G, K, w_off, x_off, asym):
    c = _case(7 + bits + G, bits, G, K, 33, 130, asym, mul=asym)
    path, got = _run(c, w_off=w_off, x_off=x_off)
    assert path == 0
    _assert_parity(c, got)
    if bits == 3:
        _assert_residual_is_one_add(c, got)


def _grid_case(G, x_mul):
    """test_fast_kernel_exact_on_a_power_of_two_grid's operands (tests/test_linear_grouped_gpu.py): 4-bit unsigned codes, K = 256."""
    rng = np.random.RandomState(G)
    B, K, O = 129, 256, 130
    NG = K // G
    return dict(bits=4, G=G, K=K, B=B, O=O, signed=False, sym=False,
                stream=pack_codes(rng.randint(0, 16, size=(O, K)), 4, False),
                x=(rng.randint(-32, 33, size=(B, K)) / 8.0).astype(np.float32),
                x_mul=rng.choice(x_mul, size=K).astype(np.float32),
                scale=(2.0 ** rng.randint(-3, 1, size=O * NG)).astype(np.float32),
                zero=(rng.randint(12, 20, size=O * NG) / 2.0).astype(np.float32),
                bias=(rng.randint(-512, 513, size=O) / 256.0).astype(np.float32))


@pytest.mark.parametrize("G", [32, 64, 128])
def test_fast_kernel_exact_on_a_power_of_two_grid(G):
    """x multiples of 2^-3 in [-4, 4] and x_mul in {0.5, 1, 2}: x' is bf16-exact, the rounding is the identity, every term is a
    multiple of 2^-8 and, as asserted from the float64 reference, sum |term| < 2^24 units: every partial sum in any order is an
    fp32 number, so the result equals float64 bit for bit."""
    c = _grid_case(G, [0.5, 1.0, 2.0])
    assert np.array_equal(_xprime(c), c["x"] * c["x_mul"][None, :])
    exact, mag = ref.forward(_xprime(c), None, c["stream"], 4, False, c["scale"], c["zero"], G, c["bias"], c["O"], terms=True)
    assert mag.max() < 2.0 ** 24 * 2.0 ** -8
    path, got = _run(c)
    assert path == 1
    assert np.array_equal(got.cpu().numpy().astype(np.float64), exact)


def test_x_mul_product_is_rounded_to_nearest_even():
    """x_mul = 1.01 makes every product inexact in bf16: the parity rule against the ROUNDED x' pins the rounding itself (a
    kernel that kept the fp32 product, or truncated it, is off by up to 2^-8 of every term)."""
    c = _grid_case(64, [1.01])
    assert not np.array_equal(_xprime(c), c["x"] * c["x_mul"][None, :])
    path, got = _run(c)
    assert path == 1
    _assert_parity(c, got)


def test_packed_grouped_linear_on_bf16_rows():
    """__call__ on a bf16 tensor is the new entry point byte for byte (and call_bf16_residual its residual form); on x.float() it
    is still the fp32 entry point."""
    c = _case(3, 4, 64, 128, 70, 132, True, mul=True)
    t = lambda k: torch.from_numpy(c[k]).cuda()
    lin = PackedGroupedLinear(t("stream"), torch.tensor([4, 0, c["O"], c["K"]], dtype=torch.int32), t("scale"), -t("zero"), c["G"],
                              awq_scale=1.0 / t("x_mul"), bias=t("bias"))
    x = t("x").to(torch.bfloat16).view(2, 35, c["K"])
    want = capi.quantlinear_grouped_bf16_input(x.view(-1, c["K"]), lin.wq(), c["G"], lin.bias, c["O"], x_mul=lin.x_mul, symmetric=False)
    assert torch.equal(lin(x).view(-1, c["O"]), want)
    res = torch.randn(70, c["O"], device="cuda")
    assert torch.equal(lin.call_bf16_residual(x, res), want + res)
    want32 = capi.quantlinear_grouped_float_input(x.float().view(-1, c["K"]), lin.wq(), c["G"], lin.bias, c["O"], x_mul=lin.x_mul)
    assert torch.equal(lin(x.float()).view(-1, c["O"]), want32)
