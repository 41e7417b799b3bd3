"""GPU: qe_quantconv2d_awq_fused against the compositions its contract names, byte for byte, and against the float64 reference
(tests/awq_conv_ref.py); the plain route, the memory contract, two PackedAwqConv2d layers chained through call_packed."""
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from quantize_amd import capi, packed

import awq_conv_ref as ref
from arena import FILLS, Arena, same_bytes
from conftest import conv_tolerance
from test_conv_awq_gpu import PLAIN, _case                                      # the operand generator and the plain geometries
from test_linear_grouped_fused_gpu import QMAX, QMIN, _quantiser, _requant      # the quantiser's recipe: 2 sigma on 48 codes around 128

pytestmark = pytest.mark.gpu
PLANES = ((7, 7), (10, 13), (14, 14), (16, 16))        # P = 49 byte stores, 130 a partial tile, 196 dwords (T = 128), 256 16-byte stores
# bits x G x (w_symmetric, x_symmetric) x IC in {G, 3G}; the plane, N, OC, the quantiser's shape and the misaligned views rotate
FUSED = [(n,) + f for n, f in enumerate((bits, G, wsym, xsym, ki) for bits in (4, 8) for G in (32, 64, 128) for wsym in (0, 1)
                                        for xsym in (0, 1) for ki in range(2))]


def _fused_case(n, bits, G, wsym, xsym, ki):
    hw, N, OC = PLANES[(n + n // 4) % 4], (1, 3)[(n + n // 3) % 2], (4, 130)[(n // 2 + ki) % 2]
    c = _case(500 + n, bits, G, (G, 3 * G)[ki], N, OC, hw, bool(wsym), bool(xsym))
    return dict(c, shape=(N, OC) + hw, per_channel=(n + n // 6) % 2 == 0, codes_off=(n // 3) % 2, out_off=(n // 5) % 2)


def _operands(c, put=lambda t, **kw: t):
    t = lambda k: put(torch.from_numpy(c[k]).cuda())
    xq = capi.qparam(t("x_stream"), c["x_bits"], c["x_signed"], t("sx"), t("zx"))
    wq = capi.qparam(t("w_stream"), c["w_bits"], c["w_signed"], t("sw"), t("zw"))
    sh = capi.conv_shape(c["N"], c["IC"], c["H"], c["W"], c["OC"], c["KH"], c["KW"], c["stride"], c["padding"])
    return (xq, wq, c["G"], t("bias"), sh), dict(x_symmetric=c["xsym"], w_symmetric=c["wsym"])


def _view(shape, dtype, off):                           # uninitialised, `off` elements past an aligned address
    return torch.empty(int(np.prod(shape)) + off, dtype=dtype, device="cuda")[off:].view(shape)


def _chain(c):
    xd, wd = ref.dequantised(c)
    return F.conv2d(torch.from_numpy(xd), torch.from_numpy(wd), torch.from_numpy(c["bias"]), c["stride"], c["padding"])


def _composed(a, kw, rq, relu, identity=None):
    """The contract's composition: (fp32, codes, status) of [relu](qe_quantconv2d_awq [+ identity]) then qe_quantize_pack."""
    y = capi.quantconv2d_awq(*a, relu=relu and identity is None, **kw)
    y = y if identity is None else torch.relu(y + identity) if relu else y + identity
    return (y,) + capi.quantize_pack(y, *rq._keep, rq.qmin, rq.qmax, rq.n_bits, False, inner=y.shape[2] * y.shape[3])


@pytest.mark.parametrize("n,bits,G,wsym,xsym,ki", FUSED)
def test_fused_codes(n, bits, G, wsym, xsym, ki):
    """Byte for byte against the composition, status included; and against float64 where the exact pre-clamp value v lies inside
    [0, 255]: |code - v| <= 0.5 + allowed / s_o + 2^-14 (test_linear_grouped_fused_gpu.py's bound: the rounding, conv_tolerance's
    bound on y through a slope of at most 1, the quantiser's own two fp32 roundings below 512 codes)."""
    c = _fused_case(n, bits, G, wsym, xsym, ki)
    a, kw = _operands(c)
    for relu in (False, True):
        y64 = ref.forward(dict(c, relu=relu))
        s, z = _quantiser(dict(O=c["OC"]), y64, c["per_channel"])
        v = y64 / s.astype(np.float64).reshape(-1, 1, 1) + 128.0
        inside = (v >= 0) & (v <= 255)
        assert inside.mean() > 0.5                          # a condition on the inputs: before the device result is looked at
        rq = _requant(s, z)
        y, want, want_status = _composed(a, kw, rq, relu)
        codes = _view(y.numel(), torch.uint8, c["codes_off"])
        assert capi.conv_awq_fused_path(*a[:3], a[4], relu=relu, rq=rq, codes=codes, **kw) == 1
        out, got, status = capi.quantconv2d_awq_fused(*a, relu=relu, rq=rq, codes=codes, **kw)
        assert out is None and same_bytes(got, want) and int(status) == int(want_status)
        _, allowed = conv_tolerance(y.cpu().numpy(), y64, (F.relu(_chain(c)) if relu else _chain(c)).numpy())
        err = np.abs(got.cpu().numpy().reshape(v.shape).astype(np.float64) - v) - allowed / s.reshape(-1, 1, 1) - 2.0 ** -14
        print("relu %d: inside %d of %d, status %d, worst excess over 0.5: %.3g" % (relu, inside.sum(), v.size, int(status), (err - 0.5)[inside].max()))
        assert (err[inside] <= 0.5).all()


@pytest.mark.parametrize("n,bits,G,wsym,xsym,ki,special", [f + (None,) for f in FUSED] + [FUSED[13] + ("nan",), FUSED[13] + ("inf",)])
def test_block_end(n, bits, G, wsym, xsym, ki, special):
    """out (out of place, in place) and codes (with out, alone) against the composition byte for byte; out against float64.
    special: a NaN in the identity passes through and always raises the flag; +inf clamps to qmax = 255, inside the code range,
    and does not (a per-tensor quantiser 16 sigma wide to either side, so nothing else clamps)."""
    c = _fused_case(n, bits, G, wsym, xsym, ki)
    a, kw = _operands(c)
    idt = torch.from_numpy(np.random.RandomState(n).randn(*c["shape"]).astype(np.float32))
    exact = np.maximum(ref.forward(c) + idt.numpy().astype(np.float64), 0.0)
    s, z = _quantiser(dict(O=c["OC"]), exact, c["per_channel"] and not special)
    if special:
        idt[0, 1, 0, 5], s = float(special), s * 3.0
    rq = _requant(s, z)
    ident = _view(c["shape"], torch.float32, c["out_off"]).copy_(idt)
    want, want_codes, want_status = _composed(a, kw, rq, True, ident)
    out, codes = _view(c["shape"], torch.float32, c["out_off"]), _view(want.numel(), torch.uint8, c["codes_off"])
    assert capi.conv_awq_fused_path(*a[:3], a[4], identity=ident, relu=True, out=out, rq=rq, codes=codes, **kw) == 1
    _, _, status = capi.quantconv2d_awq_fused(*a, identity=ident, relu=True, out=out, rq=rq, codes=codes, **kw)
    assert same_bytes(out, want) and same_bytes(codes, want_codes) and int(status) == int(want_status)
    none, only, status = capi.quantconv2d_awq_fused(*a, identity=ident, relu=True, rq=rq, **kw)
    assert none is None and same_bytes(only, want_codes) and int(status) == int(want_status)
    assert capi.quantconv2d_awq_fused(*a, identity=ident, relu=True, out=ident, **kw)[0] is ident and same_bytes(ident, want)
    if special:
        assert int(status) == (special == "nan") and not torch.isfinite(out[0, 1, 0, 5])
        return
    err, allowed = conv_tolerance(out.cpu().numpy(), exact, torch.relu(_chain(c) + idt).numpy())
    assert err.max() <= allowed, (err.max(), allowed)


@pytest.mark.parametrize("name", [k for k in PLAIN if k != "stream+1"])
def test_plain_route(name):
    """Identity + ReLU + per-channel 8-bit codes on the plain kernel; on 3x3 also 4-bit codes: through out, refused without it."""
    g = dict(PLAIN[name])
    c = _case(17 + len(name), g.pop("w_bits", 4), g.pop("G", 32), g.pop("IC", 64), 2, 5, (7, 6), False, False, **g)
    a, kw = _operands(c)
    ident = torch.from_numpy(np.random.RandomState(3).randn(2, 5, *ref.out_hw(c)).astype(np.float32)).cuda()
    s, z = _quantiser(dict(O=5), ref.forward(c), True)
    for rq in [_requant(s, z)] + [capi.requant(torch.ones(1, device="cuda"), torch.zeros(1, device="cuda"), 0, 15, 4, False)] * (name == "3x3"):
        want, want_codes, want_status = _composed(a, kw, rq, True, ident)
        out, codes = torch.empty_like(want), torch.empty_like(want_codes)
        assert capi.conv_awq_fused_path(*a[:3], a[4], identity=ident, relu=True, out=out, rq=rq, codes=codes, **kw) == 0
        _, _, status = capi.quantconv2d_awq_fused(*a, identity=ident, relu=True, out=out, rq=rq, codes=codes, **kw)
        assert same_bytes(out, want) and same_bytes(codes, want_codes) and int(status) == int(want_status)
    if name == "3x3":       # rq is the 4-bit one
        assert capi.conv_awq_fused_path(*a[:3], a[4], identity=ident, relu=True, rq=rq, codes=codes, **kw) == -1
        with pytest.raises(capi.QeError, match=re.escape(capi.lib().qe_error_string(capi.QE_ERR_UNSUPPORTED).decode())):
            capi.quantconv2d_awq_fused(*a, identity=ident, relu=True, rq=rq, **kw)


@pytest.mark.parametrize("kernel,bits,G,IC,hw,sym", [("fast-codes", 4, 64, 128, (14, 14), True), ("fast-end", 4, 32, 96, (7, 7), False),
                                                     ("plain-end", 3, 48, 96, (7, 7), False)])
def test_memory_contract(kernel, bits, G, IC, hw, sym):
    """Under both fills: guards and inputs unchanged, every output byte written, (out, codes, status) equal to the plain call's."""
    c = _case(41, bits, G, IC, 3, 132, hw, sym, sym)
    shape, end = (3, 132) + hw, kernel != "fast-codes"
    idt = torch.from_numpy(np.random.RandomState(4).randn(*shape).astype(np.float32)).cuda() if end else None
    s, z = _quantiser(dict(O=132), ref.forward(c), True)
    a, kw = _operands(c)
    plain = capi.quantconv2d_awq_fused(*a, identity=idt, relu=True, out="new" if end else None, rq=_requant(s, z), **kw)
    assert capi.conv_awq_fused_path(*a[:3], a[4], identity=idt, out=plain[0], rq=_requant(s, z), codes=plain[1], **kw) == (kernel != "plain-end")
    for fill in FILLS:
        arena = Arena("cuda", fill)
        a, kw = _operands(c, arena.place)
        out = arena.blank(shape, torch.float32, name="out") if end else None
        got = capi.quantconv2d_awq_fused(*a, identity=arena.place(idt) if end else None, relu=True, out=out, rq=_requant(s, z, arena.place),
                                         codes=arena.blank(int(np.prod(shape)), name="codes"), status=arena.status(), **kw)
        arena.check(kernel)
        assert all(g is None if p is None else same_bytes(g, p) for g, p in zip(got, plain))


def _awq_layer(rng, IC, OC, x, G=32):
    """A 1x1 W4 asymmetric PackedAwqConv2d on the device: min / max per group of the awq-scaled weight, min / max of x / awq_scale."""
    w, awq = torch.from_numpy(rng.randn(OC, IC, 1, 1).astype(np.float32) * 0.1), torch.from_numpy(rng.uniform(0.5, 2.0, IC).astype(np.float32))
    g = (w * awq.reshape(1, IC, 1, 1)).reshape(-1, G)
    scale, xp = (g.max(1).values - g.min(1).values) / 15.0, x.cpu() / awq.reshape(1, IC, 1, 1)
    layer = packed.PackedAwqConv2d.from_awq(w, (scale, g.min(1).values / scale, 0, 15, awq), 4, False, G, bias=torch.from_numpy(rng.randn(OC).astype(np.float32)))
    layer.set_quantizer((xp.max() - xp.min()) / 255.0, xp.min() * 255.0 / (xp.max() - xp.min()), 0, 255)
    return layer.to("cuda")


def test_two_layer_chain_fused_equals_layers():
    """64 -> 32 -> 64, the second layer closing a residual over the first's input: consumer= / identity= against the separate steps."""
    rng = np.random.RandomState(9)
    x = torch.from_numpy(rng.randn(2, 64, 7, 7).astype(np.float32)).cuda()
    l1 = _awq_layer(rng, 64, 32, x)
    c1, d1 = l1.quantize(x)
    h = torch.relu(l1.call_packed(c1, d1))
    l2 = _awq_layer(rng, 32, 64, h)
    c2, d2 = l2.quantize(h)
    y = torch.relu(l2.call_packed(c2, d2) + x)
    c2f, d2f = l1.call_packed(c1, d1, relu=True, consumer=l2)
    assert tuple(d2f) == tuple(d2) and same_bytes(c2f, c2)
    assert same_bytes(l2.call_packed(c2f, d2f, relu=True, identity=x), y)
