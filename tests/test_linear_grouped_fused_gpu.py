"""GPU: qe_quantlinear_grouped_residual / _requant against the compositions their contract names, byte for byte, and against the
float64 reference (tests/linear_grouped_codes_ref.py); the two-pass route; the memory contract; a packed ViT with a grouped MLP."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from quantize_amd import capi, packed_vit, synthetic

import linear_grouped_codes_ref as ref
from arena import FILLS, Arena, same_bytes
from conftest import conv_tolerance
from awq_cases import linear_case as _case               # the operand generator of the plain entry point's tests

pytestmark = pytest.mark.gpu
QMIN, QMAX = -16.0, 255.0          # unsigned stored codes with a clamp below their range: a clamped negative code trips the flag
# bits x G x (w_symmetric, x_symmetric) x K in {G, 3G}; B (1, 127, 129), O, per-row sx and the quantiser's shape rotate
FUSED = [(n,) + f for n, f in enumerate((bits, G, wsym, xsym, ki) for bits in (4, 8) for G in (32, 64, 128) for wsym in (0, 1)
                                        for xsym in (0, 1) for ki in range(2))]


def _fused_case(n, bits, G, wsym, xsym, ki, Os):
    return _case(300 + n, bits, G, (G, 3 * G)[ki], (1, 127, 129)[(n + n // 3) % 3], Os[(n // 2 + ki) % 2], bool(wsym), bool(xsym),
                 per_row=(n + n // 6) % 2 == 0)


def _operands(c, put=lambda t, **kw: t):
    """(positional head of every call, keywords): the operands on the device, through an Arena's place when given."""
    t = lambda k: put(torch.from_numpy(c[k]).cuda())
    xq = capi.qparam(t("x_stream"), c["x_bits"], c["x_signed"], t("sx"), t("zx"))
    wq = capi.qparam(t("w_stream"), c["w_bits"], c["w_signed"], t("sw"), t("zw"))
    return (xq, wq, c["G"], t("bias"), c["B"], c["K"], c["O"]), dict(x_symmetric=c["xsym"], w_symmetric=c["wsym"])


def _paths(a, kw, rq=None, codes=None):
    xq, wq, G, _, B, K, O = a
    return (rq and capi.linear_grouped_requant_path(xq, wq, G, B, K, O, rq, codes, **kw), capi.linear_grouped_residual_path(xq, wq, G, B, K, O, **kw))


def _quantiser(c, y64, per_feature):
    """scale, zero (module convention, host): 2 sigma of y on 48 codes around 128, so the middle half of [0, 255] is used;
    every 5th feature of a per-feature quantiser has a scale 8 x too small: both clamps and the range flag."""
    s = np.full(c["O"] if per_feature else 1, y64.std() / 24.0 + 1e-3, np.float32)
    s[1::5] /= 8.0 if per_feature else 1.0
    return s, np.full_like(s, -128.0)


def _requant(s, z, put=lambda t, **kw: t):
    return capi.requant(put(torch.from_numpy(s).cuda()), put(torch.from_numpy(z).cuda()), QMIN, QMAX, 8, False)


def _two_pass_codes(a, kw, s, z, act):
    y = capi.quantlinear_grouped(*a, **kw)
    codes, _, status = capi.quantize_pack_act(y, torch.from_numpy(s).cuda(), torch.from_numpy(z).cuda(), QMIN, QMAX, 8, False, act=act)
    return y, codes, status


@pytest.mark.parametrize("n,bits,G,wsym,xsym,ki", FUSED)
def test_fused_residual(n, bits, G, wsym, xsym, ki):
    c = _fused_case(n, bits, G, wsym, xsym, ki, (4, 130))          # 130: the element store arm
    a, kw = _operands(c)
    res = torch.from_numpy(np.random.RandomState(n).randn(c["B"], c["O"]).astype(np.float32)).cuda()
    assert _paths(a, kw)[1] == 1
    want = capi.quantlinear_grouped(*a, **kw) + res
    got = capi.quantlinear_grouped_residual(*a, res, **kw)
    inplace = res.clone()
    assert capi.quantlinear_grouped_residual(*a, inplace, out=inplace, **kw) is inplace
    assert same_bytes(got, want) and same_bytes(inplace, want)
    xd, wd = ref.dequantised(c)
    chain = (F.linear(torch.from_numpy(xd), torch.from_numpy(wd), torch.from_numpy(c["bias"])) + res.cpu()).numpy()
    err, allowed = conv_tolerance(got.cpu().numpy(), ref.forward(c) + res.cpu().numpy().astype(np.float64), chain)
    print("max err %.3g allowed %.3g" % (err.max(), allowed))
    assert err.max() <= allowed


@pytest.mark.parametrize("n,bits,G,wsym,xsym,ki", FUSED)
def test_fused_codes(n, bits, G, wsym, xsym, ki):
    """Against float64, where the exact pre-clamp value v = act(y64) / s_o - z_o lies inside the stored range [0, 255]:
    |code - v| <= 0.5 + Lip allowed / s_o + A.  The kernel rounds v32 = fl(fl(act32(y32) / s) - z) to the nearest integer
    (0.5); |y32 - y64| <= allowed (conv_tolerance on y) grows by at most Lip, the largest slope of the activation (1, and 1.13
    for GELU), and shrinks to code units by 1 / s_o.  A is the quantiser's own fp32 rounding: |v| + |z| < 512, so the division
    and the subtraction are off by at most 2^-15 + 2^-16 < 2^-14; GELU's fp32 evaluation (erff within 4 ulp, a sum and two
    products) is within 8 * 2^-24 relative, 2^-12 at 512 codes."""
    c = _fused_case(n, bits, G, wsym, xsym, ki, (16, 144))         # one piece; a second column tile with a partial wave
    a, kw = _operands(c)
    y64 = ref.forward(c)
    xd, wd = ref.dequantised(c)
    for act, lip, arith in ((None, 1.0, 2.0 ** -14), ("gelu", 1.13, 2.0 ** -14 + 2.0 ** -12)):
        for per_feature in (False, True):
            s, z = _quantiser(c, y64, per_feature)
            rq = _requant(s, z)
            assert _paths(a, kw, rq)[0] == 1
            y, want, want_status = _two_pass_codes(a, kw, s, z, act)
            got, status = capi.quantlinear_grouped_requant(*a, rq, act=act, **kw)
            assert same_bytes(got, want) and int(status) == int(want_status)
            # the flag is exercised: below 0 only y itself goes (gelu(y) > -0.17), and one row may miss the few small scales
            assert int(status) == 1 or not per_feature or act is not None or c["B"] == 1
            chain = F.linear(torch.from_numpy(xd), torch.from_numpy(wd), torch.from_numpy(c["bias"])).numpy()
            _, allowed = conv_tolerance(y.cpu().numpy(), y64, chain)
            t = torch.from_numpy(y64)
            v = (t * 0.5 * (1 + torch.erf(t / 2 ** 0.5)) if act else t).numpy() / s.astype(np.float64) - z
            inside = (v >= 0) & (v <= 255)
            err = np.abs(got.cpu().numpy().reshape(v.shape).astype(np.float64) - v) - lip * allowed / s - arith
            print("%s per_feature %d: inside %d of %d, worst excess over 0.5: %.3g" % (act, per_feature, inside.sum(), v.size, (err - 0.5)[inside].max()))
            assert inside.mean() > 0.5 and (err[inside] <= 0.5).all()


@pytest.mark.parametrize("what", ["bits3", "O130", "codes+1"])
def test_two_pass_route(what):
    c = _case(77, 3 if what == "bits3" else 4, 32, 96, 33, 130 if what == "O130" else 144, False, False, per_row=True)
    a, kw = _operands(c)
    s, z = _quantiser(c, ref.forward(c), True)
    rq, L = _requant(s, z), capi.lib()
    codes = torch.empty(c["B"] * c["O"] + 1, dtype=torch.uint8, device="cuda")[what == "codes+1":][:c["B"] * c["O"]]
    assert _paths(a, kw, rq, codes) == (0, int(what != "bits3"))
    head = (ctypes.byref(a[0]), ctypes.byref(a[1]), c["G"], 0, 0, c["B"], c["K"], c["O"])
    need = L.qe_quantlinear_grouped_requant_workspace_size(*head, ctypes.byref(rq), codes.data_ptr())
    y, want, want_status = _two_pass_codes(a, kw, s, z, "gelu")
    _, status = capi.quantlinear_grouped_requant(*a, rq, act="gelu", codes=codes, workspace=torch.empty(need, dtype=torch.uint8, device="cuda"), **kw)
    assert need >= c["B"] * c["O"] * 4 and same_bytes(codes, want) and int(status) == int(want_status)
    if what == "bits3":
        assert L.qe_quantlinear_grouped_residual_workspace_size(*head) == need >= c["B"] * c["O"] * 4
        got = capi.quantlinear_grouped_residual(*a, y, workspace=torch.empty(need, dtype=torch.uint8, device="cuda"), **kw)
        assert same_bytes(got, y + y)


@pytest.mark.parametrize("form", ["codes", "residual"])
def test_memory_contract(form):
    """Inside guard bands under both fills: guards and inputs unchanged, every output byte written, the outputs equal."""
    c = _case(41, 4, 32, 96, 129, 144, False, False, per_row=True)
    s, z = _quantiser(c, ref.forward(c), True)
    outs = []
    for fill in FILLS:
        arena = Arena("cuda", fill)
        a, kw = _operands(c, arena.place)
        if form == "codes":
            out = arena.blank(c["B"] * c["O"], name="codes")
            capi.quantlinear_grouped_requant(*a, _requant(s, z, arena.place), act="gelu", codes=out, status=arena.status(), **kw)
        else:
            out = arena.blank((c["B"], c["O"]), torch.float32, name="out")
            capi.quantlinear_grouped_residual(*a, arena.place(torch.ones(c["B"], c["O"], device="cuda")), out=out, **kw)
        arena.check(form)
        outs.append(out.clone())
    assert same_bytes(outs[0], outs[1])


@pytest.mark.parametrize("grouped", [(True, True), (True, False)], ids=["fc1+fc2", "fc1 into a per-row fc2"])
def test_vit_with_grouped_mlp_fused_equals_layers(grouped):
    """The packed ViT's own invariant: every fused form is bit-identical to its two-pass form, so the logits are."""
    cfg = dict(image_size=16, patch=4, width=64, heads=2, mlp=128, depth=2)
    sd = packed_vit.calibrated_state_dict("vit_tiny_test", mlp_group_size=32, mlp_w_bits=4, mlp_grouped=grouped, **cfg)
    model = packed_vit.PackedViT.from_state_dict(sd, 2)
    assert [type(l).__name__ for b in model.blocks for l in (b.fc1, b.fc2)] == ["PackedGroupedLinear", "PackedGroupedLinear" if grouped[1] else "PackedLinear"] * 2
    images = synthetic.calibration_images(None, 2, 16, 0)("cuda")
    fused, layers = model(images, route="fused"), model(images, route="layers")
    assert torch.isfinite(fused).all() and same_bytes(fused, layers)
