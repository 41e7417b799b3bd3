"""GPU: a packed WideResNet end to end.  On the exact models of tests/wrn_exact.py both routes of PackedWideResNet, the engine-free
float64 model and an fp32 torch forward agree bit for bit (pooled features and logits, every image); on a calibrated synthetic
model the fused route equals the layers route bit for bit; with check=False the fused route never synchronises with the host; an
image that does not end on an 8 x 8 map raises; and on G14 (b), what the reference's own modules wrote, the two routes agree bit
for bit and lie within twice the reference's own distance of the float64 model."""
import pytest
import torch

import wrn_exact as we
from conftest import Golden
from quantize_amd import capi
from quantize_amd.packed_wideresnet import PackedWideResNet, calibrated_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# no_fold: quantisers at block boundaries that are signed, have a non-zero zero point or are per channel (so no ReLU folds into
# their clamp and conv1 / convShortcut of block2.layer.0 and of block3.layer.0 take two sets of codes), and a signed consumer inside a block
CASES = {"w8a8": dict(), "w4a4": dict(w_bits=4, a_bits=4),
         "no_fold": dict(seed=3, variants={"block2.layer.0.convShortcut": {"signed": True}, "block1.layer.1.conv1": {"zero": 3},
                                           "block3.layer.0.conv1": {"per_channel": True}, "block2.layer.1.conv2": {"signed": True}})}


@pytest.mark.parametrize("case", sorted(CASES))
def test_exact_models_agree_bit_for_bit(case):
    sd = we.exact_state_dict(**CASES[case])
    f64 = we.Float64WideResNet(sd)
    model = PackedWideResNet.from_state_dict({k: v.to(DEV) for k, v in sd.items()}, bn_eps=0.0)
    b = model.blocks()
    insts = {capi.affine_relu_quantize_pack_path(3, k.conv1.IC, P, [c.requant() for c in k.consumers()])
             for k, P in zip(b, (1024, 1024, 1024, 256, 256, 64))}
    assert insts == ({0} if case == "w4a4" else {1})           # W4A4 packs sub-8-bit codes: the plain instance
    assert [len(k.consumers()) for k in b] == ([1, 1, 2, 1, 2, 1] if case == "no_fold" else [1] * 6)
    x = we.images(3, 32, 11)
    r = f64.forward(x)
    assert not r.near_tie.any()
    p32, l32 = we.fp32_packed_forward(sd, x)
    assert torch.equal(l32.double(), r.logits) and torch.equal(p32.double(), r.features)
    for route in ("layers", "fused"):
        logits, pooled = model.forward(x.to(DEV), route=route)
        assert torch.equal(pooled.cpu().double(), r.features), (case, route)
        assert torch.equal(logits.cpu().double(), r.logits), (case, route)
        assert torch.equal(logits.cpu(), l32) and torch.equal(pooled.cpu(), p32)


@pytest.mark.parametrize("kw", [dict(), dict(a_bits=6)], ids=["w8a8", "a6"])
def test_fused_equals_layers_on_a_calibrated_model(kw):
    sd = calibrated_state_dict(device=DEV, depth=16, widen=2, num_classes=16, seed=2, **kw)
    model = PackedWideResNet.from_state_dict(sd)
    g = torch.Generator(device="cpu").manual_seed(5)
    x = torch.randn(3, 3, 32, 32, generator=g).to(DEV)
    lf, pf = model.forward(x, route="fused")
    ll, pl = model.forward(x, route="layers")
    assert torch.isfinite(ll).all() and ll.abs().max() > 0 and pl.abs().max() > 0
    assert torch.equal(pf, pl) and torch.equal(lf, ll)


def test_fused_route_does_not_synchronise():
    sd = calibrated_state_dict(device=DEV, depth=10, widen=2, num_classes=16, seed=4)
    model = PackedWideResNet.from_state_dict(sd)
    g = torch.Generator(device="cpu").manual_seed(6)
    x = torch.randn(2, 3, 32, 32, generator=g).to(DEV)
    ref = model(x, route="fused", check=True)                 # warm-up: prepared tables, one host read of the flags
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = model(x, route="fused", check=False)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert torch.equal(out, ref)


def test_an_image_that_does_not_end_on_8x8_raises():
    sd = calibrated_state_dict(device=DEV, depth=10, widen=1, num_classes=4, seed=1)
    model = PackedWideResNet.from_state_dict(sd)
    for size in ((64, 64), (32, 28), (16, 16)):
        for route in ("fused", "layers"):
            with pytest.raises(ValueError, match="8 x 8 final map"):
                model(torch.zeros(1, 3, *size, device=DEV), route=route)


def test_g14_model_logits():
    """G14 (b).  The two routes agree bit for bit.  Against Float64WideResNet(exact=False): the engine's distance is compared with
    the reference's own on the same fixture; both are fp32 evaluations of the same function (ATen may fuse the BatchNorm's affine,
    the engine does not), so the engine is allowed twice the reference's distance.  Measured: reference 3.9e-8 on the logits
    (max |logit| 0.25) and 1.3e-7 on the pooled features, the engine 1.2e-8 and 5.1e-8."""
    g = Golden("g14_wrn.npz")
    pre = "m_w8_sd_"
    sd = {k[len(pre):]: torch.from_numpy(g._z[k]) for k in g._z.files if k.startswith(pre)}
    x = torch.from_numpy(g._z["m_w8_images"])
    f64 = we.Float64WideResNet(sd, exact=False).forward(x)
    assert not f64.near_tie.any()
    d_ref = float((torch.from_numpy(g._z["m_w8_logits"]).double() - f64.logits).abs().max())
    p_ref = float((torch.from_numpy(g._z["m_w8_pooled"]).double() - f64.features).abs().max())
    model = PackedWideResNet.from_state_dict({k: v.to(DEV) for k, v in sd.items()})
    ll, pl = model.forward(x.to(DEV), route="layers")
    lf, pf = model.forward(x.to(DEV), route="fused")
    assert torch.equal(lf, ll) and torch.equal(pf, pl)
    d = float((lf.cpu().double() - f64.logits).abs().max())
    p = float((pf.cpu().double() - f64.features).abs().max())
    print("logits: engine vs float64 %.3e, reference vs float64 %.3e; pooled: engine %.3e, reference %.3e" % (d, d_ref, p, p_ref))
    assert d <= 2 * d_ref and p <= 2 * p_ref
