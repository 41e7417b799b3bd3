"""GPU: a synthetic packed ResNet run end to end.  The fused route (codes from epilogue to epilogue, the residual block
end inside the conv kernel, the stem's maxpool on codes) gives the same layer4 features and logits, bit for bit, as the
reference's dataflow with the engine plugged in (route="layers"), for ResNet-50 and ResNet-18, with the per-layer
fallbacks, and with check=False it never synchronises with the host."""
import pytest
import torch

from quantize_amd.packed_resnet import PackedResNet, calibrated_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def r50_sd():
    return calibrated_state_dict("resnet50", device=DEV, seed=0)


def _images(N, seed, size=224):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(N, 3, size, size, generator=g).to(DEV)


def _routes_equal(model, x):
    lf, ff = model.forward(x, route="fused")
    ll, fl = model.forward(x, route="layers")
    torch.cuda.synchronize()
    assert torch.isfinite(fl).all() and fl.abs().max() > 0
    assert torch.equal(ff, fl)
    assert torch.equal(lf, ll)
    return lf


def test_resnet50_fused_equals_layers(r50_sd):
    model = PackedResNet.from_state_dict(r50_sd)
    assert model.residual_paths(4) == [1] * 16                # every block end on the conv kernel's own epilogue
    logits = _routes_equal(model, _images(4, 1))
    assert logits.shape == (4, 1000) and logits.std() > 0
    assert model.residual_paths(3)[-3:] == [0, 0, 0]          # odd batch: the 7x7 block ends take two passes
    _routes_equal(model, _images(3, 2))


def test_resnet18_fused_equals_layers():
    model = PackedResNet.from_state_dict(calibrated_state_dict("resnet18", device=DEV, seed=3))
    assert model.residual_paths(2) == [0] * 8
    _routes_equal(model, _images(2, 4))


def test_fallbacks_stay_exact(r50_sd):
    sd = dict(r50_sd)
    # a signed consumer (no ReLU fold) inside a block, a non-zero zero point, the stem's consumer signed, and a
    # downsample quantiser that differs from its block's conv1
    for name in ("layer2.1.conv2", "layer1.0.conv1"):
        sd[name + ".a_quantizer.qmin"] = torch.tensor(-128.0)
        sd[name + ".a_quantizer.qmax"] = torch.tensor(127.0)
        sd[name + ".a_quantizer.scale"] = sd[name + ".a_quantizer.scale"] * 2
    sd["layer3.1.conv3.a_quantizer.zero"] = torch.tensor([-4.0], device=DEV)
    sd["layer3.0.downsample.0.a_quantizer.scale"] = sd["layer3.0.downsample.0.a_quantizer.scale"] * 1.25
    model = PackedResNet.from_state_dict(sd)
    assert not model.stages[1][1].convs[1].folds_relu and not model.stages[0][0].convs[0].folds_relu
    assert not model.stages[2][1].convs[2].folds_relu
    _routes_equal(model, _images(2, 5))


def test_sub_8_bit_activations():
    model = PackedResNet.from_state_dict(calibrated_state_dict("resnet18", device=DEV, seed=6, a_bits=6))
    _routes_equal(model, _images(2, 7))


def test_fused_route_does_not_synchronise(r50_sd):
    model = PackedResNet.from_state_dict(r50_sd)
    x = _images(2, 8)
    ref = model(x, route="fused", check=True)                 # warm-up: prepared tables, one host read of the flags
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = model(x, route="fused", check=False)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert torch.equal(out, ref)


def test_check_raises_out_of_range(r50_sd):
    model = PackedResNet.from_state_dict(r50_sd)
    x = _images(2, 9)
    x[1, 2, 100, 100] = float("nan")                              # NaN fails the range check, as in tpack
    with pytest.raises(RuntimeError, match="out of range"):
        model(x, route="fused", check=True)
