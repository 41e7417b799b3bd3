"""CPU: PackedWideResNet's state_dict parsing and every error message, the BatchNorm affine, and the float64 model of
tests/wrn_exact.py (its exactness assertions on the exact models, no near-tie image in G14)."""
import numpy as np
import pytest
import torch

import preact_ref
import wrn_exact as we
from conftest import Golden
from quantize_amd.packed_wideresnet import PackedWideResNet, bn_affine, synthetic_state_dict


def _g14_sd():
    g = Golden("g14_wrn.npz")
    pre = "m_w8_sd_"
    return {k[len(pre):]: torch.from_numpy(g._z[k]) for k in g._z.files if k.startswith(pre)}, g


@pytest.mark.parametrize("depth,widen", [(10, 1), (16, 1), (16, 2), (22, 2)])
def test_depth_widths_strides_and_shortcuts_are_read_from_the_keys(depth, widen):
    m = PackedWideResNet.from_state_dict(synthetic_state_dict(depth=depth, widen=widen, num_classes=7))
    n = (depth - 4) // 6
    assert len(m.blocks()) == 3 * n and m.fc.O == 7 and m.fc.K == 64 * widen
    assert [b.conv1.OC for b in m.blocks()] == [16 * widen] * n + [32 * widen] * n + [64 * widen] * n
    assert [b.conv1.stride for b in m.blocks()] == ([1] * n + [2] + [1] * (n - 1)) * 1 + [2] + [1] * (n - 1)
    want = [widen != 1] + [False] * (n - 1) + [True] + [False] * (n - 1) + [True] + [False] * (n - 1)
    assert [b.shortcut is not None for b in m.blocks()] == want
    assert all(b.shortcut.KH == 1 and b.shortcut.padding == 0 and b.shortcut.stride == b.conv1.stride for b in m.blocks() if b.shortcut)
    assert [b.alpha.numel() for b in m.blocks()] == [b.conv1.IC for b in m.blocks()] and m.alpha.numel() == 64 * widen
    assert len(m.convs()) == 1 + 6 * n + sum(want) and m.final_map(32, 32) == (8, 8) and m.final_map(64, 64) == (16, 16)
    assert m.stem.bias is None and m.blocks()[0].conv1.bias is not None and m.blocks()[0].conv2.bias is None


def test_a_prefix_and_the_reference_written_state_dict_parse():
    sd = synthetic_state_dict(depth=10, widen=1)
    m = PackedWideResNet.from_state_dict({"net." + k: v for k, v in sd.items()}, prefix="net.")
    assert len(m.blocks()) == 3
    g14, _ = _g14_sd()
    m = PackedWideResNet.from_state_dict(g14)
    assert len(m.blocks()) == 6 and [b.shortcut is not None for b in m.blocks()] == [False, False, True, False, True, False]
    # conv1 and convShortcut were calibrated on the same tensor: one set of codes serves both
    assert all(len(b.consumers()) == 1 for b in m.blocks())


def test_bn_affine_is_the_contracts_fp32_sequence():
    sd, _ = _g14_sd()
    f = lambda k: sd["block2.layer.0.bn1." + k]
    alpha, shift = bn_affine(f("weight"), f("bias"), f("running_mean"), f("running_var"), 1e-5)
    a2, s2 = preact_ref.bn_affine(*(f(k).numpy() for k in ("weight", "bias", "running_mean", "running_var")), 1e-5)
    assert alpha.dtype == torch.float32 and np.array_equal(alpha.numpy(), a2) and np.array_equal(shift.numpy(), s2)
    m = PackedWideResNet.from_state_dict(sd)
    assert torch.equal(m.blocks()[2].alpha, alpha) and torch.equal(m.blocks()[2].shift, shift)
    m0 = PackedWideResNet.from_state_dict(sd, bn_eps=0.0)
    assert not torch.equal(m0.blocks()[2].alpha, alpha)


def test_every_error_message():
    sd = synthetic_state_dict(depth=16, widen=2)

    def without(*keys, **put):
        out = {k: v for k, v in sd.items() if k not in keys}
        out.update(put)
        return out

    with pytest.raises(KeyError, match=r"packed WideResNet state_dict: missing block2\.layer\.1\.bn1\.running_var"):
        PackedWideResNet.from_state_dict(without("block2.layer.1.bn1.running_var"))
    with pytest.raises(KeyError, match=r"packed WideResNet state_dict: missing net\.bn1\.weight"):
        PackedWideResNet.from_state_dict({"net." + k: v for k, v in without("bn1.weight").items()}, prefix="net.")
    with pytest.raises(KeyError, match=r"packed WideResNet state_dict: missing block1\.layer\.0\.conv2\.w_des"):
        PackedWideResNet.from_state_dict(without("block1.layer.0.conv2.w_des"))
    with pytest.raises(KeyError, match=r"packed WideResNet state_dict: missing fc\.weight"):
        PackedWideResNet.from_state_dict(without("fc.weight"))
    with pytest.raises(KeyError, match=r"packed WideResNet state_dict: stages block1\.\. not found \(have \[\]\)"):
        PackedWideResNet.from_state_dict({k: v for k, v in sd.items() if not k.startswith("block")})
    with pytest.raises(KeyError, match=r"packed WideResNet state_dict: stages block1\.\. not found \(have \[1, 3\]\)"):
        PackedWideResNet.from_state_dict({k: v for k, v in sd.items() if not k.startswith("block2.")})
    with pytest.raises(KeyError, match=r"packed WideResNet state_dict: block3 has blocks \[0, 2\]"):
        PackedWideResNet.from_state_dict(_gap(sd))
    with pytest.raises(ValueError, match=r"packed WideResNet state_dict: sub_block1 is not supported"):
        PackedWideResNet.from_state_dict(without(**{"sub_block1.layer.0.conv1.w_des": sd["block1.layer.0.conv1.w_des"]}))
    narrow = synthetic_state_dict(depth=16, widen=1)
    with pytest.raises(ValueError, match=r"fc: 64 input features and 128 bn1 channels behind a layer of 128 channels"):
        PackedWideResNet.from_state_dict(without(**{k: v for k, v in narrow.items() if k.startswith("fc.")}))
    three = {k.replace("block2.layer.1.conv1.", "block2.layer.0.convShortcut."): v for k, v in sd.items() if k.startswith("block2.layer.1.conv1.")}
    with pytest.raises(ValueError, match=r"block2\.layer\.0\.convShortcut: a 3x3 kernel where WideResNet has 1x1"):
        PackedWideResNet.from_state_dict(without(**three))
    one = {k.replace("block2.layer.0.convShortcut.", "block2.layer.0.conv2."): v for k, v in sd.items() if k.startswith("block2.layer.0.convShortcut.")}
    with pytest.raises(ValueError, match=r"block2\.layer\.0\.conv2: a 1x1 kernel where WideResNet has 3x3"):
        PackedWideResNet.from_state_dict(without(**one))
    with pytest.raises(ValueError, match=r"block2\.layer\.0: 32 -> 64 channels at stride 2 without a convShortcut"):
        PackedWideResNet.from_state_dict({k: v for k, v in sd.items() if not k.startswith("block2.layer.0.convShortcut.")})
    with pytest.raises(ValueError, match=r"block2\.layer\.0: 16 bn1, 16 conv1 and 16 convShortcut input channels behind a layer of 32"):
        PackedWideResNet.from_state_dict({k: v for k, v in sd.items() if not k.startswith("block2.layer.")} |
                                         {k: v for k, v in narrow.items() if k.startswith("block2.layer.")})
    with pytest.raises(ValueError, match="depth must be 6 n \\+ 4"):
        synthetic_state_dict(depth=18)
    with pytest.raises(ValueError, match="route must be"):
        PackedWideResNet.from_state_dict(narrow)(torch.zeros(1, 3, 32, 32), route="eager")
    with pytest.raises(ValueError, match=r"8 x 8 final map; 64 x 64 images end on 16 x 16"):
        PackedWideResNet.from_state_dict(narrow)(torch.zeros(1, 3, 64, 64))


def _gap(sd):
    """block3 with blocks 0 and 2"""
    return {k.replace("block3.layer.1.", "block3.layer.2."): v for k, v in sd.items()}


@pytest.mark.parametrize("kw", [dict(), dict(w_bits=4, a_bits=4)], ids=["w8a8", "w4a4"])
def test_the_float64_model_is_exact_on_the_exact_models(kw):
    from resnet_exact import NotExact, check_code_spread
    sd = we.exact_state_dict(**kw)
    x = we.images(3, 32, 11)
    r = we.Float64WideResNet(sd).forward(x)                     # raises NotExact where an intermediate is no fp32 value
    assert not r.near_tie.any() and r.ties > 0
    check_code_spread(r)
    p32, l32 = we.fp32_packed_forward(sd, x)
    assert torch.equal(l32.double(), r.logits) and torch.equal(p32.double(), r.features)
    # off the grid the assertions fire: the default eps makes alpha no power of two
    with pytest.raises(NotExact):
        we.Float64WideResNet(sd, bn_eps=1e-5).forward(x)


def test_no_g14_image_is_near_a_tie():
    sd, g = _g14_sd()
    x = torch.from_numpy(g._z["m_w8_images"])
    r = we.Float64WideResNet(sd, exact=False).forward(x)
    assert x.shape == (3, 3, 32, 32) and not r.near_tie.any()
    d_ref = float((torch.from_numpy(g._z["m_w8_logits"]).double() - r.logits).abs().max())
    d_pool = float((torch.from_numpy(g._z["m_w8_pooled"]).double() - r.features).abs().max())
    print("reference vs float64: logits %.3e (max |logit| %.3g), pooled %.3e" % (d_ref, float(r.logits.abs().max()), d_pool))
    assert d_ref < 1e-4 * float(r.logits.abs().max())
