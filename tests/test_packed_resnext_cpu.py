"""CPU: PackedResNet's parsing of ResNeXt state_dicts (grouped conv2 layers, the groups attribute, unchanged objects for a
plain ResNet), the float64 model's exactness assertions on the exact models of tests/resnext_exact.py, and what G12 holds."""
import pytest
import torch

import resnet_exact as rx
import resnext_exact as xe
from quantize_amd.packed import PackedConv2d, PackedGroupedConv2d
from quantize_amd.packed_resnet import PackedResNet

G12_REF_VS_FLOAT64 = 2.730e-08          # printed by tools/gen_golden_resnext.py when it wrote G12


@pytest.fixture(scope="module")
def g12():
    return xe.load_g12()


def test_g12_state_dict_yields_grouped_conv2_layers(g12):
    z, sds = g12
    assert sorted(sds) == ["g_cg16_s1_pc", "g_cg32_s2_bnfold", "g_cg4_s1_signed", "g_cg8_s2_unsigned", "m_x4"]
    m = PackedResNet.from_state_dict(sds["m_x4"])
    assert m.groups == 4 and m.kind == "bottleneck" and len(m.blocks()) == 4
    cgs = []
    for S, b in enumerate(m.blocks(), start=1):
        c1, c2, c3 = b.convs
        assert type(c1) is PackedConv2d and type(c3) is PackedConv2d and type(b.downsample) is PackedConv2d
        assert type(c2) is PackedGroupedConv2d and c2.groups == 4
        assert (c2.IC, c2.OC, c2.KH, c2.KW, c2.padding) == (c1.OC, c1.OC, 3, 3, 1) and c2.stride == (1 if S == 1 else 2)
        assert c3.IC == c2.OC
        cgs.append(c2.ICg)
    assert cgs == [4, 8, 16, 32]
    assert len(m.convs()) == 1 + 4 * 4 and m.fc.K == 256
    pre = PackedResNet.from_state_dict({"model." + k: v for k, v in sds["m_x4"].items()}, prefix="model.")
    assert pre.groups == 4


def test_plain_resnets_keep_their_objects():
    """groups == 1: the same classes as before, for G8's Bottleneck and BasicBlock models."""
    for key, (sd, images, feat, logits) in rx.load_g8().items():
        m = PackedResNet.from_state_dict(sd)
        assert m.groups == 1
        assert all(type(c) is PackedConv2d for c in m.convs()), key


def test_a_grouped_conv_in_a_basic_block_raises():
    sd = rx.exact_state_dict("resnet18", width=8, num_classes=4, image_size=32)
    sd = dict(sd)
    des = sd["layer1.0.conv2.w_des"].clone()
    des[3] = 2                                               # 8 -> 8 channels in 4 groups
    sd["layer1.0.conv2.w_des"] = des
    with pytest.raises(ValueError, match="grouped conv in a BasicBlock"):
        PackedResNet.from_state_dict(sd)


def test_mixed_groups_raise(g12):
    sd = dict(g12[1]["m_x4"])
    des = sd["layer2.0.conv2.w_des"].clone()
    des[3] = 16                                              # 32 channels in 2 groups next to layers of 4
    sd["layer2.0.conv2.w_des"] = des
    with pytest.raises(ValueError, match="different groups"):
        PackedResNet.from_state_dict(sd)


@pytest.mark.parametrize("case", ["w8a8", "no_fold"])
def test_float64_model_is_exact(case):
    kw = dict() if case == "w8a8" else dict(seed=3, variants={"layer2.0.conv3": {"signed": True}, "layer3.0.conv3": {"zero": 3}})
    sd = xe.exact_state_dict(**kw)
    model = xe.Float64ResNeXt(sd)
    assert model.groups == 4
    assert [c[1].w_codes.shape[1] for _, c, _ in model.blocks] == [4, 8, 16, 32]
    for size in (32, 64):
        r = model.forward(xe.images(2, size, 11))     # raises NotExact on any intermediate fp32 would round
        assert torch.isfinite(r.logits).all() and r.logits.abs().max() > 0
    m = PackedResNet.from_state_dict(sd)
    assert m.groups == 4
    if case == "no_fold":
        by = {c.name: c for c in m.convs()}
        assert not by["layer2.0.conv3"].folds_relu and not by["layer3.0.conv3"].folds_relu and by["layer1.0.conv3"].folds_relu


def test_g12_reference_forward_equals_float64_within_fp32_rounding(g12):
    """G12(b): the logits the reference's packed forward wrote against Float64ResNeXt on the same state_dict and images: the
    distance the generator printed, 2.73e-8 on logits of size 0.145 -- fp32 rounding alone, inside (K + 2) 2^-24 max|logits|
    with K = 256 fc terms."""
    z, sds = g12
    x = torch.from_numpy(z["m_x4_images"])
    assert tuple(x.shape) == (3, 3, 32, 32)
    r = xe.Float64ResNeXt(sds["m_x4"], exact=False).forward(x)
    ref = torch.from_numpy(z["m_x4_logits"]).double()
    d = float((ref - r.logits).abs().max())
    print("reference fp32 logits vs float64: %.3e (max |logits| %.3g)" % (d, float(ref.abs().max())))
    assert abs(d - G12_REF_VS_FLOAT64) <= 1e-11
    assert d <= 258 * 2.0 ** -24 * float(ref.abs().max())
    # (a): four grouped module runs, their settings as the tool names them
    for key, stride, signed, cg in (("g_cg4_s1_signed", 1, True, 4), ("g_cg8_s2_unsigned", 2, False, 8), ("g_cg16_s1_pc", 1, False, 16),
                                    ("g_cg32_s2_bnfold", 2, True, 32)):
        gsd = sds[key]
        geom = [int(v) for v in z[key + "_geom"]]
        assert [int(v) for v in gsd["w_des"][3:]] == [cg, 3, 3] and geom[:2] == [stride, 1]
        assert (float(gsd["a_quantizer.qmin"]) < 0) == signed
        c = PackedGroupedConv2d.from_state_dict(gsd, "", stride=stride, padding=1, in_channels=geom[2])
        assert c.ICg == cg and c.OC == c.IC == geom[2] and c.w_scale.numel() == c.OC
    assert float(sds["g_cg8_s2_unsigned"]["a_quantizer.zero"].abs().max()) > 0
    assert float(sds["g_cg16_s1_pc"]["w_zero"].abs().max()) > 0
