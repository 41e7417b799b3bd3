"""CPU: PackedResNet.from_state_dict discovers a packed torchvision ResNet's stages, blocks, geometry and quantisers from
the key layout pack() leaves, fails clearly on a missing key, and the residual block-end path query (a host-side plan)
puts all 16 ResNet-50 block ends at batch 256 on the fused conv kernels."""
import numpy as np
import pytest
import torch

import oracle
from quantize_amd import capi
from quantize_amd.packed_resnet import PackedResNet, synthetic_state_dict
from quantize_amd.synthetic import pack_codes


def test_resnet50_layout_discovered():
    m = PackedResNet.from_state_dict(synthetic_state_dict("resnet50"))
    assert m.kind == "bottleneck"
    assert [len(s) for s in m.stages] == [3, 4, 6, 3]
    assert len(m.convs()) == 53
    assert (m.stem.stride, m.stem.padding, m.stem.KH, m.stem.OC) == (2, 3, 7, 64)
    for S, stage in enumerate(m.stages, start=1):
        for B, b in enumerate(stage):
            s = (1 if S == 1 else 2) if B == 0 else 1
            assert [(c.stride, c.padding, c.KH) for c in b.convs] == [(1, 0, 1), (s, 1, 3), (1, 0, 1)], b.name
            assert (b.downsample is not None) == (B == 0)
            if b.downsample is not None:
                assert (b.downsample.stride, b.downsample.padding, b.downsample.OC) == (s, 0, b.convs[-1].OC)
    assert m.fc_des == [8, 1, 1000, 2048]
    # quantisers: the image's signed, every post-ReLU one unsigned with zero point 0 (the ReLU folds into its clamp)
    assert m.stem.a_signed and not m.stem.folds_relu
    assert all(c.folds_relu for c in m.convs()[1:])
    ends = [(sh.IC, sh.OC, sh.H) for _, sh in m.block_end_shapes(256)]
    assert ends == [(64, 256, 56)] * 3 + [(128, 512, 28)] * 4 + [(256, 1024, 14)] * 6 + [(512, 2048, 7)] * 3


def test_resnet18_layout_discovered():
    m = PackedResNet.from_state_dict(synthetic_state_dict("resnet18"))
    assert m.kind == "basic"
    assert [len(s) for s in m.stages] == [2, 2, 2, 2]
    assert m.stages[0][0].downsample is None                  # 64 -> 64, stride 1: no downsample in layer1
    for S, stage in enumerate(m.stages, start=1):
        s = 1 if S == 1 else 2
        assert [(c.stride, c.padding) for c in stage[0].convs] == [(s, 1), (1, 1)]
        if S > 1:
            assert stage[0].downsample.stride == 2
    assert m.fc_des[3] == 512
    assert [(sh.OC, sh.H, sh.KH) for _, sh in m.block_end_shapes(2)] == [(64, 56, 3)] * 2 + [(128, 28, 3)] * 2 + \
        [(256, 14, 3)] * 2 + [(512, 7, 3)] * 2


def test_signed_consumer_does_not_fold():
    sd = synthetic_state_dict("resnet18")
    sd["layer2.1.conv2.a_quantizer.zero"] = torch.tensor([3.0])
    sd["layer3.1.conv2.a_quantizer.qmin"] = torch.tensor(-128.0)
    sd["layer3.1.conv2.a_quantizer.qmax"] = torch.tensor(127.0)
    m = PackedResNet.from_state_dict(sd)
    assert not m.stages[1][1].convs[1].folds_relu
    assert not m.stages[2][1].convs[1].folds_relu and m.stages[2][1].convs[1].a_signed
    assert m.stages[3][1].convs[1].folds_relu


def test_assigning_a_quantiser_updates_what_is_derived_from_it():
    """folds_relu, q_key and the negated zero follow an assignment to a_scale / a_zero with no further call."""
    m = PackedResNet.from_state_dict(synthetic_state_dict("resnet18"))
    c, twin = m.stages[1][0].convs[0], m.stages[1][0].downsample
    assert c.folds_relu and c.q_key == twin.q_key
    c.a_scale = torch.tensor([0.5])
    assert c.folds_relu and c.q_key != twin.q_key and c.q_key[0] == (0.5,)
    c.a_zero = torch.tensor([3.0])
    assert not c.folds_relu and c.q_key[1] == (3.0,) and c._neg_a_zero.tolist() == [-3.0]
    c.a_zero = torch.tensor([0.0])
    assert c.folds_relu
    c.a_scale = torch.tensor([0.0])               # a non-positive scale never folds
    assert not c.folds_relu
    c.a_scale, twin.a_scale = torch.tensor([0.25]), torch.tensor([0.25])
    assert c.folds_relu and c.q_key == twin.q_key


@pytest.mark.parametrize("key", ["layer3.2.conv2.w_scale", "layer2.0.downsample.0.w_des", "fc.weight", "conv1.a_quantizer.qmax"])
def test_missing_key_is_named(key):
    sd = synthetic_state_dict("resnet50")
    del sd[key]
    with pytest.raises(KeyError, match=key.split(".")[0]):
        PackedResNet.from_state_dict(sd)


def test_not_a_resnet():
    sd = synthetic_state_dict("resnet18")
    for k in [k for k in sd if k.startswith("layer")]:
        del sd[k]
    with pytest.raises(KeyError, match="stages"):
        PackedResNet.from_state_dict(sd)


def test_block_end_paths_at_batch_256():
    """The residual path query reads the host-side plan only: all 16 ResNet-50 block ends at batch 256 run the residual
    epilogue inside the conv kernel, with the next block's 8-bit codes and (last block) fp32 only."""
    m = PackedResNet.from_state_dict(synthetic_state_dict("resnet50"))
    assert m.residual_paths(256) == [1] * 16
    # without codes, and with per-channel or 4-bit codes (two passes)
    b, sh = m.block_end_shapes(256)[4]
    c = b.convs[-1]
    assert (c.a_bits, c.a_signed, c.w_bits, c.w_signed) == (8, False, 8, True)
    xq, wq = c.xq(torch.empty(64, dtype=torch.uint8)), c.wq()
    assert capi.residual_path(sh, xq, wq, None) == 1
    pc = torch.ones(sh.OC)
    assert capi.residual_path(sh, xq, wq, capi.requant(pc, pc * 0, 0, 255, 8, False)) == 0
    one = torch.ones(1)
    assert capi.residual_path(sh, xq, wq, capi.requant(one, one * 0, 0, 15, 4, False)) == 0
    # ResNet-18's 3x3 block ends: two passes
    assert PackedResNet.from_state_dict(synthetic_state_dict("resnet18")).residual_paths(256) == [0] * 8


@pytest.mark.parametrize("bits,signed", [(8, True), (8, False), (4, True), (3, False)])
def test_host_pack_matches_oracle_tpack(bits, signed):
    rng = np.random.RandomState(bits)
    lo, hi = (-(1 << (bits - 1)), (1 << (bits - 1))) if signed else (0, 1 << bits)
    q = rng.randint(lo, hi, size=(5, 7, 3))
    packed, _ = oracle.tpack(q, bits, signed)
    assert np.array_equal(pack_codes(q, bits, signed), packed)
