"""GPU: relu_codes of the three conv classes -- the fused step of the packed CNNs' `fused` route -- against its own two-pass
form, byte for byte: consumer.quantize_codes(relu(fp32 output of the same layer on the same codes)).  The consumer's scale is
set by max from that fp32 output, so no code is out of range and both status words must stay 0."""
import numpy as np
import pytest
import torch

from quantize_amd import synthetic
from quantize_amd.packed import PackedConv2d, PackedDepthwiseConv2d, PackedGroupedConv2d

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, H, W = 2, 8, 8

# name: (class, input channels, conv_entries' (IC, OC, K, groups), constructor geometry)
LAYERS = {
    "dense_1x1": (PackedConv2d, 32, (32, 32, 1, 1), dict(stride=1, padding=0)),
    "dense_3x3_s1": (PackedConv2d, 16, (16, 32, 3, 1), dict(stride=1, padding=1)),
    "dense_3x3_s2": (PackedConv2d, 16, (16, 32, 3, 1), dict(stride=2, padding=1)),
    "depthwise_3x3_s1": (PackedDepthwiseConv2d, 16, (1, 16, 3, 1), dict(stride=1, padding=1)),
    "depthwise_3x3_s2": (PackedDepthwiseConv2d, 16, (1, 16, 3, 1), dict(stride=2, padding=1)),
    "grouped_3x3_g4": (PackedGroupedConv2d, 32, (32, 32, 3, 4), dict(stride=1, padding=1, in_channels=32)),
}
# name: (a_bits, signed, folds the ReLU)
CONSUMERS = {"u8_folds": (8, False, True), "s8_no_fold": (8, True, False), "u6": (6, False, True)}


@pytest.mark.parametrize("consumer_name", sorted(CONSUMERS))
@pytest.mark.parametrize("layer_name", sorted(LAYERS))
def test_relu_codes_equals_its_two_pass_form(layer_name, consumer_name):
    cls, C, (IC, OC, K, groups), geometry = LAYERS[layer_name]
    a_bits, signed, folds = CONSUMERS[consumer_name]
    rng = np.random.RandomState(7)
    layer = cls.from_state_dict(synthetic.conv_entries(rng, IC, OC, K, 8, 8, True, 1.0, groups), **geometry).to(DEV)
    consumer = PackedConv2d.from_state_dict(synthetic.conv_entries(rng, OC, 8, 1, 8, a_bits, signed, 1.0)).to(DEV)
    assert (layer.IC, layer.OC) == (C, OC) and consumer.folds_relu == folds

    x = torch.from_numpy(rng.normal(0, 1, size=(N, C, H, W)).astype(np.float32)).to(DEV)
    layer.a_scale = (x.abs().max() / layer.a_qmax).reshape(1)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    codes, des = layer.quantize_codes(x, status)

    y = torch.relu(layer.call_packed(codes, des))                 # the fp32 output: the layer's own packed-in call
    assert y.shape == (N, OC, *layer.out_hw(H, W)) and y.max() > 0
    consumer.a_scale = torch.clamp(y.max() / consumer.a_qmax, min=1e-8).reshape(1)
    want = consumer.quantize_codes(y, status)[0]

    got_status = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = layer.relu_codes(codes, N, H, W, consumer, got_status)
    assert int(status.item()) == 0 and int(got_status.item()) == 0
    assert got.dtype == torch.uint8 and got.shape == want.shape
    assert torch.equal(got, want), (layer_name, consumer_name)
    assert len(torch.unique(got)) > 8                             # a real spread of codes, not a constant stream
