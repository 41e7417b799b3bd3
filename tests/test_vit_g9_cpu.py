"""CPU: pack_vit_state_dict turns the calibrated state_dict of the reference's own (simulated) tiny ViT -- G9,
tools/gen_golden_vit.py -- into the packed layout: bit for bit what the reference's pack() writes for conv_proj and every
QuantLinear, every key consumed, the q / k / v projections packed per chunk of in_proj_weight (the step the reference's
QuantMultiheadAttention.pack() cannot take), and PackedViT reads the result."""
import os

import numpy as np
import pytest
import torch

from quantize_amd.packed_vit import PackedViT, pack_vit_state_dict

G9 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g9_vit_module.npz")


@pytest.fixture(scope="module")
def g9():
    z = np.load(G9, allow_pickle=False)
    return z, {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd_")}


def test_equals_reference_pack(g9):
    z, sd = g9
    packed = pack_vit_state_dict(sd)
    n = 0
    for k in z.files:
        if not k.startswith("ref_pack_"):
            continue
        for f in ("w_des", "w_scale", "w_zero", "weight", "bias"):
            if k.endswith("_" + f):
                layer = k[len("ref_pack_"):-len(f) - 1]
                got = packed[layer + "." + f].numpy()
                want = z[k]
                assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), k
                n += 1
                break
    assert n == 5 * 6          # conv_proj, the head and the 4 MLP linears: weight, des, scale, zero, bias each


def test_every_key_consumed_and_attention_per_chunk(g9):
    z, sd = g9
    packed = pack_vit_state_dict(sd)
    pre = "encoder.layers.encoder_layer_0.self_attention."
    w = sd[pre + "in_proj_weight"]
    for i, n in enumerate("qkv"):
        s, zz = sd[pre + n + "_proj_quantizer.scale"], sd[pre + n + "_proj_quantizer.zero"]
        q = (w[64 * i:64 * (i + 1)] / s - zz).round().clamp(-128, 127).to(torch.int64) + 128
        assert torch.equal(packed[pre + n + "_proj_weight"], q.to(torch.uint8).reshape(-1))
        assert packed[pre + n + "_proj_des"].tolist() == [8, 1, 64, 64]
    with pytest.raises(ValueError, match="no known ViT layer"):
        pack_vit_state_dict(dict(sd, **{"encoder.extra.weight": torch.zeros(3)}))
    m = PackedViT.from_state_dict(packed, 4)
    assert (m.depth, m.E, m.mlp_dim, m.patch) == tuple(int(v) for v in z["config"][[5, 2, 4, 1]])
