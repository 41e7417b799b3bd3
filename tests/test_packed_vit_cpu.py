"""CPU: a packed ViT state_dict is read from torchvision's key layout (depth, width, MLP width and patch from the tensors),
a per-channel activation quantiser on a linear is rejected, and the C ABI exports the ViT entry points."""
import pytest
import torch

from quantize_amd import capi
from quantize_amd.packed_vit import CONFIGS, PackedViT, synthetic_state_dict

VIT_SYMBOLS = ["qe_quantize_pack_act", "qe_quantlinear_requant_path", "qe_quantlinear_requant_workspace_bytes",
               "qe_quantlinear_requant", "qe_quantlinear_residual_path", "qe_quantlinear_residual_workspace_bytes",
               "qe_quantlinear_residual", "qe_quantlinear_float_input_residual_path",
               "qe_quantlinear_float_input_residual_workspace_bytes", "qe_quantlinear_float_input_residual",
               "qe_layernorm_quantize_pack_path", "qe_layernorm_quantize_pack_workspace_bytes", "qe_layernorm_quantize_pack",
               "qe_quantize_patchify"]


def test_symbols_exported():
    L = capi.lib()
    for s in VIT_SYMBOLS:
        assert s in capi.SYMBOLS and hasattr(L, s), s


@pytest.mark.parametrize("arch", ["vit_tiny_test", "vit_b_16"])
def test_key_discovery(arch):
    cfg = CONFIGS[arch]
    sd = synthetic_state_dict(arch)
    m = PackedViT.from_state_dict(sd, cfg["heads"])
    assert (m.depth, m.E, m.mlp_dim, m.patch, m.C) == (cfg["depth"], cfg["width"], cfg["mlp"], cfg["patch"], 3)
    assert m.head_lin.O == cfg["num_classes"]
    assert [b.name for b in m.blocks] == ["encoder.layers.encoder_layer_%d" % i for i in range(cfg["depth"])]
    assert len(m.linears()) == 5 * cfg["depth"] + 1


def test_depth_from_tensors_and_missing_keys():
    sd = synthetic_state_dict("vit_tiny_test", depth=3, mlp=128, width=32)
    m = PackedViT.from_state_dict(sd, 2)
    assert (m.depth, m.E, m.mlp_dim) == (3, 32, 128)
    for k in ("encoder.layers.encoder_layer_1.mlp.3.w_des", "encoder.ln.weight", "heads.head.w_des", "class_token"):
        bad = dict(sd)
        del bad[k]
        with pytest.raises(KeyError, match="missing"):
            PackedViT.from_state_dict(bad, 2)
    bad = {k: v for k, v in sd.items() if not k.startswith("encoder.layers.encoder_layer_1.")}
    with pytest.raises(KeyError, match="encoder_layer"):
        PackedViT.from_state_dict(bad, 2)


@pytest.mark.parametrize("key", ["encoder.layers.encoder_layer_0.mlp.0.a_quantizer",
                                 "encoder.layers.encoder_layer_1.self_attention.k_quantizer",
                                 "heads.head.a_quantizer"])
def test_per_channel_linear_quantizer_rejected(key):
    sd = synthetic_state_dict("vit_tiny_test")
    sd[key + ".scale"] = torch.ones(64)
    sd[key + ".zero"] = torch.zeros(64)
    with pytest.raises(ValueError, match="per-channel activation quantiser"):
        PackedViT.from_state_dict(sd, 4)


def test_per_channel_image_quantizer_rejected():
    sd = synthetic_state_dict("vit_tiny_test")
    sd["conv_proj.a_quantizer.scale"] = torch.ones(3)
    sd["conv_proj.a_quantizer.zero"] = torch.zeros(3)
    with pytest.raises(ValueError, match="per-channel image quantiser"):
        PackedViT.from_state_dict(sd, 4)
