"""G9: a tiny ViT from the reference's own quant modules, simulated on the CPU -> tests/golden/g9_vit_module.npz.

The reference can run its SIMULATED quantised ViT but cannot pack one: QuantMultiheadAttention.pack() reads the None
q_proj_weight whenever kdim == embed_dim.  This tool builds torchvision's ViT structure (torchvision is absent, so it is
restated: conv_proj, class token + position embedding, EncoderBlocks x + attn(ln_1(x)), y + mlp(ln_2(y)) with LayerNorm
eps 1e-6 and nn.GELU, final LayerNorm, head) from QuantConv2d, QuantMultiheadAttention(batch_first=True) and QuantLinear,
calibrates it, and stores
  * the calibrated, unpacked state_dict (sd_*),
  * the reference's own pack() output for conv_proj and every QuantLinear (ref_pack_<layer>_<key>),
  * the images, the simulated forward's per-block outputs and logits.
32 x 32 images, patch 8, width 64, 4 heads, MLP 256, depth 2, 10 classes.  Runs where the reference sources are, imports
them through oracle.gen_golden.import_ref_modules and changes nothing under oracle/.  usage: python tools/gen_golden_vit.py"""
import copy
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

IMG, P, E, HEADS, MLP, DEPTH, CLASSES, N = 32, 8, 64, 4, 256, 2, 10, 4
W_SET = dict(n_bits=8, symmetric=True, signed=True, granularity="channel", range={"name": "minmax"})
A_SET = dict(n_bits=8, symmetric=True, signed=True, granularity="layer", range={"name": "minmax"})


def build(mm):
    class Block(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.ln_1 = torch.nn.LayerNorm(E, eps=1e-6)
            ref = torch.nn.MultiheadAttention(E, HEADS, batch_first=True)
            self.self_attention = mm.QuantMultiheadAttention(
                E, HEADS, batch_first=True, w_setting=dict(W_SET), a_setting=dict(A_SET),
                _parameters={k: (v.detach().clone() if v is not None else None) for k, v in ref._parameters.items()},
                _modules={"out_proj": ref.out_proj})
            self.ln_2 = torch.nn.LayerNorm(E, eps=1e-6)
            fc1, fc2 = torch.nn.Linear(E, MLP), torch.nn.Linear(MLP, E)
            self.mlp = torch.nn.Sequential(
                mm.QuantLinear(E, MLP, w_setting=dict(W_SET), a_setting=dict(A_SET),
                               _parameters={"weight": fc1.weight.detach().clone(), "bias": fc1.bias.detach().clone()}),
                torch.nn.GELU(), torch.nn.Dropout(0.0),
                mm.QuantLinear(MLP, E, w_setting=dict(W_SET), a_setting=dict(A_SET),
                               _parameters={"weight": fc2.weight.detach().clone(), "bias": fc2.bias.detach().clone()}),
                torch.nn.Dropout(0.0))

        def forward(self, x):
            y = self.ln_1(x)
            y, _ = self.self_attention(y, y, y, need_weights=False)
            x = x + y
            return x + self.mlp(self.ln_2(x))

    class Encoder(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.pos_embedding = torch.nn.Parameter(torch.randn(1, (IMG // P) ** 2 + 1, E) * 0.02)
            self.layers = torch.nn.Sequential()
            for i in range(DEPTH):
                self.layers.add_module("encoder_layer_%d" % i, Block())
            self.ln = torch.nn.LayerNorm(E, eps=1e-6)

    class ViT(torch.nn.Module):
        def __init__(self):
            super().__init__()
            conv = torch.nn.Conv2d(3, E, P, stride=P)
            self.conv_proj = mm.QuantConv2d(3, E, P, stride=P, padding=0, w_setting=dict(W_SET), a_setting=dict(A_SET),
                                            _parameters={"weight": conv.weight.detach().clone(), "bias": conv.bias.detach().clone()})
            self.class_token = torch.nn.Parameter(torch.randn(1, 1, E) * 0.02)
            self.encoder = Encoder()
            head = torch.nn.Linear(E, CLASSES)
            self.heads = torch.nn.Sequential()
            self.heads.add_module("head", mm.QuantLinear(E, CLASSES, w_setting=dict(W_SET), a_setting=dict(A_SET),
                                                         _parameters={"weight": head.weight.detach().clone(),
                                                                      "bias": head.bias.detach().clone()}))

        def forward(self, x, blocks=None):
            n = x.shape[0]
            x = self.conv_proj(x).flatten(2).transpose(1, 2)
            x = torch.cat([self.class_token.expand(n, -1, -1), x], dim=1) + self.encoder.pos_embedding
            for layer in self.encoder.layers:
                x = layer(x)
                if blocks is not None:
                    blocks.append(x.clone())
            return self.heads(self.encoder.ln(x)[:, 0])

    return ViT()


def main():
    from oracle.gen_golden import import_ref_modules
    mm = import_ref_modules()
    torch.manual_seed(23)
    model = build(mm).eval()
    images = torch.randn(N, 3, IMG, IMG)
    with torch.no_grad():
        for mod in model.modules():
            if hasattr(mod, "calibrating"):
                mod.calibrating = True
        model(images)
        for mod in model.modules():
            if hasattr(mod, "calibrating"):
                mod.calibrating = False
            if isinstance(mod, mm.Quantizer):
                mod.quant(True)
        blocks = []
        logits = model(images, blocks)
    out = {}
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    for k, v in sd.items():
        out["sd_" + k] = v.numpy()
    packed_layers = ["conv_proj", "heads.head"] + ["encoder.layers.encoder_layer_%d.mlp.%d" % (i, j)
                                                    for i in range(DEPTH) for j in (0, 3)]
    for name in packed_layers:
        mod = copy.deepcopy(model.get_submodule(name))
        with torch.no_grad():
            mod.pack()
        for k, v in mod.state_dict().items():
            if k in ("weight", "w_des", "w_scale", "w_zero", "bias"):
                out["ref_pack_%s_%s" % (name, k)] = v.detach().numpy()
    out["images"] = images.numpy()
    out["logits"] = logits.numpy()
    for i, b in enumerate(blocks):
        out["block_%d" % i] = b.numpy()
    out["config"] = np.array([IMG, P, E, HEADS, MLP, DEPTH, CLASSES], np.int32)
    path = os.path.join(REPO, "tests", "golden", "g9_vit_module.npz")
    np.savez_compressed(path, **out)
    print("G9: %d arrays, %d bytes, logits std %.3g" % (len(out), os.path.getsize(path), float(logits.std())))


if __name__ == "__main__":
    main()
