#!/usr/bin/env python3
"""G11: the reference's depthwise QuantConv2d and a whole MobileNetV1 built from its modules, run through their packed
forwards -> tests/golden/g11_mobilenet.npz.

Made on the CPU the way tools/gen_golden_mha_masked.py makes G10 (oracle.gen_golden.import_ref_modules loads the
reference's module package at run time; nothing of it is stored here, data only):
  (a) four depthwise QuantConv2d modules (groups = channels, 3x3, padding 1), each calibrated, packed, its state_dict
      reloaded into a fresh module and called:  s1_signed (stride 1, signed symmetric activations), s2_unsigned (stride 2,
      unsigned asymmetric activations), s1_unsigned_pc (asymmetric per-channel weights), s2_bnfold (BatchNorm folded).
      Keys d_<name>_x, _y_packed, _geom [stride, padding], _sd_*.
  (b) one MobileNetV1 of width 8 (stem 3 -> 8, stages of 1, 2, 2, 6, 2 blocks up to 256 channels, 10 classes) on 32x32
      images: every conv + BatchNorm pair as QuantConv2d(bn_folding=...), the fc as QuantLinear, as G8 builds its ResNets.
      Keys m_w8_sd_*, m_w8_images, m_w8_pooled, m_w8_logits.
usage: python tools/gen_golden_mobilenet.py     (needs the reference checkout oracle/gen_golden.py points at)"""
import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "g11_mobilenet.npz")

W8 = dict(n_bits=8, symmetric=True, signed=True, granularity="channel", range={"name": "minmax"})
W8A = dict(n_bits=8, symmetric=False, signed=False, granularity="channel", range={"name": "minmax"})
A8S = dict(n_bits=8, symmetric=True, signed=True, granularity="layer", range={"name": "minmax"})
A8U = dict(n_bits=8, symmetric=True, signed=False, granularity="layer", range={"name": "minmax"})
A8UA = dict(n_bits=8, symmetric=False, signed=False, granularity="layer", range={"name": "minmax"})
DEPTH = (1, 2, 2, 6, 2)


def _bn_stats(bn):
    bn.weight.data.uniform_(0.5, 1.5)
    bn.bias.data.normal_(0, 0.1)
    bn.running_mean.normal_(0, 0.1)
    bn.running_var.uniform_(0.5, 1.5)


def _folding(bn):
    return {"running_mean": bn.running_mean.clone(), "running_var": bn.running_var.clone(), "weight": bn.weight.detach().clone(),
            "bias": bn.bias.detach().clone(), "eps": torch.tensor(bn.eps)}


def _quant(mm, model, on):
    for mod in model.modules():
        if isinstance(mod, mm.Quantizer):
            mod.quant(on)


def _calibrate_and_pack(mm, model, x):
    layers = [mod for mod in model.modules() if isinstance(mod, (mm.QuantConv2d, mm.QuantLinear))]
    for mod in layers:
        mod.calibrating = True
    model(x)
    for mod in layers:
        mod.calibrating = False
        mod.pack()
    return {k: v.clone() for k, v in model.state_dict().items()}


class Block(torch.nn.Module):
    """Depthwise 3x3 (groups = channels), BatchNorm, ReLU, pointwise 1x1, BatchNorm, ReLU."""

    def __init__(self, cin, cout, stride):
        super().__init__()
        nn = torch.nn
        self.conv1, self.bn1 = nn.Conv2d(cin, cin, 3, stride, 1, groups=cin, bias=False), nn.BatchNorm2d(cin)
        self.conv2, self.bn2 = nn.Conv2d(cin, cout, 1, 1, 0, bias=False), nn.BatchNorm2d(cout)

    def forward(self, x):
        return torch.relu(self.bn2(self.conv2(torch.relu(self.bn1(self.conv1(x))))))


class Net(torch.nn.Module):
    def __init__(self, width, num_classes):
        super().__init__()
        nn = torch.nn
        self.conv1, self.bn1 = nn.Conv2d(3, width, 3, 2, 1, bias=False), nn.BatchNorm2d(width)
        c = width
        for S, nb in enumerate(DEPTH, start=1):
            blocks = []
            for B in range(nb):
                blocks.append(Block(c, width << S, 2 if (B == 0 and S > 1) else 1))
                c = width << S
            setattr(self, "layer%d" % S, nn.Sequential(*blocks))
        self.fc = nn.Linear(c, num_classes)
        for m in self.modules():
            if isinstance(m, nn.BatchNorm2d):
                _bn_stats(m)

    def forward(self, x):
        x = torch.relu(self.bn1(self.conv1(x)))
        for S in range(1, len(DEPTH) + 1):
            x = getattr(self, "layer%d" % S)(x)
        self.pooled = torch.flatten(torch.nn.functional.adaptive_avg_pool2d(x, 1), 1)
        return self.fc(self.pooled)


def _fold(mm, parent, cname, bname, a_set):
    conv, bn = getattr(parent, cname), getattr(parent, bname)
    q = mm.QuantConv2d(conv.in_channels, conv.out_channels, conv.kernel_size, stride=conv.stride, padding=conv.padding,
                       groups=conv.groups, w_setting=dict(W8), a_setting=dict(a_set), bn_folding=_folding(bn),
                       _parameters={"weight": conv.weight.detach().clone(), "bias": None})
    setattr(parent, cname, q)
    setattr(parent, bname, torch.nn.Identity())


def _quantize_net(mm, model):
    _fold(mm, model, "conv1", "bn1", A8S)
    for S in range(1, len(DEPTH) + 1):
        for blk in getattr(model, "layer%d" % S):
            _fold(mm, blk, "conv1", "bn1", A8U)
            _fold(mm, blk, "conv2", "bn2", A8U)
    fc = model.fc
    model.fc = mm.QuantLinear(fc.in_features, fc.out_features, w_setting=dict(W8), a_setting=dict(A8U),
                              _parameters={"weight": fc.weight.detach().clone(), "bias": fc.bias.detach().clone()})
    return model


def main():
    from oracle import gen_golden
    mm = gen_golden.import_ref_modules()
    out, index = {}, []
    torch.manual_seed(31)
    # (a) depthwise modules: name, C, H, W, stride, weight / activation settings, BatchNorm folded
    for name, C, H, W, stride, w_set, a_set, fold in (("s1_signed", 8, 9, 11, 1, W8, A8S, False),
                                                      ("s2_unsigned", 8, 10, 7, 2, W8, A8UA, False),
                                                      ("s1_unsigned_pc", 6, 7, 7, 1, W8A, A8UA, False),
                                                      ("s2_bnfold", 8, 8, 8, 2, W8, A8S, True)):
        conv = torch.nn.Conv2d(C, C, 3, stride, 1, groups=C, bias=not fold)
        bn = torch.nn.BatchNorm2d(C)
        _bn_stats(bn)

        def make():
            kw = dict(bn_folding=_folding(bn)) if fold else {}
            params = {"weight": conv.weight.detach().clone(), "bias": None if fold else conv.bias.detach().clone()}
            return mm.QuantConv2d(C, C, 3, stride=stride, padding=1, groups=C, w_setting=dict(w_set), a_setting=dict(a_set),
                                  _parameters=params, **kw).eval()

        x = torch.randn(2, C, H, W)
        if not a_set["signed"]:
            x = torch.relu(x) + 0.37          # off zero: the asymmetric quantiser gets a zero point
        with torch.no_grad():
            sd = _calibrate_and_pack(mm, make(), x)
            m2 = make()
            m2.load_state_dict(sd)
            _quant(mm, m2, True)
            y = m2(x)
        assert torch.isfinite(y).all() and [int(v) for v in sd["w_des"][2:]] == [C, 1, 3, 3], name
        key = "d_" + name
        out[key + "_x"], out[key + "_y_packed"] = x.numpy(), y.numpy()
        out[key + "_geom"] = np.array([stride, 1], np.int32)
        for k, v in sd.items():
            out[key + "_sd_" + k] = v.numpy()
        index.append(key)
        print("G11 %s: w_des %s, %d stream bytes, max|y| %.3g" % (name, sd["w_des"].tolist(), sd["weight"].numel(), float(y.abs().max())))
    # (b) the whole model
    fmodel = Net(8, 10).eval()
    images = torch.randn(3, 3, 32, 32)
    with torch.no_grad():
        sd = _calibrate_and_pack(mm, _quantize_net(mm, copy.deepcopy(fmodel)).eval(), images)
        m2 = _quantize_net(mm, copy.deepcopy(fmodel)).eval()
        m2.load_state_dict(sd)
        _quant(mm, m2, True)
        logits = m2(images)
        pooled = m2.pooled
    assert torch.isfinite(logits).all()
    for k, v in sd.items():
        out["m_w8_sd_" + k] = v.numpy()
    out["m_w8_images"], out["m_w8_pooled"], out["m_w8_logits"] = images.numpy(), pooled.numpy(), logits.numpy()
    index.append("m_w8")
    print("G11 model: %d state_dict keys, logits std %.3g" % (len(sd), float(logits.std())))
    out["index"] = np.array(index)
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print("wrote", OUT, size, "bytes")
    assert size < 500 * 1024


if __name__ == "__main__":
    main()
