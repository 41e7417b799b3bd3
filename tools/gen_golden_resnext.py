#!/usr/bin/env python3
"""G12: the reference's grouped QuantConv2d and a whole small ResNeXt built from its modules, run through their packed
forwards -> tests/golden/g12_resnext.npz.

Made on the CPU the way tools/gen_golden_mobilenet.py makes G11 (oracle.gen_golden.import_ref_modules loads the reference's
module package at run time; nothing of it is stored here, data only):
  (a) four grouped QuantConv2d modules (3x3, padding 1, 2 or 4 groups), each calibrated, packed, its state_dict reloaded into
      a fresh module and called:  cg4_s1_signed (Cg 4, stride 1, signed symmetric activations), cg8_s2_unsigned (Cg 8, stride
      2, unsigned asymmetric activations), cg16_s1_pc (Cg 16, asymmetric per-channel weights), cg32_s2_bnfold (Cg 32, stride
      2, BatchNorm folded).  Keys g_<name>_x, _y_packed, _geom [stride, padding, in_channels], _sd_*.
  (b) one ResNeXt of Bottlenecks (1, 1, 1, 1) with 4 groups and grouped widths 16, 32, 64, 128 (Cg 4, 8, 16, 32; block outputs
      twice the width; stem 3 -> 16, 7x7 / 2, maxpool) on 32x32 images, 10 classes: every conv + BatchNorm pair as
      QuantConv2d(bn_folding=...), the fc as QuantLinear, as G8 builds its ResNets.
      Keys m_x4_sd_*, m_x4_images, m_x4_pooled, m_x4_logits.
It prints the distance of the reference's own fp32 logits from tests/resnext_exact.py's float64 model on the same state_dict:
the distance the engine is allowed in tests/test_packed_resnext_gpu.py.
usage: python tools/gen_golden_resnext.py     (needs the reference checkout oracle/gen_golden.py points at)"""
import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "g12_resnext.npz")

W8 = dict(n_bits=8, symmetric=True, signed=True, granularity="channel", range={"name": "minmax"})
W8A = dict(n_bits=8, symmetric=False, signed=False, granularity="channel", range={"name": "minmax"})
A8S = dict(n_bits=8, symmetric=True, signed=True, granularity="layer", range={"name": "minmax"})
A8U = dict(n_bits=8, symmetric=True, signed=False, granularity="layer", range={"name": "minmax"})
A8UA = dict(n_bits=8, symmetric=False, signed=False, granularity="layer", range={"name": "minmax"})
GROUPS, BASE = 4, 16


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
    """torchvision's Bottleneck with a grouped conv2 and an expansion of 2."""

    def __init__(self, cin, width, stride):
        super().__init__()
        nn = torch.nn
        self.conv1, self.bn1 = nn.Conv2d(cin, width, 1, bias=False), nn.BatchNorm2d(width)
        self.conv2, self.bn2 = nn.Conv2d(width, width, 3, stride, 1, groups=GROUPS, bias=False), nn.BatchNorm2d(width)
        self.conv3, self.bn3 = nn.Conv2d(width, 2 * width, 1, bias=False), nn.BatchNorm2d(2 * width)
        self.downsample = nn.Sequential(nn.Conv2d(cin, 2 * width, 1, stride, bias=False), nn.BatchNorm2d(2 * width))

    def forward(self, x):
        out = torch.relu(self.bn1(self.conv1(x)))
        out = torch.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        return torch.relu(out + self.downsample(x))


class Net(torch.nn.Module):
    def __init__(self, num_classes):
        super().__init__()
        nn = torch.nn
        self.conv1, self.bn1 = nn.Conv2d(3, BASE, 7, 2, 3, bias=False), nn.BatchNorm2d(BASE)
        c = BASE
        for S in range(1, 5):
            width = BASE << (S - 1)
            setattr(self, "layer%d" % S, nn.Sequential(Block(c, width, 1 if S == 1 else 2)))
            c = 2 * width
        self.fc = nn.Linear(c, num_classes)
        for m in self.modules():
            if isinstance(m, nn.BatchNorm2d):
                _bn_stats(m)

    def forward(self, x):
        x = torch.nn.functional.max_pool2d(torch.relu(self.bn1(self.conv1(x))), 3, 2, 1)
        for S in range(1, 5):
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
    for S in range(1, 5):
        for blk in getattr(model, "layer%d" % S):
            for i in (1, 2, 3):
                _fold(mm, blk, "conv%d" % i, "bn%d" % i, A8U)
            _fold(mm, blk.downsample, "0", "1", A8U)
    fc = model.fc
    model.fc = mm.QuantLinear(fc.in_features, fc.out_features, w_setting=dict(W8), a_setting=dict(A8U),
                              _parameters={"weight": fc.weight.detach().clone(), "bias": fc.bias.detach().clone()})
    return model


def main():
    from oracle import gen_golden
    import resnext_exact as xe
    mm = gen_golden.import_ref_modules()
    out, index = {}, []
    torch.manual_seed(37)
    # (a) grouped modules: name, C, groups, H, W, stride, weight / activation settings, BatchNorm folded
    for name, C, g, H, W, stride, w_set, a_set, fold in (("cg4_s1_signed", 16, 4, 9, 11, 1, W8, A8S, False),
                                                         ("cg8_s2_unsigned", 32, 4, 10, 7, 2, W8, A8UA, False),
                                                         ("cg16_s1_pc", 32, 2, 7, 7, 1, W8A, A8UA, False),
                                                         ("cg32_s2_bnfold", 64, 2, 8, 8, 2, W8, A8S, True)):
        conv = torch.nn.Conv2d(C, C, 3, stride, 1, groups=g, bias=not fold)
        bn = torch.nn.BatchNorm2d(C)
        _bn_stats(bn)

        def make():
            kw = dict(bn_folding=_folding(bn)) if fold else {}
            params = {"weight": conv.weight.detach().clone(), "bias": None if fold else conv.bias.detach().clone()}
            return mm.QuantConv2d(C, C, 3, stride=stride, padding=1, groups=g, w_setting=dict(w_set), a_setting=dict(a_set),
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
        assert torch.isfinite(y).all() and [int(v) for v in sd["w_des"][2:]] == [C, C // g, 3, 3], name
        key = "g_" + name
        out[key + "_x"], out[key + "_y_packed"] = x.numpy(), y.numpy()
        out[key + "_geom"] = np.array([stride, 1, C], np.int32)
        for k, v in sd.items():
            out[key + "_sd_" + k] = v.numpy()
        index.append(key)
        print("G12 %s: w_des %s, %d stream bytes, max|y| %.3g" % (name, sd["w_des"].tolist(), sd["weight"].numel(), float(y.abs().max())))
    # (b) the whole model
    fmodel = Net(10).eval()
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
        out["m_x4_sd_" + k] = v.numpy()
    out["m_x4_images"], out["m_x4_pooled"], out["m_x4_logits"] = images.numpy(), pooled.numpy(), logits.numpy()
    index.append("m_x4")
    f64 = xe.Float64ResNeXt(sd, exact=False)
    r = f64.forward(images)
    print("G12 model: %d state_dict keys, groups %d, logits std %.3g, max |logits| %.3g" % (
        len(sd), f64.groups, float(logits.std()), float(logits.abs().max())))
    print("G12 model: reference fp32 logits vs float64 model: max |diff| %.3e" % float((logits.double() - r.logits).abs().max()))
    out["index"] = np.array(index)
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print("wrote", OUT, size, "bytes")
    assert size < 500 * 1024


if __name__ == "__main__":
    main()
