#!/usr/bin/env python3
"""G14: the reference's BatchNorm2d -> ReLU -> Quantizer chain at a pre-activation block boundary, and a whole WideResNet built
from its modules, run through their packed forwards -> tests/golden/g14_wrn.npz.

Made on the CPU the way tools/gen_golden_mobilenet.py makes G11 (oracle.gen_golden.import_ref_modules loads the reference's
module package at run time; nothing of it is stored here, data only):
  (a) three stand-alone boundaries on stored fp32 x and identity: torch.add, an eval-mode nn.BatchNorm2d with randomised
      statistics and the default eps, ReLU, and the reference's Quantizer(s) in packed mode (integer-valued q out):
        b_u8   one per-tensor unsigned 8-bit consumer;
        b_pc   one per-channel asymmetric unsigned 8-bit consumer;
        b_two  two consumers, per-tensor unsigned 8-bit and asymmetric unsigned 4-bit.
      Keys b_<name>_x, _identity, _bn_{weight, bias, mean, var, eps}, _n_out, _q<i>_{q, scale, zero, qmin, qmax}.
      tests/preact_ref.py must reproduce every q with no element near a .5 tie: the tool draws again until that holds.
  (b) one WideResNet of depth 16, widen factor 1 (six blocks, 16 / 16 / 32 / 64 channels; block1.layer.0 equal-width,
      block2.layer.0 and block3.layer.0 with a convShortcut), 10 classes, on three 32x32 images, W8A8: the graph as the
      reference's reconstruct leaves it -- a BatchNorm folds only where it directly follows a conv in child order, which is bn2
      into the block's conv1; every block's bn1 and the final bn1 stay nn.BatchNorm2d.  Calibrated, packed, its state_dict
      reloaded.  Keys m_w8_sd_*, m_w8_images, m_w8_pooled, m_w8_logits.
usage: python tools/gen_golden_wrn.py     (needs the reference checkout oracle/gen_golden.py points at)"""
import copy
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "g14_wrn.npz")

W8 = dict(n_bits=8, symmetric=True, signed=True, granularity="channel", range={"name": "minmax"})
A8S = dict(n_bits=8, symmetric=True, signed=True, granularity="layer", range={"name": "minmax"})
A8U = dict(n_bits=8, symmetric=True, signed=False, granularity="layer", range={"name": "minmax"})
A8UAC = dict(n_bits=8, symmetric=False, signed=False, granularity="channel", range={"name": "minmax"})
A4UA = dict(n_bits=4, symmetric=False, signed=False, granularity="layer", range={"name": "minmax"})


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


# ---- (b): the float model, attribute names as the state_dict's key layout wants them ----------------------------------------------
class Block(torch.nn.Module):
    """Pre-activation basic block: bn1, ReLU, conv1 3x3 (stride), bn2, ReLU, conv2 3x3; a 1x1 convShortcut on the activated
    input where the width changes, else the identity on the block's input."""

    def __init__(self, cin, cout, stride):
        super().__init__()
        nn = torch.nn
        self.bn1 = nn.BatchNorm2d(cin)
        self.conv1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False)
        self.convShortcut = nn.Conv2d(cin, cout, 1, stride, 0, bias=False) if cin != cout else None

    def forward(self, x):
        a = torch.relu(self.bn1(x))
        out = self.conv2(torch.relu(self.bn2(self.conv1(a))))
        return torch.add(x if self.convShortcut is None else self.convShortcut(a), out)


class Stage(torch.nn.Module):
    def __init__(self, n, cin, cout, stride):
        super().__init__()
        self.layer = torch.nn.Sequential(*[Block(cin if i == 0 else cout, cout, stride if i == 0 else 1) for i in range(n)])

    def forward(self, x):
        return self.layer(x)


class Net(torch.nn.Module):
    def __init__(self, depth, widen, num_classes):
        super().__init__()
        nn = torch.nn
        n, ch = (depth - 4) // 6, [16, 16 * widen, 32 * widen, 64 * widen]
        self.conv1 = nn.Conv2d(3, ch[0], 3, 1, 1, bias=False)
        self.block1, self.block2, self.block3 = Stage(n, ch[0], ch[1], 1), Stage(n, ch[1], ch[2], 2), Stage(n, ch[2], ch[3], 2)
        self.bn1 = nn.BatchNorm2d(ch[3])
        self.fc = nn.Linear(ch[3], num_classes)
        for m in self.modules():
            if isinstance(m, nn.BatchNorm2d):
                _bn_stats(m)

    def forward(self, x):
        out = self.block3(self.block2(self.block1(self.conv1(x))))
        out = torch.relu(self.bn1(out))
        self.pooled = F.avg_pool2d(out, 8).view(-1, self.fc.in_features)
        return self.fc(self.pooled)


def _qconv(mm, conv, a_set, bn=None):
    kw = dict(bn_folding=_folding(bn)) if bn is not None else {}
    return mm.QuantConv2d(conv.in_channels, conv.out_channels, conv.kernel_size, stride=conv.stride, padding=conv.padding,
                          w_setting=dict(W8), a_setting=dict(a_set), _parameters={"weight": conv.weight.detach().clone(), "bias": None},
                          **kw)


def _quantize_net(mm, model):
    model.conv1 = _qconv(mm, model.conv1, A8S)
    for stage in (model.block1, model.block2, model.block3):
        for blk in stage.layer:
            blk.conv1 = _qconv(mm, blk.conv1, A8U, blk.bn2)            # bn2 directly follows conv1 in child order: folded
            blk.bn2 = torch.nn.Identity()
            blk.conv2 = _qconv(mm, blk.conv2, A8U)
            if blk.convShortcut is not None:
                blk.convShortcut = _qconv(mm, blk.convShortcut, A8U)
    fc = model.fc
    model.fc = mm.QuantLinear(fc.in_features, fc.out_features, w_setting=dict(W8), a_setting=dict(A8U),
                              _parameters={"weight": fc.weight.detach().clone(), "bias": fc.bias.detach().clone()})
    return model


# ---- (a) -----------------------------------------------------------------------------------------------------------------------
def _boundary(mm, name, C, H, W, settings, out):
    import preact_ref
    for attempt in range(64):
        bn = torch.nn.BatchNorm2d(C).eval()
        _bn_stats(bn)
        x, identity = torch.randn(2, C, H, W), torch.randn(2, C, H, W)
        with torch.no_grad():
            a = torch.relu(bn(torch.add(x, identity)))
            qs = []
            for a_set in settings:
                qz = mm.Quantizer(**dict(a_set), flag="activation", n_channels=C, dim=4)
                qz.calibrate(a)
                qz.quant(True)
                qz.pack(a)
                q, scale, zero = qz(a)
                qs.append((q.numpy(), scale.detach().reshape(-1).numpy(), zero.detach().reshape(-1).numpy(), float(qz.qmin), float(qz.qmax)))
        alpha, shift = preact_ref.bn_affine(bn.weight.detach().numpy(), bn.bias.detach().numpy(), bn.running_mean.numpy(),
                                            bn.running_var.numpy(), bn.eps)
        x3, i3 = x.numpy().reshape(2, C, H * W), identity.numpy().reshape(2, C, H * W)
        clean = True
        for q, scale, zero, qmin, qmax in qs:
            got = preact_ref.quantise(preact_ref.activated(x3, i3, alpha, shift)[1], scale, zero, qmin, qmax)
            clean = clean and np.array_equal(got, q.reshape(got.shape)) and not preact_ref.tie_excused(x3, i3, alpha, shift, scale, zero).any()
        if clean:
            break
        print("G14 %s: attempt %d has an element near a tie, drawing again" % (name, attempt))
    else:
        raise SystemExit("G14 %s: no clean draw" % name)
    key = "b_" + name
    out[key + "_x"], out[key + "_identity"] = x.numpy(), identity.numpy()
    out[key + "_bn_weight"], out[key + "_bn_bias"] = bn.weight.detach().numpy(), bn.bias.detach().numpy()
    out[key + "_bn_mean"], out[key + "_bn_var"], out[key + "_bn_eps"] = bn.running_mean.numpy(), bn.running_var.numpy(), np.float64(bn.eps)
    out[key + "_n_out"] = np.int32(len(qs))
    for i, (q, scale, zero, qmin, qmax) in enumerate(qs):
        for f, v in (("q", q), ("scale", scale), ("zero", zero), ("qmin", np.float32(qmin)), ("qmax", np.float32(qmax))):
            out["%s_q%d_%s" % (key, i, f)] = v
        print("G14 %s consumer %d: scale %s, zero %s, q in [%g, %g] of [%g, %g]" % (name, i, scale.shape, zero.reshape(-1)[:2], q.min(),
                                                                                   q.max(), qmin, qmax))
    return key


def main():
    from oracle import gen_golden
    mm = gen_golden.import_ref_modules()
    out, index = {}, []
    torch.manual_seed(53)
    index.append(_boundary(mm, "u8", 6, 8, 8, (A8U,), out))
    index.append(_boundary(mm, "pc", 5, 4, 4, (A8UAC,), out))
    index.append(_boundary(mm, "two", 3, 5, 7, (A8U, A4UA), out))
    # (b) the whole model
    fmodel = Net(16, 1, 10).eval()
    images = torch.randn(3, 3, 32, 32)
    with torch.no_grad():
        sd = _calibrate_and_pack(mm, _quantize_net(mm, copy.deepcopy(fmodel)).eval(), images)
        m2 = _quantize_net(mm, copy.deepcopy(fmodel)).eval()
        m2.load_state_dict(sd)
        _quant(mm, m2, True)
        logits = m2(images)
        pooled = m2.pooled
    assert torch.isfinite(logits).all()
    assert "block1.layer.0.convShortcut.w_des" not in sd and "block2.layer.0.convShortcut.w_des" in sd
    assert "block1.layer.0.bn1.running_var" in sd and "block1.layer.0.bn2.running_var" not in sd and "bn1.running_var" in sd
    for k, v in sd.items():
        out["m_w8_sd_" + k] = v.numpy()
    out["m_w8_images"], out["m_w8_pooled"], out["m_w8_logits"] = images.numpy(), pooled.numpy(), logits.numpy()
    index.append("m_w8")
    print("G14 model: %d state_dict keys, logits std %.3g" % (len(sd), float(logits.std())))
    out["index"] = np.array(index)
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print("wrote", OUT, size, "bytes")
    assert size < 500 * 1024


if __name__ == "__main__":
    main()
