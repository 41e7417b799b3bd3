"""G16: two small convolutions through the reference's AWQ range estimator, on the CPU -> tests/golden/g16_awq_conv.npz.

Layer p: 1x1, IC 64, OC 48, q_group_size 32, 4 bits, symmetric signed.  Layer k: 3x3 / padding 1, IC 32, OC 16, q_group_size
32, 4 bits, asymmetric.  For each the file holds the weight and the pre_act batch (both on coarse grids, stored as int8 with
their step: the file must stay small), the bias, the estimator's tuple (scale, zero, qmin, qmax, awq_scale) and the simulated
quantised weight w_sim = ((q + zero) * scale reshaped back) / awq_scale.  Arrays only.

AWQ.__call__ itself raises on a 4-D weight with q_group_size > 0: it flattens the groups to two dimensions and then views
the scale as (-1, 1, 1, 1) against them.  So this tool drives the estimator's OWN update / range / quantize through the grid
search its docstring and QuantConv2d.calibrate describe, with the scale viewed (-1, 1): one scale and one zero per (output
channel, group of q_group_size consecutive input channels, all taps).  Runs where the reference sources are, imports them
through oracle.gen_golden.import_ref_modules and changes nothing under oracle/.  usage: python tools/gen_golden_awq_conv.py"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

BITS, G = 4, 32
LAYERS = {"p": dict(shape=(48, 64, 1, 1), x=(2, 64, 3, 3), pad=0, kind=dict(symmetric=True, signed=True)),
          "k": dict(shape=(16, 32, 3, 3), x=(2, 32, 4, 4), pad=1, kind=dict(symmetric=False, signed=False))}
W_STEP, X_STEP = 2.0 ** -6, 2.0 ** -3


def search(est, w, pre_act, func):
    """The estimator's grid search on a 4-D weight: its statistics, range and quantize; groups of G channels x all taps."""
    org = func(pre_act, w)
    x_mean = est.update(pre_act, est.accumulate)
    best, cfgs = float("inf"), None
    for i in range(est.grid):
        s = x_mean.pow(i / est.grid).clamp(min=1e-4).view(-1)
        s = (s / (s.max() * s.min()).sqrt()).view(1, -1, 1, 1)
        g = (w * s).reshape(-1, G, *w.shape[2:]).flatten(1)
        scale, zero, qmin, qmax = est.quantize(*est.range(g, "weight", accumulate=False))
        scale, zero = scale.view(-1, 1), zero.view(-1, 1)
        w_sim = ((g / scale - zero).round().clamp(qmin, qmax) + zero).mul(scale).view(w.shape) / s
        loss = (org - func(pre_act, w_sim)).float().pow(2).mean().item()
        if loss < best:
            best, cfgs = loss, (scale, zero, qmin, qmax, s, w_sim)
    return cfgs


def main():
    from oracle.gen_golden import import_ref_modules
    import_ref_modules()
    from modelzoo.modules.range.awq import AWQ
    torch.manual_seed(16)
    out = {"steps": np.array([W_STEP, X_STEP], np.float32)}
    for name, L in LAYERS.items():
        OC, IC = L["shape"][:2]
        w_i8 = torch.randint(-15, 16, L["shape"]) + (0 if L["kind"]["symmetric"] else 4)
        # positive-mean activations with channels of very different magnitude: what AWQ's search responds to
        x_i8 = ((torch.randn(L["x"]) + 0.5) * torch.logspace(0, 1.5, IC)[torch.randperm(IC)].view(1, -1, 1, 1)).round().clamp(-127, 127)
        w, pre_act, bias = w_i8.float() * W_STEP, x_i8 * X_STEP, torch.randn(OC) * 0.05
        est = AWQ(n_bits=BITS, granularity="channel", q_group_size=G, **L["kind"])
        with torch.no_grad():
            scale, zero, qmin, qmax, awq_scale, w_sim = search(est, w, pre_act, lambda x, wt: F.conv2d(x, wt, bias, padding=L["pad"]))
        for k, v in (("bias", bias), ("scale", scale), ("zero", zero), ("awq_scale", awq_scale), ("w_sim", w_sim)):
            out["%s_%s" % (name, k)] = v.numpy().astype(np.float32)
        out["%s_weight_i8" % name] = w_i8.numpy().astype(np.int8)
        out["%s_pre_act_i8" % name] = x_i8.numpy().astype(np.int8)
        out["%s_config" % name] = np.array([BITS, G, L["pad"], qmin, qmax, int(L["kind"]["signed"])], np.int32)
    path = os.path.join(REPO, "tests", "golden", "g16_awq_conv.npz")
    np.savez_compressed(path, **out)
    print("G16: %d arrays, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
