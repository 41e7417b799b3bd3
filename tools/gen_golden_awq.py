"""G15: two small linears through the reference's AWQ range estimator, on the CPU -> tests/golden/g15_awq_linear.npz.

The reference can calibrate and SIMULATE a group-quantised AWQ weight but cannot pack one (Quantizer.simulate / pack raise
NotImplementedError in packed mode).  For each layer (64 -> 48, q_group_size 32, 4 bits; one symmetric signed, one
asymmetric) this tool stores the weight, bias and a pre_act batch, the tuple AWQ.__call__ returns (scale, zero, qmin, qmax,
awq_scale), the codes of Quantizer.simulate's AWQ branch (x * awq_scale, reshape(-1, group),
round / clamp; then w_sim = ((q + zero) * scale reshaped back) / awq_scale) and F.linear(pre_act, w_sim, bias).  Arrays only.
Runs where the reference sources are, imports them through oracle.gen_golden.import_ref_modules and changes nothing under
oracle/.  usage: python tools/gen_golden_awq.py"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

K, O, G, BITS, ROWS = 64, 48, 32, 4, 8
LAYERS = {"sym": dict(symmetric=True, signed=True), "asym": dict(symmetric=False, signed=False)}


def main():
    from oracle.gen_golden import import_ref_modules
    import_ref_modules()
    from modelzoo.modules.range.awq import AWQ
    torch.manual_seed(15)
    out = {"config": np.array([K, O, G, BITS, ROWS], np.int32)}
    for name, kind in LAYERS.items():
        w = torch.randn(O, K) * 0.1 + (0.0 if kind["symmetric"] else 0.03)
        bias = torch.randn(O) * 0.05
        # positive-mean activations with channels of very different magnitude: what AWQ's search responds to
        pre_act = (torch.randn(ROWS, K) + 0.5) * torch.logspace(-1, 1, K)[torch.randperm(K)]
        est = AWQ(n_bits=BITS, granularity="channel", q_group_size=G, **kind)
        with torch.no_grad():
            scale, zero, qmin, qmax, awq_scale = est("weight", w, pre_act=pre_act, func=F.linear, kwarg={"bias": bias})
            x = (w * awq_scale).reshape(-1, G)
            q = (x / scale - zero).round().clamp(qmin, qmax)
            w_sim = ((q + zero).mul(scale)).reshape(w.shape) / awq_scale
            y = F.linear(pre_act, w_sim, bias)
        for k, v in (("weight", w), ("bias", bias), ("pre_act", pre_act), ("scale", scale), ("zero", zero),
                     ("awq_scale", awq_scale), ("out", y)):
            out["%s_%s" % (name, k)] = v.numpy().astype(np.float32)
        out["%s_codes" % name] = q.reshape(O, K).numpy().astype(np.int8)
        out["%s_qrange" % name] = np.array([qmin, qmax, int(kind["signed"])], np.int32)
    path = os.path.join(REPO, "tests", "golden", "g15_awq_linear.npz")
    np.savez_compressed(path, **out)
    print("G15: %d arrays, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
