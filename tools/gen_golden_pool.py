#!/usr/bin/env python3
"""G13: the reference's QuantReLU, QuantMaxPool2d and QuantAdaptiveAvgPool2d run through their packed forwards ->
tests/golden/g13_pool.npz.

Made on the CPU the way tools/gen_golden_mobilenet.py makes G11 (oracle.gen_golden.import_ref_modules loads the reference's
module package at run time; nothing of it is stored here, data only).  Each layer -- relu, maxpool (3, 2, 1), maxpool (2),
adaptive average pool to (1, 1) and to (5, 7) -- under each of four activation settings (signed symmetric 8-bit, unsigned
asymmetric 8-bit, unsigned asymmetric 4-bit, unsigned asymmetric 8-bit per channel) is calibrated, packed, its state_dict
reloaded into a fresh module, switched to quantised mode (Quantizer.quant(True): without it the packed forward passes x
through) and called.  Inputs are (2, 6, 8, 9), and (2, 3, 7, 7) for the global pool; all finite.
Keys x_<signed|unsigned>_<shape> (the shared inputs), p_<layer>_<setting>_xkey (which input), _y_packed, _geom (the layer's
integers), _sd_*.
usage: python tools/gen_golden_pool.py     (needs the reference checkout oracle/gen_golden.py points at)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "g13_pool.npz")

SETTINGS = (
    ("s8", dict(n_bits=8, symmetric=True, signed=True, granularity="layer", range={"name": "minmax"})),
    ("u8a", dict(n_bits=8, symmetric=False, signed=False, granularity="layer", range={"name": "minmax"})),
    ("u4a", dict(n_bits=4, symmetric=False, signed=False, granularity="layer", range={"name": "minmax"})),
    ("u8ac", dict(n_bits=8, symmetric=False, signed=False, granularity="channel", range={"name": "minmax"})),
)
# layer, constructor arguments (also stored as _geom), input shape
LAYERS = (("relu", (), (2, 6, 8, 9)), ("maxpool321", (3, 2, 1), (2, 6, 8, 9)), ("maxpool2", (2, 2, 0), (2, 6, 8, 9)),
          ("avg11", (1, 1), (2, 3, 7, 7)), ("avg57", (5, 7), (2, 6, 8, 9)))


def _make(mm, layer, geom, a_set):
    if layer == "relu":
        return mm.QuantReLU(a_setting=dict(a_set)).eval()
    if layer.startswith("maxpool"):
        return mm.QuantMaxPool2d(geom[0], geom[1], geom[2], a_setting=dict(a_set)).eval()
    return mm.QuantAdaptiveAvgPool2d(tuple(geom), a_setting=dict(a_set)).eval()


def main():
    from oracle import gen_golden
    mm = gen_golden.import_ref_modules()
    out, index = {}, []
    torch.manual_seed(41)
    inputs = {}
    for shape in sorted({s for _, _, s in LAYERS}):
        base = torch.randn(*shape)
        tag = "x".join(map(str, shape))
        inputs["x_signed_" + tag] = base
        inputs["x_unsigned_" + tag] = base * 0.7 + 0.9     # mostly positive, some negative: the asymmetric quantiser gets a zero point
    for k, v in inputs.items():
        out[k] = v.numpy()
    for layer, geom, shape in LAYERS:
        for sname, a_set in SETTINGS:
            xkey = "x_%s_%s" % ("signed" if a_set["signed"] else "unsigned", "x".join(map(str, shape)))
            x = inputs[xkey]
            with torch.no_grad():
                m = _make(mm, layer, geom, a_set)
                m.calibrating = True
                m(x)
                m.calibrating = False
                m.pack()
                sd = {k: v.clone() for k, v in m.state_dict().items()}
                m2 = _make(mm, layer, geom, a_set)
                m2.load_state_dict(sd)
                m2.pack()
                m2.a_quantizer.quant(True)
                y = m2(x.clone())
            assert torch.isfinite(y).all() and not torch.equal(y, x), (layer, sname)
            key = "p_%s_%s" % (layer, sname)
            out[key + "_xkey"], out[key + "_y_packed"] = np.array(xkey), y.numpy()
            out[key + "_geom"] = np.array(geom, np.int32)
            for k, v in sd.items():
                out[key + "_sd_" + k] = v.numpy()
            index.append(key)
            print("G13 %s: scale %s, y %s, max|y| %.3g" % (key, tuple(sd["a_quantizer.scale"].shape), tuple(y.shape),
                                                         float(y.abs().max())))
    out["index"] = np.array(index)
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print("wrote", OUT, size, "bytes")
    assert size < 64 * 1024


if __name__ == "__main__":
    main()
