#!/usr/bin/env python3
"""Group-quantised (AWQ layout) 1x1 convolutions on 8-bit activation codes (qe_quantconv2d_awq, fast kernel) against what such a
layer had before, layer by layer: the distinct 1x1 / stride-1 layers of ResNet-50 and the 13 pointwise layers of MobileNetV1 at
batch 256, G = min(128, IC), on one MI355X in one process.  Cold caches: a 512 MiB buffer is rewritten before every timed call
(outside the device events); `--reps` repetitions per kernel with the kernels interleaved, median and range:
  awq_w4_sym / awq_w4_asym / awq_w8_sym / awq_w8_asym   qe_quantconv2d_awq (path 1); sym: both declarations given, asym: neither
  f32_conv2d      (a) torch's fp32 F.conv2d on the dequantised operands (the dequantisation is NOT timed: it flatters this route)
  per_channel_w8a8  (b) qe_quantconv2d_prepared, per-channel 8-bit weights on the same activation codes
Writes one JSON document (default profiles/conv_awq_layers.json).  Run each invocation under its own time limit.
usage: python tools/bench_conv_awq.py [--net resnet50|mobilenet_v1|all]"""
import argparse, json, os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch
import torch.nn.functional as F
from quantize_amd import capi
from quantize_amd.synthetic import pack_codes

# (IC, OC, H = W)
RESNET50 = [(64, 64, 56), (64, 256, 56), (256, 64, 56), (256, 128, 56), (128, 512, 28), (512, 128, 28), (512, 256, 28),
            (256, 1024, 14), (1024, 256, 14), (1024, 512, 14), (512, 2048, 7), (2048, 512, 7)]
MOBILENET = [(32, 64, 112), (64, 128, 56), (128, 128, 56), (128, 256, 28), (256, 256, 28), (256, 512, 14), (512, 512, 14),
             (512, 1024, 7), (1024, 1024, 7)]      # 13 layers, 9 distinct shapes (512 -> 512 @14 five times)
ap = argparse.ArgumentParser()
ap.add_argument("--net", default="all")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "conv_awq_layers.json"))
args = ap.parse_args()
dev = torch.device("cuda", 0)
rng = np.random.RandomState(16)
N = args.batch
up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)


def timed(fn):
    flush.fill_(1)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


nets = {"resnet50": RESNET50, "mobilenet_v1": MOBILENET}
result = {"batch": N, "reps": args.reps, "unit": "ms per call, cold caches", "layers": {}}
for net in (nets if args.net == "all" else [args.net]):
    for IC, OC, HW in nets[net]:
        G, P = min(128, IC), HW * HW
        NG = IC // G
        sh = capi.conv_shape(N, IC, HW, HW, OC, 1, 1, 1, 0)
        xc = rng.randint(0, 256, (N, IC, HW, HW), dtype=np.uint8)      # an 8-bit stream IS its stored bytes
        xs = up(xc.reshape(-1))
        sx, zx0, zxa = up(np.array([0.02], np.float32)), torch.zeros(1, device=dev), up(np.array([128.3], np.float32))
        x_sym, x_asym = capi.qparam(xs, 8, True, sx, zx0), capi.qparam(xs, 8, False, sx, zxa)
        xf = (xs.view(N, IC, HW, HW).float() - 128.0) * 0.02
        bias = up(rng.randn(OC).astype(np.float32))
        out = torch.empty((N, OC, HW, HW), dtype=torch.float32, device=dev)
        sg, zg0 = up(rng.uniform(1e-3, 2e-3, OC * NG).astype(np.float32)), torch.zeros(OC * NG, device=dev)
        w = {}
        for bits in (4, 8):
            h = 1 << (bits - 1)
            wc = rng.randint(0, 2 * h, (OC, IC))
            w[bits, "sym"] = capi.qparam(up(pack_codes(wc - h, bits, True)), bits, True, sg, zg0)
            w[bits, "asym"] = capi.qparam(up(pack_codes(wc, bits, False)), bits, False, sg,
                                          up((h + rng.uniform(-0.5, 0.5, OC * NG)).astype(np.float32)))
            assert capi.conv_awq_path(x_sym, w[bits, "sym"], G, sh, x_symmetric=True, w_symmetric=True) == 1
            assert capi.conv_awq_path(x_asym, w[bits, "asym"], G, sh) == 1
        wf = (up(wc - 128).float() * 1.5e-3).view(OC, IC, 1, 1)
        w8_ch = capi.qparam(w[8, "sym"]._keep[0], 8, True, up(rng.uniform(1e-3, 2e-3, OC).astype(np.float32)), torch.zeros(OC, device=dev))
        prepared = capi.conv_prepare(w8_ch, bias, sh, 8)
        ws = torch.empty(int(capi.lib().qe_quantconv2d_prepared_workspace_bytes(sh, 8, 8)), dtype=torch.uint8, device=dev)
        awq = lambda bits, kind, xq: lambda: capi.quantconv2d_awq(xq, w[bits, kind], G, bias, sh, out=out, x_symmetric=kind == "sym",
                                                                  w_symmetric=kind == "sym")
        kernels = {"awq_w4_sym": awq(4, "sym", x_sym), "awq_w4_asym": awq(4, "asym", x_asym), "awq_w8_sym": awq(8, "sym", x_sym),
                   "awq_w8_asym": awq(8, "asym", x_asym), "f32_conv2d": lambda: F.conv2d(xf, wf, bias),
                   "per_channel_w8a8": lambda: capi.quantconv2d_prepared(x_sym, w8_ch, bias, sh, prepared, out=out, workspace=ws)}
        times = {k: [] for k in kernels}
        for fn in kernels.values():      # untimed: code objects, library heuristics
            fn()
        for _ in range(args.reps):
            for k, fn in kernels.items():
                times[k].append(timed(fn))
        row = {k: {"ms": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in times.items()}
        spread = lambda k: max(times[k]) - min(times[k])
        for k in [k for k in kernels if k.startswith("awq_")]:
            row[k]["below_f32_by_more_than_the_spreads"] = bool(row["f32_conv2d"]["ms"] - row[k]["ms"] > max(spread(k), spread("f32_conv2d")))
            row[k]["over_per_channel_w8a8"] = round(row[k]["ms"] / row["per_channel_w8a8"]["ms"], 3)
            row[k]["TOPs"] = round(2.0 * N * P * IC * OC / row[k]["ms"] / 1e9, 1)
        # the NCHW store at 4 OC bytes per pixel, at the 5.1 TB/s a store-only kernel reaches here (profiles/r02c_probe_store_occ.txt)
        row["store_ms_at_5.1TBps"] = round(4.0 * N * P * OC / 5.1e9, 4)
        row["store_share_of_awq_w4_sym"] = round(row["store_ms_at_5.1TBps"] / row["awq_w4_sym"]["ms"], 3)
        result["layers"]["%s %d->%d @%dx%d" % (net, IC, OC, HW, HW)] = row
        print(net, IC, OC, HW, json.dumps(row), flush=True)
        del xs, xf, out, ws
        torch.cuda.empty_cache()
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print(json.dumps({"written": args.out}))
