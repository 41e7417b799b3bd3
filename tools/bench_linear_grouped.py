#!/usr/bin/env python3
"""Group-quantised (AWQ layout) linears against the routes the engine had for fp32 rows before them: the ViT-B/16 linears at
batch 256 (50,432 token rows; 768->768, 768->2304, 768->3072, 3072->768), group size 128.  Timed as tools/bench_linear.py
times its per-shape table (one untimed call, then device events around `--calls` calls on operands resident in HBM), `--reps`
times per kernel with the kernels interleaved, so the run-to-run spread of each is in the result:
  grouped_w4_sym / grouped_w4_asym / grouped_w8   qe_quantlinear_grouped_float_input, fast kernel (path 1)
  per_row_w4_path0   qe_quantlinear_float_input with per-row 4-bit weights: the order-preserving fp32 kernel (path 0), the only
                     route 4-bit weights on fp32 rows had (qe_linear.hip, a translation unit this kernel's unit does not touch)
  per_row_w8_mfma    qe_quantlinear_float_input with per-row 8-bit weights: linear_f32_mfma_kernel (path 1)
  torch_fp32         F.linear on the dequantised fp32 weights
Writes one JSON document (default profiles/linear_grouped.json).  usage: python tools/bench_linear_grouped.py [--out FILE]"""
import argparse, json, os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch
import torch.nn.functional as F
from quantize_amd import capi
from quantize_amd.synthetic import pack_codes

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--rows", type=int, default=256 * 197)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "linear_grouped.json"))
args = ap.parse_args()
dev = torch.device("cuda", 0)
G, B = 128, args.rows
rng = np.random.RandomState(3)


def timed(fn):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / args.calls


result = {"rows": B, "group_size": G, "calls": args.calls, "reps": args.reps, "unit": "ms per call", "shapes": {}}
for K, O in ((768, 768), (768, 2304), (768, 3072), (3072, 768)):
    NG = K // G
    x = torch.from_numpy((rng.randn(B, K) + 0.5).astype(np.float32)).to(dev)
    xm = torch.from_numpy(rng.uniform(0.5, 2.0, K).astype(np.float32)).to(dev)
    bias = torch.from_numpy(rng.randn(O).astype(np.float32)).to(dev)
    out = torch.empty((B, O), dtype=torch.float32, device=dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    w4u, w4s = up(pack_codes(rng.randint(0, 16, (O, K)), 4, False)), up(pack_codes(rng.randint(-8, 8, (O, K)), 4, True))
    w8s = up(pack_codes(rng.randint(-128, 128, (O, K)), 8, True))
    sg, zg0 = up(rng.uniform(1e-3, 2e-3, O * NG).astype(np.float32)), torch.zeros(O * NG, device=dev)
    zga = up((8 + rng.uniform(-0.5, 0.5, O * NG)).astype(np.float32))
    sr, zr = up(rng.uniform(1e-3, 2e-3, O).astype(np.float32)), torch.zeros(O, device=dev)
    wf = torch.from_numpy(rng.randn(O, K).astype(np.float32) * 0.02).to(dev)
    q4s_g, q4a_g, q8s_g = capi.qparam(w4s, 4, True, sg, zg0), capi.qparam(w4u, 4, False, sg, zga), capi.qparam(w8s, 8, True, sg, zg0)
    q4_row, q8_row = capi.qparam(w4s, 4, True, sr, zr), capi.qparam(w8s, 8, True, sr, zr)
    assert capi.linear_grouped_float_input_path(x, q4s_g, G, B, K, O, x_mul=xm, symmetric=True) == 1
    assert capi.linear_grouped_float_input_path(x, q4a_g, G, B, K, O, x_mul=xm) == 1
    assert capi.linear_float_input_path(x, q4_row, B, K, O) == 0 and capi.linear_float_input_path(x, q8_row, B, K, O) == 1
    kernels = {
        "grouped_w4_sym": lambda: capi.quantlinear_grouped_float_input(x, q4s_g, G, bias, O, x_mul=xm, out=out, symmetric=True),
        "grouped_w4_asym": lambda: capi.quantlinear_grouped_float_input(x, q4a_g, G, bias, O, x_mul=xm, out=out),
        "grouped_w8": lambda: capi.quantlinear_grouped_float_input(x, q8s_g, G, bias, O, x_mul=xm, out=out, symmetric=True),
        "per_row_w4_path0": lambda: capi.quantlinear_float_input(x, q4_row, bias, O, out=out),
        "per_row_w8_mfma": lambda: capi.quantlinear_float_input(x, q8_row, bias, O, out=out),
        "torch_fp32": lambda: F.linear(x, wf, bias, ),
    }
    times = {k: [] for k in kernels}
    for _ in range(args.reps):
        for k, fn in kernels.items():
            times[k].append(timed(fn))
    row = {k: {"ms": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in times.items()}
    p0 = times["per_row_w4_path0"]
    row["path0_spread_ms"] = round(max(p0) - min(p0), 4)
    # the condition: every fast W4 timing is below every path-0 timing by more than the path-0 spread
    row["w4_margin_ms"] = round(min(p0) - max(times["grouped_w4_sym"] + times["grouped_w4_asym"]), 4)
    row["w4_faster_than_path0"] = bool(row["w4_margin_ms"] > row["path0_spread_ms"])
    row["w4_sym_over_w8_mfma"] = round(row["grouped_w4_sym"]["ms"] / row["per_row_w8_mfma"]["ms"], 3)
    row["TFLOPs_w4_sym"] = round(2.0 * B * K * O / row["grouped_w4_sym"]["ms"] / 1e9, 1)
    result["shapes"]["%dx%d->%d" % (B, K, O)] = row
    print(K, O, json.dumps(row), flush=True)
    del x, out
    torch.cuda.empty_cache()
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print(json.dumps({"written": args.out, "all_faster": all(r["w4_faster_than_path0"] for r in result["shapes"].values())}))
