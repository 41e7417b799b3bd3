#!/usr/bin/env python3
"""Group-quantised (AWQ layout) linears on 8-bit activation CODES (qe_quantlinear_grouped, the int8 matrix cores) against what a
caller who holds codes had before, at the shapes and by the protocol of tools/bench_linear_grouped.py: the ViT-B/16 linears at
batch 256 (50,432 token rows; 768->768, 768->2304, 768->3072, 3072->768), group size 128; one untimed call, then device events
around `--calls` calls on operands resident in HBM, `--reps` times per kernel with the kernels interleaved, median and range:
  codes_w4_sym / codes_w4_asym / codes_w8_sym / codes_w8_asym   qe_quantlinear_grouped, fast kernel (path 1); sym: both
                     declarations given, asym: neither (unsigned codes, fractional zeros of both operands)
  f32rows_w4_sym / f32rows_w4_asym   qe_quantlinear_grouped_float_input on the same weights with the activations dequantised
                     to fp32 rows beforehand (the dequantisation itself is NOT timed: the figure flatters this route)
  per_row_w8a8       qe_quantlinear, per-row 8-bit weights on the same activation codes (its int8 MFMA kernel)
Writes one JSON document (default profiles/linear_grouped_codes.json).  usage: python tools/bench_linear_grouped_codes.py"""
import argparse, json, os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch
from quantize_amd import capi
from quantize_amd.synthetic import pack_codes

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--rows", type=int, default=256 * 197)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "linear_grouped_codes.json"))
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
up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
for K, O in ((768, 768), (768, 2304), (768, 3072), (3072, 768)):
    NG = K // G
    xc = rng.randint(0, 256, (B, K), dtype=np.uint8)      # an 8-bit stream IS its stored bytes: u as unsigned codes, u - 128 as signed
    xu = xs = up(xc.reshape(-1))
    sx, zx0, zxa = up(np.array([0.02], np.float32)), torch.zeros(1, device=dev), up(np.array([128.3], np.float32))
    x_sym, x_asym = capi.qparam(xs, 8, True, sx, zx0), capi.qparam(xu, 8, False, sx, zxa)
    xf_sym = up(((xc.astype(np.float32) - 128) * np.float32(0.02)))
    xf_asym = up(((xc.astype(np.float32) - np.float32(128.3)) * np.float32(0.02)))
    bias = up(rng.randn(O).astype(np.float32))
    out = torch.empty((B, O), dtype=torch.float32, device=dev)
    sg, zg0 = up(rng.uniform(1e-3, 2e-3, O * NG).astype(np.float32)), torch.zeros(O * NG, device=dev)
    w = {}
    for bits in (4, 8):
        h = 1 << (bits - 1)
        wc = rng.randint(0, 2 * h, (O, K))
        w[bits, "sym"] = capi.qparam(up(pack_codes(wc - h, bits, True)), bits, True, sg, zg0)
        w[bits, "asym"] = capi.qparam(up(pack_codes(wc, bits, False)), bits, False, sg, up((h + rng.uniform(-0.5, 0.5, O * NG)).astype(np.float32)))
    sr, zr = up(rng.uniform(1e-3, 2e-3, O).astype(np.float32)), torch.zeros(O, device=dev)
    w8_row = capi.qparam(w[8, "sym"]._keep[0], 8, True, sr, zr)
    for bits in (4, 8):
        assert capi.linear_grouped_path(x_sym, w[bits, "sym"], G, B, K, O, x_symmetric=True, w_symmetric=True) == 1
        assert capi.linear_grouped_path(x_asym, w[bits, "asym"], G, B, K, O) == 1
    assert capi.linear_grouped_float_input_path(xf_sym, w[4, "sym"], G, B, K, O, symmetric=True) == 1
    assert capi.linear_path(x_sym, w8_row, B, K, O) == 1
    codes = lambda bits, kind, xq: lambda: capi.quantlinear_grouped(xq, w[bits, kind], G, bias, B, K, O, out=out, x_symmetric=kind == "sym",
                                                                    w_symmetric=kind == "sym")
    kernels = {
        "codes_w4_sym": codes(4, "sym", x_sym), "codes_w4_asym": codes(4, "asym", x_asym),
        "codes_w8_sym": codes(8, "sym", x_sym), "codes_w8_asym": codes(8, "asym", x_asym),
        "f32rows_w4_sym": lambda: capi.quantlinear_grouped_float_input(xf_sym, w[4, "sym"], G, bias, O, out=out, symmetric=True),
        "f32rows_w4_asym": lambda: capi.quantlinear_grouped_float_input(xf_asym, w[4, "asym"], G, bias, O, out=out),
        "per_row_w8a8": lambda: capi.quantlinear(x_sym, w8_row, bias, B, K, O, out=out),
    }
    times = {k: [] for k in kernels}
    for _ in range(args.reps):
        for k, fn in kernels.items():
            times[k].append(timed(fn))
    row = {k: {"ms": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in times.items()}
    f32 = times["f32rows_w4_sym"] + times["f32rows_w4_asym"]
    new = [t for k, v in times.items() if k.startswith("codes_") for t in v]
    row["f32rows_spread_ms"] = round(max(max(times[k]) - min(times[k]) for k in ("f32rows_w4_sym", "f32rows_w4_asym")), 4)
    # the expectation: every timing of the new kernel is below every fp32-rows timing by more than the fp32-rows spread
    row["margin_ms"] = round(min(f32) - max(new), 4)
    row["faster_than_f32rows"] = bool(row["margin_ms"] > row["f32rows_spread_ms"])
    for k in ("codes_w4_sym", "codes_w4_asym", "codes_w8_sym", "codes_w8_asym"):
        row[k + "_over_per_row_w8a8"] = round(row[k]["ms"] / row["per_row_w8a8"]["ms"], 3)
    row["f32rows_w4_sym_over_codes_w4_sym"] = round(row["f32rows_w4_sym"]["ms"] / row["codes_w4_sym"]["ms"], 3)
    row["TOPs_codes_w4_sym"] = round(2.0 * B * K * O / row["codes_w4_sym"]["ms"] / 1e9, 1)
    result["shapes"]["%dx%d->%d" % (B, K, O)] = row
    print(K, O, json.dumps(row), flush=True)
    del xu, xs, xf_sym, xf_asym, out
    torch.cuda.empty_cache()
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print(json.dumps({"written": args.out, "all_faster": all(r["faster_than_f32rows"] for r in result["shapes"].values())}))
