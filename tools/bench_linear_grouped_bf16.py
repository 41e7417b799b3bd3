#!/usr/bin/env python3
"""Group-quantised (AWQ layout) linears on bf16 rows against what the engine offered the same bf16 tensor before them: the
ViT-B/16 linears at batch 256 (50,432 token rows; 768->768, 768->2304, 768->3072, 3072->768), group size 128.  Timed as
tools/bench_linear_grouped.py times its table (one untimed call, then device events around `--calls` calls on operands
resident in HBM), `--reps` times per entry with the entries alternated, so the run-to-run spread of each is in the result.
Per weight form (w4 / w8 x sym: zeros 0, no x_mul | asym: fractional zeros and an x_mul):
  bf16_<form>          qe_quantlinear_grouped_bf16_input, fast kernel (path 1), the rows read as stored
  widen_f32_<form>     x.float() followed by qe_quantlinear_grouped_float_input (path 1) on the copy, timed together
and, for scale, per_row_w8_bf16: qe_quantlinear_bf16_input with per-row 8-bit weights on the same rows (path 1).
The criterion per shape and form: the new kernel's median lies below the composition's by more than the sum of the two
spreads (max - min over the reps).  Writes one JSON document (default profiles/linear_grouped_bf16.json).
usage: python tools/bench_linear_grouped_bf16.py [--out FILE]"""
import argparse, json, os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch
from quantize_amd import capi
from quantize_amd.synthetic import pack_codes

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--rows", type=int, default=256 * 197)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "linear_grouped_bf16.json"))
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
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    x = up((rng.randn(B, K) + 0.5).astype(np.float32)).to(torch.bfloat16)
    xm, bias = up(rng.uniform(0.5, 2.0, K).astype(np.float32)), up(rng.randn(O).astype(np.float32))
    out = torch.empty((B, O), dtype=torch.float32, device=dev)
    sg, sr, zr = up(rng.uniform(1e-3, 2e-3, O * NG).astype(np.float32)), up(rng.uniform(1e-3, 2e-3, O).astype(np.float32)), torch.zeros(O, device=dev)
    forms = {}                                                 # name -> (operand, x_mul, symmetric)
    for bits in (4, 8):
        signed, unsigned = up(pack_codes(rng.randint(-(1 << (bits - 1)), 1 << (bits - 1), (O, K)), bits, True)), \
            up(pack_codes(rng.randint(0, 1 << bits, (O, K)), bits, False))
        za = up(((1 << (bits - 1)) + rng.uniform(-0.5, 0.5, O * NG)).astype(np.float32))
        forms["w%d_sym" % bits] = (capi.qparam(signed, bits, True, sg, torch.zeros(O * NG, device=dev)), None, True)
        forms["w%d_asym" % bits] = (capi.qparam(unsigned, bits, False, sg, za), xm, False)
    q8_row = capi.qparam(forms["w8_sym"][0]._keep[0], 8, True, sr, zr)     # the same signed 8-bit stream, one scale per row
    entries = {}
    for name, (wq, m, sym) in forms.items():
        assert capi.linear_grouped_bf16_input_path(x, wq, G, B, K, O, x_mul=m, symmetric=sym) == 1
        assert capi.linear_grouped_float_input_path(256, wq, G, B, K, O, x_mul=m, symmetric=sym) == 1
        entries["bf16_" + name] = lambda wq=wq, m=m, sym=sym: capi.quantlinear_grouped_bf16_input(x, wq, G, bias, O, x_mul=m, symmetric=sym, out=out)
        entries["widen_f32_" + name] = lambda wq=wq, m=m, sym=sym: capi.quantlinear_grouped_float_input(x.float(), wq, G, bias, O, x_mul=m, out=out, symmetric=sym)
    assert capi.quantlinear_bf16_input_path(x, q8_row, B, K, O) == 1
    entries["per_row_w8_bf16"] = lambda: capi.quantlinear_bf16_input(x, q8_row, bias, O, out=out)
    times = {k: [] for k in entries}
    for _ in range(args.reps):
        for k, fn in entries.items():
            times[k].append(timed(fn))
    row = {k: {"ms": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4), "spread": round(max(v) - min(v), 4)}
           for k, v in times.items()}
    for name in forms:
        new, old = row["bf16_" + name], row["widen_f32_" + name]
        row[name + "_speedup"] = round(old["ms"] / new["ms"], 3)
        row[name + "_meets_criterion"] = bool(old["ms"] - new["ms"] > old["spread"] + new["spread"])
    row["TFLOPs_bf16_w4_sym"] = round(2.0 * B * K * O / row["bf16_w4_sym"]["ms"] / 1e9, 1)
    result["shapes"]["%dx%d->%d" % (B, K, O)] = row
    print(K, O, json.dumps(row), flush=True)
    del x, out
    torch.cuda.empty_cache()
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print(json.dumps({"written": args.out, "all_meet_criterion": all(v for r in result["shapes"].values() for k, v in r.items() if k.endswith("_meets_criterion"))}))
