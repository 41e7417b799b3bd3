#!/usr/bin/env python3
"""The fused forms of the group-quantised (AWQ layout) linears on 8-bit activation codes against the two passes a caller ran
before them, at the shapes and by the protocol of tools/bench_linear_grouped_codes.py: the ViT-B/16 MLP at batch 256 (50,432
token rows), group size 128; one untimed call, then device events around `--calls` calls on operands resident in HBM, `--reps`
times per form with the forms interleaved, median and range.  Per operand setting (w4 / w8, sym: both declarations given, asym:
unsigned codes and fractional zeros of both operands):
  fc1_fused     qe_quantlinear_grouped_requant, 768 -> 3072, GELU, fc2's per-feature quantiser (path 1)
  fc1_two_pass  qe_quantlinear_grouped into fp32, then qe_quantize_pack_act
  fc2_fused     qe_quantlinear_grouped_residual, 3072 -> 768 on fc1's codes (path 1)
  fc2_two_pass  qe_quantlinear_grouped into fp32, then one elementwise add
  mlp_fused / mlp_two_pass   the two chained
Each fused result is compared with its two-pass result byte for byte at these sizes before anything is timed.
Writes one JSON document (default profiles/linear_grouped_fused.json).  usage: python tools/bench_linear_grouped_fused.py"""
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
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "linear_grouped_fused.json"))
args = ap.parse_args()
dev = torch.device("cuda", 0)
G, B, E, M = 128, args.rows, 768, 3072
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


def weights(O, K, bits, sym):
    h, NG = 1 << (bits - 1), K // G
    wc = rng.randint(0, 2 * h, (O, K))
    sg = up(rng.uniform(1e-3, 2e-3, O * NG).astype(np.float32) * (16.0 if bits == 4 else 1.0))
    if sym:
        return capi.qparam(up(pack_codes(wc - h, bits, True)), bits, True, sg, torch.zeros(O * NG, device=dev))
    return capi.qparam(up(pack_codes(wc, bits, False)), bits, False, sg, up((h + rng.uniform(-0.5, 0.5, O * NG)).astype(np.float32)))


result = {"rows": B, "group_size": G, "calls": args.calls, "reps": args.reps, "unit": "ms per call", "settings": {}}
up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
x_bytes = up(rng.randint(0, 256, B * E, dtype=np.uint8))     # an 8-bit stream IS its stored bytes: unsigned codes u, signed u - 128
sx1, sx2 = up(np.array([0.02], np.float32)), up(np.array([0.03], np.float32))
s2 = up(rng.uniform(0.02, 0.04, M).astype(np.float32))       # fc2's quantiser as fc1 applies it: one scale per hidden feature
b1, b2 = up(rng.randn(M).astype(np.float32) * 0.1), up(rng.randn(E).astype(np.float32) * 0.1)
res = up(rng.randn(B, E).astype(np.float32))
y1, y2 = torch.empty((B, M), dtype=torch.float32, device=dev), torch.empty((B, E), dtype=torch.float32, device=dev)
c2 = [torch.empty(B * M, dtype=torch.uint8, device=dev) for _ in range(2)]      # fused, two-pass
o2 = [torch.empty((B, E), dtype=torch.float32, device=dev) for _ in range(2)]
status = torch.zeros(1, dtype=torch.int32, device=dev)
for bits in (4, 8):
    for kind in ("sym", "asym"):
        sym = kind == "sym"
        zero = torch.zeros(1, device=dev) if sym else up(np.array([128.3], np.float32))     # kernel convention
        x1, w1, w2 = capi.qparam(x_bytes, 8, sym, sx1, zero), weights(M, E, bits, sym), weights(E, M, bits, sym)
        qmin, qmax = (-128.0, 127.0) if sym else (0.0, 255.0)
        z2 = -zero.repeat(M).contiguous()                                                  # module convention
        rq = capi.requant(s2, z2, qmin, qmax, 8, sym)
        x2 = [capi.qparam(c, 8, sym, sx2, zero) for c in c2]
        kw = dict(x_symmetric=sym, w_symmetric=sym)
        assert capi.linear_grouped_requant_path(x1, w1, G, B, E, M, rq, c2[0], **kw) == 1
        assert capi.linear_grouped_residual_path(x2[0], w2, G, B, M, E, **kw) == 1

        def fc1_fused():
            capi.quantlinear_grouped_requant(x1, w1, G, b1, B, E, M, rq, act="gelu", codes=c2[0], status=status, **kw)

        def fc1_two_pass():
            capi.quantlinear_grouped(x1, w1, G, b1, B, E, M, out=y1, **kw)
            capi.quantize_pack_act(y1, s2, z2, qmin, qmax, 8, sym, act="gelu", out=c2[1], status=status)

        def fc2_fused():
            capi.quantlinear_grouped_residual(x2[0], w2, G, b2, B, M, E, res, out=o2[0], **kw)

        def fc2_two_pass():
            capi.quantlinear_grouped(x2[1], w2, G, b2, B, M, E, out=y2, **kw)
            torch.add(y2, res, out=o2[1])

        forms = {"fc1_fused": fc1_fused, "fc1_two_pass": fc1_two_pass, "fc2_fused": fc2_fused, "fc2_two_pass": fc2_two_pass,
                 "mlp_fused": lambda: (fc1_fused(), fc2_fused()), "mlp_two_pass": lambda: (fc1_two_pass(), fc2_two_pass())}
        forms["mlp_fused"](), forms["mlp_two_pass"]()
        torch.cuda.synchronize()
        assert torch.equal(c2[0], c2[1]) and torch.equal(o2[0].view(torch.int32), o2[1].view(torch.int32)), "fused != two-pass"
        times = {k: [] for k in forms}
        for _ in range(args.reps):
            for k, fn in forms.items():
                times[k].append(timed(fn))
        row = {k: {"ms": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in times.items()}
        for part in ("fc1", "fc2", "mlp"):
            f, t = times[part + "_fused"], times[part + "_two_pass"]
            spread = max(max(f) - min(f), max(t) - min(t))
            row[part] = {"fused_over_two_pass": round(float(np.median(f) / np.median(t)), 3), "spread_ms": round(spread, 4),
                         "margin_ms": round(min(t) - max(f), 4), "below_by_more_than_spread": bool(min(t) - max(f) > spread)}
        result["settings"]["w%d_%s" % (bits, kind)] = row
        print(bits, kind, json.dumps(row), flush=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print(json.dumps({"written": args.out, "all_below": all(r[p]["below_by_more_than_spread"] for r in result["settings"].values()
                                                        for p in ("fc1", "fc2", "mlp"))}))
