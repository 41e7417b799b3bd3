#!/usr/bin/env python3
"""The fp32 attention core alone: qe_attention (the engine) against torch's F.scaled_dot_product_attention on the same
(N L, E) projection buffers -- the engine reads them in place, torch gets the (N, H, L, d) views the ViT's _attention
passes it.  The two alternate step by step, timed with device events after a warm-up; medians are reported.
Useful TFLOP/s counts 4 N H L S d (QK^T and PV, padding not counted); `of_peak` is the share of the 157.3 TFLOP/s fp32
matrix-pipe peak.  Prints one JSON line.
usage: python tools/bench_attention.py [--steps 20] [--warmup 3] [--batches 64 256]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_TF = 157.3
SHAPES = {"vit_b_16": (197, 12, 64), "vit_l_16": (197, 16, 64), "vit_h_14": (257, 16, 80), "vit_b_32": (50, 12, 64)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 256])
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from quantize_amd import capi

    dev = "cuda:0"
    res = {"metric": "attention_core_fp32", "unit": "ms", "peak_tflops": PEAK_TF, "path": {}, "shapes": {}}
    for name, (L, H, d) in SHAPES.items():
        res["path"][name] = capi.attention_path(L, L, H, d)
        for N in args.batches:
            E = H * d
            g = torch.Generator(device="cpu").manual_seed(N + L)
            q, k, v = (torch.randn(N * L, E, generator=g).to(dev) for _ in range(3))
            out = torch.empty_like(q)
            views = [t.view(N, L, H, d).transpose(1, 2) for t in (q, k, v)]
            times = {"engine": [], "torch": []}
            with torch.no_grad():
                for i in range(args.warmup + args.steps):
                    for who in ("engine", "torch"):
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record()
                        if who == "engine":
                            capi.attention(q, k, v, N, L, H, out=out)
                        else:
                            ref = F.scaled_dot_product_attention(*views)
                        b.record()
                        torch.cuda.synchronize()
                        if i >= args.warmup:
                            times[who].append(a.elapsed_time(b))
                diff = float((out.view(N, L, H, d).transpose(1, 2) - ref).abs().max())
            flop = 4.0 * N * H * L * L * d
            row = {"N": N, "L": L, "H": H, "d": d, "max_abs_engine_minus_torch": diff}
            for who, t in times.items():
                ms = sorted(t)[len(t) // 2]
                row[who + "_ms"] = ms
                row[who + "_tflops"] = flop / (ms * 1e-3) / 1e12
                row[who + "_of_peak"] = row[who + "_tflops"] / PEAK_TF
            row["speedup"] = row["torch_ms"] / row["engine_ms"]
            res["shapes"]["%s_N%d" % (name, N)] = row
            del q, k, v, out, views, ref
            torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
