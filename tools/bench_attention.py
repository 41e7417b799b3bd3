#!/usr/bin/env python3
"""The attention core alone: qe_attention (the fp32 engine kernel) and qe_attention_bf16 (its bf16 matrix-core form,
precision="bf16") against torch's F.scaled_dot_product_attention on the same (N L, E) fp32 projection buffers -- the engine
reads them in place, torch gets the (N, H, L, d) views the ViT's _attention passes it.  They alternate step by step, timed
with device events after a warm-up; medians are reported.  For orientation a fourth column times torch's own bf16 SDPA on
inputs cast to bf16 beforehand (`torch_bf16_precast`): it reads half the bytes the other three read and writes bf16; and next
to it `bf16_stored`, the engine's bf16 kernel on q / k / v cast to bf16 beforehand (qe_attention_bf16_stored: bf16 rows in,
fp32 out -- what the ViT runs with qkv="bf16"), and `bf16_ctx`, the same kernel with a bf16 context (qe_attention_bf16_ctx: bf16
rows in, bf16 rows out -- ctx="bf16").
Useful TFLOP/s counts 4 N H L S d (QK^T and PV, padding not counted); `of_peak` is the share of the 157.3 TFLOP/s fp32
matrix-pipe peak, given for the two fp32 columns only.  Prints one JSON line (`metric` keeps its name, attention_core_fp32:
the buffers are fp32 in every column but the pre-cast one).
--mask gives both the same mask: `causal` (the engine's flag, torch's is_causal), `causal-additive` (the -inf tril as an
(L, L) float mask), `additive2d` (a finite (L, L) float mask), `padding` (ragged key padding: the engine reads an (N, L) key
bias, torch the merged (N, 1, 1, L) mask it would build itself).  The FLOP count stays the unmasked one, so a causal row's
TFLOP/s is an equivalent rate, not work done.
usage: python tools/bench_attention.py [--steps 20] [--warmup 3] [--batches 64 256] [--mask none] [--shapes clip_text ...]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_TF = 157.3
SHAPES = {"vit_b_16": (197, 12, 64), "vit_l_16": (197, 16, 64), "vit_h_14": (257, 16, 80), "vit_b_32": (50, 12, 64),
          "clip_text": (77, 8, 64)}
MASKS = ["none", "causal", "causal-additive", "additive2d", "padding"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--mask", choices=MASKS, default="none")
    ap.add_argument("--shapes", nargs="+", choices=list(SHAPES), default=list(SHAPES))
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from quantize_amd import capi

    dev = "cuda:0"
    res = {"metric": "attention_core_fp32", "unit": "ms", "peak_tflops": PEAK_TF, "mask": args.mask, "path": {}, "bf16_path": {},
           "shapes": {}}
    for name in args.shapes:
        L, H, d = SHAPES[name]
        res["path"][name] = capi.attention_path(L, L, H, d)
        res["bf16_path"][name] = capi.attention_bf16_path(L, L, H, d)
        for N in args.batches:
            E = H * d
            g = torch.Generator(device="cpu").manual_seed(N + L)
            q, k, v = (torch.randn(N * L, E, generator=g).to(dev) for _ in range(3))
            out = torch.empty_like(q)
            views = [t.view(N, L, H, d).transpose(1, 2) for t in (q, k, v)]
            views16 = [t.to(torch.bfloat16) for t in views]             # cast once, outside the timed region
            ekw, tkw = {}, {}
            if args.mask == "causal":
                ekw, tkw = dict(causal=True), dict(is_causal=True)
            elif args.mask in ("causal-additive", "additive2d"):
                if args.mask == "additive2d":
                    m = (2.0 * torch.randn(L, L, generator=g)).to(dev)
                else:
                    m = torch.full((L, L), float("-inf")).triu_(1).to(dev)
                ekw, tkw = dict(mask=m), dict(attn_mask=m)
            elif args.mask == "padding":
                lengths = torch.randint(L // 2, L + 1, (N,), generator=g)
                kb = torch.zeros(N, L).masked_fill_(torch.arange(L)[None, :] >= lengths[:, None], float("-inf")).to(dev)
                ekw, tkw = dict(key_bias=kb), dict(attn_mask=kb.view(N, 1, 1, L))
            out16 = torch.empty_like(q)
            q16, k16, v16 = (t.to(torch.bfloat16) for t in (q, k, v))      # (N L, E) bf16 rows, cast outside the timed region
            out_st = torch.empty_like(q)
            out_ctx = torch.empty_like(q16)
            tkw16 = {n: (m.to(torch.bfloat16) if torch.is_tensor(m) else m) for n, m in tkw.items()}
            times = {"engine": [], "bf16": [], "bf16_stored": [], "bf16_ctx": [], "torch": [], "torch_bf16_precast": []}
            with torch.no_grad():
                for i in range(args.warmup + args.steps):
                    for who in times:
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record()
                        if who == "engine":
                            capi.attention(q, k, v, N, L, H, out=out, **ekw)
                        elif who == "bf16":
                            capi.attention(q, k, v, N, L, H, out=out16, precision="bf16", **ekw)
                        elif who == "bf16_stored":
                            capi.attention(q16, k16, v16, N, L, H, out=out_st, precision="bf16", **ekw)
                        elif who == "bf16_ctx":
                            capi.attention(q16, k16, v16, N, L, H, out=out_ctx, precision="bf16", out_dtype=torch.bfloat16, **ekw)
                        elif who == "torch_bf16_precast":
                            F.scaled_dot_product_attention(*views16, **tkw16)
                        else:
                            ref = F.scaled_dot_product_attention(*views, **tkw)
                        b.record()
                        torch.cuda.synchronize()
                        if i >= args.warmup:
                            times[who].append(a.elapsed_time(b))
                diff = float((out.view(N, L, H, d).transpose(1, 2) - ref).abs().max())
            flop = 4.0 * N * H * L * L * d
            row = {"N": N, "L": L, "H": H, "d": d, "max_abs_engine_minus_torch": diff,
                   "max_abs_bf16_minus_torch": float((out16.view(N, L, H, d).transpose(1, 2) - ref).abs().max()),
                   "max_abs_bf16_stored_minus_torch": float((out_st.view(N, L, H, d).transpose(1, 2) - ref).abs().max())}
            for who, t in times.items():
                ms = sorted(t)[len(t) // 2]
                row[who + "_ms"] = ms
                row[who + "_tflops"] = flop / (ms * 1e-3) / 1e12
                if who in ("engine", "torch"):              # the fp32 matrix-pipe peak is no yardstick for the bf16 columns
                    row[who + "_of_peak"] = row[who + "_tflops"] / PEAK_TF
            row["speedup"] = row["torch_ms"] / row["engine_ms"]
            row["bf16_speedup_over_engine"] = row["engine_ms"] / row["bf16_ms"]
            row["bf16_stored_speedup_over_bf16"] = row["bf16_ms"] / row["bf16_stored_ms"]
            row["bf16_ctx_speedup_over_bf16_stored"] = row["bf16_stored_ms"] / row["bf16_ctx_ms"]
            row["bf16_ctx_is_bf16_stored_rounded"] = bool(torch.equal(out_ctx.view(torch.int16), out_st.to(torch.bfloat16).view(torch.int16)))
            res["shapes"]["%s_N%d" % (name, N)] = row
            del q, k, v, out, out16, views, views16, ref, q16, k16, v16, out_st, out_ctx
            torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
