"""Time a packed ViT-B/16 forward (W8A8, 224 x 224) end to end on the engine, both routes of PackedViT in one process,
alternating, with device events, at each batch size; print one JSON line.

  route="layers"  the reference's dataflow with the engine plugged in (torch LayerNorm, per-linear quantise + pack, fp32
                  linear outputs, torch GELU and residual adds);
  route="fused"   LayerNorm + q / k / v codes in one pass, GELU + codes and the residual adds in the linears' epilogues,
                  the patch embedding as a GEMM on the matrix cores, no host synchronisation (check=False).

The HBM bytes reported are ALGORITHMIC (the byte model below, per token row outside the attention core and the GEMM
operands both routes share), not counters.  --attention torch engine engine_bf16 also times both routes with the engine's
fp32 and bf16 attention cores (keys fused_engine_ms, layers_engine_bf16_ms, ...); the default, torch, keeps the output as
it was.  --qkv fp32 bf16 adds, for the fused route with engine_bf16 only (the one combination that takes it), the forward with
the q / k / v projections stored as bf16 rows (key fused_engine_bf16_qkv_bf16_ms); it alternates with the others step by step.
--ctx fp32 bf16 adds, on top of --qkv bf16 (the one combination that takes it), the forward whose attention context is bf16
rows that out_proj reads in place (key fused_engine_bf16_qkv_bf16_ctx_bf16_ms), alternating in the same way.
usage: python tools/bench_vit_forward.py [--batches 64 256] [--steps 10] [--warmup 2] [--attention torch [engine] [engine_bf16]]
                                         [--qkv fp32 [bf16]] [--ctx fp32 [bf16]]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def byte_model(N, E=768, M=3072, depth=12, tokens=197):
    """(layers, fused) HBM bytes per forward between the GEMMs of the encoder blocks (fp32 = 4 B, codes = 1 B).
    layers, per block and row: LN1 (read 4E, write 4E), three quantize_pack passes (3 x (4E + E)), out_proj output + the
    add (4E write, 3 x 4E add), LN2 (8E), fc1's quantize_pack (5E), fc1 output 4M written, GELU (8M), fc2's quantize_pack
    (5M), fc2 output + the add (4E + 12E).  fused: LN1 + 3 codes (4E + 3E), out_proj's epilogue add (4E read + 4E write),
    LN2 + codes (4E + E), fc1's codes (M written), fc2's epilogue add (8E)."""
    rows = N * tokens
    lay = (8 * E + 15 * E + 16 * E + 8 * E + 5 * E + 4 * M + 8 * M + 5 * M + 16 * E) * rows * depth
    fus = (7 * E + 8 * E + 5 * E + M + 8 * E) * rows * depth
    return lay, fus


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--attention", nargs="+", choices=["torch", "engine", "engine_bf16"], default=["torch"])
    ap.add_argument("--qkv", nargs="+", choices=["fp32", "bf16"], default=["fp32"])
    ap.add_argument("--ctx", nargs="+", choices=["fp32", "bf16"], default=["fp32"])
    args = ap.parse_args()
    import torch
    from quantize_amd.packed_vit import CONFIGS, PackedViT, calibrated_state_dict

    dev = "cuda:0"
    sd = calibrated_state_dict("vit_b_16", device=dev, seed=0)
    model = PackedViT.from_state_dict(sd, CONFIGS["vit_b_16"]["heads"])
    res = {"metric": "vit_b_16_forward", "unit": "ms", "batches": {}}
    for N in args.batches:
        g = torch.Generator(device="cpu").manual_seed(N)
        x = torch.randn(N, 3, 224, 224, generator=g).to(dev)
        runs = [(route, att, qkv, ctx) for att in args.attention for route in ("fused", "layers")
                for qkv in args.qkv if qkv == "fp32" or (route, att) == ("fused", "engine_bf16")
                for ctx in args.ctx if ctx == "fp32" or (route, att, qkv) == ("fused", "engine_bf16", "bf16")]
        times = {r: [] for r in runs}
        with torch.no_grad():
            for i in range(args.warmup + args.steps):
                for route, att, qkv, ctx in runs:
                    kw = {} if qkv == "fp32" else {"qkv": qkv}
                    if ctx != "fp32":
                        kw["ctx"] = ctx
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    model(x, route, check=False, attention=att, **kw) if route == "fused" else model(x, route, attention=att)
                    b.record()
                    torch.cuda.synchronize()
                    if i >= args.warmup:
                        times[(route, att, qkv, ctx)].append(a.elapsed_time(b))
        lay, fus = byte_model(N)
        out = {}
        for (route, att, qkv, ctx), t in times.items():
            med = sorted(t)[len(t) // 2]
            sfx = ("" if att == "torch" else "_" + att) + ("" if qkv == "fp32" else "_qkv_" + qkv) + ("" if ctx == "fp32" else "_ctx_" + ctx)
            out["%s%s_ms" % (route, sfx)] = med
            out["%s%s_img_s" % (route, sfx)] = N / med * 1e3
        out.update({"byte_model_layers_GB": lay / 1e9, "byte_model_fused_GB": fus / 1e9})
        res["batches"][str(N)] = out
        del x
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
