"""Time a packed wrn_40_2 forward (batch 256, 32 x 32, W8A8, synthetic weights) end to end on the engine, both routes of
PackedWideResNet in one process, alternating, with device events; print one JSON line.

  route="layers"  the reference's dataflow with the engine plugged in (per-layer quantise + pack, fp32 conv outputs, torch add /
                  affine / ReLU);
  route="fused"   one qe_affine_relu_quantize_pack per block boundary, conv1 -> conv2 through the re-quantising epilogue, no host
                  synchronisation (check=False).
usage: python tools/bench_wrn_forward.py [--batch 256] [--steps 20] [--warmup 3] [--out profiles/wrn_forward.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from quantize_amd.packed_wideresnet import PackedWideResNet, calibrated_state_dict
    dev = "cuda:0"
    model = PackedWideResNet.from_state_dict(calibrated_state_dict(device=dev, depth=40, widen=2, seed=0))
    g = torch.Generator(device="cpu").manual_seed(1)
    x = torch.randn(args.batch, 3, 32, 32, generator=g).to(dev)
    routes = ["layers", "fused"]
    run = {"layers": lambda: model(x, route="layers"), "fused": lambda: model(x, route="fused", check=False)}
    for _ in range(args.warmup):
        for r in routes:
            run[r]()
    torch.cuda.synchronize()
    times = {r: [] for r in routes}
    outs = {}
    for _ in range(args.steps):
        for r in routes:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            outs[r] = run[r]()
            b.record()
            b.synchronize()
            times[r].append(a.elapsed_time(b))
    res = {"metric": "packed_wrn_40_2_forward", "batch": args.batch, "image": 32, "bits": "W8A8", "steps": args.steps,
           "warmup": args.warmup, "blocks": len(model.blocks()),
           "boundary_consumers": sorted({len(b.consumers()) for b in model.blocks()})}
    for r in routes:
        t = sorted(times[r])
        ms = t[len(t) // 2]
        res[r] = {"ms_per_step": round(ms, 4), "ms_min": round(t[0], 4), "images_per_s": round(args.batch / ms * 1e3, 1)}
    res["fused_over_layers"] = round(res["fused"]["ms_per_step"] / res["layers"]["ms_per_step"], 4)
    res["logits_equal"] = bool(torch.equal(outs["fused"], outs["layers"]))
    try:
        model(x, route="fused", check=True)           # reads the accumulated range flags once
        res["fused_status_ok"] = True
    except RuntimeError:
        res["fused_status_ok"] = False
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
