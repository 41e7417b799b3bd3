"""Time a packed ResNet-50 forward (batch 256, 224 x 224, W8A8) end to end on the engine, both routes of PackedResNet in
one process, alternating, with device events; print one JSON line.

  route="layers"  the reference's dataflow with the engine plugged in (per-layer quantise + pack, fp32 conv outputs, torch
                  ReLU / + / maxpool);
  route="fused"   codes from epilogue to epilogue, the residual block end inside the conv kernel, the stem's maxpool on
                  codes, no host synchronisation (check=False).

The HBM bytes reported are ALGORITHMIC (the byte model below: every tensor the route materialises written once and read
once per consumer; weights excluded), not counters.  The tensors each route counts are listed in DESIGN.md section 4c-bis
(the fused route writes no fp32 at the three stage-boundary block ends).  usage: python tools/bench_resnet_forward.py [--batch 256] [--steps 20]
[--warmup 3]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BPS = 8.0e12


def byte_model(N, H=224):
    """(layers, fused) HBM bytes of one forward, weights excluded, from quantize_amd.resnet50's layer table."""
    from quantize_amd.resnet50 import conv_layers, out_size
    layers = conv_layers()
    el_in = lambda l: N * l.IC * l.H * l.H
    el_out = lambda l: N * l.OC * out_size(l) ** 2
    lay = fus = 0
    # image
    img = N * 3 * H * H
    lay += 4 * img + 1 * img                   # quantize_pack: fp32 in, codes out
    fus += 4 * img + 1 * img
    for l in layers:
        i, o = el_in(l), el_out(l)
        if l.name != "conv1":
            lay += 4 * i + i                   # quantize_pack of the fp32 input (the stem's image counted above)
        lay += i + 4 * o                       # conv: codes in, fp32 out
        if l.name == "conv1":
            lay += 8 * o                       # relu
            p = o // 4
            lay += 4 * o + 4 * p               # maxpool
            fus += i + o + o + o // 4          # conv -> codes, maxpool on codes
        elif l.name.endswith("conv3"):
            lay += 12 * o + 8 * o              # + identity (2 reads, 1 write), relu
            last = l.name.startswith("layer4.2")
            nxt_ds = l.name.split(".")[1] == "{}".format({1: 2, 2: 3, 3: 5}.get(int(l.name[5]), -1))
            fus += i + 4 * o                   # codes in, identity read
            fus += (4 * o if (last or not nxt_ds) else 0) + (0 if last else o)
        elif l.name.endswith("downsample"):
            fus += i + 4 * o                   # codes in, fp32 identity out
        else:
            lay += 8 * o                       # relu
            fus += i + o                       # codes in, codes out
    feat = N * 2048 * 49
    lay += 4 * feat
    fus += 4 * feat
    return lay, fus


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--route", default="both", choices=["both", "fused", "layers"], help="'fused' alone: for profiler runs")
    args = ap.parse_args()
    import torch
    from quantize_amd.packed_resnet import PackedResNet, calibrated_state_dict
    dev = "cuda:0"
    model = PackedResNet.from_state_dict(calibrated_state_dict("resnet50", device=dev, seed=0))
    g = torch.Generator(device="cpu").manual_seed(1)
    x = torch.randn(args.batch, 3, 224, 224, generator=g).to(dev)
    routes = ["layers", "fused"] if args.route == "both" else [args.route]
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
    lay_b, fus_b = byte_model(args.batch)
    res = {"metric": "packed_resnet50_forward", "batch": args.batch, "image": 224, "bits": "W8A8", "steps": args.steps,
           "warmup": args.warmup, "residual_paths": model.residual_paths(args.batch)}
    for r in routes:
        t = sorted(times[r])
        ms = t[len(t) // 2]
        by = lay_b if r == "layers" else fus_b
        res[r] = {"ms_per_step": round(ms, 4), "ms_min": round(t[0], 4), "images_per_s": round(args.batch / ms * 1e3, 1),
                  "hbm_bytes_model": by, "hbm_fraction_of_8TBps": round(by / (ms * 1e-3) / HBM_BPS, 4)}
    if args.route == "both":
        res["fused_over_layers"] = round(res["fused"]["ms_per_step"] / res["layers"]["ms_per_step"], 4)
        res["logits_equal"] = bool(torch.equal(outs["fused"], outs["layers"]))
        try:
            model(x, route="fused", check=True)   # reads the accumulated range flags once
            res["fused_status_ok"] = True
        except RuntimeError:
            res["fused_status_ok"] = False
    print(json.dumps(res))


if __name__ == "__main__":
    main()
