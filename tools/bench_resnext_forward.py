"""Whole-model time of a packed ResNeXt-50 32x4d (synthetic weights, calibrated) on both routes of PackedResNet: warm,
back-to-back forwards timed with device events, median of --reps.  The fused route runs with check=False (no host read).
usage: python tools/bench_resnext_forward.py [--batch 256] [--reps 10] [--groups 32] [--width-per-group 4] [--size 224]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--groups", type=int, default=32)
    ap.add_argument("--width-per-group", type=int, default=4)
    ap.add_argument("--size", type=int, default=224)
    args = ap.parse_args()
    import torch
    from forward_routes import time_routes
    from quantize_amd.packed_resnet import PackedResNet, calibrated_state_dict
    dev = "cuda:0"
    sd = calibrated_state_dict("resnet50", device=dev, image_size=args.size, calib_batch=4, groups=args.groups,
                               width_per_group=args.width_per_group)
    model = PackedResNet.from_state_dict(sd)
    assert model.groups == args.groups
    g = torch.Generator(device="cpu").manual_seed(3)
    x = torch.randn(args.batch, 3, args.size, args.size, generator=g).to(dev)
    print(json.dumps({"metric": "resnext50_forward", "batch": args.batch, "groups": args.groups,
                      "width_per_group": args.width_per_group, "size": args.size, "reps": args.reps,
                      **time_routes(model, x, args.reps)}))


if __name__ == "__main__":
    main()
