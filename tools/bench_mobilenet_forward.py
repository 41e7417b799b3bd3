"""Whole-model time of a packed MobileNetV1 (synthetic weights, calibrated) on both routes of PackedMobileNetV1: warm,
back-to-back forwards timed with device events, median of --reps.  The fused route runs with check=False (no host read).
usage: python tools/bench_mobilenet_forward.py [--batch 256] [--reps 10] [--width 32] [--size 224]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--width", type=int, default=32)
    ap.add_argument("--size", type=int, default=224)
    args = ap.parse_args()
    import torch
    from forward_routes import time_routes
    from quantize_amd.packed_mobilenet import PackedMobileNetV1, calibrated_state_dict
    dev = "cuda:0"
    sd = calibrated_state_dict(device=dev, width=args.width, image_size=args.size, calib_batch=8)
    model = PackedMobileNetV1.from_state_dict(sd)
    g = torch.Generator(device="cpu").manual_seed(3)
    x = torch.randn(args.batch, 3, args.size, args.size, generator=g).to(dev)
    print(json.dumps({"metric": "mobilenet_v1_forward", "batch": args.batch, "width": args.width, "size": args.size,
                      "reps": args.reps, **time_routes(model, x, args.reps)}))


if __name__ == "__main__":
    main()
