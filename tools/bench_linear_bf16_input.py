#!/usr/bin/env python3
"""out_proj of a packed ViT, alone: qe_quantlinear_float_input_residual on fp32 rows against qe_quantlinear_bf16_input with
the residual on the same values rounded to bf16, in one session, alternating step by step, with device events.

Shapes: out_proj (K = O = width, B = images x tokens) of ViT-B/16 (768, 197 tokens), ViT-L/16 (1024, 197) and ViT-H/14
(1280, 257) at 64 and 256 images.  Each step times `--reps` back-to-back calls of one entry point (in place: out = residual);
the figure is the median over `--steps` steps of the time per call.  GB/s is against the bytes the residual form has to
move, 2 B K + 8 B O + K O for the bf16 rows (4 B K + ... for the fp32 rows); mfma_share is the time v_mfma_f32_32x32x16_bf16
needs for the kernel's products at the matrix pipe's bf16 peak (DENSE_BF16_TFLOPS below) over the measured time -- three
MFMAs per product for the fp32 rows' exact split, one for the bf16 rows.

--entry float_input binds only qe_quantlinear_float_input_residual, straight from the library QE_LIB names: an earlier build
of libqe_hip.so (one without the bf16-input entry) can be timed with the same code, for a parent-vs-parent spread.
usage: python tools/bench_linear_bf16_input.py [--steps 20] [--warmup 3] [--reps 10] [--batches 64 256] [--entry both|float_input]"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODELS = {"vit_b_16": (768, 197), "vit_l_16": (1024, 197), "vit_h_14": (1280, 257)}
DENSE_BF16_TFLOPS = 2500.0          # MI355X matrix pipe, bf16 dense


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 64])
    ap.add_argument("--entry", choices=["both", "float_input"], default="both")
    args = ap.parse_args()
    import torch
    from quantize_amd import capi, loader

    dev = torch.device("cuda", 0)
    if args.entry == "both":
        L = capi.lib()
    else:
        L = ctypes.CDLL(os.environ.get("QE_LIB") or loader.lib_path())
        f = L.qe_quantlinear_float_input_residual
        f.restype, f.argtypes = capi.PROTOTYPES["qe_quantlinear_float_input_residual"]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device=dev).manual_seed(5)
    res = {"metric": "out_proj_alone", "unit": "ms per call", "entry": args.entry, "steps": args.steps, "reps": args.reps, "shapes": {}}
    for name, (E, tokens) in MODELS.items():
        for N in args.batches:
            B, K, O = N * tokens, E, E
            x = torch.randn(B, K, generator=g, device=dev)
            x16 = x.to(torch.bfloat16)
            w = torch.randint(0, 256, (O * K,), generator=g, device=dev, dtype=torch.int32).to(torch.uint8)
            sw = torch.rand(O, generator=g, device=dev) * 5e-4 + 2.5e-4
            wq = capi.qparam(w, 8, 1, sw, torch.zeros(O, device=dev))
            bias = torch.randn(O, generator=g, device=dev) * 0.02
            out = torch.zeros(B, O, device=dev)
            calls = {"float_input_fp32_rows": lambda: L.qe_quantlinear_float_input_residual(
                x.data_ptr(), ctypes.byref(wq), bias.data_ptr(), B, K, O, out.data_ptr(), out.data_ptr(), None, 0, stream)}
            if args.entry == "both":
                assert capi.quantlinear_bf16_input_path(x16, wq, B, K, O) == 1 and capi.linear_float_input_residual_path(x, wq, B, K, O) == 1
                calls["bf16_input_bf16_rows"] = lambda: L.qe_quantlinear_bf16_input(
                    x16.data_ptr(), ctypes.byref(wq), bias.data_ptr(), B, K, O, out.data_ptr(), out.data_ptr(), None, 0, stream)
            times = {k: [] for k in calls}
            for i in range(args.warmup + args.steps):
                for k, call in calls.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(args.reps):
                        rc = call()
                    b.record()
                    torch.cuda.synchronize()
                    assert rc == 0, (k, rc)
                    if i >= args.warmup:
                        times[k].append(a.elapsed_time(b) / args.reps)
            row = {}
            for k, t in times.items():
                t = sorted(t)
                ms = t[len(t) // 2]
                xb, mf = (2, 1) if k.startswith("bf16") else (4, 3)
                nbytes = xb * B * K + 8 * B * O + K * O
                row[k] = {"ms": round(ms, 5), "min_ms": round(t[0], 5), "max_ms": round(t[-1], 5), "GBs": round(nbytes / ms / 1e6, 1),
                          "mfma_share": round(mf * 2.0 * B * K * O / (DENSE_BF16_TFLOPS * 1e9) / ms, 3)}
            if len(row) == 2:
                row["speedup"] = round(row["float_input_fp32_rows"]["ms"] / row["bf16_input_bf16_rows"]["ms"], 3)
            res["shapes"]["%s_N%d_%dx%d->%d" % (name, N, B, K, O)] = row
            del x, x16, out
            torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
