"""Cold per-layer bytes/s of the residual block-end instances against the plain fp32 instance on the same layer: the four
ResNet-50 block-end shapes (1x1 convs, batch 256, W8A8) on the resident-tile kernels (qe_conv_pwr.hip).

For every layer, each form is launched alone after a 1 GiB overwrite of a scratch buffer (cold L2 / MALL), timed with
device events; the median of --reps launches is kept.  Algorithmic bytes (each tensor once, weights excluded):
  fp32        x codes in + fp32 out                               (qe_quantconv2d_prepared)
  res_f32_q   x codes + fp32 identity in, fp32 out + 8-bit codes  (qe_quantconv2d_residual_prepared, rq, out)
  res_q       x codes + fp32 identity in, 8-bit codes out         (stage boundaries: out = NULL)
  res_f32     x codes + fp32 identity in, fp32 out                (the last block: rq = NULL)
ratio = (bytes/s of the form) / (bytes/s of fp32).  QE_LIB=<path> runs another build of the library (A/B of variants).
usage: python tools/bench_residual_layers.py [--batch 256] [--reps 10]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LAYERS = [(64, 256, 56), (128, 512, 28), (256, 1024, 14), (512, 2048, 7)]     # IC, OC, H of the block ends


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import torch
    from quantize_amd import capi
    dev = "cuda:0"
    N = args.batch
    g = torch.Generator(device="cpu").manual_seed(0)
    flush = torch.empty(1 << 28, dtype=torch.float32, device=dev)              # 1 GiB
    rows = []
    for IC, OC, H in LAYERS:
        P = H * H
        x = torch.randint(0, 256, (N * IC * P,), generator=g, dtype=torch.uint8).to(dev)
        w = torch.randint(0, 256, (OC * IC,), generator=g, dtype=torch.uint8).to(dev)
        sx, zx = torch.tensor([0.02], device=dev), torch.tensor([0.0], device=dev)
        sw, zw = (torch.rand(OC, generator=g) * 4e-4 + 2e-4).to(dev), torch.zeros(OC, device=dev)
        bias = (torch.randn(OC, generator=g) * 0.1).to(dev)
        sh = capi.conv_shape(N, IC, H, H, OC, 1, 1, 1, 0)
        xq, wq = capi.qparam(x, 8, False, sx, zx), capi.qparam(w, 8, True, sw, zw)
        prep = capi.conv_prepare(wq, bias, sh, 8)
        y = capi.quantconv2d_prepared(xq, wq, bias, sh, prep)
        identity = torch.randn(y.shape, generator=g).to(dev) * float(y.std())
        out = torch.empty_like(y)
        codes = torch.empty(y.numel(), dtype=torch.uint8, device=dev)
        st = torch.zeros(1, dtype=torch.int32, device=dev)
        rq = capi.requant(torch.relu(y + identity).max().reshape(1) / 255.0, torch.zeros(1, device=dev), 0, 255, 8, False)
        assert capi.residual_path(sh, xq, wq, rq) == 1 and capi.residual_path(sh, xq, wq, None) == 1
        nx, ny = x.numel(), y.numel()
        forms = {
            "fp32": (lambda: capi.quantconv2d_prepared(xq, wq, bias, sh, prep, out=out), nx + 4 * ny),
            "res_f32_q": (lambda: capi.quantconv2d_residual_prepared(xq, wq, bias, sh, prep, identity, rq=rq, out=out,
                                                                     codes=codes, status=st), nx + 4 * ny + 4 * ny + ny),
            "res_q": (lambda: capi.quantconv2d_residual_prepared(xq, wq, bias, sh, prep, identity, rq=rq, out=None, codes=codes,
                                                                 status=st), nx + 4 * ny + ny),
            "res_f32": (lambda: capi.quantconv2d_residual_prepared(xq, wq, bias, sh, prep, identity, rq=None, out=out,
                                                                   status=st), nx + 4 * ny + 4 * ny),
        }
        row = {"layer": "%d->%d @%dx%d" % (IC, OC, H, H)}
        for name, (fn, nbytes) in forms.items():
            fn()
            ts = []
            for _ in range(args.reps):
                flush.fill_(1.0)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ts.append(a.elapsed_time(b))
            ms = sorted(ts)[len(ts) // 2]
            row[name] = {"us": round(ms * 1e3, 1), "GB": round(nbytes / 1e9, 4), "TBps": round(nbytes / (ms * 1e-3) / 1e12, 3)}
        for name in ("res_f32_q", "res_q", "res_f32"):
            row[name]["ratio_vs_fp32"] = round(row[name]["TBps"] / row["fp32"]["TBps"], 3)
        rows.append(row)
        del x, y, identity, out, codes
    print(json.dumps({"metric": "residual_block_end_cold_per_layer", "batch": N, "reps": args.reps,
                      "lib": os.path.basename(os.environ.get("QE_LIB", "") or "libqe_hip.so"), "layers": rows}))


if __name__ == "__main__":
    main()
