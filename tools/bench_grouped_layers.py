"""Cold per-layer time and bytes/s of the seven distinct grouped 3x3 layers of ResNeXt-50 32x4d at 224x224 (batch 256, W8A8)
on the fast grouped family (qe_conv_grp.hip), alternated in the same process with torch's fp32 F.conv2d(groups=32) on the
dequantised activations -- the reference's packed forward on this GPU, and what a grouped layer had to run on before these
kernels.

Each form is launched alone after a 1 GiB overwrite of a scratch buffer (cold L2 / MALL), timed with device events; the
forms alternate inside every repetition and the median of --reps launches is kept.  Algorithmic bytes (each tensor once,
weights excluded):
  codes       8-bit codes in, the consumer's 8-bit codes out (ReLU in the epilogue)      1 B in + 1 B out per element
  f32         8-bit codes in, fp32 out                                                  1 B in + 4 B out
  torch       fp32 dequantised activations in, fp32 out (F.conv2d, groups=32)           4 B in + 4 B out
frac_hbm = bytes / time / 6.3 TB/s (the achievable HBM rate of the microarchitecture notes).
usage: python tools/bench_grouped_layers.py [--batch 256] [--reps 10]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# C, H (input side), stride of the seven distinct grouped layers (32 groups), in forward order
LAYERS = [(128, 56, 1), (256, 56, 2), (256, 28, 1), (512, 28, 2), (512, 14, 1), (1024, 14, 2), (1024, 7, 1)]
GROUPS = 32
HBM = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from quantize_amd import capi
    dev = "cuda:0"
    N = args.batch
    g = torch.Generator(device="cpu").manual_seed(0)
    flush = torch.empty(1 << 28, dtype=torch.float32, device=dev)              # 1 GiB
    rows = []
    for C, H, s in LAYERS:
        cg = C // GROUPS
        x = torch.randint(0, 256, (N, C, H, H), generator=g, dtype=torch.uint8).to(dev)
        w = torch.randint(0, 256, (C * cg * 9,), generator=g, dtype=torch.uint8).to(dev)
        sx, zx = torch.tensor([0.02], device=dev), torch.tensor([0.0], device=dev)
        sw, zw = (torch.rand(C, generator=g) * 4e-3 + 2e-3).to(dev) / cg ** 0.5, torch.zeros(C, device=dev)
        bias = (torch.randn(C, generator=g) * 0.1).to(dev)
        sh = capi.conv_shape(N, C, H, H, C, 3, 3, s, 1)
        xq, wq = capi.qparam(x.reshape(-1), 8, False, sx, zx), capi.qparam(w, 8, True, sw, zw)
        y, _, _ = capi.quantconv2d_grouped(xq, wq, bias, sh, GROUPS, relu=True)
        rq = capi.requant(y.max().reshape(1) / 255.0, torch.zeros(1, device=dev), 0, 255, 8, False)
        assert capi.grouped_path(sh, GROUPS, xq, wq, rq) == 1
        plan = capi.grouped_plan_info(sh, GROUPS, xq, wq, rq)
        codes = torch.empty(y.numel(), dtype=torch.uint8, device=dev)
        st = torch.zeros(1, dtype=torch.int32, device=dev)
        xf = (x.float() - zx) * sx
        wf = ((w.view(C, cg, 3, 3).float() - 128.0) * sw.view(C, 1, 1, 1)).contiguous()
        ref = torch.relu(F.conv2d(xf, wf, bias, stride=s, padding=1, groups=GROUPS))
        assert float((ref - y).abs().max()) <= 1e-3 * float(ref.abs().max())
        nx, ny = x.numel(), y.numel()
        forms = {
            "codes": (lambda: capi.quantconv2d_grouped(xq, wq, bias, sh, GROUPS, relu=True, rq=rq, out=None, codes=codes, status=st),
                      nx + ny),
            "f32": (lambda: capi.quantconv2d_grouped(xq, wq, bias, sh, GROUPS, relu=True, out=y, status=st), nx + 4 * ny),
            "torch": (lambda: F.conv2d(xf, wf, bias, stride=s, padding=1, groups=GROUPS), 4 * nx + 4 * ny),
        }
        ts = {k: [] for k in forms}
        for fn, _ in forms.values():
            fn()
        for _ in range(args.reps):
            for name, (fn, _) in forms.items():
                flush.fill_(1.0)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ts[name].append(a.elapsed_time(b))
        row = {"layer": "C%d Cg%d %dx%d s%d" % (C, cg, H, H, s), "kernel": capi.GRP_KERNELS[plan.kernel], "slab": plan.slab,
               "TH": plan.TH, "TW": plan.TW, "tiles": plan.tiles, "blocks": plan.blocks, "lds": plan.lds}
        for name, (_, nbytes) in forms.items():
            ms = sorted(ts[name])[len(ts[name]) // 2]
            row[name] = {"us": round(ms * 1e3, 1), "MB": round(nbytes / 1e6, 2), "TBps": round(nbytes / (ms * 1e-3) / 1e12, 3),
                         "frac_hbm": round(nbytes / (ms * 1e-3) / HBM, 3)}
        row["codes_vs_torch_time"] = round(row["torch"]["us"] / row["codes"]["us"], 2)
        row["f32_vs_torch_time"] = round(row["torch"]["us"] / row["f32"]["us"], 2)
        rows.append(row)
        print("%-20s codes %8.1f us %5.2f TB/s | f32 %8.1f us %5.2f TB/s | torch %8.1f us %5.2f TB/s" % (
            row["layer"], row["codes"]["us"], row["codes"]["TBps"], row["f32"]["us"], row["f32"]["TBps"], row["torch"]["us"],
            row["torch"]["TBps"]), file=sys.stderr)
        del x, y, xf, ref, codes
    tot = {k: round(sum(r[k]["us"] for r in rows), 1) for k in ("codes", "f32", "torch")}
    print(json.dumps({"metric": "grouped_cold_per_layer", "batch": N, "groups": GROUPS, "reps": args.reps, "hbm_Bps": HBM,
                      "total_us": tot, "layers": rows}))


if __name__ == "__main__":
    main()
