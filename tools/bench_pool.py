"""Cold time per call and bytes/s of the quantised ReLU / pooling kernels (qe_pool.hip), each next to what the package could do
on the same data before them, alternated in the same process.

  module forms (fp32 in, fp32 out) on ResNet-50's stem tensor (256, 64, 112, 112) and tail (256, 2048, 7, 7):
      qe_quant_relu, qe_quant_maxpool2d (3, 2, 1), qe_quant_adaptive_avgpool2d (1, 1)
      vs the torch sequence of the reference's packed forward: round(x / s - z).clamp -> (q + z) * s -> relu | max_pool2d | mean
  qe_avgpool2d_codes (8-bit codes in, the consumer's 8-bit codes out) on the pooled tensors of CLIP's RN50 at 224 x 224 -- the
      stem's AvgPool2d(2), the AvgPool2d(2) in front of conv3 and in the downsample of the first block of layer2 / 3 / 4 -- and on
      wrn_40_2's (256, 128, 8, 8) tail
      vs dequantise in torch -> F.avg_pool2d -> qe_quantize_pack, and vs qe_maxpool2d_codes with the same window on the same
      codes (the codes-domain pool the package had: the rate a byte-in, byte-out pool reaches here).

Each form is launched alone after a 1 GiB overwrite of a scratch buffer (cold L2 / MALL), timed with device events; the forms
alternate inside every repetition and the median of --reps launches is kept.  Bytes are algorithmic (each tensor once).
frac_hbm = bytes / time / 6.3 TB/s, the achievable HBM rate the depthwise table (profiles/dwconv_layers.json) uses.
usage: python tools/bench_pool.py [--batch 256] [--reps 10] [--out profiles/pool_layers.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM = 6.3e12

# name, C, H, kernel (0: the whole plane)
CODES_TENSORS = [("clip stem", 64, 112, 2), ("clip layer2 conv2", 128, 56, 2), ("clip layer2 downsample", 256, 56, 2),
                 ("clip layer3 conv2", 256, 28, 2), ("clip layer3 downsample", 512, 28, 2), ("clip layer4 conv2", 512, 14, 2),
                 ("clip layer4 downsample", 1024, 14, 2), ("wrn_40_2 tail", 128, 8, 8)]
MODULE_TENSORS = [("resnet50 stem", 64, 112), ("resnet50 tail", 2048, 7)]


def measure(torch, forms, reps, flush):
    ts = {k: [] for k in forms}
    for fn, _ in forms.values():
        fn()
    for _ in range(reps):
        for name, (fn, _) in forms.items():
            flush.fill_(1.0)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[name].append(a.elapsed_time(b))
    row = {}
    for name, (_, nbytes) in forms.items():
        ms = sorted(ts[name])[len(ts[name]) // 2]
        row[name] = {"us": round(ms * 1e3, 1), "MB": round(nbytes / 1e6, 2), "TBps": round(nbytes / (ms * 1e-3) / 1e12, 3),
                     "frac_hbm": round(nbytes / (ms * 1e-3) / HBM, 3)}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pool_layers.json"))
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from quantize_amd import capi
    dev = "cuda:0"
    N = args.batch
    g = torch.Generator(device="cpu").manual_seed(0)
    flush = torch.empty(1 << 28, dtype=torch.float32, device=dev)              # 1 GiB
    rows = []
    for name, C, H in MODULE_TENSORS:
        x = torch.randn(N, C, H, H, generator=g).to(dev)
        s, z = torch.tensor([4.0 / 255], device=dev), torch.tensor([-127.0], device=dev)
        rq = capi.requant(s, z, 0.0, 255.0, 8, False)

        def qdq():
            return ((x / s - z).round().clamp(0.0, 255.0) + z).mul_(s)

        nx = x.numel()
        for form, fn, ref, ny in (
                ("relu", lambda o: capi.quant_relu(x, rq, out=o), lambda: F.relu(qdq(), inplace=True), nx),
                ("maxpool 3,2,1", lambda o: capi.quant_maxpool2d(x, rq, 3, 2, 1, out=o), lambda: F.max_pool2d(qdq(), 3, 2, 1),
                 N * C * ((H - 1) // 2 + 1) ** 2),
                ("adaptive avgpool 1,1", lambda o: capi.quant_adaptive_avgpool2d(x, rq, 1, out=o),
                 lambda: F.adaptive_avg_pool2d(qdq(), 1), N * C)):
            out = fn(None)
            want = ref()
            assert float((want - out).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max())), (name, form)
            row = measure(torch, {"engine": (lambda: fn(out), 4 * nx + 4 * ny), "torch": (ref, 4 * nx + 4 * ny)}, args.reps, flush)
            row.update(tensor="%s (%d, %d, %d, %d)" % (name, N, C, H, H), form=form,
                       engine_vs_torch_time=round(row["torch"]["us"] / row["engine"]["us"], 2))
            rows.append(row)
            print("%-44s %-22s engine %8.1f us %5.2f TB/s | torch %9.1f us" % (row["tensor"], form, row["engine"]["us"],
                                                                              row["engine"]["TBps"], row["torch"]["us"]), file=sys.stderr)
            del out, want
        del x
    for name, C, H, k in CODES_TENSORS:
        x = torch.randint(0, 256, (N, C, H, H), generator=g, dtype=torch.uint8).to(dev)
        sx, zx = torch.tensor([0.02], device=dev), torch.tensor([3.0], device=dev)
        xq = capi.qparam(x.reshape(-1), 8, False, sx, zx)
        OH = H // k
        rq = capi.requant(torch.tensor([0.02], device=dev), torch.zeros(1, device=dev), 0.0, 255.0, 8, False)
        path = capi.POOL_KERNELS[capi.avgpool2d_codes_path(xq, N, C, H, H, k, k, relu=True, rq=rq, out=0)]
        y, codes, st = capi.avgpool2d_codes(xq, N, C, H, H, k, k, relu=True, rq=rq)
        mp = torch.empty(N * C * OH * OH, dtype=torch.uint8, device=dev)

        def torch_seq():
            t = F.avg_pool2d(F.relu((x.float() - zx) * sx), k)
            return capi.quantize_pack(t, *rq._keep, 0.0, 255.0, 8, False, status=st)[0]

        ref = F.avg_pool2d(F.relu((x.float() - zx) * sx), k)
        assert float((ref - y).abs().max()) <= 1e-5 * float(ref.abs().max()) and int(st.item()) == 0
        nx, ny = x.numel(), N * C * OH * OH
        row = measure(torch, {"codes": (lambda: capi.avgpool2d_codes(xq, N, C, H, H, k, k, relu=True, rq=rq, out=None, codes=codes, status=st), nx + ny),
                              "f32": (lambda: capi.avgpool2d_codes(xq, N, C, H, H, k, k, relu=True, out=y, status=st), nx + 4 * ny),
                              "maxpool2d_codes": (lambda: capi.maxpool2d_codes(x, 8, N, C, H, H, k, k, 0, out=mp), nx + ny),
                              "torch": (torch_seq, nx + ny)}, args.reps, flush)
        row.update(tensor="%s (%d, %d, %d, %d)" % (name, N, C, H, H), form="avgpool2d_codes k%d s%d relu" % (k, k), instance=path,
                   codes_vs_torch_time=round(row["torch"]["us"] / row["codes"]["us"], 2),
                   codes_vs_maxpool_codes_rate=round(row["codes"]["TBps"] / row["maxpool2d_codes"]["TBps"], 2))
        rows.append(row)
        print("%-44s %-6s codes %8.1f us %5.2f TB/s | f32 %8.1f us | maxpool codes %8.1f us %5.2f TB/s | torch %9.1f us" % (
            row["tensor"], path, row["codes"]["us"], row["codes"]["TBps"], row["f32"]["us"], row["maxpool2d_codes"]["us"],
            row["maxpool2d_codes"]["TBps"], row["torch"]["us"]), file=sys.stderr)
        del x, y, codes, ref, mp
    result = {"metric": "pool_cold_per_call", "batch": N, "reps": args.reps, "hbm_Bps": HBM, "rows": rows}
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
