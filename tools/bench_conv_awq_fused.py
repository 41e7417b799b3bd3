#!/usr/bin/env python3
"""The fused epilogues of the group-quantised (AWQ layout) 1x1 convolution (qe_quantconv2d_awq_fused, path 1) against the
composition the library offered before them, layer by layer: the 1x1 / stride-1 layers of ResNet-50 and MobileNetV1 of
tools/bench_conv_awq.py at batch 256, G = min(128, IC), W4 symmetric and W4 asymmetric, a per-channel 8-bit consumer
quantiser, on one MI355X in one process.  Cold caches as there: a 512 MiB buffer is rewritten before every timed call
(outside the device events); `--reps` repetitions with the variants interleaved, median and range:
  codes_relu           fused: ReLU + codes                    | composed: qe_quantconv2d_awq(relu) -> qe_quantize_pack
  end_codes / end_both fused: + identity, ReLU, codes [+ out] | composed: qe_quantconv2d_awq -> torch add_ / relu_ -> qe_quantize_pack
The composition runs on --parent-lib, a libqe_hip.so built from the parent commit (default: this build's own library, whose
fp32 kernels are the parent's instruction for instruction).  The codes of both routes are compared before anything is timed.
Writes one JSON document (default profiles/conv_awq_fused.json).  Run each invocation under its own time limit.
usage: python tools/bench_conv_awq_fused.py [--net resnet50|mobilenet_v1|all] [--parent-lib PATH]"""
import argparse, ctypes, json, os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch
from quantize_amd import capi
from quantize_amd.synthetic import pack_codes

# (IC, OC, H = W)
RESNET50 = [(64, 64, 56), (64, 256, 56), (256, 64, 56), (256, 128, 56), (128, 512, 28), (512, 128, 28), (512, 256, 28),
            (256, 1024, 14), (1024, 256, 14), (1024, 512, 14), (512, 2048, 7), (2048, 512, 7)]
MOBILENET = [(32, 64, 112), (64, 128, 56), (128, 128, 56), (128, 256, 28), (256, 256, 28), (256, 512, 14), (512, 512, 14),
             (512, 1024, 7), (1024, 1024, 7)]
ap = argparse.ArgumentParser()
ap.add_argument("--net", default="all")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "conv_awq_fused.json"))
args = ap.parse_args()
dev = torch.device("cuda", 0)
rng = np.random.RandomState(16)
N = args.batch
up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
P_LIB = capi.lib() if args.parent_lib is None else ctypes.CDLL(args.parent_lib)
for name in ("qe_quantconv2d_awq", "qe_quantize_pack"):
    getattr(P_LIB, name).restype, getattr(P_LIB, name).argtypes = capi.PROTOTYPES[name]


def timed(fn):
    flush.fill_(1)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


nets = {"resnet50": RESNET50, "mobilenet_v1": MOBILENET}
result = {"batch": N, "reps": args.reps, "unit": "ms per call, cold caches", "parent_lib": args.parent_lib is not None, "layers": {}}
missed = []
for net in (nets if args.net == "all" else [args.net]):
    for IC, OC, HW in nets[net]:
        G, P = min(128, IC), HW * HW
        NG, n = IC // G, N * OC * HW * HW
        sh = capi.conv_shape(N, IC, HW, HW, OC, 1, 1, 1, 0)
        xs = torch.randint(0, 256, (N * IC * P,), dtype=torch.uint8, device=dev)      # an 8-bit stream IS its stored bytes
        sx = up(np.array([0.02], np.float32))
        bias = up(rng.randn(OC).astype(np.float32))
        sg = up(rng.uniform(1e-3, 2e-3, OC * NG).astype(np.float32))
        wc = rng.randint(0, 16, (OC, IC))
        ops = {"w4_sym": (capi.qparam(xs, 8, True, sx, torch.zeros(1, device=dev)),
                          capi.qparam(up(pack_codes(wc - 8, 4, True)), 4, True, sg, torch.zeros(OC * NG, device=dev)), True),
               "w4_asym": (capi.qparam(xs, 8, False, sx, up(np.array([128.3], np.float32))),
                           capi.qparam(up(pack_codes(wc, 4, False)), 4, False, sg, up((8 + rng.uniform(-0.5, 0.5, OC * NG)).astype(np.float32))), False)}
        identity = torch.randn((N, OC, HW, HW), device=dev)
        out = torch.empty((N, OC, HW, HW), dtype=torch.float32, device=dev)
        codes, codes_p = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        # bias and identity are N(0, 1) and the conv term is smaller: about 128 codes to either side hold +- 2.5 sigma or more
        rq = capi.requant(up(rng.uniform(0.02, 0.04, OC).astype(np.float32)), torch.full((OC,), -128.0, device=dev), 0, 255, 8, False)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

        def composed(xq, wq, sym, end):
            def run():
                capi.check(P_LIB.qe_quantconv2d_awq(ctypes.byref(xq), ctypes.byref(wq), G, int(sym), int(sym), bias.data_ptr(), ctypes.byref(sh),
                                                    0 if end else 1, out.data_ptr(), stream))
                if end:
                    out.add_(identity).relu_()
                capi.check(P_LIB.qe_quantize_pack(out.data_ptr(), n, rq.scale, rq.zero, OC, P, 0.0, 255.0, 8, 0, codes_p.data_ptr(),
                                                  status.data_ptr(), stream))
            return run

        def fused(xq, wq, sym, end, both):
            return lambda: capi.quantconv2d_awq_fused(xq, wq, G, bias, sh, identity=identity if end else None, relu=True, out=out if both else None,
                                                      rq=rq, codes=codes, status=status, x_symmetric=sym, w_symmetric=sym)

        row = {}
        for kind, (xq, wq, sym) in ops.items():
            assert capi.conv_awq_fused_path(xq, wq, G, sh, identity=identity, relu=True, rq=rq, codes=codes, x_symmetric=sym, w_symmetric=sym) == 1
            kernels = {"codes_relu": fused(xq, wq, sym, False, False), "codes_relu_composed": composed(xq, wq, sym, False),
                       "end_codes": fused(xq, wq, sym, True, False), "end_both": fused(xq, wq, sym, True, True),
                       "end_composed": composed(xq, wq, sym, True)}
            for a, b in (("codes_relu", "codes_relu_composed"), ("end_codes", "end_composed"), ("end_both", "end_composed")):      # untimed, and compared
                kernels[a](), kernels[b]()
                assert torch.equal(codes, codes_p), (net, IC, OC, HW, kind, a)
            times = {k: [] for k in kernels}
            for _ in range(args.reps):
                for k, fn in kernels.items():
                    times[k].append(timed(fn))
            r = {k: {"ms": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in times.items()}
            spread = lambda k: max(times[k]) - min(times[k])
            for a, b in (("codes_relu", "codes_relu_composed"), ("end_codes", "end_composed"), ("end_both", "end_composed")):
                r[a]["of_composed"] = round(r[a]["ms"] / r[b]["ms"], 3)
                r[a]["below_composed_by_more_than_the_spreads"] = bool(r[b]["ms"] - r[a]["ms"] > max(spread(a), spread(b)))
                if not r[a]["below_composed_by_more_than_the_spreads"]:
                    missed.append("%s %d->%d @%dx%d %s %s" % (net, IC, OC, HW, HW, kind, a))
            row[kind] = r
        result["layers"]["%s %d->%d @%dx%d" % (net, IC, OC, HW, HW)] = row
        print(net, IC, OC, HW, json.dumps(row), flush=True)
        del xs, identity, out, codes, codes_p
        torch.cuda.empty_cache()
result["missed_the_expectation"] = missed
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print(json.dumps({"written": args.out, "missed": len(missed)}))
