"""Cold time per call and bytes/s of qe_affine_relu_quantize_pack (qe_preact.hip) on each distinct block boundary of wrn_40_2 at
batch 256 -- (256, 32, 32, 32), (256, 64, 16, 16), (256, 128, 8, 8) -- with one and two 8-bit consumers, with and without
sum_out, next to the sequence it replaces on what the package could do before it, alternated in the same process:
torch.add, the affine as two torch ops, torch.relu, capi.quantize_pack per consumer.

Each form is launched alone after a 1 GiB overwrite of a scratch buffer (cold L2 / MALL), timed with device events; the forms
alternate inside every repetition and the median of --reps launches is kept.  Bytes are algorithmic (each tensor once): x and
identity read, the codes and sum_out written -- the sequence is charged the same bytes, not what its five passes really move.
frac_hbm = bytes / time / 6.3 TB/s, the achievable HBM rate the other per-layer tables use.
usage: python tools/bench_preact.py [--batch 256] [--reps 10] [--out profiles/preact_layers.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM = 6.3e12
TENSORS = [("block1 / block2.0", 32, 32), ("block2 / block3.0", 64, 16), ("block3", 128, 8)]


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preact_layers.json"))
    args = ap.parse_args()
    import torch
    from quantize_amd import capi
    dev = "cuda:0"
    N = args.batch
    g = torch.Generator(device="cpu").manual_seed(0)
    flush = torch.empty(1 << 28, dtype=torch.float32, device=dev)              # 1 GiB
    rows = []
    for name, C, H in TENSORS:
        x = torch.randn(N, C, H, H, generator=g).to(dev)
        identity = torch.randn(N, C, H, H, generator=g).to(dev)
        alpha = (torch.rand(C, generator=g) + 0.5).to(dev)
        shift = (torch.randn(C, generator=g) * 0.1).to(dev)
        scales = [torch.tensor([6.0 / 255], device=dev), torch.tensor([7.0 / 255], device=dev)]
        zero = torch.zeros(1, device=dev)
        n = x.numel()
        for n_out in (1, 2):
            rqs = [capi.requant(s, zero, 0.0, 255.0, 8, False) for s in scales[:n_out]]
            for with_sum in (False, True):
                st = torch.zeros(1, dtype=torch.int32, device=dev)
                codes, s_out, _, _ = capi.affine_relu_quantize_pack(x, alpha, shift, identity=identity, rqs=rqs,
                                                                    sum_out="new" if with_sum else None, status=st)
                seq_codes = [torch.empty_like(c) for c in codes]

                def sequence():
                    s = torch.add(x, identity)
                    t = s * alpha.view(1, -1, 1, 1)
                    t = t + shift.view(1, -1, 1, 1)
                    a = torch.relu(t)
                    for sc, out in zip(scales, seq_codes):
                        capi.quantize_pack(a, sc, zero, 0.0, 255.0, 8, False, out=out, status=st)
                    return s

                s_ref = sequence()
                assert all(torch.equal(a, b) for a, b in zip(codes, seq_codes)) and int(st.item()) == 0, (name, n_out, with_sum)
                assert not with_sum or torch.equal(s_out, s_ref)
                inst = capi.PREACT_KERNELS[capi.affine_relu_quantize_pack_path(N, C, H * H, rqs, sum_out=256 if with_sum else 0)]
                nbytes = 8 * n + n_out * n + (4 * n if with_sum else 0)
                row = measure(torch, {"fused": (lambda: capi.affine_relu_quantize_pack(x, alpha, shift, identity=identity, rqs=rqs,
                                                                                       sum_out=s_out, codes=codes, status=st), nbytes),
                                      "sequence": (sequence, nbytes)}, args.reps, flush)
                row.update(tensor="%s (%d, %d, %d, %d)" % (name, N, C, H, H), consumers=n_out, sum_out=with_sum, instance=inst,
                           sequence_over_fused_time=round(row["sequence"]["us"] / row["fused"]["us"], 2))
                rows.append(row)
                print("%-40s consumers %d sum_out %d  %-5s fused %8.1f us %5.2f TB/s | sequence %9.1f us" % (
                    row["tensor"], n_out, with_sum, inst, row["fused"]["us"], row["fused"]["TBps"], row["sequence"]["us"]), file=sys.stderr)
        del x, identity
    result = {"metric": "preact_cold_per_call", "batch": N, "reps": args.reps, "hbm_Bps": HBM, "rows": rows,
              "fused_not_slower_on_every_row": all(r["fused"]["us"] <= r["sequence"]["us"] for r in rows)}
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
