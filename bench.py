#!/usr/bin/env python3
"""Headline benchmark: quant-conv2d images/s at batch 256 per GPU (ResNet-50 conv stack, W8A8).

    python bench.py --gpus 1 --steps K --warmup W                      (1 GPU)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W         (N GPUs, one rank each)

One "step" = one pass of the hot path over one batch: the 53 convolutions of ResNet-50
(each layer an independent packed-int conv problem with synthetic operands of
the right shape, activations and weights already packed and resident in HBM), called through the
C ABI `qe_quantconv2d_prepared` with the layer's weights prepared once at set-up (`qe_conv_prepare`:
a packed layer's weights do not change between forward passes; `--per-call-prepare` restores the
form in which the reference's `quantconv2d` op re-lays them out inside every call), followed by
the top-1 tail: avg-pool + a synthetic 2048->1000 fc on the last layer's output, an all-gather of
the logits over RCCL when N > 1, and an argmax.  Images shard across ranks (weak scaling: 256 per
GPU), no data-path collective other than that all-gather.

Prints ONE JSON line on rank 0 (contract in the task statement) with `roofline` (measured live
with HIP events on the launch stream) and `cpu_baseline` objects.  `cpu_baseline` is the baseline
north_star names -- the reference's own packed-forward CPU fallback, `F.conv2d` on the dequantised
tensors (quantconv2d.py:207-210) through torch-CPU on the box's host cores, bounded sample;
`cpu_baseline_port` is the oracle's CPU restatement of the reference KERNEL loop (OpenMP).
"""
import argparse
import ctypes
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

HBM_PEAK_GBS = 8000.0       # MI355X HBM3E spec (MI355X_MICROARCH.md: 8.0 TB/s; 6.29 TB/s measured copy)
INT8_MFMA_PEAK_TOPS = 5000.0  # dense int8 = 2x bf16 (~2.5 PF)
DUMP_BUDGET_BYTES = 60 * 1000 * 1000   # --dump-outputs: all .npy payloads together, under 64 MB with the file headers
DUMP_SEED = 7919


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256, help="images per GPU")
    ap.add_argument("--w-bits", type=int, default=8)
    ap.add_argument("--a-bits", type=int, default=8)
    ap.add_argument("--asymmetric", action="store_true", help="unsigned activations with z_x = 133.2578 (SURVEY 8d)")
    ap.add_argument("--per-layer", action="store_true", help="also time every layer on its own (untimed region)")
    ap.add_argument("--cold", action="store_true",
                    help="--per-layer: overwrite 1 GiB before every timed call, so inputs come from HBM as they do inside "
                         "the stack (repeating one layer keeps its input in the 256 MB Infinity Cache otherwise)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-images", type=int, default=16, help="images of the CPU-baseline sample (about 15 s on 16 cores)")
    ap.add_argument("--cpu-fallback-images", type=int, default=32,
                    help="images of the reference-fallback sample (torch-CPU F.conv2d on dequantised tensors)")
    ap.add_argument("--float-input", action="store_true",
                    help="the quantconv2d_float_input operator instead: fp32 NCHW activations x packed weights on the same 53-layer "
                         "stack (22.32 GB algorithmic per batch-256); reported under its own metric name, never as the headline")
    ap.add_argument("--fused-requant", action="store_true",
                    help="SEPARATE measurement (not the headline contract, whose outputs are fp32): every conv stores the 8-bit "
                         "codes of the consumer's activation quantiser instead (qe_quantconv2d_requant_prepared), 1 B per output")
    ap.add_argument("--two-pass", action="store_true",
                    help="with --fused-requant: produce the same codes the reference's way, conv to fp32 and then the fused "
                         "quantise+pack kernel (qe_quantconv2d_prepared + qe_quantize_pack): the comparison line for the fused epilogue")
    ap.add_argument("--per-call-prepare", action="store_true",
                    help="re-lay-out the 3x3 / stem weights inside every call (qe_quantconv2d, as round 1 timed it) instead of "
                         "once per layer at set-up (qe_conv_prepare + qe_quantconv2d_prepared: a packed layer's weights do not "
                         "change between forward passes)")
    ap.add_argument("--layers", type=str, default="", help="comma list of layer indices (debug)")
    ap.add_argument("--layer-streams", type=int, default=1,
                    help="DIAGNOSTIC: issue layer i on stream i %% S (the 53 problems are independent in this bench; a real network's "
                         "layers are not) -- bounds what co-scheduling kernels of different phases could buy")
    ap.add_argument("--branch-streams", action="store_true",
                    help="the downsample branch of a stage's first block on a second stream beside conv1..conv3 of that block "
                         "(the concurrency a real, dependent ResNet-50 forward has); fork at the block's input, join at its end")
    ap.add_argument("--mb-stagger", type=int, default=0,
                    help="with --microbatches M: micro-batch m starts m*K layers behind micro-batch 0")
    ap.add_argument("--microbatches", type=int, default=1,
                    help="split the batch into M micro-batches, each walking the 53 layers on its own HIP stream (kernels of "
                         "different micro-batches overlap; not the headline, whose roofline is per launch)")
    ap.add_argument("--graph", action="store_true",
                    help="replay the 53 layer calls as one captured hipGraph instead of launching them one by one "
                         "(measured: no gain, the step is not dispatch-bound: 4.684 vs 4.669 ms)")
    ap.add_argument("--dump-outputs", metavar="DIR", default="",
                    help="after the timed steps, write what the last step computed to DIR/<name>.npy (float32): every conv "
                         "layer's output (a fixed, seeded sample of it when the layer is larger than its share of the 64 MB "
                         "budget; 8-bit packed bytes with --fused-requant), the logits and the top-1 predictions (rank 0)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


class Layer:
    """Device-resident operands + prebuilt C-ABI argument structs of one conv problem."""

    def __init__(self, idx, spec, N, dev, args, rank, capi, resnet50, torch):
        self.idx, self.spec, self.N = idx, spec, N
        s = resnet50.synth_layer(spec, idx, N, dev, x_bits=args.a_bits, w_bits=args.w_bits,
                                 asymmetric=args.asymmetric, rank=rank)
        self.float_input = bool(getattr(args, "float_input", False))
        self.wp, st2 = capi.tpack(s["qw"].reshape(-1), args.w_bits, s["w_sign"])
        assert int(st2.item()) == 0
        if self.float_input:
            # fp32 activations ~ N(0, 0.5), seed 5000 + idx (+ rank): the operator takes them as they are (no quantisation)
            gx = torch.Generator(device=dev)
            gx.manual_seed(5000 + idx + 1000003 * rank)
            self.xf = torch.randn((N, spec.IC, spec.H, spec.H), generator=gx, device=dev) * 0.5
            self.xp = None
        else:
            self.xp, st = capi.tpack(s["qx"].reshape(-1), args.a_bits, s["x_sign"])
            assert int(st.item()) == 0
        del s["qx"]
        self.sx, self.zx, self.sw, self.zw, self.bias = s["sx"], s["zx"], s["sw"].reshape(-1), s["zw"].reshape(-1), s["bias"]
        self.x_sign = s["x_sign"]
        self.sh = capi.conv_shape(N, spec.IC, spec.H, spec.H, spec.OC, spec.K, spec.K, spec.stride, spec.pad)
        self.wq = capi.qparam(self.wp, args.w_bits, True, self.sw, self.zw)
        oh, ow = capi.out_hw(self.sh)
        self.out = torch.empty((N, spec.OC, oh, ow), dtype=torch.float32, device=dev)
        if self.float_input:
            L = capi.lib()
            bias_p = ctypes.c_void_p(self.bias.data_ptr()) if self.bias is not None else None
            self.path = capi.float_input_path(self.sh, self.wq)
            self.prepared = capi.conv_f32_prepare(self.wq, self.bias, self.sh)     # once, outside the timed region
            self.bytes = resnet50.algorithmic_bytes(spec, N, args.a_bits, args.w_bits, float_input=True)
            self.ops = 2 * resnet50.macs_per_image(spec) * N
            pp = ctypes.c_void_p(self.prepared.data_ptr()) if self.prepared.numel() else None
            self._call = (L.qe_quantconv2d_float_input_prepared, ctypes.c_void_p(self.xf.data_ptr()), ctypes.byref(self.wq), bias_p,
                          ctypes.byref(self.sh), pp, ctypes.c_size_t(self.prepared.numel()), ctypes.c_void_p(self.out.data_ptr()))
            return
        self.xq = capi.qparam(self.xp, args.a_bits, s["x_sign"], self.sx, self.zx)
        L = capi.lib()
        bias_p = ctypes.c_void_p(self.bias.data_ptr()) if self.bias is not None else None
        self.prepared = None
        if args.per_call_prepare:
            need = capi.workspace_bytes(self.sh, args.a_bits, args.w_bits)
        else:
            # weights prepared ONCE here, outside the timed region (reference: pack() runs once, quantconv2d.py:187-192)
            self.prepared = capi.conv_prepare(self.wq, self.bias, self.sh, args.a_bits)
            need = int(L.qe_quantconv2d_prepared_workspace_bytes(ctypes.byref(self.sh), args.a_bits, args.w_bits))
        self.ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        self.path = capi.conv_path(self.sh, self.xq, self.wq)
        self.bytes = resnet50.algorithmic_bytes(spec, N, args.a_bits, args.w_bits)
        self.ops = 2 * resnet50.macs_per_image(spec) * N
        if getattr(args, "fused_requant", False):
            # consumer's quantiser: per tensor, signed 8 bit, scale from the layer's own output statistics (one untimed call)
            y = capi.quantconv2d_prepared(self.xq, self.wq, self.bias, self.sh, self.prepared)
            self.rq_s = (y.abs().max() / 127.0).reshape(1).float()
            self.rq_z = torch.zeros(1, device=dev)
            del y
            self.rq = capi.requant(self.rq_s, self.rq_z, -128.0, 127.0, 8, True)
            self.fused = capi.requant_path(self.sh, self.xq, self.wq, self.rq)
            need = int(L.qe_quantconv2d_requant_workspace_bytes(ctypes.byref(self.sh), ctypes.byref(self.xq), ctypes.byref(self.wq),
                                                                ctypes.byref(self.rq)))
            self.ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
            self.out = None
            self.out_q = torch.empty(N * spec.OC * oh * ow, dtype=torch.uint8, device=dev)
            self.status = torch.zeros(1, dtype=torch.int32, device=dev)
            self.bytes = resnet50.algorithmic_bytes(spec, N, args.a_bits, args.w_bits) - 3 * N * spec.OC * oh * ow
            pp = ctypes.c_void_p(self.prepared.data_ptr()) if self.prepared.numel() else None
            self._call = (L.qe_quantconv2d_requant_prepared, ctypes.byref(self.xq), ctypes.byref(self.wq), bias_p,
                          ctypes.byref(self.sh), pp, ctypes.c_size_t(self.prepared.numel()), ctypes.byref(self.rq),
                          ctypes.c_void_p(self.out_q.data_ptr()), ctypes.c_void_p(self.status.data_ptr()),
                          ctypes.c_void_p(self.ws.data_ptr()), ctypes.c_size_t(self.ws.numel()))
            if getattr(args, "two_pass", False):
                self.fused = 0
                self.out = torch.empty((N, spec.OC, oh, ow), dtype=torch.float32, device=dev)
                need = int(L.qe_quantconv2d_prepared_workspace_bytes(ctypes.byref(self.sh), args.a_bits, args.w_bits))
                self.ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
                self._call = (L.qe_quantconv2d_prepared, ctypes.byref(self.xq), ctypes.byref(self.wq), bias_p,
                              ctypes.byref(self.sh), pp, ctypes.c_size_t(self.prepared.numel()),
                              ctypes.c_void_p(self.out.data_ptr()),
                              ctypes.c_void_p(self.ws.data_ptr()), ctypes.c_size_t(self.ws.numel()))
                self._call2 = (L.qe_quantize_pack, ctypes.c_void_p(self.out.data_ptr()), ctypes.c_int64(N * spec.OC * oh * ow),
                               ctypes.c_void_p(self.rq_s.data_ptr()), ctypes.c_void_p(self.rq_z.data_ptr()), 1, ctypes.c_int64(oh * ow),
                               ctypes.c_float(-128.0), ctypes.c_float(127.0), 8, 1, ctypes.c_void_p(self.out_q.data_ptr()),
                               ctypes.c_void_p(self.status.data_ptr()))
        elif self.prepared is None:
            self._call = (L.qe_quantconv2d, ctypes.byref(self.xq), ctypes.byref(self.wq), bias_p,
                          ctypes.byref(self.sh), ctypes.c_void_p(self.out.data_ptr()),
                          ctypes.c_void_p(self.ws.data_ptr()), ctypes.c_size_t(self.ws.numel()))
        else:
            pp = ctypes.c_void_p(self.prepared.data_ptr()) if self.prepared.numel() else None
            self._call = (L.qe_quantconv2d_prepared, ctypes.byref(self.xq), ctypes.byref(self.wq), bias_p,
                          ctypes.byref(self.sh), pp, ctypes.c_size_t(self.prepared.numel()),
                          ctypes.c_void_p(self.out.data_ptr()),
                          ctypes.c_void_p(self.ws.data_ptr()), ctypes.c_size_t(self.ws.numel()))

    def run(self, stream_ptr):
        f = self._call
        rc = f[0](*f[1:], stream_ptr)
        if rc != 0:
            raise RuntimeError("conv call failed on layer %s: %d" % (self.spec.name, rc))
        f2 = getattr(self, "_call2", None)
        if f2 is not None:
            rc = f2[0](*f2[1:], stream_ptr)
            if rc != 0:
                raise RuntimeError("quantize_pack call failed on layer %s: %d" % (self.spec.name, rc))


def usable_cores():
    """The cores this process may really use (cgroup quota / affinity), not the host's core count."""
    avail = len(os.sched_getaffinity(0))
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            avail = max(1, min(avail, int(int(quota) / int(period))))
    except Exception:
        pass
    return avail


def cpu_fallback_baseline(layers, args, torch):
    """north_star's "reference's CPU fallback": what the reference's packed QuantConv2d.forward really executes
    today (modelzoo/modules/quantconv2d.py:207-210, the native call is commented out): dequantise both operands and
    call F.conv2d -- here on the host cores through torch-CPU (oneDNN), all usable cores, on the first
    `cpu_fallback_images` images of every layer's batch.  The dequantisation is inside the timed region, as it is
    inside the reference's forward.  No reference code runs: the integer codes come from the engine's own tunpack."""
    import torch.nn.functional as F
    from quantize_amd import capi
    n_img = args.cpu_fallback_images
    cores = usable_cores()
    old = torch.get_num_threads()
    torch.set_num_threads(cores)
    work = []
    for L in layers:
        sp = L.spec
        n_x = n_img * sp.IC * sp.H * sp.H
        if L.float_input:
            qw = capi.tunpack(L.wp, sp.OC * sp.IC * sp.K * sp.K, args.w_bits, True).reshape(sp.OC, sp.IC, sp.K, sp.K).cpu()
            work.append((L.xf[:n_img].cpu(), None, None, qw, L.sw.cpu().reshape(-1, 1, 1, 1), L.zw.cpu().reshape(-1, 1, 1, 1),
                         None if L.bias is None else L.bias.cpu(), sp.stride, sp.pad))
            continue
        qx = capi.tunpack(L.xp[: (n_x * args.a_bits + 7) // 8], n_x, args.a_bits, L.x_sign).reshape(n_img, sp.IC, sp.H, sp.H).cpu()
        qw = capi.tunpack(L.wp, sp.OC * sp.IC * sp.K * sp.K, args.w_bits, True).reshape(sp.OC, sp.IC, sp.K, sp.K).cpu()
        work.append((qx, L.sx.cpu(), L.zx.cpu(), qw, L.sw.cpu().reshape(-1, 1, 1, 1), L.zw.cpu().reshape(-1, 1, 1, 1),
                     None if L.bias is None else L.bias.cpu(), sp.stride, sp.pad))
    def run():
        for qx, sx, zx, qw, sw, zw, b, st, pd in work:
            xin = qx if sx is None else (qx.float() - zx) * sx          # float-input operator: activations as they are
            F.conv2d(xin, (qw.float() - zw) * sw, b, st, pd)
    with torch.no_grad():
        run()                      # warm-up: oneDNN primitive creation
        t0 = time.perf_counter()
        run()
        dt = time.perf_counter() - t0
    torch.set_num_threads(old)
    return {"value": n_img / dt, "unit": "images/s", "cores": cores, "threads": cores, "kind": "reference",
            "what": "the reference's packed-forward fallback arithmetic (its CUDA kernels have no CPU form; no reference code runs)",
            "sample": "%d images through all %d conv layers: torch-CPU F.conv2d((q - z) * s, (q - z) * s, bias) as in "
                      "the reference's packed forward (quantconv2d.py:207-210), dequantisation timed, %.1f s"
                      % (n_img, len(layers), dt)}


def cpu_baseline(layers, args, torch):
    """The oracle (CPU restatement of quantconv2d.cu:78-141, fp32 mul+add chain) on a bounded sample:
    the first `cpu_images` images of every layer's batch, OpenMP over outputs on all host cores."""
    import numpy as np
    import oracle
    n_img = args.cpu_images
    avail = usable_cores()
    oracle.set_num_threads(avail)
    threads = oracle.num_threads()
    work = []
    if layers and layers[0].float_input:
        for L in layers:
            sp = L.spec
            wd = np.array([args.w_bits, 1, sp.OC, sp.IC, sp.K, sp.K], np.int32)
            work.append((L.xf[:n_img].cpu().numpy(), L.wp.cpu().numpy(), wd, L.sw.cpu().numpy(), L.zw.cpu().numpy(),
                         None if L.bias is None else L.bias.cpu().numpy(), sp.stride, sp.pad))
        t0 = time.perf_counter()
        for w in work:
            oracle.quantconv2d_float_input(*w, mode="fp32")
        dt = time.perf_counter() - t0
        return {"value": n_img / dt, "unit": "images/s", "cores": threads, "threads": threads, "kind": "port",
                "sample": "%d images through all %d conv layers (oracle/qe_oracle.c float-input loop, OpenMP over outputs), %.1f s"
                          % (n_img, len(layers), dt)}
    for L in layers:
        sp = L.spec
        per_img = sp.IC * sp.H * sp.H * args.a_bits // 8
        xp = L.xp[: n_img * per_img].cpu().numpy()
        xd = np.array([args.a_bits, 1 if L.x_sign else 0, n_img, sp.IC, sp.H, sp.H], np.int32)
        wd = np.array([args.w_bits, 1, sp.OC, sp.IC, sp.K, sp.K], np.int32)
        work.append((xp, xd, L.sx.cpu().numpy(), L.zx.cpu().numpy(), L.wp.cpu().numpy(), wd,
                     L.sw.cpu().numpy(), L.zw.cpu().numpy(),
                     None if L.bias is None else L.bias.cpu().numpy(), sp.stride, sp.pad))
    t0 = time.perf_counter()
    for w in work:
        oracle.quantconv2d(*w, mode="fp32")
    dt = time.perf_counter() - t0
    return {"value": n_img / dt, "unit": "images/s", "cores": threads, "threads": threads, "kind": "port",
            "sample": "%d images through all %d conv layers (oracle/qe_oracle.c, OpenMP over outputs), %.1f s"
                      % (n_img, len(layers), dt)}


def dump_outputs(out_dir, layers, mb_layers, logits, pred, torch):
    """--dump-outputs: the results of the last timed step as float32 .npy files.  A layer's output is written whole when it
    fits its share of DUMP_BUDGET_BYTES, otherwise as a sorted sample of flat positions drawn from a CPU generator seeded by
    the layer's index: the positions depend only on the arguments, so two builds' dumps compare element for element."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    extras = {"logits": logits.float(), "pred": pred.float()}
    share = max(1, (DUMP_BUDGET_BYTES - sum(4 * t.numel() for t in extras.values())) // (4 * len(layers)))
    for i, L in enumerate(layers):
        parts = [m[i] for m in mb_layers] if mb_layers else [L]
        if getattr(L, "out_q", None) is not None:       # --fused-requant: the packed 8-bit codes the caller receives
            y = torch.cat([p.out_q for p in parts]).float()
        else:
            y = torch.cat([p.out for p in parts])
        if y.numel() > share:
            g = torch.Generator().manual_seed(DUMP_SEED + L.idx)
            pos = torch.randint(y.numel(), (share,), generator=g).sort().values
            y = y.reshape(-1)[pos.to(y.device)]
        np.save(os.path.join(out_dir, "%02d_%s.npy" % (L.idx, L.spec.name)), y.cpu().numpy())
    for name, t in extras.items():
        np.save(os.path.join(out_dir, name + ".npy"), t.cpu().numpy())


def main():
    args = parse_args()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if args.gpus > 1:
            sys.exit("bench.py --gpus %d must be launched with torch.distributed.run --nproc-per-node %d "
                     "(WORLD_SIZE=%d)" % (args.gpus, args.gpus, world))
    import torch
    import torch.distributed as dist
    from quantize_amd import capi, resnet50
    from quantize_amd import dist as qdist

    assert torch.cuda.is_available(), "bench.py needs a GPU (no CPU fallback exists)"
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    specs = resnet50.conv_layers()
    if args.layers:
        keep = [int(v) for v in args.layers.split(",")]
        specs = [specs[i] for i in keep]
    N = args.batch
    if args.fused_requant:
        assert not args.float_input and not args.per_call_prepare and args.a_bits == 8, "--fused-requant: W8A8-style packed path"
        import copy
        args_last = copy.copy(args)
        args_last.fused_requant = False      # the last conv feeds the fp32 classifier head, not a quantiser
    layers = [Layer(i, sp, N, dev, args_last if (args.fused_requant and i == len(specs) - 1) else args, rank, capi, resnet50, torch)
              for i, sp in enumerate(specs)]

    # top-1 tail: avg-pool + synthetic fc on the last conv output, identical weights on every rank
    g = torch.Generator(device=dev)
    g.manual_seed(4242)
    last = layers[-1]
    fc_w = torch.randn(1000, last.spec.OC, generator=g, device=dev) * 0.02

    stream = torch.cuda.Stream(device=dev)
    sp = ctypes.c_void_p(stream.cuda_stream)

    M = args.microbatches
    if M > 1:
        assert N % M == 0 and not args.graph and not args.fused_requant
        # micro-batch m = its own operands of N / M images per layer and its own stream; `layers` (whole batch) is kept for
        # the tail and the byte counts
        mb_layers = [[Layer(i, spc, N // M, dev, args, rank, capi, resnet50, torch) for i, spc in enumerate(specs)] for _ in range(M)]
        mb_streams = [torch.cuda.Stream(device=dev) for _ in range(M)]
        mb_sp = [ctypes.c_void_p(st.cuda_stream) for st in mb_streams]
        mb_ev = [torch.cuda.Event() for _ in range(M)]
        fork_ev = torch.cuda.Event()

    LS = args.layer_streams
    if LS > 1:
        assert M == 1 and not args.graph
        ls_streams = [torch.cuda.Stream(device=dev) for _ in range(LS)]
        ls_sp = [ctypes.c_void_p(st.cuda_stream) for st in ls_streams]
        ls_ev = [torch.cuda.Event() for _ in range(LS)]
        ls_fork = torch.cuda.Event()
    if M > 1 and args.mb_stagger:
        stag_ev = [torch.cuda.Event() for _ in range(M)]

    BR = args.branch_streams
    if BR:
        assert M == 1 and LS == 1 and not args.graph and not args.layers
        br_stream = torch.cuda.Stream(device=dev)
        br_sp = ctypes.c_void_p(br_stream.cuda_stream)
        br_fork = [torch.cuda.Event() for _ in range(4)]
        br_join = [torch.cuda.Event() for _ in range(4)]
        names = [L.spec.name for L in layers]

    def step():
        if BR:
            k = 0
            for i, L in enumerate(layers):
                nm = names[i]
                if nm.endswith(".0.conv1"):
                    br_fork[k].record(stream)            # the block's input is ready
                    br_stream.wait_event(br_fork[k])
                    layers[names.index(nm[:-5] + "downsample")].run(br_sp)
                    br_join[k].record(br_stream)
                if nm.endswith(".downsample"):
                    stream.wait_event(br_join[k])        # the block's end: residual add needs both branches
                    k += 1
                    continue
                L.run(sp)
            return
        if LS > 1:
            ls_fork.record(stream)
            for s_ in ls_streams:
                s_.wait_event(ls_fork)
            for i, L in enumerate(layers):
                L.run(ls_sp[i % LS])
            for m in range(LS):
                ls_ev[m].record(ls_streams[m])
                stream.wait_event(ls_ev[m])
            return
        if M > 1:
            fork_ev.record(stream)
            for m in range(M):
                mb_streams[m].wait_event(fork_ev)
            K = args.mb_stagger
            for i in range(len(specs) + K * (M - 1)):   # interleaved issue order; each stream stays in order
                for m in range(M):
                    li = i - m * K
                    if li < 0 or li >= len(specs):
                        continue
                    if K and m > 0 and li == 0:         # micro-batch m starts when micro-batch m-1 has finished K layers
                        mb_streams[m].wait_event(stag_ev[m - 1])
                    mb_layers[m][li].run(mb_sp[m])
                    if K and li == K - 1 and m + 1 < M:
                        stag_ev[m].record(mb_streams[m])
            for m in range(M):
                mb_ev[m].record(mb_streams[m])
                stream.wait_event(mb_ev[m])
            return
        for L in layers:
            L.run(sp)

    def tail():
        if last.out.shape[2] * last.out.shape[3] <= 240:
            feats = capi.global_avgpool(last.out)   # on the current stream; torch's mean(dim=(2,3)) takes 70 us here (1.5 TB/s)
        else:                                       # --layers debug subsets ending on a large map
            feats = last.out.mean(dim=(2, 3))
        logits = feats @ fc_w.t()
        logits = qdist.gather_logits(logits, equal_shards=True) if world > 1 else logits
        return logits, logits.argmax(dim=1)

    # --graph: capture the kernel launches of a step (53 convs + 2 gathers; + the weight preps with --per-call-prepare) once into a hipGraph and
    # replay it per step (same kernels, arguments and stream order; only the per-launch dispatch gaps go).
    graph = None
    launch_mode = "eager C-ABI calls"
    if M > 1:
        launch_mode_mb = "eager C-ABI calls, %d micro-batches of %d images on %d streams" % (M, N // M, M)
        with torch.cuda.stream(stream):
            layers[-1].run(sp)                 # the tail's input
    with torch.cuda.stream(stream):
        if args.graph:
            step()                   # first calls outside capture (lazy one-time attribute setup in the library)
            logits, pred = tail()
            stream.synchronize()
            try:
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=stream):
                    step()
                launch_mode = "hipGraph replay of the captured layer calls"
            except Exception as e:   # capture unsupported here: say so and run eagerly
                print("hipGraph capture failed (%s); eager launches" % (e,), file=sys.stderr)
                graph = None
    run_step = graph.replay if graph is not None else step
    if M > 1:
        launch_mode = launch_mode_mb + (", staggered by %d layers" % args.mb_stagger if args.mb_stagger else "")
    if BR:
        launch_mode = "eager C-ABI calls, the 4 downsample branches on a second stream beside conv1..3 of their block"
    if LS > 1:
        launch_mode = "DIAGNOSTIC: layer i on stream i %% %d (independent problems co-scheduled)" % LS

    with torch.cuda.stream(stream):
        for _ in range(args.warmup):
            run_step()
            logits, pred = tail()
        stream.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        ev0 = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps)]
        ev1 = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps)]
        t0 = time.perf_counter()
        for k in range(args.steps):
            ev0[k].record(stream)
            run_step()
            ev1[k].record(stream)
            logits, pred = tail()
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        t1 = time.perf_counter()
    elapsed = t1 - t0
    if world > 1:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    assert pred.numel() == N * world
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, layers, mb_layers if M > 1 else None, logits, pred, torch)

    conv_ms = sum(a.elapsed_time(b) for a, b in zip(ev0, ev1)) / args.steps
    total_bytes = sum(L.bytes for L in layers)
    total_ops = sum(L.ops for L in layers)
    n_launch = len(layers)
    achieved_gbs = total_bytes / (conv_ms * 1e-3) / 1e9

    per_layer = None
    if args.per_layer and rank == 0:
        per_layer = []
        reps = 5
        with torch.cuda.stream(stream):
            flush = torch.empty(1 << 28, dtype=torch.float32, device=dev) if args.cold else None
            for L in layers:
                L.run(sp)
                if args.cold:
                    ms = 0.0
                    for _ in range(reps):
                        flush.fill_(1.0)
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record(stream)
                        L.run(sp)
                        b.record(stream)
                        stream.synchronize()
                        ms += a.elapsed_time(b) / reps
                else:
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(stream)
                    for _ in range(reps):
                        L.run(sp)
                    b.record(stream)
                    stream.synchronize()
                    ms = a.elapsed_time(b) / reps
                per_layer.append({"i": L.idx, "name": L.spec.name,
                                  "shape": [L.spec.IC, L.spec.OC, L.spec.K, L.spec.stride, L.spec.pad, L.spec.H],
                                  "path": "mfma" if L.path else "generic", "ms": round(ms, 4),
                                  "GBs": round(L.bytes / ms / 1e6, 1), "TOPs": round(L.ops / ms / 1e9, 1),
                                  "hbm_frac": round(L.bytes / ms / 1e6 / HBM_PEAK_GBS, 3),
                                  "mfma_frac": round(L.ops / ms / 1e9 / INT8_MFMA_PEAK_TOPS, 3)})
        os.makedirs(os.path.join(REPO, "gpurun_out"), exist_ok=True)
        with open(os.path.join(REPO, "gpurun_out", "per_layer.json"), "w") as f:
            json.dump(per_layer, f, indent=1)
        tot = sum(p["ms"] for p in per_layer)
        for p in per_layer:
            print("%2d %-22s %-26s %-7s %8.4f ms %7.1f GB/s (%.2f) %7.1f TOP/s (%.2f)" % (
                p["i"], p["name"], p["shape"], p["path"], p["ms"], p["GBs"], p["hbm_frac"], p["TOPs"], p["mfma_frac"]),
                file=sys.stderr)
        print("sum of isolated layer times: %.3f ms" % tot, file=sys.stderr)

    if rank == 0:
        # HBM bytes per launch come from separate rocprofv3 --pmc passes (tools/profile_round.sh); the file records
        # the fingerprint of the kernel sources it was measured at and the number is reported only while the sources
        # are still those -- otherwise null, never a stale figure.
        traffic, traffic_tag = None, None
        slug = None
        if not args.layers and N == 256 and not args.two_pass and not args.per_call_prepare:
            if args.float_input and args.w_bits == 8:
                slug = "_float_input"
            elif args.fused_requant and args.w_bits == 8 and args.a_bits == 8 and not args.asymmetric:
                slug = "_fused_requant"
            elif args.w_bits == 4 and args.a_bits == 4 and not args.asymmetric:
                slug = "_w4a4"
            elif args.w_bits == 8 and args.a_bits == 8:
                slug = "_asymmetric" if args.asymmetric else ""
        tpath = os.path.join(REPO, "profiles", "traffic%s.json" % (slug or ""))
        if slug is not None and os.path.exists(tpath):
            try:
                from quantize_amd.build import source_sha16
                tj = json.load(open(tpath))
                if tj.get("source_sha16") == source_sha16():
                    traffic, traffic_tag = tj.get("hbm_bytes_per_launch"), tj.get("tag")
            except Exception:
                traffic = None
        result = {
            "metric": ("quant-conv2d images/sec at batch 256 (ResNet-50, W%dA%d)" % (args.w_bits, args.a_bits)) if not args.float_input
                      else "quantconv2d_float_input images/sec at batch 256 (ResNet-50, W%d, fp32 activations)" % args.w_bits,
            "value": N * world * args.steps / elapsed,
            "unit": "images/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16x3 (exact split of f32) x int codes, f32 accumulate" if args.float_input else "int8",
            "data": "synthetic",
            "config": {"workload": ("ResNet-50 conv stack (53 convs), W%dA%d packed-int quantconv2d, "
                                    "NCHW (256,3,224,224) per GPU, fp32 NCHW outputs" % (args.w_bits, args.a_bits)) if not args.float_input
                                   else "ResNet-50 conv stack (53 convs), quantconv2d_float_input: fp32 NCHW activations x packed W%d weights, "
                                        "fp32 NCHW outputs" % args.w_bits,
                       "batch_per_gpu": N, "global_batch": N * world,
                       "parallelism": "batch-sharded x%d, all-gather of logits" % world,
                       "launch": launch_mode,
                       "weights": "re-laid-out inside every call" if args.per_call_prepare else
                                  "prepared once per layer at set-up (qe_conv_prepare), packed activations per call",
                       "layers": n_launch, "kernel_paths": {"mfma": sum(L.path for L in layers),
                                                            "generic": sum(1 - L.path for L in layers)}},
            "roofline": {"bound": "hbm",
                         "kernel": ("conv_f32_mfma_kernel + conv_f32_stem_kernel (bf16 x3 MFMA), 53 launches per step, one per layer"
                                    if args.float_input else
                                    "conv_mfma_{flat,flatg,sm2,ws,smallic,}_kernel + conv_pwr{,7}_kernel + conv_flatd_kernel: one launch per layer, 53 per step (the event span "
                                    "also holds the 2 gather launches of the strided 1x1 layers%s)"
                                    % (" and the 17 weight-prep launches" if args.per_call_prepare else "; weights prepared at set-up")),
                         "achieved": achieved_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved_gbs / HBM_PEAK_GBS,
                         "traffic": traffic,
                         "traffic_measured_at": traffic_tag,
                         "bytes_per_launch": total_bytes / n_launch,
                         "avg_launch_ms": conv_ms / n_launch,
                         "conv_stack_ms": conv_ms,
                         "int8_tops": total_ops / (conv_ms * 1e-3) / 1e12,
                         "mfma_frac": total_ops / (conv_ms * 1e-3) / 1e12 / INT8_MFMA_PEAK_TOPS},
        }
        if args.fused_requant:
            n_f = sum(1 for L in layers if getattr(L, "fused", 0))
            result["metric"] += ", fused re-quantisation (NOT the headline contract)"
            result["config"]["workload"] = ("ResNet-50 conv stack (53 convs), W%dA%d packed-int quantconv2d with the consumer's 8-bit "
                                            "activation quantiser fused into the epilogue: 1-byte NCHW codes out of 52 layers, fp32 out of "
                                            "the last; %d layers store the codes from the conv kernel itself, %d take conv + quantise-pack "
                                            "inside the call" % (args.w_bits, args.a_bits, n_f, len(layers) - 1 - n_f))
            result["roofline"]["kernel"] = "the headline's kernels with the re-quantising epilogue (flatd layers on conv_mfma_flatg_kernel)"
            result["roofline"]["note"] = "algorithmic bytes with 1 B per output element (activations in + weights + codes out)"
            if args.two_pass:
                result["metric"] = result["metric"].replace("fused re-quantisation", "re-quantisation in TWO passes (conv to fp32, then quantise+pack)")
                result["roofline"]["kernel"] = "the headline's kernels + tpack_kernel<float, 8, 1> per layer (52 more launches)"
        if world == 1 and not args.no_cpu_baseline and not args.fused_requant:
            # two legs on the box's host cores: the reference's own packed-forward FALLBACK (F.conv2d on dequantised tensors),
            # which is what north_star names, and the CPU port of the reference KERNEL (oracle) as an extra key
            result["cpu_baseline"] = cpu_fallback_baseline(layers, args, torch)
            result["cpu_baseline_port"] = cpu_baseline(layers, args, torch)
        print(json.dumps(result), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
