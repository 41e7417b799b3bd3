"""Exact-arithmetic packed WideResNets and an engine-free float64 model of the reference's packed dataflow, on the pattern of
tests/mobilenet_exact.py (tests/resnet_exact.py's helpers and quantiser arithmetic are reused; see its docstring for why exactness).

The model: a 3x3 stem, three stages of pre-activation basic blocks (bn1, ReLU, conv1 3x3, the folded bn2 as conv1's bias, ReLU,
conv2 3x3, plus the block's input or a 1x1 convShortcut of the activated input), a last BatchNorm and ReLU, the mean over the 8x8
final map (64 elements: exact in fp32) and the fc.  On top of resnet_exact's grid the unfolded BatchNorms are exact too:
bn_eps = 0, running variances in {1/4, 1, 4} and power-of-two gammas (of either sign) make alpha = gamma / sqrt(var) a power of
two, and beta and the running means lie on a 2^-4 grid, so shift = beta - mean * alpha and s * alpha + shift round nowhere."""
import re

import numpy as np
import torch
import torch.nn.functional as F

from resnet_exact import (Float64ResNet, Result, _Layer, _pack, _qrange, _quantizer_entries, calibrated_exact,  # noqa: F401
                          exact_fc_entries, images, weight_cap, PC_RATIO)

WIDTHS = (16, 32, 64)
W_CAP = 15                # |weight code| <= 15 whatever w_bits: a grid coarse enough for the mean of 64 features to be an fp32 value
BN_FIELDS = ("weight", "bias", "running_mean", "running_var")


class _BN:
    def __init__(self, sd, name, eps):
        self.name = name
        g, b, m, v = (sd[name + "." + f].detach().cpu().double().reshape(-1) for f in BN_FIELDS)
        self.params32 = tuple(sd[name + "." + f].detach().cpu().float().reshape(-1) for f in BN_FIELDS)
        self.alpha = g / torch.sqrt(v + eps)
        self.shift = b - m * self.alpha

    def __call__(self, s):
        return torch.relu(s * self.alpha.view(1, -1, 1, 1) + self.shift.view(1, -1, 1, 1))


class Float64WideResNet(Float64ResNet):
    """The reference's WideResNet on a packed state_dict, in float64 on the host.  The quantiser, the exactness assertions and
    the calibration are Float64ResNet's; the graph and the BatchNorms are this class's."""

    def __init__(self, sd, exact=True, bn_eps=None):
        """exact=False: the same arithmetic without the exactness assertions (state_dicts off the exact grid: G14), and the
        BatchNorms' default eps."""
        self.exact = exact
        self.bn_eps = (0.0 if exact else 1e-5) if bn_eps is None else bn_eps
        sd = {k: v for k, v in sd.items()}
        self.stem = _Layer(sd, "conv1", 1, 1)
        stages = {}
        for k in sd:
            m = re.match(r"block(\d+)\.layer\.(\d+)\.conv1\.w_des$", k)
            if m:
                stages.setdefault(int(m.group(1)), set()).add(int(m.group(2)))
        assert sorted(stages) == list(range(1, len(stages) + 1)) and stages, sorted(stages)
        self.blocks = []
        for S in sorted(stages):
            for B in sorted(stages[S]):
                pre = "block%d.layer.%d." % (S, B)
                s = 2 if (S > 1 and B == 0) else 1
                sc = _Layer(sd, pre + "convShortcut", s, 0) if (pre + "convShortcut.w_des") in sd else None
                self.blocks.append((pre[:-1], _BN(sd, pre + "bn1", self.bn_eps), _Layer(sd, pre + "conv1", s, 1), _Layer(sd, pre + "conv2", 1, 1), sc))
        self.bn = _BN(sd, "bn1", self.bn_eps)
        self.fc = _Layer(sd, "fc")

    def layers(self):
        out = [self.stem]
        for _, _, c1, c2, sc in self.blocks:
            out += [c1, c2] + ([sc] if sc is not None else [])
        return out + [self.fc]

    def forward(self, images, calibrate=None):
        """Result for an N x 3 x 32 x 32 batch (features: the pooled (N, C) features)."""
        self._ties, self._stats = 0, {}
        inputs = {}

        def run(L, t):
            if calibrate is not None:
                self._calibrate(L, t, calibrate.get(L.name, {}))
            inputs[L.name] = t
            return self._conv(L, self._quantize(L, t, check=self.exact)[0])

        y = run(self.stem, images.double().cpu())
        for name, bn, c1, c2, sc in self.blocks:
            a = bn(y)
            self._exact(a, name + " activated input")
            o = run(c2, torch.relu(run(c1, a)))
            y = o + (y if sc is None else run(sc, a))
            self._exact(y, name + " residual sum")
        a = self.bn(y)
        self._exact(a, "activated features")
        assert tuple(a.shape[2:]) == (8, 8), "avg_pool2d(out, 8) is the global pool only on an 8 x 8 map"
        pooled = a.sum(dim=(2, 3)) / 64
        self._exact(pooled, "pooled features")
        fc = self.fc
        if calibrate is not None:
            self._calibrate(fc, pooled, calibrate.get("fc", {}))
        inputs["fc"] = pooled
        q, v = self._quantize(fc, pooled, check=self.exact)
        # off the exact grid the engine's fp32 features differ from these in the last bits: an fc code may then round either way
        # when it lies this close to a .5 tie (resnet_exact's margin)
        mean_exact = pooled == pooled.float().double()
        tol = torch.clamp((v + fc.a_zero).abs() * 2.0 ** -21, min=2.0 ** -20)
        near = ((v - torch.floor(v) - 0.5).abs() <= tol) & ~mean_exact & (v > fc.qmin - 1) & (v < fc.qmax + 1)
        logits = F.linear((q + fc.a_zero) * fc.a_scale, fc.weights(), fc.bias)
        self._exact(logits, "logits")
        return Result(features=pooled, logits=logits, near_tie=near.any(dim=1), ties=self._ties, inputs=inputs, stats=dict(self._stats))


def exact_bn_entries(rng, sd, name, C):
    pow2 = lambda lo, hi: 2.0 ** rng.randint(lo, hi + 1, size=C)
    sd.update({name + ".weight": torch.from_numpy((pow2(-1, 1) * np.where(rng.uniform(size=C) < 0.2, -1.0, 1.0)).astype(np.float32)),
               name + ".bias": torch.from_numpy((rng.randint(-8, 9, size=C) / 16.0).astype(np.float32)),
               name + ".running_mean": torch.from_numpy((rng.randint(-8, 9, size=C) / 16.0).astype(np.float32)),
               name + ".running_var": torch.from_numpy((4.0 ** rng.randint(-1, 2, size=C)).astype(np.float32)),
               name + ".num_batches_tracked": torch.tensor(0, dtype=torch.int64)})


def exact_conv_entries(rng, sd, name, IC, OC, K, gain, spec, w_bits, a_bits, signed_in=False):
    """resnet_exact.exact_conv_entries with the weight codes capped at W_CAP: the residual stream is never re-quantised, so the sum
    of the 64 activated features of a plane must stay below 2^24 units of the finest conv grid."""
    qmin, qmax = _qrange(a_bits, signed_in or spec.get("signed", False))
    z = float(spec.get("zero", 0))
    a_max = int(max(abs(qmin + z), abs(qmax + z))) * (PC_RATIO if spec.get("per_channel") else 1)
    cap = min(weight_cap(IC * K * K, a_max, w_bits), W_CAP)
    q = rng.randint(-cap, cap + 1, size=(OC, IC, K, K))
    target = gain * np.sqrt(2.0 / (IC * K * K)) / (cap / np.sqrt(3.0))                   # He-scaled
    ws = 2.0 ** (np.round(np.log2(target)) + rng.randint(-1, 2, size=OC))                 # powers of two, differing per channel
    sd.update({name + ".weight": _pack(q, w_bits),
               name + ".w_des": torch.tensor([w_bits, 1, OC, IC, K, K], dtype=torch.int32),
               name + ".w_scale": torch.from_numpy(ws.astype(np.float32).reshape(OC, 1, 1, 1)),
               name + ".w_zero": torch.zeros((OC, 1, 1, 1), dtype=torch.float32),
               name + ".bias": torch.from_numpy(rng.normal(0, 0.05, size=OC).astype(np.float32))})
    _quantizer_entries(sd, name, qmin, qmax, z)


def exact_state_dict(w_bits=8, a_bits=8, seed=0, depth=16, widen=1, num_classes=10, calib_images=None, variants=None):
    """A packed WideResNet state_dict (the key layout of quantize_amd.packed_wideresnet.synthetic_state_dict) with exact fp32
    arithmetic under bn_eps = 0, calibrated on Float64WideResNet.  variants = {layer name: spec} as
    resnet_exact.exact_state_dict: signed, zero, per_channel, scale_mult."""
    variants = variants or {}
    rng = np.random.RandomState(seed)
    sd = {}

    def conv(name, IC, OC, K, gain=1.0, signed_in=False, bias=False):
        exact_conv_entries(rng, sd, name, IC, OC, K, gain, variants.get(name, {}), w_bits, a_bits, signed_in)
        if not bias:
            del sd[name + ".bias"]

    conv("conv1", 3, 16, 3, signed_in=True)
    C = 16
    for S, width in enumerate(WIDTHS, start=1):
        planes = width * widen
        for B in range((depth - 4) // 6):
            pre = "block%d.layer.%d" % (S, B)
            exact_bn_entries(rng, sd, pre + ".bn1", C)
            conv(pre + ".conv1", C, planes, 3, bias=True)
            conv(pre + ".conv2", planes, planes, 3, gain=0.3)
            if C != planes:
                conv(pre + ".convShortcut", C, planes, 1)
            C = planes
    exact_bn_entries(rng, sd, "bn1", C)
    exact_fc_entries(rng, sd, num_classes, C, variants.get("fc", {}), w_bits, a_bits)
    return calibrated_exact(Float64WideResNet(sd), sd, calib_images, 2, 32, seed, variants)


def fp32_packed_forward(sd, x, bn_eps=0.0):
    """The reference's packed forward in fp32 on the host: every Quant module quantises its input (round(x / s - z).clamp),
    dequantises (q + z) * s and calls F.conv2d / F.linear on the dequantised weights; the unfolded BatchNorms are ATen's
    eval-mode batch_norm; all fp32.  Returns (pooled features, logits)."""
    m = Float64WideResNet(sd, bn_eps=bn_eps)
    y = x.float().cpu()

    def deq_in(L, t):
        s, z = L.a_view(L.a_scale.float(), t), L.a_view(L.a_zero.float(), t)
        return ((t / s - z).round().clamp(L.qmin, L.qmax) + z) * s

    def w32(L):
        shape = [-1] + [1] * (L.w_codes.dim() - 1)
        return (L.w_codes.float() + L.w_zero.float().view(shape)) * L.w_scale.float().view(shape)

    def conv(L, t):
        return F.conv2d(deq_in(L, t), w32(L), None if L.bias is None else L.bias.float(), L.stride, L.padding)

    def bn(b, t):
        g, beta, mean, var = b.params32
        return torch.relu(torch.batch_norm(t, g, beta, mean, var, False, 0.0, bn_eps, False))      # F.batch_norm refuses eps = 0

    y = conv(m.stem, y)
    for _, b, c1, c2, sc in m.blocks:
        a = bn(b, y)
        y = torch.add(y if sc is None else conv(sc, a), conv(c2, torch.relu(conv(c1, a))))
    pooled = F.avg_pool2d(bn(m.bn, y), 8).flatten(1)
    fc = m.fc
    return pooled, F.linear(deq_in(fc, pooled), w32(fc), None if fc.bias is None else fc.bias.float())
