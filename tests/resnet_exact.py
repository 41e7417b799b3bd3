"""Exact-arithmetic packed ResNets and an engine-free float64 model of the reference's packed dataflow.

Quantisation is discontinuous: one fp32 rounding difference flips a code and the flip runs through every later layer, so a
float64 model matches an fp32 engine only loosely on arbitrary weights.  The packed ResNets built here are chosen so that
fp32 makes no rounding at all:

  * every scale is a power of two (x / s, (q + z) * s and every product are exact), weight scales per output channel and
    different between channels, activation scales per tensor (per channel on chosen consumers);
  * zero points are integers;
  * each bias is an integer number of its output channel's grid units s_x * s_w[oc];
  * K * max|q_x + z_x| * max|q_w + z_w| + |bias units| < 2^24 for every conv and the fc (K = IC * KH * KW), so every
    partial sum, in any summation order, is an integer below 2^24 grid units: exact in fp32.

Then the engine (both routes of PackedResNet), the reference's fp32 packed forward and Float64ResNet below must agree bit
for bit.  Float64ResNet asserts that exactness on every intermediate it computes, counts the exact .5 ties its quantisers
meet (round half to even decides them), and imports nothing from the engine: it reads only the state_dict, unpacking the
weight codes with the C oracle.  The quantiser is the reference's (modelzoo/modules/quantizer.py:31,215):
q = round(x / s - z).clamp(qmin, qmax), dequantised as (q + z) * s.
"""
import os
import re

import numpy as np
import torch
import torch.nn.functional as F

import oracle

TWO24 = 1 << 24
BIAS_UNITS = 1 << 12          # |bias| in its grid units: part of the 2^24 budget
PC_RATIO = 4                  # per-channel activation scales lie in [s_tensor / PC_RATIO, s_tensor]
ARCHS = {"resnet18": ("basic", [2, 2, 2, 2]), "resnet50": ("bottleneck", [3, 4, 6, 3])}


class NotExact(AssertionError):
    pass


def _pow2_ceil(v):
    return float(2.0 ** np.ceil(np.log2(v)))


def _qrange(bits, signed):
    return (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if signed else (0, (1 << bits) - 1)


def weight_cap(K, a_max, w_bits, bias_units=BIAS_UNITS):
    """The largest |weight code| with K * a_max * cap + bias_units < 2^24 (and within w_bits)."""
    cap = min((1 << (w_bits - 1)) - 1, (TWO24 - 1 - bias_units) // (K * a_max))
    assert cap >= 1, "no weight code fits the 2^24 budget at K=%d" % K
    assert K * a_max * cap + bias_units < TWO24
    return int(cap)


# ---------------------------------------------------------------------------------------------
# The float64 model
# ---------------------------------------------------------------------------------------------
class _Layer:
    """One packed conv or linear as float64 host tensors: the weights dequantised from the unpacked codes, the activation
    quantiser, the bias and the geometry."""

    def __init__(self, sd, name, stride=1, padding=0):
        g = lambda k: sd[name + "." + k].detach().cpu()
        self.name, self.stride, self.padding = name, stride, padding
        des = g("w_des").numpy().astype(np.int64)
        codes = oracle.tunpack(g("weight").numpy(), des).astype(np.float64)
        self.w_bits, self.w_sign = int(des[0]), bool(des[1])
        self.w_codes = torch.from_numpy(codes)
        self.w_scale = g("w_scale").double().reshape(-1)
        self.w_zero = g("w_zero").double().reshape(-1)
        self.bias = g("bias").double().reshape(-1) if (name + ".bias") in sd else None
        self.a_scale = g("a_quantizer.scale").double().reshape(-1)
        self.a_zero = g("a_quantizer.zero").double().reshape(-1)
        self.qmin, self.qmax = float(g("a_quantizer.qmin")), float(g("a_quantizer.qmax"))
        self.K = int(np.prod(des[3:]))

    def weights(self):
        shape = [-1] + [1] * (self.w_codes.dim() - 1)
        return (self.w_codes + self.w_zero.view(shape)) * self.w_scale.view(shape)

    def a_view(self, t, x):
        shape = [1] * x.dim()
        if t.numel() > 1:
            shape[1] = -1
        return t.view(shape)


class Result:
    """features (layer4 output), logits, per-image near_tie flags of the fc codes, the number of exact .5 ties met, the fp32
    input of every conv (name -> tensor, forward order) and per-quantiser code statistics."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class Float64ResNet:
    """torchvision's ResNet on a packed state_dict, in float64 on the host: stem conv 7x7 / 2 pad 3, ReLU, maxpool 3 / 2 / 1;
    in a stage's first block the stride sits on the Bottleneck's conv2 (the BasicBlock's conv1) and on the downsample; each
    block ends with relu(conv + identity); then adaptive average pooling and the fc through its own quantiser."""

    def __init__(self, sd, exact=True):
        """exact=False: the same arithmetic without the exactness assertions (state_dicts off the exact grid: G11, G12)."""
        self.exact = exact
        sd = {k: v for k, v in sd.items()}
        self.stem = _Layer(sd, "conv1", 2, 3)
        stages = self._stages(sd)
        self.bottleneck = 3 in next(iter(stages[1].values()))
        self.blocks = []
        for S in sorted(stages):
            for B in sorted(stages[S]):
                pre = "layer%d.%d." % (S, B)
                s = 2 if (S > 1 and B == 0) else 1
                if self.bottleneck:
                    convs = [_Layer(sd, pre + "conv1", 1, 0), _Layer(sd, pre + "conv2", s, 1), _Layer(sd, pre + "conv3", 1, 0)]
                else:
                    convs = [_Layer(sd, pre + "conv1", s, 1), _Layer(sd, pre + "conv2", 1, 1)]
                ds = _Layer(sd, pre + "downsample.0", s, 0) if (pre + "downsample.0.w_des") in sd else None
                self.blocks.append((pre[:-1], convs, ds))
        self.fc = _Layer(sd, "fc")

    @staticmethod
    def _stages(sd):
        """{stage: {block: the conv numbers it has}} of the keys layerS.B.convN.w_des; the stages must be 1..n."""
        stages = {}
        for k in sd:
            m = re.match(r"layer(\d+)\.(\d+)\.conv(\d)\.w_des$", k)
            if m:
                stages.setdefault(int(m.group(1)), {}).setdefault(int(m.group(2)), set()).add(int(m.group(3)))
        assert sorted(stages) == list(range(1, len(stages) + 1)) and stages, sorted(stages)
        return stages

    def layers(self):
        out = [self.stem]
        for _, convs, ds in self.blocks:
            out += convs + ([ds] if ds is not None else [])
        return out + [self.fc]

    # ---- the arithmetic ----
    def _exact(self, t, what):
        if self.exact and not torch.equal(t, t.float().double()):
            bad = (t != t.float().double()).nonzero()[0].tolist()
            raise NotExact("%s is not exact in fp32 (first at %s: %r)" % (what, bad, float(t[tuple(bad)])))

    def _quantize(self, L, x, check=True):
        v = x / L.a_view(L.a_scale, x) - L.a_view(L.a_zero, x)
        if check:
            self._exact(v, L.name + " input x / s - z")
        r = torch.round(v)                                   # half to even, as torch.round in the reference
        inside = (r >= L.qmin) & (r <= L.qmax)
        self._ties += int(((v - torch.floor(v)) == 0.5)[inside].sum()) if check else 0
        q = r.clamp(L.qmin, L.qmax)
        self._stats[L.name] = (float((q == q.min()).double().mean()), float(q.min()), float(q.max()), L.qmin, L.qmax)
        return q, v

    def _conv(self, L, q):
        x = (q + L.a_view(L.a_zero, q)) * L.a_view(L.a_scale, q)
        y = F.conv2d(x, L.weights(), L.bias, L.stride, L.padding, 1, getattr(L, "groups", 1))
        self._exact(y, L.name + " output")
        return y

    def _calibrate(self, L, x, spec):
        """Activation scale by max, rounded up to a power of two (times spec['scale_mult']); per channel when asked, kept in
        [s_tensor / PC_RATIO, s_tensor]; then the bias snapped to its grid."""
        z = float(L.a_zero.reshape(-1)[0])
        dims = [d for d in range(x.dim()) if d != 1]

        def need(hi, lo):
            s = torch.full_like(hi, 2.0 ** -24)
            s = torch.maximum(s, torch.where(hi > 0, hi / (L.qmax + z), s))
            if L.qmin + z < 0:
                s = torch.maximum(s, torch.where(lo < 0, lo / (L.qmin + z), s))
            return s
        s_t = _pow2_ceil(float(need(x.max().reshape(1), x.min().reshape(1)))) * spec.get("scale_mult", 1.0)
        if spec.get("per_channel"):
            s = need(x.amax(dim=dims), x.amin(dim=dims)).clamp(min=s_t / PC_RATIO, max=s_t)
            s = torch.tensor([_pow2_ceil(float(v)) for v in s], dtype=torch.float64).clamp(max=s_t)
            L.a_zero = L.a_zero.reshape(-1)[:1].repeat(s.numel())
        else:
            s = torch.tensor([s_t], dtype=torch.float64)
        L.a_scale = s
        if L.bias is not None:
            g = s.min() * L.w_scale
            L.bias = torch.round(L.bias / g).clamp(-BIAS_UNITS, BIAS_UNITS) * g

    def forward(self, images, calibrate=None):
        """Result for an N x 3 x H x W batch.  calibrate={name: spec} sets every activation scale (and snaps every bias)
        from this batch as it goes; spec keys: per_channel, scale_mult."""
        self._ties, self._stats = 0, {}
        inputs = {}

        def run(L, t):
            if calibrate is not None:
                self._calibrate(L, t, calibrate.get(L.name, {}))
            inputs[L.name] = t
            return self._conv(L, self._quantize(L, t)[0])

        y = F.max_pool2d(torch.relu(run(self.stem, images.double().cpu())), 3, 2, 1)
        for name, convs, ds in self.blocks:
            identity = run(ds, y) if ds is not None else y
            o = y
            for c in convs[:-1]:
                o = torch.relu(run(c, o))
            y = torch.relu(run(convs[-1], o) + identity)
            self._exact(y, name + " residual sum")
        feat = y
        P = feat.shape[2] * feat.shape[3]
        pooled = feat.sum(dim=(2, 3)) / P
        exact_pool = (P & (P - 1)) == 0
        if exact_pool:
            self._exact(pooled, "pooled features")
        fc = self.fc
        if calibrate is not None:
            self._calibrate(fc, pooled, calibrate.get("fc", {}))
        inputs["fc"] = pooled
        q, v = self._quantize(fc, pooled, check=exact_pool)
        # the engine's mean is fp32 (sum / P, correctly rounded): an element whose float64 mean is not an fp32 value may
        # round either way when it lies this close to a .5 tie (two fp32 roundings of |v + z| at most, with margin)
        mean_exact = pooled == pooled.float().double()
        tol = torch.clamp((v + fc.a_zero).abs() * 2.0 ** -21, min=2.0 ** -20)
        near = ((v - torch.floor(v) - 0.5).abs() <= tol) & ~mean_exact & (v > fc.qmin - 1) & (v < fc.qmax + 1)
        logits = F.linear((q + fc.a_zero) * fc.a_scale, fc.weights(), fc.bias)
        self._exact(logits, "logits")
        return Result(features=feat, logits=logits, near_tie=near.any(dim=1), ties=self._ties, inputs=inputs,
                      stats=dict(self._stats))

    def write_back(self, sd):
        """The calibrated activation scales / zeros and the snapped biases into a state_dict (fp32, as pack() stores them)."""
        for L in self.layers():
            sd[L.name + ".a_quantizer.scale"] = L.a_scale.float().reshape(sd[L.name + ".a_quantizer.scale"].shape
                                                                          if L.a_scale.numel() == 1 else (-1,))
            sd[L.name + ".a_quantizer.zero"] = L.a_zero.float().reshape(sd[L.name + ".a_quantizer.zero"].shape
                                                                        if L.a_zero.numel() == 1 else (-1,))
            if L.bias is not None:
                sd[L.name + ".bias"] = L.bias.float()
        return sd


def check_code_spread(result):
    """Guard against a degenerate construction: every quantiser's codes use a real part of its range."""
    for name, (frac_min, lo, hi, qmin, qmax) in result.stats.items():
        assert frac_min < 0.9, "%s: %.0f%% of the codes are the minimum" % (name, 100 * frac_min)
        assert hi - lo >= (qmax - qmin) / 4, "%s: codes span only [%g, %g] of [%g, %g]" % (name, lo, hi, qmin, qmax)


# ---------------------------------------------------------------------------------------------
# The exact state_dict
# ---------------------------------------------------------------------------------------------
def _pack(q, bits):
    return torch.from_numpy(oracle.tpack(np.asarray(q, dtype=np.int64), bits, True)[0].copy())


def images(n, size, seed):
    """A seeded N x 3 x size x size batch (size: one side, or (H, W))."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    H, W = (size, size) if isinstance(size, int) else size
    return torch.randn(n, 3, H, W, generator=g)


def _quantizer_entries(sd, name, qmin, qmax, z):
    sd.update({name + ".a_quantizer.scale": torch.tensor([1.0], dtype=torch.float32),
               name + ".a_quantizer.zero": torch.tensor([z], dtype=torch.float32),
               name + ".a_quantizer.qmin": torch.tensor(float(qmin)), name + ".a_quantizer.qmax": torch.tensor(float(qmax))})


def exact_conv_entries(rng, sd, name, per_group, OC, K, gain, spec, w_bits, a_bits, signed_in=False):
    """The entries of conv `name` into sd.  per_group: the input channels a weight sees (IC, IC / groups, 1 for depthwise);
    spec: the layer's variant (exact_state_dict)."""
    qmin, qmax = _qrange(a_bits, signed_in or spec.get("signed", False))
    z = float(spec.get("zero", 0))
    a_max = int(max(abs(qmin + z), abs(qmax + z))) * (PC_RATIO if spec.get("per_channel") else 1)
    cap = weight_cap(per_group * K * K, a_max, w_bits)
    q = rng.randint(-cap, cap + 1, size=(OC, per_group, K, K))
    target = gain * np.sqrt(2.0 / (per_group * K * K)) / (cap / np.sqrt(3.0))        # He-scaled
    ws = 2.0 ** (np.round(np.log2(target)) + rng.randint(-1, 2, size=OC))             # powers of two, differing per channel
    sd.update({name + ".weight": _pack(q, w_bits),
               name + ".w_des": torch.tensor([w_bits, 1, OC, per_group, K, K], dtype=torch.int32),
               name + ".w_scale": torch.from_numpy(ws.astype(np.float32).reshape(OC, 1, 1, 1)),
               name + ".w_zero": torch.zeros((OC, 1, 1, 1), dtype=torch.float32),
               name + ".bias": torch.from_numpy(rng.normal(0, 0.05, size=OC).astype(np.float32))})
    _quantizer_entries(sd, name, qmin, qmax, z)


def exact_fc_entries(rng, sd, num_classes, K, spec, w_bits, a_bits):
    """The fc's entries into sd: an unsigned quantiser behind the pooled features."""
    qmin, qmax = _qrange(a_bits, False)
    z = float(spec.get("zero", 0))
    cap = weight_cap(K, int(max(abs(qmin + z), abs(qmax + z))), w_bits)
    q = rng.randint(-cap, cap + 1, size=(num_classes, K))
    ws = 2.0 ** (np.round(np.log2(np.sqrt(1.0 / K) / cap)) + rng.randint(-1, 2, size=(num_classes, 1)))
    sd.update({"fc.weight": _pack(q, w_bits),
               "fc.w_des": torch.tensor([w_bits, 1, num_classes, K], dtype=torch.int32),
               "fc.w_scale": torch.from_numpy(ws.astype(np.float32)),
               "fc.w_zero": torch.zeros((num_classes, 1), dtype=torch.float32),
               "fc.bias": torch.from_numpy(rng.normal(0, 0.05, size=num_classes).astype(np.float32))})
    _quantizer_entries(sd, "fc", qmin, qmax, z)


def exact_state_dict(arch="resnet50", w_bits=8, a_bits=8, seed=0, width=64, num_classes=1000, calib_images=None,
                     image_size=224, variants=None):
    """A packed ResNet state_dict in synthetic_state_dict's key layout with exact fp32 arithmetic (module docstring),
    calibrated on Float64ResNet at image_size (one side, or (H, W)).  variants = {layer name: spec} changes one consumer's activation quantiser:
      signed=True        qmin / qmax signed (no ReLU fold);
      zero=<int>         a non-zero integer zero point;
      per_channel=True   per-channel activation scales;
      scale_mult=2.0     the calibrated scale times a power of two (a downsample quantiser differing from conv1's).
    Returns the state_dict (host tensors)."""
    variants = variants or {}
    kind, depth = ARCHS[arch]
    rng = np.random.RandomState(seed)
    sd = {}

    def conv(name, IC, OC, K, gain, signed_in=False):
        exact_conv_entries(rng, sd, name, IC, OC, K, gain, variants.get(name, {}), w_bits, a_bits, signed_in)

    conv("conv1", 3, width, 7, 1.0, signed_in=True)
    inplanes, exp = width, (4 if kind == "bottleneck" else 1)
    for S, nb in enumerate(depth, start=1):
        planes = width * (1 << (S - 1))
        for B in range(nb):
            pre = "layer%d.%d" % (S, B)
            if kind == "bottleneck":
                conv(pre + ".conv1", inplanes, planes, 1, 1.0)
                conv(pre + ".conv2", planes, planes, 3, 1.0)
                conv(pre + ".conv3", planes, planes * 4, 1, 0.3)
            else:
                conv(pre + ".conv1", inplanes, planes, 3, 1.0)
                conv(pre + ".conv2", planes, planes, 3, 0.3)
            if B == 0 and (S > 1 or inplanes != planes * exp):
                conv(pre + ".downsample.0", inplanes, planes * exp, 1, 1.0)
            inplanes = planes * exp
    exact_fc_entries(rng, sd, num_classes, inplanes, variants.get("fc", {}), w_bits, a_bits)
    return calibrated_exact(Float64ResNet(sd), sd, calib_images, 2, image_size, seed, variants)


def calibrated_exact(model, sd, calib_images, n, image_size, seed, variants):
    """sd with the scales, zeros and snapped biases of `model` (built on sd) calibrated on calib_images, or on n seeded ones."""
    model.forward(images(n, image_size, seed + 1) if calib_images is None else calib_images, calibrate=variants)
    return model.write_back(sd)


# ---------------------------------------------------------------------------------------------
# G8: whole packed ResNets written by the reference's own modules (oracle/gen_golden.py gen_g8)
# ---------------------------------------------------------------------------------------------
G8 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g8_resnet_module.npz")


def load_g8():
    """{case: (state_dict, images, features, logits)} -- the complete state_dict the reference wrote, as host tensors."""
    z = np.load(G8, allow_pickle=False)
    out = {}
    for key in [str(k) for k in z["index"]]:
        pre = key + "_sd_"
        sd = {k[len(pre):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre)}
        out[key] = (sd, torch.from_numpy(z[key + "_images"]), torch.from_numpy(z[key + "_features"]),
                    torch.from_numpy(z[key + "_logits"]))
    return out
