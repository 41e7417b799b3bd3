"""Exact-arithmetic packed MobileNetV1s and an engine-free float64 model of the reference's packed dataflow, on the pattern of
tests/resnet_exact.py (whose helpers and quantiser arithmetic this module reuses; see its docstring for why exactness).

The model: a 3x3 stride-2 stem, five stages of (depthwise 3x3, pointwise 1x1) blocks with a ReLU behind every convolution
(stride 2 on the first depthwise layer of stages 2..5), global average pooling, fc.  Width 8 (channel counts 8 .. 256) and
32x32 or 64x64 images: the final planes are 1x1 or 2x2, so the mean is exact in fp32 and every image takes part in the logit
comparison.  Every scale is a power of two, zero points are integers, biases lie on their grids, and
K * max|q_x + z_x| * max|q_w + z_w| + |bias units| < 2^24 with K = 9 for a depthwise layer."""
import numpy as np
import torch
import torch.nn.functional as F

from resnet_exact import (BIAS_UNITS, PC_RATIO, Float64ResNet, Result, _Layer, _pack, _qrange, calibrated_exact,  # noqa: F401
                          exact_conv_entries, exact_fc_entries, images, weight_cap)

DEPTH = (1, 2, 2, 6, 2)


class Float64MobileNetV1(Float64ResNet):
    """The reference's MobileNetV1 on a packed state_dict, in float64 on the host.  The quantiser, the exactness assertions
    and the calibration are Float64ResNet's; the graph is this class's."""

    def __init__(self, sd, exact=True):
        """exact=False: the same arithmetic without the exactness assertions (state_dicts off the exact grid: G11)."""
        self.exact = exact
        sd = {k: v for k, v in sd.items()}
        self.stem = _Layer(sd, "conv1", 2, 1)
        stages = self._stages(sd)
        self.blocks = []
        for S in sorted(stages):
            for B in sorted(stages[S]):
                pre = "layer%d.%d." % (S, B)
                dw = _Layer(sd, pre + "conv1", 2 if (S > 1 and B == 0) else 1, 1)
                assert dw.w_codes.shape[1] == 1, "%sconv1 is not depthwise" % pre
                dw.groups = dw.w_codes.shape[0]
                self.blocks.append((pre[:-1], dw, _Layer(sd, pre + "conv2", 1, 0)))
        self.fc = _Layer(sd, "fc")

    def layers(self):
        out = [self.stem]
        for _, dw, pw in self.blocks:
            out += [dw, pw]
        return out + [self.fc]

    def forward(self, images, calibrate=None):
        """Result for an N x 3 x H x W batch (features: the pooled (N, C) features)."""
        self._ties, self._stats = 0, {}
        inputs = {}
        y = images.double().cpu()
        for L in self.layers()[:-1]:
            if calibrate is not None:
                self._calibrate(L, y, calibrate.get(L.name, {}))
            inputs[L.name] = y
            y = torch.relu(self._conv(L, self._quantize(L, y, check=self.exact)[0]))
        P = y.shape[2] * y.shape[3]
        assert not self.exact or (P & (P - 1)) == 0, "the final plane must hold a power of two of elements for an exact mean"
        pooled = y.sum(dim=(2, 3)) / P
        self._exact(pooled, "pooled features")
        fc = self.fc
        if calibrate is not None:
            self._calibrate(fc, pooled, calibrate.get("fc", {}))
        inputs["fc"] = pooled
        q, v = self._quantize(fc, pooled, check=self.exact)
        logits = F.linear((q + fc.a_zero) * fc.a_scale, fc.weights(), fc.bias)
        self._exact(logits, "logits")
        return Result(features=pooled, logits=logits, near_tie=torch.zeros(images.shape[0], dtype=torch.bool), ties=self._ties,
                      inputs=inputs, stats=dict(self._stats))


def exact_state_dict(w_bits=8, a_bits=8, seed=0, width=8, num_classes=10, calib_images=None, image_size=32, variants=None,
                     depth=DEPTH):
    """A packed MobileNetV1 state_dict (the key layout of quantize_amd.packed_mobilenet.synthetic_state_dict) with exact fp32
    arithmetic, calibrated on Float64MobileNetV1.  variants = {layer name: spec} as resnet_exact.exact_state_dict: signed,
    zero, per_channel, scale_mult -- signed=True or a non-zero zero makes a consumer whose quantiser does not fold the ReLU."""
    variants = variants or {}
    rng = np.random.RandomState(seed)
    sd = {}

    def conv(name, IC, OC, K, signed_in=False, depthwise=False):
        exact_conv_entries(rng, sd, name, 1 if depthwise else IC, OC, K, 1.0, variants.get(name, {}), w_bits, a_bits, signed_in)

    conv("conv1", 3, width, 3, signed_in=True)
    C = width
    for S, nb in enumerate(depth, start=1):
        planes = width * (1 << S)
        for B in range(nb):
            pre = "layer%d.%d" % (S, B)
            conv(pre + ".conv1", C, C, 3, depthwise=True)
            conv(pre + ".conv2", C, planes, 1)
            C = planes
    exact_fc_entries(rng, sd, num_classes, C, variants.get("fc", {}), w_bits, a_bits)
    return calibrated_exact(Float64MobileNetV1(sd), sd, calib_images, 3, image_size, seed, variants)


def fp32_packed_forward(sd, x):
    """The reference's packed forward in fp32 on the host: every Quant module quantises its input
    (round(x / s - z).clamp), dequantises (q + z) * s and calls F.conv2d / F.linear on the dequantised weights, all fp32.
    Returns (pooled features, logits)."""
    m = Float64MobileNetV1(sd)
    y = x.float().cpu()

    def deq_in(L, t):
        s, z = L.a_view(L.a_scale.float(), t), L.a_view(L.a_zero.float(), t)
        return ((t / s - z).round().clamp(L.qmin, L.qmax) + z) * s

    def w32(L):
        shape = [-1] + [1] * (L.w_codes.dim() - 1)
        return (L.w_codes.float() + L.w_zero.float().view(shape)) * L.w_scale.float().view(shape)

    for L in m.layers()[:-1]:
        b = None if L.bias is None else L.bias.float()
        y = torch.relu(F.conv2d(deq_in(L, y), w32(L), b, L.stride, L.padding, 1, getattr(L, "groups", 1)))
    pooled = torch.flatten(F.adaptive_avg_pool2d(y, (1, 1)), 1)
    fc = m.fc
    return pooled, F.linear(deq_in(fc, pooled), w32(fc), None if fc.bias is None else fc.bias.float())
