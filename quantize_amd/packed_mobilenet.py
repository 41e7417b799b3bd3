"""A packed MobileNetV1 run end to end on the engine.

The reference's model (modelzoo/cnns/mobilenet/mobilenetv1.py) is a 3x3 stride-2 stem and five stages of blocks, each a
depthwise 3x3 convolution (groups = channels; stride 2 on the first block of stages 2..5) followed by a 1x1 convolution, a
ReLU behind every convolution, global average pooling and a linear classifier.  With the BatchNorms folded the runners' packing
leaves the keys conv1.*, layerS.B.conv1.* (depthwise), layerS.B.conv2.* (1x1) and fc.*.  PackedMobileNetV1 takes that
state_dict and runs it two ways:

  route="layers"  the reference's dataflow with the engine plugged in: every conv with fp32 output (PackedConv2d /
                  PackedDepthwiseConv2d, activations quantised + packed on the device), torch ReLU, qe_global_avgpool,
                  PackedLinear for the fc;
  route="fused"   the image is quantised once; the stem and every 1x1 conv write the next depthwise layer's codes
                  (qe_quantconv2d_requant_prepared, the ReLU folded into the clamp where the consumer's codes are unsigned
                  with zero point 0, else fp32 + relu + quantize_pack), every depthwise layer writes the following 1x1 conv's
                  codes from its own epilogue with the ReLU applied there (qe_quantconv2d_depthwise), and the last 1x1 conv
                  writes fp32, followed by ReLU, pool and fc on the same kernels as `layers`.

Every fused step is bit-identical to its layers form, so the logits of the two routes agree bit for bit.  With check=False
the fused route makes no device -> host copy: every range flag accumulates in one device int32."""
import re

import numpy as np
import torch

from . import capi
from .packed import OUT_OF_RANGE, PackedConv2d, PackedDepthwiseConv2d, PackedLinear
from .packed_resnet import _conv_entries, pack_codes

DEPTH = (1, 2, 2, 6, 2)          # blocks per stage of the reference's model; from_state_dict reads them from the keys


class _Block:
    def __init__(self, name, dw, pw):
        self.name, self.dw, self.pw = name, dw, pw


class PackedMobileNetV1:
    def __init__(self, stem, blocks, fc):
        self.stem, self._blocks, self.fc = stem, blocks, fc

    @classmethod
    def from_state_dict(cls, sd, prefix=""):
        sd = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}

        def layer(kind, name, **geometry):
            try:
                return kind.from_state_dict(sd, name + ".", **geometry)
            except KeyError as e:
                raise KeyError("packed MobileNetV1 state_dict: missing %s%s" % (prefix, e.args[0])) from None

        def square(c, name, k):
            if c.KH != k or c.KW != k:
                raise ValueError("%s: a %dx%d kernel where MobileNetV1 has %dx%d" % (name, c.KH, c.KW, k, k))
            return c

        stem = square(layer(PackedConv2d, "conv1", stride=2, padding=1), "conv1", 3)
        found = {}
        for k in sd:
            m = re.match(r"layer(\d+)\.(\d+)\.conv1\.w_des$", k)
            if m:
                found.setdefault(int(m.group(1)), set()).add(int(m.group(2)))
        if not found or sorted(found) != list(range(1, len(found) + 1)):
            raise KeyError("packed MobileNetV1 state_dict: stages layer1.. not found (have %s)" % sorted(found))
        blocks, C = [], stem.OC
        for S in sorted(found):
            if sorted(found[S]) != list(range(len(found[S]))):
                raise KeyError("packed MobileNetV1 state_dict: layer%d has blocks %s" % (S, sorted(found[S])))
            for B in sorted(found[S]):
                pre = "layer%d.%d" % (S, B)
                dw = square(layer(PackedDepthwiseConv2d, pre + ".conv1", stride=2 if (B == 0 and S > 1) else 1, padding=1),
                            pre + ".conv1", 3)
                pw = square(layer(PackedConv2d, pre + ".conv2", stride=1, padding=0), pre + ".conv2", 1)
                if dw.C != C or pw.IC != C:
                    raise ValueError("%s: %d depthwise and %d pointwise input channels behind a layer of %d" % (pre, dw.C, pw.IC, C))
                C = pw.OC
                blocks.append(_Block(pre, dw, pw))
        fc = layer(PackedLinear, "fc")
        if fc.K != C:
            raise ValueError("fc: %d input features behind a layer of %d channels" % (fc.K, C))
        return cls(stem, blocks, fc)

    def blocks(self):
        return list(self._blocks)

    def convs(self):
        out = [self.stem]
        for b in self._blocks:
            out += [b.dw, b.pw]
        return out

    def to(self, device):
        for layer in self.convs() + [self.fc]:
            layer.to(device)
        return self

    # ---- the two routes ----
    def __call__(self, images, route="fused", check=True):
        return self.forward(images, route, check)[0]

    def forward(self, images, route="fused", check=True):
        """(logits, pooled features)."""
        if route == "layers":
            feat = self._layers(images)
            pooled = capi.global_avgpool(feat)
            return self.fc(pooled, route="packed"), pooled
        if route != "fused":
            raise ValueError("route must be 'fused' or 'layers'")
        status = torch.zeros(1, dtype=torch.int32, device=images.device)
        feat = self._fused(images.contiguous(), status)
        pooled = capi.global_avgpool(feat)
        logits = self.fc.call_packed(*self.fc.quantize_codes(pooled, status), status=status)
        if check and int(status.item()) != 0:
            raise RuntimeError(OUT_OF_RANGE)
        return logits, pooled

    def _layers(self, x, observe=None):
        """observe(conv, its fp32 input) is called in front of every conv (calibration)."""
        y = x
        for c in self.convs():
            if observe is not None:
                observe(c, y)
            y = torch.relu(c(y, route="packed"))
        return y

    @staticmethod
    def _conv_codes(c, codes, N, H, W, consumer, status):
        """c's output (behind its ReLU) as consumer's codes, as PackedResNet._conv_codes."""
        sh, xq, wq, prep = c.operands(codes, N, H, W)
        if consumer.folds_relu:
            return capi.quantconv2d_requant_prepared(xq, wq, c.bias, sh, prep, consumer.requant(), status=status)[0]
        y = torch.relu(capi.quantconv2d_prepared(xq, wq, c.bias, sh, prep))
        return consumer.quantize_codes(y, status)[0]

    def _fused(self, images, status):
        N, _, H, W = images.shape
        codes = self.stem.quantize_codes(images, status)[0]
        producer = self.stem
        for i, b in enumerate(self._blocks):
            codes = self._conv_codes(producer, codes, N, H, W, b.dw, status)
            H, W = producer.out_hw(H, W)
            des = (b.dw.a_bits, int(b.dw.a_signed), N, b.dw.C, H, W)
            codes = b.dw.call_packed(codes, des, consumer=b.pw, relu=True, status=status)[0]
            H, W = b.dw.out_hw(H, W)
            producer = b.pw
        sh, xq, wq, prep = producer.operands(codes, N, H, W)
        return torch.relu(capi.quantconv2d_prepared(xq, wq, producer.bias, sh, prep))

    # ---- calibration (synthetic models, tests, tools) ----
    def calibrate(self, images):
        """Every activation quantiser's scale from the max of what reaches it in one `layers` pass, as PackedResNet.calibrate."""
        def observe(c, t):
            s = (t.abs().max() if c.a_signed else t.clamp(min=0).max()) / c.a_qmax
            c.a_scale = torch.clamp(s, min=1e-8).reshape(1)
        with torch.no_grad():
            pooled = capi.global_avgpool(self._layers(images, observe))
            self.fc.a_scale = torch.clamp(pooled.clamp(min=0).max() / self.fc.a_qmax, min=1e-8).reshape(1)
        return self

    def state_dict_scales(self):
        out = {c.name + ".a_quantizer.scale": c.a_scale for c in self.convs()}
        out["fc.a_quantizer.scale"] = self.fc.a_scale
        return out


def _dw_entries(rng, C, w_bits, a_bits):
    e = _conv_entries(rng, 1, C, 3, w_bits, a_bits, False, 1.0)          # (C, 1, 3, 3): one 9-tap filter per channel
    return e


def synthetic_state_dict(num_classes=1000, w_bits=8, a_bits=8, seed=0, width=32, depth=DEPTH):
    """A packed MobileNetV1 state_dict in the key layout pack() leaves (host tensors, scales not calibrated: 1.0).  `width`
    is the stem's output channels (32 in the reference's model) and scales every channel count; random b-bit weights,
    He-scaled, folded biases; post-ReLU quantisers unsigned, the image quantiser signed."""
    rng = np.random.RandomState(seed)
    sd = {}

    def put(prefix, entries):
        for k, v in entries.items():
            sd[prefix + "." + k] = v

    put("conv1", _conv_entries(rng, 3, width, 3, w_bits, a_bits, True, 1.0))
    C = width
    for S, nb in enumerate(depth, start=1):
        planes = width * (1 << S)
        for B in range(nb):
            pre = "layer%d.%d" % (S, B)
            put(pre + ".conv1", _dw_entries(rng, C, w_bits, a_bits))
            put(pre + ".conv2", _conv_entries(rng, C, planes, 1, w_bits, a_bits, False, 1.0))
            C = planes
    lim = (1 << (w_bits - 1)) - 1
    qf = rng.randint(-lim, lim + 1, size=(num_classes, C))
    sd.update({"fc.weight": torch.from_numpy(pack_codes(qf, w_bits, True)),
               "fc.w_des": torch.tensor([w_bits, 1, num_classes, C], dtype=torch.int32),
               "fc.w_scale": torch.from_numpy((np.sqrt(1.0 / C) / lim * rng.uniform(0.8, 1.2, size=(num_classes, 1))).astype(np.float32)),
               "fc.w_zero": torch.zeros((num_classes, 1), dtype=torch.float32),
               "fc.bias": torch.from_numpy(rng.normal(0, 0.05, size=num_classes).astype(np.float32)),
               "fc.a_quantizer.scale": torch.tensor([1.0], dtype=torch.float32),
               "fc.a_quantizer.zero": torch.tensor([0.0], dtype=torch.float32),
               "fc.a_quantizer.qmin": torch.tensor(0.0), "fc.a_quantizer.qmax": torch.tensor(float((1 << a_bits) - 1))})
    return sd


def calibrated_state_dict(device="cuda", calib_images=None, calib_batch=4, image_size=224, **kw):
    """synthetic_state_dict on `device` with every activation quantiser calibrated by max from one `layers` pass."""
    sd = {k: v.to(device) for k, v in synthetic_state_dict(**kw).items()}
    if calib_images is None:
        g = torch.Generator(device="cpu").manual_seed(kw.get("seed", 0) + 1)
        calib_images = torch.randn(calib_batch, 3, image_size, image_size, generator=g).to(device)
    model = PackedMobileNetV1.from_state_dict(sd).calibrate(calib_images)
    for k, v in model.state_dict_scales().items():
        sd[k] = v.detach().clone()
    return sd
