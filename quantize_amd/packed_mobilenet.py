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
import numpy as np
import torch

from . import synthetic
from .packed import PackedConv2d, PackedDepthwiseConv2d, PackedLinear
from .packed_cnn import PackedCNN

DEPTH = (1, 2, 2, 6, 2)          # blocks per stage of the reference's model; from_state_dict reads them from the keys


class _Block:
    def __init__(self, name, dw, pw):
        self.name, self.dw, self.pw = name, dw, pw


class PackedMobileNetV1(PackedCNN):
    FAMILY = "MobileNetV1"

    def __init__(self, stem, blocks, fc):
        self.stem, self._blocks, self.fc = stem, blocks, fc

    @classmethod
    def from_state_dict(cls, sd, prefix=""):
        sd, layer = cls._open(sd, prefix)

        def square(c, name, k):
            if c.KH != k or c.KW != k:
                raise ValueError("%s: a %dx%d kernel where MobileNetV1 has %dx%d" % (name, c.KH, c.KW, k, k))
            return c

        stem = square(layer(PackedConv2d, "conv1", stride=2, padding=1), "conv1", 3)
        found = cls._stages(sd, r"layer(\d+)\.(\d+)\.conv1\.w_des$")
        blocks, C = [], stem.OC
        for S in sorted(found):
            for B in cls._block_indices(found, S):
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

    # ---- the two routes ----
    def forward(self, images, route="fused", check=True):
        """(logits, pooled features)."""
        logits, _, pooled = self._run(images, route, check)
        return logits, pooled

    def _layers(self, x, observe=None):
        """observe(conv, its fp32 input) is called in front of every conv (calibration)."""
        y = x
        for c in self.convs():
            if observe is not None:
                observe(c, y)
            y = torch.relu(c(y, route="packed"))
        return y

    def _fused(self, images, status):
        N, _, H, W = images.shape
        codes = self.stem.quantize_codes(images, status)[0]
        convs = self.convs()
        for c, consumer in zip(convs[:-1], convs[1:]):       # stem -> dw -> pw -> dw -> ...: each writes the next one's codes
            codes = c.relu_codes(codes, N, H, W, consumer, status)
            H, W = c.out_hw(H, W)
        return torch.relu(convs[-1].fp32_from_codes(codes, N, H, W))


def synthetic_state_dict(num_classes=1000, w_bits=8, a_bits=8, seed=0, width=32, depth=DEPTH):
    """A packed MobileNetV1 state_dict in the key layout pack() leaves (host tensors, scales not calibrated: 1.0).  `width`
    is the stem's output channels (32 in the reference's model) and scales every channel count; random b-bit weights,
    He-scaled, folded biases; post-ReLU quantisers unsigned, the image quantiser signed."""
    rng = np.random.RandomState(seed)
    sd = {}

    def conv(name, IC, OC, K, signed=False):
        synthetic.put(sd, name, synthetic.conv_entries(rng, IC, OC, K, w_bits, a_bits, signed, 1.0))

    conv("conv1", 3, width, 3, signed=True)
    C = width
    for S, nb in enumerate(depth, start=1):
        planes = width * (1 << S)
        for B in range(nb):
            pre = "layer%d.%d" % (S, B)
            conv(pre + ".conv1", 1, C, 3)            # depthwise, (C, 1, 3, 3): one 9-tap filter per channel
            conv(pre + ".conv2", C, planes, 1)
            C = planes
    synthetic.put(sd, "fc", synthetic.fc_entries(rng, num_classes, C, w_bits, a_bits))
    return sd


def calibrated_state_dict(device="cuda", calib_images=None, calib_batch=4, image_size=224, **kw):
    """synthetic_state_dict on `device` with every activation quantiser calibrated by max from one `layers` pass."""
    images = synthetic.calibration_images(calib_images, calib_batch, image_size, kw.get("seed", 0))
    return synthetic.calibrated(synthetic_state_dict(**kw), device, PackedMobileNetV1.from_state_dict, images,
                                PackedMobileNetV1.state_dict_scales)
