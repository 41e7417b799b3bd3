"""A packed WideResNet run end to end on the engine.

The reference's model (modelzoo/cnns/wideresnet.py: wrn_40_2, the CIFAR / RobustBench family) is pre-activation: a 3x3 stem,
three stages of basic blocks -- bn1, ReLU, conv1 3x3 (stride 2 on the first block of stages 2 and 3), bn2, ReLU, conv2 3x3, and the
block's input (or, where the width changes, a 1x1 convShortcut of the activated input) added to conv2's output -- then a last
BatchNorm, ReLU, avg_pool2d(8) and a linear classifier.  The reference folds a BatchNorm only where it directly follows a conv in
child order, which is bn2 into conv1 of its block.  Every block's bn1 and the final bn1 stay BatchNorm2d modules behind the
residual add and in front of a quantiser, so pack() leaves the keys conv1.*, block{1,2,3}.layer.{i}.{bn1, conv1, conv2,
convShortcut}.*, bn1.* and fc.*.  PackedWideResNet takes that state_dict and runs it two ways:

  route="layers"  the reference's dataflow with the engine plugged in: every conv with fp32 output (PackedConv2d, activations
                  quantised + packed on the device), torch.add, the BatchNorm as the per-channel affine ATen applies in eval mode
                  (one multiplication and one addition, two torch ops), torch.relu, qe_global_avgpool, PackedLinear for the fc;
  route="fused"   one qe_affine_relu_quantize_pack call per block boundary: the previous block's conv2 output and its stream (or
                  its shortcut's output) in, the codes of the next block's conv1 (and of its convShortcut where their quantisers
                  differ) out, the residual stream only where the next block adds to it.  Inside a block conv1 writes conv2's
                  codes from its own epilogue (the folded bn2 is its bias, the ReLU folds into the clamp where it can); conv2 and
                  the shortcut write fp32.  The tail is the same kernel with no consumer and the activated tensor as its output.

alpha = gamma / sqrt(var + eps) and shift = beta - mean * alpha are derived once, at load time, on the host in fp32; both routes
read the same two arrays, so the two routes agree bit for bit.  With check=False the fused route makes no device -> host copy."""
import numpy as np
import torch

from . import capi, synthetic
from .packed import PackedConv2d, PackedLinear
from .packed_cnn import PackedCNN

WIDTHS = (16, 32, 64)            # times the widen factor: the three stages of the reference's model (the stem is 16 wide)


def bn_affine(weight, bias, mean, var, eps):
    """(alpha, shift) of an eval-mode BatchNorm as host fp32 tensors, each step one fp32 operation: invstd = 1 / sqrt(var + eps),
    alpha = gamma * invstd, shift = beta - mean * alpha."""
    g, b, m, v = (t.detach().cpu().numpy().astype(np.float32).reshape(-1) for t in (weight, bias, mean, var))
    invstd = np.float32(1.0) / np.sqrt(v + np.float32(eps))
    alpha = g * invstd
    shift = b - m * alpha
    return torch.from_numpy(alpha.astype(np.float32)), torch.from_numpy(shift.astype(np.float32))


class _Block:
    def __init__(self, name, alpha, shift, conv1, conv2, shortcut):
        self.name, self.alpha, self.shift, self.conv1, self.conv2, self.shortcut = name, alpha, shift, conv1, conv2, shortcut

    def consumers(self):
        """The distinct quantisers that read the activated input: conv1, and convShortcut where its quantiser is another."""
        if self.shortcut is None or self.shortcut.q_key == self.conv1.q_key:
            return [self.conv1]
        return [self.conv1, self.shortcut]


def _affine(y, alpha, shift):
    t = y * alpha.view(1, -1, 1, 1)
    t = t + shift.view(1, -1, 1, 1)
    return torch.relu(t)


class PackedWideResNet(PackedCNN):
    FAMILY = "WideResNet"

    def __init__(self, stem, blocks, alpha, shift, fc):
        self.stem, self._blocks, self.alpha, self.shift, self.fc = stem, blocks, alpha, shift, fc

    @classmethod
    def from_state_dict(cls, sd, prefix="", bn_eps=1e-5):
        """bn_eps: the BatchNorms' eps, which a state_dict does not hold (nn.BatchNorm2d's default)."""
        sd, layer = cls._open(sd, prefix)
        if any(k.startswith("sub_block1.") for k in sd):
            raise ValueError("packed WideResNet state_dict: %ssub_block1 is not supported" % prefix)

        def square(c, name, k):
            if c.KH != k or c.KW != k:
                raise ValueError("%s: a %dx%d kernel where WideResNet has %dx%d" % (name, c.KH, c.KW, k, k))
            return c

        def bn(name):
            try:
                fields = [sd[name + "." + f] for f in ("weight", "bias", "running_mean", "running_var")]
                return tuple(t.to(fields[0].device) for t in bn_affine(*fields, bn_eps))       # derived on the host, kept beside the layers
            except KeyError as e:
                raise KeyError("packed %s state_dict: missing %s%s" % (cls.FAMILY, prefix, e.args[0])) from None

        stem = square(layer(PackedConv2d, "conv1", stride=1, padding=1), "conv1", 3)
        found = cls._stages(sd, r"block(\d+)\.layer\.(\d+)\.conv1\.w_des$", stage="block")
        blocks, C = [], stem.OC
        for S in sorted(found):
            for B in cls._block_indices(found, S, stage="block"):
                pre = "block%d.layer.%d" % (S, B)
                stride = 2 if (B == 0 and S > 1) else 1
                alpha, shift = bn(pre + ".bn1")
                conv1 = square(layer(PackedConv2d, pre + ".conv1", stride=stride, padding=1), pre + ".conv1", 3)
                conv2 = square(layer(PackedConv2d, pre + ".conv2", stride=1, padding=1), pre + ".conv2", 3)
                shortcut = None
                if pre + ".convShortcut.w_des" in sd:
                    shortcut = square(layer(PackedConv2d, pre + ".convShortcut", stride=stride, padding=0), pre + ".convShortcut", 1)
                if alpha.numel() != C or conv1.IC != C or (shortcut is not None and shortcut.IC != C):
                    raise ValueError("%s: %d bn1, %d conv1%s input channels behind a layer of %d" % (
                        pre, alpha.numel(), conv1.IC, "" if shortcut is None else " and %d convShortcut" % shortcut.IC, C))
                if conv2.IC != conv1.OC or conv2.OC != conv1.OC or (shortcut is not None and shortcut.OC != conv1.OC):
                    raise ValueError("%s: conv1 makes %d channels, conv2 takes %d and makes %d%s" % (
                        pre, conv1.OC, conv2.IC, conv2.OC, "" if shortcut is None else ", convShortcut makes %d" % shortcut.OC))
                if (shortcut is None) != (conv1.OC == C and stride == 1):
                    raise ValueError("%s: %d -> %d channels at stride %d %s a convShortcut" % (
                        pre, C, conv1.OC, stride, "without" if shortcut is None else "with"))
                C = conv1.OC
                blocks.append(_Block(pre, alpha, shift, conv1, conv2, shortcut))
        alpha, shift = bn("bn1")
        fc = layer(PackedLinear, "fc")
        if alpha.numel() != C or fc.K != C:
            raise ValueError("fc: %d input features and %d bn1 channels behind a layer of %d channels" % (fc.K, alpha.numel(), C))
        return cls(stem, blocks, alpha, shift, fc)

    def blocks(self):
        return list(self._blocks)

    def convs(self):
        out = [self.stem]
        for b in self._blocks:
            out += [b.conv1, b.conv2] + ([b.shortcut] if b.shortcut is not None else [])
        return out

    def to(self, device):
        super().to(device)
        for holder in [self] + self._blocks:
            holder.alpha, holder.shift = holder.alpha.to(device), holder.shift.to(device)
        return self

    # ---- the two routes ----
    def final_map(self, H, W):
        for c in [self.stem] + [b.conv1 for b in self._blocks]:
            H, W = c.out_hw(H, W)
        return H, W

    def forward(self, images, route="fused", check=True):
        """(logits, pooled features).  avg_pool2d(out, 8) is the global pool only on an 8 x 8 final map: 32 x 32 images."""
        fm = self.final_map(*images.shape[2:])
        if fm != (8, 8):
            raise ValueError("PackedWideResNet: avg_pool2d(out, 8) is the global pool only on an 8 x 8 final map; %d x %d images "
                             "end on %d x %d" % (images.shape[2], images.shape[3], fm[0], fm[1]))
        logits, _, pooled = self._run(images, route, check)
        return logits, pooled

    def _layers(self, x, observe=None):
        """observe(conv, its fp32 input) is called in front of every conv (calibration)."""
        def run(c, t):
            if observe is not None:
                observe(c, t)
            return c(t, route="packed")

        y = run(self.stem, x)
        for b in self._blocks:
            a = _affine(y, b.alpha, b.shift)
            o = run(b.conv2, torch.relu(run(b.conv1, a)))
            y = torch.add(o, y if b.shortcut is None else run(b.shortcut, a))
        return _affine(y, self.alpha, self.shift)

    def _fused(self, images, status):
        N, _, H, W = images.shape
        x = self.stem.fp32_from_codes(self.stem.quantize_codes(images, status)[0], N, H, W)
        identity = None                                        # x + identity is the stream in front of the next block
        for b in self._blocks:
            adds = b.shortcut is None                          # this block adds the stream itself to its conv2
            cons = b.consumers()
            codes, s, _, _ = capi.affine_relu_quantize_pack(x, b.alpha, b.shift, identity=identity, rqs=[c.requant() for c in cons],
                                                            sum_out=identity if adds else None, status=status)
            stream = x if identity is None else s              # in place on the old stream
            mid = b.conv1.relu_codes(codes[0], N, H, W, b.conv2, status)
            if not adds:
                stream = b.shortcut.fp32_from_codes(codes[-1], N, H, W)
            H, W = b.conv1.out_hw(H, W)
            x, identity = b.conv2.fp32_from_codes(mid, N, H, W), stream
        return capi.affine_relu_quantize_pack(x, self.alpha, self.shift, identity=identity, act_out="new", status=status)[2]


def synthetic_state_dict(num_classes=10, w_bits=8, a_bits=8, seed=0, depth=40, widen=2):
    """A packed WideResNet state_dict in the key layout pack() leaves (host tensors, scales not calibrated: 1.0): random b-bit
    weights, He-scaled; conv1 of a block carries the folded bn2 as its bias, the other convs have none (the reference's convs are
    bias-free); BatchNorm statistics for every unfolded bn1; post-ReLU quantisers unsigned, the image quantiser signed."""
    if (depth - 4) % 6 != 0 or depth < 10:
        raise ValueError("WideResNet depth must be 6 n + 4; got %d" % depth)
    rng = np.random.RandomState(seed)
    sd = {}

    def conv(name, IC, OC, K, signed=False, gain=1.0, bias=False):
        entries = synthetic.conv_entries(rng, IC, OC, K, w_bits, a_bits, signed, gain)
        if not bias:
            del entries["bias"]
        synthetic.put(sd, name, entries)

    conv("conv1", 3, 16, 3, signed=True)
    C = 16
    for S, width in enumerate(WIDTHS, start=1):
        planes = width * widen
        for B in range((depth - 4) // 6):
            pre = "block%d.layer.%d" % (S, B)
            synthetic.put(sd, pre + ".bn1", synthetic.bn_entries(rng, C))
            conv(pre + ".conv1", C, planes, 3, bias=True)
            conv(pre + ".conv2", planes, planes, 3, gain=0.3)
            if C != planes:
                conv(pre + ".convShortcut", C, planes, 1)
            C = planes
    synthetic.put(sd, "bn1", synthetic.bn_entries(rng, C))
    synthetic.put(sd, "fc", synthetic.fc_entries(rng, num_classes, C, w_bits, a_bits))
    return sd


def calibrated_state_dict(device="cuda", calib_images=None, calib_batch=4, image_size=32, **kw):
    """synthetic_state_dict on `device` with every activation quantiser calibrated by max from one `layers` pass."""
    images = synthetic.calibration_images(calib_images, calib_batch, image_size, kw.get("seed", 0))
    return synthetic.calibrated(synthetic_state_dict(**kw), device, PackedWideResNet.from_state_dict, images,
                                PackedWideResNet.state_dict_scales)
