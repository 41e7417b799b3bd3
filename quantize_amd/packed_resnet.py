"""A packed torchvision ResNet run end to end on the engine.

The reference's PTQ / QAT runners turn a torchvision ResNet into QuantConv2d layers with the BatchNorm folded into weight
and bias (modelzoo/reconstruct.py): what remains between the convolutions is plain torch -- ReLU, the residual `+`,
MaxPool2d, AdaptiveAvgPool2d -- and a QuantLinear fc.  PackedResNet takes the state_dict pack() leaves for such a model
(keys conv1.*, layerS.B.conv{1,2,3}.*, layerS.B.downsample.0.*, fc.*) and runs it two ways:

  route="layers"  the reference's dataflow with the engine plugged in: every conv through PackedConv2d (activations
                  quantised + packed on the device, fp32 output), torch ReLU / + / max_pool2d, PackedLinear for the fc;
  route="fused"   the image is quantised once; every conv writes the codes of the layer that reads its output
                  (qe_quantconv2d_requant_prepared, the ReLU folded into an unsigned zero-point-0 clamp), the stem's
                  maxpool runs on the codes (qe_maxpool2d_codes), and each block's last conv adds the identity, applies the
                  ReLU and writes the fp32 block output and / or the next block's codes (qe_quantconv2d_residual_prepared).

Both routes pool with qe_global_avgpool and run the fc on the same kernels, so their logits agree bit for bit.  Where a
fused step would not be exact, the fused route takes the layers route's form for that step only:
  * the ReLU folds into the consumer's clamp only when its codes are unsigned with zero point 0 -- else fp32 + relu +
    quantize_pack;
  * when a stage-first block's downsample quantiser differs from its conv1 quantiser, the downsample's codes come from
    quantize_pack of the fp32 block input;
  * sub-8-bit stem codes go through the fp32 maxpool.
With check=False the fused route makes no device -> host copy or synchronisation: every range flag accumulates in one
device int32, read once at the end when check=True.
"""
import numpy as np
import torch
import torch.nn.functional as F

from . import capi, synthetic
from .packed import PackedConv2d, PackedGroupedConv2d, PackedLinear
from .packed_cnn import PackedCNN
from .synthetic import pack_codes  # noqa: F401  (a public name of this module: earlier importers read it from here)


class _Block:
    def __init__(self, name, convs, downsample, stride):
        self.name, self.convs, self.downsample, self.stride = name, convs, downsample, stride


class PackedResNet(PackedCNN):
    """A packed torchvision ResNet (Bottleneck: ResNet-50 / 101 / 152, BasicBlock: ResNet-18 / 34) on the engine."""
    FAMILY = "ResNet"

    def __init__(self, stem, stages, fc, kind, groups=1):
        self.stem, self.stages, self.fc, self.kind, self.groups = stem, stages, fc, kind, groups

    @property
    def fc_des(self):
        """The fc's weight description [n_bits, sign, out_features, in_features], from the layer's host values."""
        return [self.fc.w_bits, int(self.fc.w_signed), self.fc.O, self.fc.K]

    @classmethod
    def from_state_dict(cls, sd, prefix=""):
        """torchvision's geometry: stem 7x7 / 2 pad 3; in a stage's first block the stride sits on the Bottleneck's conv2
        (the BasicBlock's conv1) and on the downsample; 3x3 convs pad 1, 1x1 convs pad 0."""
        sd, layer = cls._open(sd, prefix)

        def conv(name, stride, padding, in_channels=None):
            """in_channels: what feeds the layer; a w_des that names fewer input channels is a grouped layer's (ResNeXt)."""
            if in_channels is not None and (name + ".w_des") in sd and int(sd[name + ".w_des"][3]) < in_channels:
                c = layer(PackedGroupedConv2d, name, stride=stride, padding=padding, in_channels=in_channels)
            else:
                c = layer(PackedConv2d, name, stride=stride, padding=padding)
            if c.KH != 2 * padding + 1 or c.KW != c.KH:
                raise ValueError("%s: a %dx%d kernel where torchvision's ResNet has %dx%d" % (name, c.KH, c.KW, 2 * padding + 1,
                                                                                           2 * padding + 1))
            return c

        stem = conv("conv1", 2, 3)
        found = cls._stages(sd, r"layer(\d+)\.(\d+)\.conv(\d)\.w_des$")
        kinds = {tuple(sorted(c)) for blocks in found.values() for c in blocks.values()}
        if kinds == {(1, 2, 3)}:
            kind = "bottleneck"
        elif kinds == {(1, 2)}:
            kind = "basic"
        else:
            raise ValueError("packed ResNet state_dict: blocks with conv sets %s are neither Bottleneck nor BasicBlock" % sorted(kinds))
        stages, groups = [], set()
        for S in sorted(found):
            blocks = []
            for B in cls._block_indices(found, S):
                pre = "layer%d.%d." % (S, B)
                s = (1 if S == 1 else 2) if B == 0 else 1
                if kind == "bottleneck":
                    c1 = conv(pre + "conv1", 1, 0)
                    convs = [c1, conv(pre + "conv2", s, 1, c1.OC), conv(pre + "conv3", 1, 0)]
                    groups.add(getattr(convs[1], "groups", 1))
                else:
                    convs = [conv(pre + "conv1", s, 1), conv(pre + "conv2", 1, 1)]
                    if convs[1].IC != convs[0].OC:
                        raise ValueError("%sconv2: a grouped conv in a BasicBlock is not supported (w_des names %d input channels, "
                                         "conv1 has %d outputs)" % (pre, convs[1].IC, convs[0].OC))
                ds = conv(pre + "downsample.0", s, 0) if (pre + "downsample.0.w_des") in sd else None
                if B == 0 and ds is None and (s != 1 or convs[0].IC != convs[-1].OC):
                    raise KeyError("packed ResNet state_dict: missing %s%sdownsample.0.w_des" % (prefix, pre))
                blocks.append(_Block(pre[:-1], convs, ds, s))
            stages.append(blocks)
        fc = layer(PackedLinear, "fc")
        if len(groups) > 1:
            raise ValueError("packed ResNet state_dict: the Bottlenecks' conv2 layers have different groups %s" % sorted(groups))
        return cls(stem, stages, fc, kind, groups.pop() if groups else 1)

    # ---- introspection ----
    def blocks(self):
        return [b for st in self.stages for b in st]

    def convs(self):
        out = [self.stem]
        for b in self.blocks():
            out += b.convs + ([b.downsample] if b.downsample is not None else [])
        return out

    def block_end_shapes(self, N, H=224, W=224):
        """(block, qe_conv_shape of its last conv) for every block at an N x 3 x H x W input."""
        H, W = self.stem.out_hw(H, W)
        H, W = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
        res = []
        for b in self.blocks():
            for c in b.convs[:-1]:
                H, W = c.out_hw(H, W)
            res.append((b, b.convs[-1].shape(N, H, W)))
            H, W = b.convs[-1].out_hw(H, W)
        return res

    def residual_paths(self, N, H=224, W=224):
        """qe_quantconv2d_residual_path of every block end at an N x 3 x H x W input, with the codes the fused route asks
        for there (the next block's conv1 quantiser; none after the last block).  Host-side plan only: no device work."""
        blocks = self.blocks()
        res = []
        for i, (b, sh) in enumerate(self.block_end_shapes(N, H, W)):
            c = b.convs[-1]
            codes = torch.empty(64, dtype=torch.uint8, device=c.weight.device)      # the plan reads only its alignment
            rq = blocks[i + 1].convs[0].requant() if i + 1 < len(blocks) else None
            res.append(capi.residual_path(sh, c.xq(codes), c.wq(), rq))
        return res

    # ---- the two routes ----
    def features(self, images, route="fused", check=True):
        """The layer4 feature map (fp32, N x C x 7 x 7 at 224 x 224)."""
        return self.forward(images, route, check)[1]

    def forward(self, images, route="fused", check=True):
        """(logits, layer4 features)."""
        return self._run(images, route, check)[:2]

    def _layers(self, x, observe=None):
        """observe(conv, its fp32 input) is called in front of every conv (calibration)."""
        def run(c, t):
            if observe is not None:
                observe(c, t)
            return c(t, route="packed")
        y = F.max_pool2d(torch.relu(run(self.stem, x)), 3, 2, 1)
        for b in self.blocks():
            identity = run(b.downsample, y) if b.downsample is not None else y
            o = y
            for c in b.convs[:-1]:
                o = torch.relu(run(c, o))
            y = torch.relu(run(b.convs[-1], o) + identity)
        return y

    def _fused(self, images, status):
        N, _, H, W = images.shape
        blocks = self.blocks()
        first = blocks[0]
        c1 = first.convs[0]
        stem = self.stem
        codes = stem.quantize_codes(images, status)[0]
        Hs, Ws = stem.out_hw(H, W)
        Hp, Wp = (Hs + 2 - 3) // 2 + 1, (Ws + 2 - 3) // 2 + 1
        xin = None
        if c1.folds_relu and c1.a_bits == 8 and first.downsample is not None and first.downsample.q_key == c1.q_key:
            # stem -> layer1.0.conv1's codes (ReLU folded), then the maxpool on the codes: nothing else reads the fp32
            s_codes = stem.relu_codes(codes, N, H, W, c1, status)
            xcodes = capi.maxpool2d_codes(s_codes, 8, N, stem.OC, Hs, Ws, 3, 2, 1)
        else:
            xin = F.max_pool2d(torch.relu(stem.fp32_from_codes(codes, N, H, W)), 3, 2, 1)
            xcodes = c1.quantize_codes(xin, status)[0]
        H, W = Hp, Wp
        for i, b in enumerate(blocks):
            nxt = blocks[i + 1] if i + 1 < len(blocks) else None
            # the identity: the downsample's fp32 output (its codes shared with conv1, or quantised from the fp32 input)
            if b.downsample is not None:
                ds = b.downsample
                dcodes = xcodes if ds.q_key == b.convs[0].q_key else ds.quantize_codes(xin, status)[0]
                identity = ds.fp32_from_codes(dcodes, N, H, W)
            else:
                identity = xin
            o, Ho, Wo = xcodes, H, W
            for c, cn in zip(b.convs[:-1], b.convs[1:]):
                o = c.relu_codes(o, N, Ho, Wo, cn, status)
                Ho, Wo = c.out_hw(Ho, Wo)
            last = b.convs[-1]
            # the block end: fp32 out unless the next block only reads codes (its identity is its downsample's output,
            # whose codes are conv1's)
            need_f32 = nxt is None or nxt.downsample is None or nxt.downsample.q_key != nxt.convs[0].q_key
            sh, xq, wq, prep = last.operands(o, N, Ho, Wo)
            rq = nxt.convs[0].requant() if nxt is not None else None
            out = identity if need_f32 else None       # in place: nothing else reads the identity after this conv
            xin, xcodes, _ = capi.quantconv2d_residual_prepared(xq, wq, last.bias, sh, prep, identity, rq=rq, out=out,
                                                                status=status)
            H, W = last.out_hw(Ho, Wo)
        return xin


# ---------------------------------------------------------------------------------------------
# Synthetic packed ResNets (tests and tools/bench_resnet_forward.py share this construction)
# ---------------------------------------------------------------------------------------------
ARCHS = {"resnet18": ("basic", [2, 2, 2, 2]), "resnet34": ("basic", [3, 4, 6, 3]), "resnet50": ("bottleneck", [3, 4, 6, 3])}


def synthetic_state_dict(arch="resnet50", num_classes=1000, w_bits=8, a_bits=8, seed=0, width=64, groups=1, width_per_group=64):
    """A packed ResNet state_dict in the key layout pack() leaves (host tensors, scales not calibrated: 1.0).  Random
    b-bit weights, He-scaled (block-end convs at gain 0.3 so activations stay O(1) through 16 blocks), folded biases;
    post-ReLU activation quantisers unsigned, the image quantiser signed.  See calibrated_state_dict.
    groups / width_per_group: torchvision's ResNeXt Bottleneck (resnext50_32x4d: arch="resnet50", groups=32,
    width_per_group=4) -- conv1 and conv2 have planes * width_per_group / 64 * groups channels, conv2 is grouped."""
    kind, depth = ARCHS[arch]
    rng = np.random.RandomState(seed)
    sd = {}

    def conv(name, IC, OC, K, gain=1.0, signed=False, groups=1):
        synthetic.put(sd, name, synthetic.conv_entries(rng, IC, OC, K, w_bits, a_bits, signed, gain, groups))

    conv("conv1", 3, width, 7, signed=True)
    inplanes, exp = width, (4 if kind == "bottleneck" else 1)
    for S, nb in enumerate(depth, start=1):
        planes = width * (1 << (S - 1))
        for B in range(nb):
            pre = "layer%d.%d" % (S, B)
            if kind == "bottleneck":
                mid = planes * width_per_group // 64 * groups
                conv(pre + ".conv1", inplanes, mid, 1)
                conv(pre + ".conv2", mid, mid, 3, groups=groups)
                conv(pre + ".conv3", mid, planes * 4, 1, gain=0.3)
            else:
                conv(pre + ".conv1", inplanes, planes, 3)
                conv(pre + ".conv2", planes, planes, 3, gain=0.3)
            if B == 0 and (S > 1 or inplanes != planes * exp):
                conv(pre + ".downsample.0", inplanes, planes * exp, 1)
            inplanes = planes * exp
    synthetic.put(sd, "fc", synthetic.fc_entries(rng, num_classes, inplanes, w_bits, a_bits))
    return sd


def calibrated_state_dict(arch="resnet50", device="cuda", calib_images=None, calib_batch=4, image_size=224, **kw):
    """synthetic_state_dict on `device` with every activation quantiser calibrated by max from one `layers` pass."""
    images = synthetic.calibration_images(calib_images, calib_batch, image_size, kw.get("seed", 0))
    return synthetic.calibrated(synthetic_state_dict(arch, **kw), device, PackedResNet.from_state_dict, images,
                                PackedResNet.state_dict_scales)
