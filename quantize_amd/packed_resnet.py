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
import re

import numpy as np
import torch
import torch.nn.functional as F

from . import capi
from .packed import OUT_OF_RANGE, PackedConv2d, PackedGroupedConv2d, PackedLinear


class _Block:
    def __init__(self, name, convs, downsample, stride):
        self.name, self.convs, self.downsample, self.stride = name, convs, downsample, stride


def _stage_keys(sd):
    found = {}
    for k in sd:
        m = re.match(r"layer(\d+)\.(\d+)\.conv(\d)\.w_des$", k)
        if m:
            found.setdefault(int(m.group(1)), {}).setdefault(int(m.group(2)), set()).add(int(m.group(3)))
    return found


class PackedResNet:
    """A packed torchvision ResNet (Bottleneck: ResNet-50 / 101 / 152, BasicBlock: ResNet-18 / 34) on the engine."""

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
        sd = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}

        def conv(name, stride, padding, in_channels=None):
            """in_channels: what feeds the layer; a w_des that names fewer input channels is a grouped layer's (ResNeXt)."""
            try:
                if in_channels is not None and (name + ".w_des") in sd and int(sd[name + ".w_des"][3]) < in_channels:
                    c = PackedGroupedConv2d.from_state_dict(sd, name + ".", stride=stride, padding=padding, in_channels=in_channels)
                else:
                    c = PackedConv2d.from_state_dict(sd, name + ".", stride=stride, padding=padding)
            except KeyError as e:
                raise KeyError("packed ResNet state_dict: missing %s%s" % (prefix, e.args[0])) from None
            if c.KH != 2 * padding + 1 or c.KW != c.KH:
                raise ValueError("%s: a %dx%d kernel where torchvision's ResNet has %dx%d" % (name, c.KH, c.KW, 2 * padding + 1,
                                                                                           2 * padding + 1))
            return c

        stem = conv("conv1", 2, 3)
        found = _stage_keys(sd)
        if sorted(found) != list(range(1, len(found) + 1)) or not found:
            raise KeyError("packed ResNet state_dict: stages layer1.. not found (have %s)" % sorted(found))
        kinds = {tuple(sorted(c)) for blocks in found.values() for c in blocks.values()}
        if kinds == {(1, 2, 3)}:
            kind = "bottleneck"
        elif kinds == {(1, 2)}:
            kind = "basic"
        else:
            raise ValueError("packed ResNet state_dict: blocks with conv sets %s are neither Bottleneck nor BasicBlock" % sorted(kinds))
        stages, groups = [], set()
        for S in sorted(found):
            if sorted(found[S]) != list(range(len(found[S]))):
                raise KeyError("packed ResNet state_dict: layer%d has blocks %s" % (S, sorted(found[S])))
            blocks = []
            for B in sorted(found[S]):
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
        try:
            fc = PackedLinear.from_state_dict(sd, "fc.")
        except KeyError as e:
            raise KeyError("packed ResNet state_dict: missing %s%s" % (prefix, e.args[0])) from None
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

    def to(self, device):
        for layer in self.convs() + [self.fc]:
            layer.to(device)
        return self

    # ---- the two routes ----
    def __call__(self, images, route="fused", check=True):
        return self.forward(images, route, check)[0]

    def features(self, images, route="fused", check=True):
        """The layer4 feature map (fp32, N x C x 7 x 7 at 224 x 224)."""
        return self.forward(images, route, check)[1]

    def forward(self, images, route="fused", check=True):
        """(logits, layer4 features)."""
        if route == "layers":
            feat = self._layers(images)
        elif route == "fused":
            status = torch.zeros(1, dtype=torch.int32, device=images.device)
            feat = self._fused(images.contiguous(), status)
        else:
            raise ValueError("route must be 'fused' or 'layers'")
        pooled = capi.global_avgpool(feat)
        if route == "layers":
            logits = self.fc(pooled, route="packed")
        else:
            logits = self.fc.call_packed(*self.fc.quantize_codes(pooled, status), status=status)
            if check and int(status.item()) != 0:
                raise RuntimeError(OUT_OF_RANGE)
        return logits, feat

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

    def _conv_codes(self, c, codes, N, H, W, consumer, status):
        """c's output as consumer's codes: fused into c's epilogue where the ReLU folds, else fp32 + relu + quantize_pack.
        A grouped conv (ResNeXt's conv2) applies the ReLU in its own epilogue, whatever the consumer's quantiser."""
        if isinstance(c, PackedGroupedConv2d):
            return c.call_packed(codes, (c.a_bits, int(c.a_signed), N, c.IC, H, W), consumer, relu=True, status=status)[0]
        sh, xq, wq, prep = c.operands(codes, N, H, W)
        if consumer.folds_relu:
            return capi.quantconv2d_requant_prepared(xq, wq, c.bias, sh, prep, consumer.requant(), status=status)[0]
        y = torch.relu(capi.quantconv2d_prepared(xq, wq, c.bias, sh, prep))
        return consumer.quantize_codes(y, status)[0]

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
            s_codes = self._conv_codes(stem, codes, N, H, W, c1, status)
            xcodes = capi.maxpool2d_codes(s_codes, 8, N, stem.OC, Hs, Ws, 3, 2, 1)
        else:
            sh, xq, wq, prep = stem.operands(codes, N, H, W)
            xin = F.max_pool2d(torch.relu(capi.quantconv2d_prepared(xq, wq, stem.bias, sh, prep)), 3, 2, 1)
            xcodes = c1.quantize_codes(xin, status)[0]
        H, W = Hp, Wp
        for i, b in enumerate(blocks):
            nxt = blocks[i + 1] if i + 1 < len(blocks) else None
            # the identity: the downsample's fp32 output (its codes shared with conv1, or quantised from the fp32 input)
            if b.downsample is not None:
                ds = b.downsample
                dcodes = xcodes if ds.q_key == b.convs[0].q_key else ds.quantize_codes(xin, status)[0]
                sh, xq, wq, prep = ds.operands(dcodes, N, H, W)
                identity = capi.quantconv2d_prepared(xq, wq, ds.bias, sh, prep)
            else:
                identity = xin
            o, Ho, Wo = xcodes, H, W
            for c, cn in zip(b.convs[:-1], b.convs[1:]):
                o = self._conv_codes(c, o, N, Ho, Wo, cn, status)
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

    # ---- calibration (synthetic models, tests, tools) ----
    def calibrate(self, images):
        """Set every activation quantiser's scale from the max of what reaches it in one `layers` pass (by max, as the
        existing bottleneck test does): unsigned quantisers take max / qmax, signed ones max|x| / qmax."""
        def observe(c, t):
            if c.a_signed:
                s = t.abs().max() / c.a_qmax
            else:
                s = t.clamp(min=0).max() / c.a_qmax
            c.a_scale = torch.clamp(s, min=1e-8).reshape(1)
        with torch.no_grad():
            feat = self._layers(images, observe)
            pooled = capi.global_avgpool(feat)
            self.fc.a_scale = torch.clamp(pooled.clamp(min=0).max() / self.fc.a_qmax, min=1e-8).reshape(1)
        return self

    def state_dict_scales(self):
        """{key: tensor} of every activation scale, in the state_dict's key layout."""
        out = {c.name + ".a_quantizer.scale": c.a_scale for c in self.convs()}
        out["fc.a_quantizer.scale"] = self.fc.a_scale
        return out


# ---------------------------------------------------------------------------------------------
# Synthetic packed ResNets (tests and tools/bench_resnet_forward.py share this construction)
# ---------------------------------------------------------------------------------------------
ARCHS = {"resnet18": ("basic", [2, 2, 2, 2]), "resnet34": ("basic", [3, 4, 6, 3]), "resnet50": ("bottleneck", [3, 4, 6, 3])}


def pack_codes(q, n_bits, signed):
    """tpack on the host: integer codes -> the little-endian b-bit stream (stored value q + 2^(b-1) when signed)."""
    q = np.asarray(q, dtype=np.int64).reshape(-1)
    stored = (q + ((1 << (n_bits - 1)) if signed else 0)).astype(np.uint64)
    if n_bits == 8:
        return stored.astype(np.uint8)
    bits = ((stored[:, None] >> np.arange(n_bits, dtype=np.uint64)) & 1).astype(np.uint8).reshape(-1)
    return np.packbits(bits, bitorder="little")


def _conv_entries(rng, IC, OC, K, w_bits, a_bits, a_signed, gain, groups=1):
    lim = (1 << (w_bits - 1)) - 1
    IC //= groups                  # the input channels a weight sees: pack() stores w_des [b, s, OC, IC / groups, KH, KW]
    q = rng.randint(-lim, lim + 1, size=(OC, IC, K, K))
    std_q = np.sqrt(((2 * lim + 1) ** 2 - 1) / 12.0)
    ws = gain * np.sqrt(2.0 / (IC * K * K)) / std_q * rng.uniform(0.8, 1.2, size=OC)     # He-scaled
    qmin, qmax = (-(1 << (a_bits - 1)), (1 << (a_bits - 1)) - 1) if a_signed else (0, (1 << a_bits) - 1)
    return {"weight": torch.from_numpy(pack_codes(q, w_bits, True)),
            "w_des": torch.tensor([w_bits, 1, OC, IC, K, K], dtype=torch.int32),
            "w_scale": torch.from_numpy(ws.astype(np.float32).reshape(OC, 1, 1, 1)),
            "w_zero": torch.zeros((OC, 1, 1, 1), dtype=torch.float32),
            "bias": torch.from_numpy(rng.normal(0, 0.05, size=OC).astype(np.float32)),        # the folded BatchNorm's shift
            "a_quantizer.scale": torch.tensor([1.0], dtype=torch.float32),
            "a_quantizer.zero": torch.tensor([0.0], dtype=torch.float32),
            "a_quantizer.qmin": torch.tensor(float(qmin)), "a_quantizer.qmax": torch.tensor(float(qmax))}


def synthetic_state_dict(arch="resnet50", num_classes=1000, w_bits=8, a_bits=8, seed=0, width=64, groups=1, width_per_group=64):
    """A packed ResNet state_dict in the key layout pack() leaves (host tensors, scales not calibrated: 1.0).  Random
    b-bit weights, He-scaled (block-end convs at gain 0.3 so activations stay O(1) through 16 blocks), folded biases;
    post-ReLU activation quantisers unsigned, the image quantiser signed.  See calibrated_state_dict.
    groups / width_per_group: torchvision's ResNeXt Bottleneck (resnext50_32x4d: arch="resnet50", groups=32,
    width_per_group=4) -- conv1 and conv2 have planes * width_per_group / 64 * groups channels, conv2 is grouped."""
    kind, depth = ARCHS[arch]
    rng = np.random.RandomState(seed)
    sd = {}

    def put(prefix, entries):
        for k, v in entries.items():
            sd[prefix + "." + k] = v

    put("conv1", _conv_entries(rng, 3, width, 7, w_bits, a_bits, True, 1.0))
    inplanes, exp = width, (4 if kind == "bottleneck" else 1)
    for S, nb in enumerate(depth, start=1):
        planes = width * (1 << (S - 1))
        for B in range(nb):
            pre = "layer%d.%d" % (S, B)
            if kind == "bottleneck":
                mid = planes * width_per_group // 64 * groups
                put(pre + ".conv1", _conv_entries(rng, inplanes, mid, 1, w_bits, a_bits, False, 1.0))
                put(pre + ".conv2", _conv_entries(rng, mid, mid, 3, w_bits, a_bits, False, 1.0, groups))
                put(pre + ".conv3", _conv_entries(rng, mid, planes * 4, 1, w_bits, a_bits, False, 0.3))
            else:
                put(pre + ".conv1", _conv_entries(rng, inplanes, planes, 3, w_bits, a_bits, False, 1.0))
                put(pre + ".conv2", _conv_entries(rng, planes, planes, 3, w_bits, a_bits, False, 0.3))
            if B == 0 and (S > 1 or inplanes != planes * exp):
                put(pre + ".downsample.0", _conv_entries(rng, inplanes, planes * exp, 1, w_bits, a_bits, False, 1.0))
            inplanes = planes * exp
    lim = (1 << (w_bits - 1)) - 1
    qf = rng.randint(-lim, lim + 1, size=(num_classes, inplanes))
    sd.update({"fc.weight": torch.from_numpy(pack_codes(qf, w_bits, True)),
               "fc.w_des": torch.tensor([w_bits, 1, num_classes, inplanes], dtype=torch.int32),
               "fc.w_scale": torch.from_numpy((np.sqrt(1.0 / inplanes) / lim * rng.uniform(0.8, 1.2, size=(num_classes, 1)))
                                              .astype(np.float32)),
               "fc.w_zero": torch.zeros((num_classes, 1), dtype=torch.float32),
               "fc.bias": torch.from_numpy(rng.normal(0, 0.05, size=num_classes).astype(np.float32)),
               "fc.a_quantizer.scale": torch.tensor([1.0], dtype=torch.float32),
               "fc.a_quantizer.zero": torch.tensor([0.0], dtype=torch.float32),
               "fc.a_quantizer.qmin": torch.tensor(0.0), "fc.a_quantizer.qmax": torch.tensor(float((1 << a_bits) - 1))})
    return sd


def calibrated_state_dict(arch="resnet50", device="cuda", calib_images=None, calib_batch=4, image_size=224, **kw):
    """synthetic_state_dict on `device` with every activation quantiser calibrated by max from one `layers` pass."""
    sd = {k: v.to(device) for k, v in synthetic_state_dict(arch, **kw).items()}
    if calib_images is None:
        g = torch.Generator(device="cpu").manual_seed(kw.get("seed", 0) + 1)
        calib_images = torch.randn(calib_batch, 3, image_size, image_size, generator=g).to(device)
    model = PackedResNet.from_state_dict(sd).calibrate(calib_images)
    for k, v in model.state_dict_scales().items():
        sd[k] = v.detach().clone()
    return sd
