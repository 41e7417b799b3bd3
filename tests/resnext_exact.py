"""Exact-arithmetic packed ResNeXts and an engine-free float64 model of the reference's packed dataflow, on the pattern of
tests/resnet_exact.py (whose helpers and quantiser arithmetic this module reuses; see its docstring for why exactness).

The model is torchvision's ResNet of Bottlenecks whose conv2 is a grouped 3x3 convolution: w_des names IC / groups input
channels, fewer than conv1 has outputs.  Every scale is a power of two, zero points are integers, biases lie on their grids,
and K * max|q_x + z_x| * max|q_w + z_w| + |bias units| < 2^24 with K = 9 * IC / groups for a grouped layer."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from resnet_exact import BIAS_UNITS, PC_RATIO, Float64ResNet, Result, _Layer, _pack, _qrange, weight_cap  # noqa: F401

G12 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g12_resnext.npz")


class Float64ResNeXt(Float64ResNet):
    """The reference's ResNeXt on a packed state_dict, in float64 on the host.  The quantiser, the exactness assertions, the
    calibration and the graph are Float64ResNet's; conv2 of every Bottleneck runs with its groups."""

    def __init__(self, sd, exact=True):
        """exact=False: the same arithmetic without the exactness assertions (state_dicts off the exact grid: G12)."""
        self.exact = exact
        super().__init__(sd)
        assert self.bottleneck, "a ResNeXt is built of Bottlenecks"
        groups = set()
        for _, convs, _ in self.blocks:
            fed, per_group = convs[0].w_codes.shape[0], convs[1].w_codes.shape[1]
            assert fed % per_group == 0
            convs[1].groups = fed // per_group
            groups.add(convs[1].groups)
        assert len(groups) == 1
        self.groups = groups.pop()

    def _exact(self, t, what):
        if self.exact:
            Float64ResNet._exact(t, what)

    def _conv(self, L, q):
        x = (q + L.a_view(L.a_zero, q)) * L.a_view(L.a_scale, q)
        y = F.conv2d(x, L.weights(), L.bias, L.stride, L.padding, 1, getattr(L, "groups", 1))
        self._exact(y, L.name + " output")
        return y


def exact_state_dict(depth=(1, 1, 1, 1), groups=4, base=16, w_bits=8, a_bits=8, seed=0, num_classes=10, calib_images=None,
                     image_size=32, variants=None):
    """A packed ResNeXt state_dict in quantize_amd.packed_resnet.synthetic_state_dict's key layout with exact fp32 arithmetic,
    calibrated on Float64ResNeXt.  Stage S has a grouped width of base << (S - 1) (base 16 and 4 groups: Cg 4, 8, 16, 32)
    and 2 * width block outputs; the stem has `base` channels.  variants = {layer name: spec} as
    resnet_exact.exact_state_dict (signed, zero, per_channel, scale_mult)."""
    variants = variants or {}
    rng = np.random.RandomState(seed)
    sd = {}

    def conv(name, IC, OC, K, gain, signed_in=False, g=1):
        spec = variants.get(name, {})
        signed = signed_in or spec.get("signed", False)
        qmin, qmax = _qrange(a_bits, signed)
        z = float(spec.get("zero", 0))
        a_max = int(max(abs(qmin + z), abs(qmax + z))) * (PC_RATIO if spec.get("per_channel") else 1)
        per_group = IC // g
        cap = weight_cap(per_group * K * K, a_max, w_bits)
        q = rng.randint(-cap, cap + 1, size=(OC, per_group, K, K))
        target = gain * np.sqrt(2.0 / (per_group * K * K)) / (cap / np.sqrt(3.0))
        ws = 2.0 ** (np.round(np.log2(target)) + rng.randint(-1, 2, size=OC))
        sd.update({name + ".weight": _pack(q, w_bits),
                   name + ".w_des": torch.tensor([w_bits, 1, OC, per_group, K, K], dtype=torch.int32),
                   name + ".w_scale": torch.from_numpy(ws.astype(np.float32).reshape(OC, 1, 1, 1)),
                   name + ".w_zero": torch.zeros((OC, 1, 1, 1), dtype=torch.float32),
                   name + ".bias": torch.from_numpy(rng.normal(0, 0.05, size=OC).astype(np.float32)),
                   name + ".a_quantizer.scale": torch.tensor([1.0], dtype=torch.float32),
                   name + ".a_quantizer.zero": torch.tensor([z], dtype=torch.float32),
                   name + ".a_quantizer.qmin": torch.tensor(float(qmin)),
                   name + ".a_quantizer.qmax": torch.tensor(float(qmax))})

    conv("conv1", 3, base, 7, 1.0, signed_in=True)
    inplanes = base
    for S, nb in enumerate(depth, start=1):
        width = base << (S - 1)
        for B in range(nb):
            pre = "layer%d.%d" % (S, B)
            conv(pre + ".conv1", inplanes, width, 1, 1.0)
            conv(pre + ".conv2", width, width, 3, 1.0, g=groups)
            conv(pre + ".conv3", width, 2 * width, 1, 0.3)
            if B == 0:
                conv(pre + ".downsample.0", inplanes, 2 * width, 1, 1.0)
            inplanes = 2 * width
    spec = variants.get("fc", {})
    qmin, qmax = _qrange(a_bits, False)
    z = float(spec.get("zero", 0))
    cap = weight_cap(inplanes, int(max(abs(qmin + z), abs(qmax + z))), w_bits)
    qf = rng.randint(-cap, cap + 1, size=(num_classes, inplanes))
    wf = 2.0 ** (np.round(np.log2(np.sqrt(1.0 / inplanes) / cap)) + rng.randint(-1, 2, size=(num_classes, 1)))
    sd.update({"fc.weight": _pack(qf, w_bits),
               "fc.w_des": torch.tensor([w_bits, 1, num_classes, inplanes], dtype=torch.int32),
               "fc.w_scale": torch.from_numpy(wf.astype(np.float32)),
               "fc.w_zero": torch.zeros((num_classes, 1), dtype=torch.float32),
               "fc.bias": torch.from_numpy(rng.normal(0, 0.05, size=num_classes).astype(np.float32)),
               "fc.a_quantizer.scale": torch.tensor([1.0], dtype=torch.float32),
               "fc.a_quantizer.zero": torch.tensor([z], dtype=torch.float32),
               "fc.a_quantizer.qmin": torch.tensor(float(qmin)), "fc.a_quantizer.qmax": torch.tensor(float(qmax))})
    if calib_images is None:
        calib_images = images(2, image_size, seed + 1)
    model = Float64ResNeXt(sd)
    model.forward(calib_images, calibrate=variants)
    return model.write_back(sd)


def images(n, size, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(n, 3, size, size, generator=g)


def load_g12():
    """(z, {key: state_dict}) of tests/golden/g12_resnext.npz: the four grouped module runs g_<name> and the model m_x4."""
    z = np.load(G12, allow_pickle=False)
    sds = {}
    for key in [str(k) for k in z["index"]]:
        pre = key + "_sd_"
        sds[key] = {k[len(pre):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre)}
    return z, sds
