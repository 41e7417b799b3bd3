"""Exact-arithmetic packed ResNeXts and an engine-free float64 model of the reference's packed dataflow, on the pattern of
tests/resnet_exact.py (whose helpers and quantiser arithmetic this module reuses; see its docstring for why exactness).

The model is torchvision's ResNet of Bottlenecks whose conv2 is a grouped 3x3 convolution: w_des names IC / groups input
channels, fewer than conv1 has outputs.  Every scale is a power of two, zero points are integers, biases lie on their grids,
and K * max|q_x + z_x| * max|q_w + z_w| + |bias units| < 2^24 with K = 9 * IC / groups for a grouped layer."""
import os

import numpy as np
import torch

from resnet_exact import (BIAS_UNITS, PC_RATIO, Float64ResNet, Result, _Layer, _pack, _qrange, calibrated_exact,  # noqa: F401
                          exact_conv_entries, exact_fc_entries, images, weight_cap)

G12 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g12_resnext.npz")


class Float64ResNeXt(Float64ResNet):
    """The reference's ResNeXt on a packed state_dict, in float64 on the host.  The quantiser, the exactness assertions, the
    calibration and the graph are Float64ResNet's; conv2 of every Bottleneck runs with its groups."""

    def __init__(self, sd, exact=True):
        super().__init__(sd, exact)
        assert self.bottleneck, "a ResNeXt is built of Bottlenecks"
        groups = set()
        for _, convs, _ in self.blocks:
            fed, per_group = convs[0].w_codes.shape[0], convs[1].w_codes.shape[1]
            assert fed % per_group == 0
            convs[1].groups = fed // per_group
            groups.add(convs[1].groups)
        assert len(groups) == 1
        self.groups = groups.pop()


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
        exact_conv_entries(rng, sd, name, IC // g, OC, K, gain, variants.get(name, {}), w_bits, a_bits, signed_in)

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
    exact_fc_entries(rng, sd, num_classes, inplanes, variants.get("fc", {}), w_bits, a_bits)
    return calibrated_exact(Float64ResNeXt(sd), sd, calib_images, 2, image_size, seed, variants)


def load_g12():
    """(z, {key: state_dict}) of tests/golden/g12_resnext.npz: the four grouped module runs g_<name> and the model m_x4."""
    z = np.load(G12, allow_pickle=False)
    sds = {}
    for key in [str(k) for k in z["index"]]:
        pre = key + "_sd_"
        sds[key] = {k[len(pre):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre)}
    return z, sds
