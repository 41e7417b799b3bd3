"""What the packed CNN runners (PackedResNet, PackedMobileNetV1, PackedWideResNet) share: everything but the graph.

A family derives from PackedCNN and supplies FAMILY (its name in from_state_dict's messages), from_state_dict, convs(),
_layers(x, observe) and _fused(images, status) -- both return the fp32 feature map the head pools -- and its own forward,
which picks what it returns beside the logits from _run.  Both routes pool with qe_global_avgpool and run the fc on the same
kernels; on the fused route every range flag accumulates in one device int32, read once at the end when check=True."""
import re

import torch

from . import capi
from .packed import OUT_OF_RANGE


class PackedCNN:
    FAMILY = None

    # ---- from_state_dict's helpers ----
    @classmethod
    def _open(cls, sd, prefix):
        """(the entries under `prefix` with it stripped, layer(kind, name, **geometry): kind.from_state_dict of them, a
        missing key reported under its full name)."""
        sd = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}

        def layer(kind, name, **geometry):
            try:
                return kind.from_state_dict(sd, name + ".", **geometry)
            except KeyError as e:
                raise KeyError("packed %s state_dict: missing %s%s" % (cls.FAMILY, prefix, e.args[0])) from None
        return sd, layer

    @classmethod
    def _stages(cls, sd, pattern, stage="layer"):
        """{stage: {block: the pattern's further groups as a set of ints}} of the keys matching `pattern` (groups 1 and 2:
        stage and block index); the stages must be 1..n.  `stage`: what the family's key layout calls one (in messages)."""
        found = {}
        for k in sd:
            m = re.match(pattern, k)
            if m:
                found.setdefault(int(m.group(1)), {}).setdefault(int(m.group(2)), set()).update(int(g) for g in m.groups()[2:])
        if not found or sorted(found) != list(range(1, len(found) + 1)):
            raise KeyError("packed %s state_dict: stages %s1.. not found (have %s)" % (cls.FAMILY, stage, sorted(found)))
        return found

    @classmethod
    def _block_indices(cls, found, S, stage="layer"):
        """Stage S's block indices, which must be 0..n-1."""
        if sorted(found[S]) != list(range(len(found[S]))):
            raise KeyError("packed %s state_dict: %s%d has blocks %s" % (cls.FAMILY, stage, S, sorted(found[S])))
        return sorted(found[S])

    def to(self, device):
        for layer in self.convs() + [self.fc]:
            layer.to(device)
        return self

    # ---- the two routes ----
    def __call__(self, images, route="fused", check=True):
        return self.forward(images, route, check)[0]

    def _run(self, images, route, check):
        """(logits, the feature map, its pooled features)."""
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
        return logits, feat, pooled

    # ---- calibration (synthetic models, tests, tools) ----
    def calibrate(self, images):
        """Set every activation quantiser's scale from the max of what reaches it in one `layers` pass: unsigned quantisers
        take max / qmax, signed ones max|x| / qmax; the fc's from the pooled features."""
        def observe(c, t):
            s = (t.abs().max() if c.a_signed else t.clamp(min=0).max()) / c.a_qmax
            c.a_scale = torch.clamp(s, min=1e-8).reshape(1)
        with torch.no_grad():
            pooled = capi.global_avgpool(self._layers(images, observe))
            self.fc.a_scale = torch.clamp(pooled.clamp(min=0).max() / self.fc.a_qmax, min=1e-8).reshape(1)
        return self

    def state_dict_scales(self):
        """{key: tensor} of every activation scale, in the state_dict's key layout."""
        out = {c.name + ".a_quantizer.scale": c.a_scale for c in self.convs()}
        out["fc.a_quantizer.scale"] = self.fc.a_scale
        return out
