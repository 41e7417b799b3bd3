"""The synthetic packed models are what every forward figure in the README was measured on and what most model tests run:
their bytes must not drift.  SHA-256 over the sorted keys of a state_dict (key, dtype, shape and bytes of each tensor),
against constants recorded at the commit before the builders moved into quantize_amd/synthetic.py."""
import hashlib

import pytest

from quantize_amd import packed_mobilenet, packed_resnet, packed_vit


def digest(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        t = sd[k].detach().cpu().contiguous()
        for part in (k, str(t.dtype), str(tuple(t.shape))):
            h.update(part.encode())
        h.update(t.numpy().tobytes())
    return h.hexdigest()


CASES = [
    ("resnet18", lambda: packed_resnet.synthetic_state_dict("resnet18", num_classes=10, width=8, seed=3),
     "f69d38d6f61cb013352d34d64d625355c52b21f8d17245f7e387a4409c46ce1d"),
    ("resnext50", lambda: packed_resnet.synthetic_state_dict("resnet50", num_classes=10, width=16, groups=4, width_per_group=16,
                                                             seed=1),
     "eaee07fa5cf8cd556f1ff6827ea5eac88bf0de13064e18c0cb3970433defaabb"),
    ("resnet50_w4a6", lambda: packed_resnet.synthetic_state_dict("resnet50", num_classes=10, width=8, w_bits=4, a_bits=6),
     "16198dfe3f05a238cd3cca1fc6549f7beab92d2c1d648f4b2bc5f2b01b0c8cea"),
    ("mobilenet", lambda: packed_mobilenet.synthetic_state_dict(width=8, num_classes=16, seed=2),
     "0a0c352fd95b9a640f68a629b1861ee91207f00434dfeebd9900fb6353b9383c"),
    ("mobilenet_depth", lambda: packed_mobilenet.synthetic_state_dict(width=8, num_classes=5, depth=(1, 1, 3)),
     "eb843f12fbe626cfb6aa5331549a0ebb8196277240637f8ec6956609557e4cef"),
    ("vit_tiny", lambda: packed_vit.synthetic_state_dict("vit_tiny_test"),
     "bee97887d7d35e46f5b3f8398b126907e8c7b92055b720b79d889c02c253d461"),
    ("vit_tiny_over", lambda: packed_vit.synthetic_state_dict("vit_tiny_test", depth=3, mlp=128, width=32),
     "c8f3aca2f9185715361ce2339f840784a60711e39a156211683b0b5e92fb6eca"),
]


@pytest.mark.parametrize("name,build,want", CASES, ids=[c[0] for c in CASES])
def test_synthetic_state_dict_bytes(name, build, want):
    assert digest(build()) == want, name
