"""GPU: the packed ResNet on the engine against an independent float64 model, bit for bit.

The models come from resnet_exact.exact_state_dict: power-of-two scales, integer zero points, biases on their grids and
partial sums below 2^24 grid units, so fp32 rounds nothing and both routes of PackedResNet must equal Float64ResNet exactly
-- layer4 features of every image, and the logits of every image whose fc codes cannot flip on the fp32 mean of the 7x7
average pooling.  Every case runs both routes against the float64 model (not only against each other) and asserts which
residual block-end path it took."""
import time

import pytest
import torch

from quantize_amd import capi
from quantize_amd.packed_resnet import PackedResNet
from resnet_exact import Float64ResNet, check_code_spread, exact_state_dict, load_g8

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# every fallback of the fused route in one model: the stem's consumer and one inside a block signed (no ReLU fold), a
# non-zero integer zero point, per-channel activation scales inside a block and on a block's conv1 (two-pass block end),
# a downsample quantiser that differs from its block's conv1, and an fc quantiser with a non-zero zero point
FALLBACKS = {"layer1.0.conv1": {"signed": True}, "layer2.1.conv2": {"signed": True}, "layer3.1.conv3": {"zero": -3},
             "layer2.2.conv2": {"per_channel": True}, "layer3.3.conv1": {"per_channel": True},
             "layer3.0.downsample.0": {"scale_mult": 2.0}, "fc": {"zero": -3}}


@pytest.fixture(scope="module")
def r50():
    sd = exact_state_dict("resnet50", seed=0)
    return sd, Float64ResNet(sd)


def _engine(sd):
    return PackedResNet.from_state_dict({k: v.to(DEV) for k, v in sd.items()})


def _images(N, seed, size=224):
    """N x 3 x H x W normal images; size is one side or (H, W)."""
    H, W = (size, size) if isinstance(size, int) else size
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(N, 3, H, W, generator=g)


def _first_departure(model, ref, x):
    """The first conv whose fp32 input on the layers route differs from the float64 model's."""
    got = {}
    model._layers(x.to(DEV), lambda c, t: got.setdefault(c.name, t.detach().cpu().double()))
    for name, t in ref.inputs.items():
        if name in got and not torch.equal(got[name], t):
            return name
    return "none (the difference is after layer4)"


def _check(model, f64, x, label):
    """Both routes equal the float64 model (features always, logits of the images with no near-tie fc code)."""
    t0 = time.perf_counter()
    ref = f64.forward(x)
    check_code_spread(ref)
    assert ref.ties > 0, "%s: no exact .5 tie was exercised" % label
    assert ref.logits.std() > 0
    feat, logits = ref.features.float(), ref.logits.float()
    keep = ~ref.near_tie
    assert int(ref.near_tie.sum()) <= x.shape[0] // 4, "%s: %d near-tie images" % (label, int(ref.near_tie.sum()))
    for route in ("fused", "layers"):
        lg, ft = model.forward(x.to(DEV), route=route)
        lg, ft = lg.cpu(), ft.cpu()
        if not torch.equal(ft, feat):
            n = int((ft != feat).sum())
            raise AssertionError("%s, route=%s: %d layer4 features differ from the float64 model; the layers route departs "
                                 "first at %s" % (label, route, n, _first_departure(model, ref, x)))
        assert torch.equal(lg[keep], logits[keep]), "%s, route=%s: logits differ from the float64 model" % (label, route)
        assert lg.std() > 0
    print("%s: %d exact ties, %d near-tie images excluded, %.2f s" % (label, ref.ties, int(ref.near_tie.sum()),
                                                                      time.perf_counter() - t0))
    return ref


def test_resnet50_w8a8_batch2(r50):
    sd, f64 = r50
    model = _engine(sd)
    assert model.residual_paths(2) == [1] * 16                 # every block end on the conv kernel's RES epilogue
    _check(model, f64, _images(2, 11), "a: ResNet-50 W8A8 N=2")


def test_resnet50_w8a8_batch3(r50):
    sd, f64 = r50
    model = _engine(sd)
    assert model.residual_paths(3) == [1] * 13 + [0] * 3      # the three 7x7 block ends take two passes
    _check(model, f64, _images(3, 12), "b: ResNet-50 W8A8 N=3")


def test_resnet50_w8a8_batch1(r50):
    sd, f64 = r50
    _check(_engine(sd), f64, _images(1, 13), "c: ResNet-50 W8A8 N=1")


def test_resnet50_pwr_disabled(r50):
    sd, f64 = r50
    with capi.knobs(QE_PWR="0"):
        model = _engine(sd)
        assert model.residual_paths(2) == [0] * 16                 # every block end on the two-pass route
        _check(model, f64, _images(2, 14), "d: ResNet-50 W8A8 QE_PWR=0")


def test_resnet50_fallbacks():
    sd = exact_state_dict("resnet50", seed=1, variants=FALLBACKS)
    model = _engine(sd)
    assert [c.name for c in model.convs() if not c.folds_relu] == ["conv1", "layer1.0.conv1", "layer2.1.conv2",
                                                                   "layer3.1.conv3"]
    assert model.stages[2][3].convs[0].a_scale.numel() == 1024 and model.stages[1][2].convs[1].a_scale.numel() == 128
    assert len(set(model.stages[1][2].convs[1].a_scale.tolist())) > 1      # the channels' scales differ
    ds = model.stages[2][0]
    assert ds.downsample.q_key != ds.convs[0].q_key
    assert model.fc.a_zero.tolist() == [-3.0]
    assert model.residual_paths(2) == [1] * 9 + [0] + [1] * 6   # layer3.2's end writes per-channel codes: two passes
    _check(model, Float64ResNet(sd), _images(2, 15), "e: ResNet-50 W8A8 fallbacks")


def test_resnet50_w4a4():
    sd = exact_state_dict("resnet50", seed=2, w_bits=4, a_bits=4)
    _check(_engine(sd), Float64ResNet(sd), _images(2, 16), "f: ResNet-50 W4A4")


@pytest.mark.parametrize("a_bits", [8, 6])
def test_resnet18(a_bits):
    sd = exact_state_dict("resnet18", seed=3, a_bits=a_bits)
    model = _engine(sd)
    assert model.residual_paths(2) == [0] * 8                  # BasicBlock 3x3 block ends: two passes
    _check(model, Float64ResNet(sd), _images(2, 17), "g: ResNet-18 W8A%d" % a_bits)


def test_resnet50_batch256(r50):
    sd, f64 = r50
    model = _engine(sd)
    assert model.residual_paths(256) == [1] * 16
    x = _images(256, 18)
    lf, ff = model.forward(x.to(DEV), route="fused")
    ll, fl = model.forward(x.to(DEV), route="layers")
    assert torch.equal(ff, fl) and torch.equal(lf, ll)
    ff, lf = ff.cpu(), lf.cpu()
    ties = 0
    for i in (0, 131, 255):
        ref = f64.forward(x[i:i + 1])
        ties += ref.ties
        assert torch.equal(ff[i:i + 1], ref.features.float()), "batch-256 row %d: features differ from float64" % i
        if not bool(ref.near_tie[0]):
            assert torch.equal(lf[i:i + 1], ref.logits.float()), "batch-256 row %d: logits differ from float64" % i
    assert ties > 0
    print("h: ResNet-50 W8A8 N=256, rows 0 / 131 / 255: %d exact ties" % ties)


# Off the 224 x 224 ResNet-50 geometry: non-square images, a narrower network and odd plane sizes move the block ends onto
# other resident-tile instances or off them.  Each model is calibrated at the geometry it runs.
GEOMETRIES = [
    # label, exact_state_dict arguments, image size, block-end paths at N = 2
    ("i: ResNet-50 at 224x320", dict(image_size=(224, 320)), (224, 320),
     [1] * 7 + [0] * 9),             # layer1 56x80 on <4,2,224>, layer2 28x40 on <4,4,224>; 14x20 and 7x10: two passes
    ("j: ResNet-50 width 32", dict(width=32), (224, 224),
     [0] * 3 + [1] * 10 + [0] * 3),  # IC = 32 and 256 -> 1024 @7x7 take two passes; layer2 on <4,2,196>, layer3 <4,4,196>
    ("k: ResNet-50 at 200x200", dict(image_size=200), (200, 200),
     [0] * 13 + [1] * 3),            # planes 50 / 25 / 13 / 7: every stride-2 layer rounds; only layer4 (pwr7) fuses
]


@pytest.mark.parametrize("label,kw,size,paths", GEOMETRIES, ids=["224x320", "width32", "200x200"])
def test_resnet50_other_geometries(label, kw, size, paths):
    sd = exact_state_dict("resnet50", seed=20, **kw)
    model = _engine(sd)
    assert model.residual_paths(2, *size) == paths
    ref = _check(model, Float64ResNet(sd), _images(2, 21, size), label)
    H, W = size
    for _ in range(5):
        H, W = (H + 1) // 2, (W + 1) // 2
    assert tuple(ref.features.shape[2:]) == (H, W)


@pytest.mark.parametrize("case", ["m_bottleneck", "m_basic"])
def test_g8_reference_resnet(case):
    """Both routes on a state_dict the reference's own QuantConv2d / QuantLinear modules wrote equal the reference's packed
    forward of the whole model (layer4 features and logits) bit for bit."""
    sd, images, feat, logits = load_g8()[case]
    model = _engine(sd)
    for route in ("fused", "layers"):
        lg, ft = model.forward(images.to(DEV), route=route)
        assert torch.equal(ft.cpu(), feat), "%s, route=%s: features differ from the reference" % (case, route)
        assert torch.equal(lg.cpu(), logits), "%s, route=%s: logits differ from the reference" % (case, route)
