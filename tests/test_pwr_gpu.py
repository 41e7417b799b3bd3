"""GPU: the resident-tile 1x1 kernel (qe_conv_pwr.hip) vs the oracle: every instance (tests/pwr_instances.py), planes that
are one tile (14x14: the 4-byte patched tail of the tensor), several tiles (28x28, 56x56), an fp32 `out` that is only
4-byte aligned, one to sixteen strips per wave, channel groups (QE_PWR_GROUPS), more tiles than XCDs, symmetric and asymmetric operands
(S_x / S_w terms), per-tensor weight scales, no bias -- each also with the kernel disabled (QE_PWR=0), and a batch-256
launch checked by batch independence."""
import numpy as np
import pytest

import oracle
import pwr_instances
from quantize_amd import capi
from test_conv_gpu import DEV, _random_case, _run_case, _assert_conv_close, _t, engine  # noqa: F401

pytestmark = pytest.mark.gpu

SHAPES = [
    # N, IC, H, W, OC, K, stride, pad
    (2, 256, 14, 14, 1024, 1, 1, 0),    # ResNet-50 layer3 expansion: whole-plane tiles, 4 strips per wave (8 waves)
    (3, 256, 14, 14, 128, 1, 1, 0),     # fewer than two strips per wave: the flat kernels (pwr_plan refuses it)
    (1, 128, 14, 14, 160, 1, 1, 0),     # 5 strips on 4 waves: fewer than two per wave, the flat kernels
    (2, 64, 14, 14, 256, 1, 1, 0),
    (2, 128, 28, 28, 512, 1, 1, 0),     # ResNet-50 layer2 expansion: 4 tiles of 196 pixels per plane
    (1, 256, 28, 28, 512, 1, 1, 0),     # the dense form of layer2's downsample branch
    (3, 256, 56, 56, 512, 1, 2, 0),     # ResNet-50 layer2.0.downsample: the stride-2 form (even columns of even rows, fetched once per tile)
    (2, 64, 56, 56, 256, 1, 2, 0),      # stride 2, IC = 64
    (1, 128, 56, 56, 512, 1, 2, 0),     # stride 2, IC = 128
    (2, 64, 28, 64, 256, 1, 2, 0),      # stride 2, 64-byte input rows (8 pieces), 14 x 32 output planes = 2 tiles of 224
    (1, 64, 56, 56, 256, 1, 1, 0),      # ResNet-50 layer1 expansion: 14 tiles of 224 pixels per plane
    (2, 256, 56, 56, 128, 1, 1, 0),     # layer2.0.conv1
    (40, 64, 14, 14, 192, 1, 1, 0),     # more tiles than XCDs; 6 strips on 4 waves: the flat kernels
    (1, 128, 28, 16, 128, 1, 1, 0),     # 448-pixel planes; 4 strips on 4 waves: the flat kernels
    (3, 128, 14, 14, 288, 1, 1, 0),     # 9 strips on 4 waves (uneven)
    (5, 64, 28, 28, 512, 1, 1, 0),      # 20 tiles, four strips per wave
    (4, 512, 7, 7, 2048, 1, 1, 0),      # ResNet-50 layer4 expansion: 7x7 planes, 2 images per tile, the tensor's last byte patched
    (8, 512, 7, 7, 512, 1, 1, 0),       # 7x7, one channel group, two strips per wave
    (4, 256, 7, 7, 768, 1, 1, 0),       # 7x7, 4 images per tile, 3 strips per wave
    (8, 128, 7, 7, 1024, 1, 1, 0),      # 7x7, IC = 128
    (5, 512, 7, 7, 1024, 1, 1, 0),      # odd batch: not a whole number of tiles -> the ring kernel keeps it
]


@pytest.mark.parametrize("pwr", ["1", "0"])
def test_pwr_vs_oracle(engine, pwr):
    """pwr = 1: every eligible layer on the resident-tile kernel (one tile per workgroup; the patched
    tail of the tensor in a late tile); 0: kernel disabled."""
    rng = np.random.RandomState(4242)
    env = {"QE_PWR": "0" if pwr == "0" else "2"}      # 2: every eligible layer (default 1 = whole-plane tiles only)
    with capi.knobs(**env):
        for shp in SHAPES:
            for (asgn, zeros, w_pc, bias) in [(1, False, True, True), (0, True, True, True), (1, True, False, False)]:
                case = _random_case(rng, *shp, 8, 1 if asgn else 0, 8, asgn, w_pc=w_pc, a_pc=False, zeros=zeros, bias=bias)
                y, o32, o64 = _run_case(engine, case, via_capi=True)
                assert case["path"] == 1
                _assert_conv_close(y, o64, o32, "pwr=%s %s asgn=%d zeros=%s w_pc=%s" % (pwr, shp, asgn, zeros, w_pc), case["fma"])
                if not zeros:
                    assert np.abs(y.astype(np.float64) - o64).max() <= 1e-5


def test_pwr_every_instance_vs_oracle(engine):
    """Every row of the instance table in fp32 (its plain conv_pwr_kernel / conv_pwr7_kernel instance) against the oracle,
    the operand variants taking turns over the rows."""
    rng = np.random.RandomState(2025)
    variants = [(1, False, True, True), (0, True, True, True), (1, True, False, False)]
    for i, (shp, base, note, env) in enumerate(pwr_instances.ROWS):
        asgn, zeros, w_pc, bias = variants[i % len(variants)]
        with capi.knobs(**(env or {})):
            case = _random_case(rng, *shp, 8, 1 if asgn else 0, 8, asgn, w_pc=w_pc, a_pc=False, zeros=zeros, bias=bias)
            y, o32, o64 = _run_case(engine, case, via_capi=True)
        assert case["path"] == 1
        _assert_conv_close(y, o64, o32, "%s %s (%s) asgn=%d zeros=%s w_pc=%s" % (pwr_instances.kernel_name(base + (False, False)),
                                                                                 shp, note, asgn, zeros, w_pc), case["fma"])


@pytest.mark.parametrize("shape", [(2, 64, 28, 16, 256, 1, 1, 0), (2, 128, 28, 28, 512, 1, 1, 0)], ids=["tw224", "tw196"])
def test_pwr_unaligned_fp32_out(engine, shape):
    """An fp32 `out` 4, 8 and 12 bytes past a 16-byte boundary on a resident-tile layer (tiles of 224 and of 196 pixels):
    the result meets the oracle and nothing outside `out` is written."""
    import torch
    rng = np.random.RandomState(406)
    case = _random_case(rng, *shape, 8, 1, 8, 1, w_pc=True, a_pc=False, zeros=True, bias=True)
    wp, wd, sw, zw = case["w"]
    xp, xd, sx, zx = case["x"]
    N, IC, H, W, OC = shape[:5]
    sh = capi.conv_shape(N, IC, H, W, OC, 1, 1, 1, 0)
    xq = capi.qparam(_t(xp), int(xd[0]), int(xd[1]), _t(sx), _t(zx))
    wq = capi.qparam(_t(wp), int(wd[0]), int(wd[1]), _t(sw), _t(zw))
    chains = [oracle.quantconv2d(xp, xd, sx, zx, wp, wd, sw, zw, case["bias"], 1, 0, mode=m) for m in ("fp32", "fp32_fma")]
    _, o64 = oracle.quantconv2d(xp, xd, sx, zx, wp, wd, sw, zw, case["bias"], 1, 0, mode="f64", return_f64=True)
    n = N * OC * H * W
    with capi.knobs(QE_PWR="2"):
        assert capi.conv_path(sh, xq, wq) == 1
        for off in (1, 2, 3):
            buf = torch.full((n + 8,), -7.5, dtype=torch.float32, device=DEV)
            out = buf[off:off + n].view(N, OC, H, W)
            assert out.data_ptr() % 16 == 4 * off
            capi.quantconv2d(xq, wq, _t(case["bias"]), sh, out=out)
            torch.cuda.synchronize()
            b = buf.cpu().numpy()
            assert (b[:off] == -7.5).all() and (b[off + n:] == -7.5).all(), "offset %d: written outside out" % (4 * off)
            _assert_conv_close(b[off:off + n].reshape(N, OC, H, W), o64, chains[0], "%s out + %d bytes" % (shape, 4 * off),
                               chains[1])


@pytest.mark.parametrize("groups", ["2", "4"])
def test_pwr_channel_groups(engine, groups):
    rng = np.random.RandomState(77)
    with capi.knobs(QE_PWR="2", QE_PWR_GROUPS=groups):
        for shp in [(2, 256, 14, 14, 1024, 1, 1, 0), (1, 128, 28, 28, 512, 1, 1, 0), (1, 64, 56, 56, 256, 1, 1, 0)]:
            case = _random_case(rng, *shp, 8, 0, 8, 1, w_pc=True, a_pc=False, zeros=True, bias=True)
            y, o32, o64 = _run_case(engine, case, via_capi=True)
            _assert_conv_close(y, o64, o32, "groups=%s %s" % (groups, shp), case["fma"])


def test_pwr_batch256_independence(engine):
    """The batch-256 launch geometry (256 / 1024 / 3584 workgroups): image i of the batched call == the same image alone."""
    with capi.knobs(QE_PWR="2"):
        _batch256_independence(engine)


def _batch256_independence(engine):
    import torch
    rng = np.random.RandomState(5)
    for (ic, hw, oc) in [(256, 14, 1024), (128, 28, 512), (64, 56, 256)]:
        n = 256
        xq = torch.from_numpy(rng.randint(-128, 128, size=(n, ic, hw, hw)).astype(np.int8)).cuda()
        wq = torch.from_numpy(rng.randint(-128, 128, size=(oc, ic, 1, 1)).astype(np.int8)).cuda()
        ws = torch.from_numpy(rng.uniform(2.5e-4, 7.5e-4, size=(oc,)).astype(np.float32)).cuda()
        wz = torch.zeros(oc, dtype=torch.float32, device="cuda")
        xs = torch.tensor([2e-3], dtype=torch.float32, device="cuda")
        xz = torch.zeros(1, dtype=torch.float32, device="cuda")
        b = torch.from_numpy(rng.normal(0, 0.1, size=(oc,)).astype(np.float32)).cuda()
        xp, xd = engine.tpack(xq, 8, True)
        wp, wd = engine.tpack(wq, 8, True)
        full = engine.quantconv2d(xp, xd, xs, xz, wp, wd, ws.view(oc, 1, 1, 1), wz.view(oc, 1, 1, 1), b, 1, 0)
        for i in (0, 1, 100, 255):
            xpi, xdi = engine.tpack(xq[i:i + 1].contiguous(), 8, True)
            one = engine.quantconv2d(xpi, xdi, xs, xz, wp, wd, ws.view(oc, 1, 1, 1), wz.view(oc, 1, 1, 1), b, 1, 0)
            assert torch.equal(full[i:i + 1], one), (ic, hw, oc, i)
        # and against plain integer arithmetic on one image
        ref = torch.nn.functional.conv2d(xq[255:256].double(), wq.double()) * (2e-3 * ws.double().view(1, oc, 1, 1)) + b.double().view(1, oc, 1, 1)
        assert (full[255:256].double() - ref).abs().max().item() <= 1e-5


WIDE_SHAPES = [
    # N, IC, H, W, OC, K, stride, pad -- deep 1x1 reductions into a multiple of 256 output channels
    (2, 1024, 14, 14, 256, 1, 1, 0),    # ResNet-50 layer3 reduction: whole-plane tiles of 224 slots
    (1, 1024, 14, 14, 512, 1, 1, 0),    # layer4.0.conv1: two channel tiles
    (2, 512, 28, 28, 256, 1, 1, 0),     # layer3.0.conv1: 160-pixel tiles (5 column tiles), ragged last tile
    (1, 512, 14, 14, 1024, 1, 1, 0),    # the dense form of layer3's downsample branch
    (3, 640, 12, 12, 256, 1, 1, 0),     # 144-pixel planes, 5 stages of 128 channels
    (2, 512, 28, 28, 1024, 1, 2, 0),    # strided: gather pass + the dense problem above
]


def test_deep_1x1_reductions_vs_oracle(engine):
    """Deep 1x1 reductions into a multiple of 256 output channels (ResNet-50 layer3 / layer4 shapes, their strided form)
    on the kernels the planner picks by default, against the oracle."""
    rng = np.random.RandomState(808)
    for shp in WIDE_SHAPES:
        for (asgn, zeros, w_pc, bias) in [(1, False, True, True), (0, True, True, True), (1, True, False, False)]:
            case = _random_case(rng, *shp, 8, 1 if asgn else 0, 8, asgn, w_pc=w_pc, a_pc=False, zeros=zeros, bias=bias)
            y, o32, o64 = _run_case(engine, case, via_capi=True)
            assert case["path"] == 1
            _assert_conv_close(y, o64, o32, "%s asgn=%d zeros=%s" % (shp, asgn, zeros), case["fma"])
            if not zeros:
                assert np.abs(y.astype(np.float64) - o64).max() <= 1e-5
