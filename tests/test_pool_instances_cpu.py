"""CPU: the instance table of qe_avgpool2d_codes against the host-side plan, and tests/pool_ref.py against the reference's own
packed forwards (G13) and against torch.

The bound of the average forms: a sequential fp32 sum of cnt terms and one division is within cnt * u (first order) of the exact
mean, one more u for the second order: (cnt + 1) * 2^-24 * max|tap| per output."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pool_instances as pi
import pool_ref
from conftest import Golden
from quantize_amd import capi

U = 2.0 ** -24


@pytest.fixture(scope="module")
def g13():
    return Golden("g13_pool.npz")


def _case(g13, key):
    x = g13._z[str(g13.get(key, "xkey"))]
    sd = {f: g13.get(key, "sd_a_quantizer." + f) for f in ("scale", "zero", "qmin", "qmax")}
    return x, sd, g13.get(key, "y_packed"), [int(v) for v in g13.get(key, "geom")]


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_symbols_and_instance_names():
    for name in ("qe_quant_relu", "qe_quant_maxpool2d", "qe_quant_adaptive_avgpool2d", "qe_avgpool2d_codes", "qe_avgpool2d_codes_path"):
        assert name in capi.PROTOTYPES and hasattr(capi.lib(), name)
    assert capi.POOL_KERNELS == ("plain", "pair", "plane")


def test_every_instance_is_reached_in_every_epilogue():
    seen = set()
    for k, row in enumerate(pi.ROWS):
        for ep in pi.EPILOGUES:
            for relu in (False, True):
                got = pi.path(k, ep, relu)
                # a sub-8-bit consumer moves a problem to the plain instance; without codes the geometry alone decides
                want = row[0] if (ep != "out" or row[7] != "u4") else ("pair" if row[2] == 2 else "plane" if pi.out_hw(row) == (1, 1) else "plain")
                assert got >= 0 and capi.POOL_KERNELS[got] == want, (pi.row_id(k), ep, relu)
                seen.add((capi.POOL_KERNELS[got], ep))
    assert seen == {(i, ep) for i in capi.POOL_KERNELS for ep in pi.EPILOGUES}


def test_the_instance_does_not_depend_on_an_alignment():
    for k in range(len(pi.ROWS)):
        for ep in pi.EPILOGUES:
            want = pi.path(k, ep)
            for x_ptr, out_ptr, codes_ptr in ((257, 260, 259), (263, 268, 257), (256, 256, 256)):
                assert pi.path(k, ep, x_ptr=x_ptr, out_ptr=out_ptr, codes_ptr=codes_ptr) == want, (pi.row_id(k), ep)


def test_refused_requests_have_no_instance():
    fake = pi._Fake
    x4 = capi.qparam(fake(1), 4, 0, fake(1), fake(1))
    assert capi.avgpool2d_codes_path(x4, 2, 3, 8, 8, 2) == -1                            # sub-8-bit x
    x8 = capi.qparam(fake(1), 8, 0, fake(1), fake(1))
    assert capi.avgpool2d_codes_path(x8, 1, 1, 2, 32897, 0, output_size=(1, 1)) == -1    # 65794 * 255 >= 2^24
    assert capi.avgpool2d_codes_path(x8, 1, 1, 273, 241, 0, output_size=(1, 1)) == 2     # 65793 * 255 == 2^24 - 1
    assert capi.avgpool2d_codes_path(x8, 1, 1, 300, 300, 257, 1) == -1                   # a fixed window as large
    assert capi.avgpool2d_codes_path(x8, 1, 1, 8, 8, 3, 2, out=0) == -1                  # neither out nor codes


@pytest.mark.parametrize("layer", ["relu", "maxpool321", "maxpool2"])
def test_pool_ref_reproduces_g13_relu_and_max_bit_for_bit(g13, layer):
    keys = [k for k in g13.index if k.startswith("p_%s_" % layer)]
    assert len(keys) == 4
    for key in keys:
        x, sd, want, geom = _case(g13, key)
        q = (sd["scale"], sd["zero"], float(sd["qmin"]), float(sd["qmax"]))
        got = pool_ref.quant_relu(x, *q) if layer == "relu" else pool_ref.quant_maxpool2d(x, *q, *geom)
        assert same_bits(got, want), key


@pytest.mark.parametrize("layer", ["avg11", "avg57"])
def test_pool_ref_reproduces_g13_avg_within_the_bound(g13, layer):
    keys = [k for k in g13.index if k.startswith("p_%s_" % layer)]
    assert len(keys) == 4
    for key in keys:
        x, sd, want, geom = _case(g13, key)
        got, cnt, amax = pool_ref.quant_adaptive_avgpool2d(x, sd["scale"], sd["zero"], float(sd["qmin"]), float(sd["qmax"]), *geom)
        bound = (cnt + 1) * U * amax
        err = np.abs(got.astype(np.float64) - want.astype(np.float64))
        print("%s: max err %.3g, min bound %.3g" % (key, err.max(), bound.min()))
        assert (err <= bound).all(), key


def test_adaptive_windows_equal_torchs():
    axes = {(row[1][2], pi.out_hw(row)[0]) for row in pi.ROWS if not row[2]} | {(row[1][3], pi.out_hw(row)[1]) for row in pi.ROWS if not row[2]}
    axes |= {(s[2], o[0]) for s in pi.SHAPES for o in pi.AVG_SIZES} | {(s[3], o[1]) for s in pi.SHAPES for o in pi.AVG_SIZES}
    for n_in, n_out in sorted(axes):
        member = F.adaptive_avg_pool1d(torch.eye(n_in).unsqueeze(0), n_out)[0].numpy() > 0        # [i, o]: i in window o
        for o, (lo, hi) in enumerate(pool_ref.windows(n_in, n_out)):
            assert np.flatnonzero(member[:, o]).tolist() == list(range(lo, hi)), (n_in, n_out, o)


def test_kernel2_codes_value_equals_avg_pool2d_of_the_dequantised_codes():
    rng = np.random.default_rng(5)
    stored = rng.integers(0, 256, size=(2, 6, 8, 8)).astype(np.uint8)
    for sign, scale, zero_p in ((0, [0.0371], [117.37]), (1, np.linspace(0.01, 0.05, 6), np.linspace(-20.5, 31.25, 6))):
        q = pool_ref.decode(stored, sign)
        s, z = np.asarray(scale, np.float32), np.asarray(zero_p, np.float32)
        got = pool_ref.avgpool2d_codes(q, s, z, 2, 2, 4, 4)
        deq = (torch.from_numpy(q.astype(np.float32)) - torch.from_numpy(pool_ref._bc(z, 6))) * torch.from_numpy(pool_ref._bc(s, 6))
        want = F.avg_pool2d(deq, 2).numpy()
        amax = F.max_pool2d(deq.abs(), 2).numpy().astype(np.float64)
        err = np.abs(got.astype(np.float64) - want.astype(np.float64))
        print("sign %d: max err %.3g, min bound %.3g" % (sign, err.max(), (5 * U * amax).min()))
        assert (err <= 5 * U * amax).all()


def test_from_state_dict_pool_geometry(g13):
    from quantize_amd import packed
    sd = {}
    for name, key in (("act", "p_relu_s8"), ("pool", "p_maxpool321_u8ac"), ("head.avg", "p_avg57_u4a")):
        for f in ("scale", "zero", "qmin", "qmax"):
            sd["%s.a_quantizer.%s" % (name, f)] = torch.from_numpy(np.asarray(g13.get(key, "sd_a_quantizer." + f)))
    assert packed.from_state_dict(sd) == {}                                     # the default: unchanged behaviour
    layers = packed.from_state_dict(sd, pool_geometry={"act": ("relu",), "pool": ("maxpool", 3, 2, 1), "head.avg": ("adaptive_avgpool", (5, 7))})
    assert [type(layers[k]).__name__ for k in ("act", "pool", "head.avg")] == ["PackedReLU", "PackedMaxPool2d", "PackedAdaptiveAvgPool2d"]
    assert (layers["pool"].kernel, layers["pool"].stride, layers["pool"].padding) == (3, 2, 1) and layers["pool"].a_scale.numel() == 6
    assert (layers["head.avg"].a_bits, layers["head.avg"].a_signed, layers["head.avg"].output_size) == (4, False, (5, 7))
    with pytest.raises(ValueError):
        packed.from_state_dict(sd, pool_geometry={"act": ("avgpool", 2)})
    with pytest.raises(capi.QeError):
        packed.PackedMaxPool2d.from_state_dict(sd, "pool.", kernel_size=3, dilation=2)
