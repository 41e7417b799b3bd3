"""GPU: the module forms qe_quant_relu, qe_quant_maxpool2d and qe_quant_adaptive_avgpool2d against tests/pool_ref.py -- bit for
bit, NaN-aware: the header's fp32 sequences are the contract -- and the reference's own packed forwards (G13) through the
Packed* classes.

The average form additionally against float64: a sequential fp32 sum of cnt terms and one division is within cnt * u of the exact
mean to first order, one more u for the second order: |out - exact| <= (cnt + 1) * 2^-24 * max|qdq(tap)| per output.  G13's
averages come from torch, which is within the same bound of float64, hence twice the bound between the two."""
import numpy as np
import pytest
import torch

import pool_instances as pi
import pool_ref
from conftest import Golden
from quantize_amd import capi, packed

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24


@pytest.fixture(scope="module")
def g13():
    return Golden("g13_pool.npz")


def eq_nan(got, want, bits=True):
    """Same NaN positions, and elsewhere the same bits (bits=False: the same values, where the header leaves the sign of a zero open)."""
    if got.shape != want.shape or got.dtype != np.float32 or want.dtype != np.float32:
        return False
    nan = np.isnan(want)
    if not np.array_equal(nan, np.isnan(got)):
        return False
    return np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]) if bits else np.array_equal(got[~nan], want[~nan])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def off4(t):
    """A copy of t that starts 4 bytes past a 16-byte boundary."""
    raw = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    assert raw.data_ptr() % 16 == 0
    v = raw[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def rq_of(q):
    scale, zero, lo, hi = q
    return capi.requant(dev(scale), dev(zero), lo, hi, 8, 0)          # n_bits and sign are ignored by the module forms


CASES = [(s, w) for s in pi.SHAPES for w in pi.QUANTISERS]
IDS = ["%s-%d%s%s" % ("x".join(map(str, s)), w[0], "su"[1 - w[1]], "c" if w[2] else "") for s, w in CASES]


@pytest.mark.parametrize("shape,which", CASES, ids=IDS)
def test_relu(shape, which):
    q = pi.module_quantiser(shape, which)
    for nonfinite in (False, True):
        x = pi.module_input(shape, nonfinite=nonfinite)
        want = pool_ref.quant_relu(x, *q)
        assert eq_nan(capi.quant_relu(dev(x), rq_of(q)).cpu().numpy(), want)
        # x and out 4 bytes off a 16-byte boundary, then in place
        xm = off4(dev(x))
        out = off4(torch.zeros(shape, dtype=torch.float32, device=DEV))
        assert capi.quant_relu(xm, rq_of(q), out=out) is out and eq_nan(out.cpu().numpy(), want)
        assert torch.equal(torch.nan_to_num(xm.cpu()), torch.nan_to_num(torch.from_numpy(x)))
        assert capi.quant_relu(xm, rq_of(q), out=xm) is xm and eq_nan(xm.cpu().numpy(), want)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1021, 1024, 1027, 4099])
def test_relu_flat_tails(n):
    """Flat tensors whose length is no multiple of the 4 elements of a thread, per channel with inner = 5: channels change inside a
    thread's elements, at every phase against the 16-byte store grid."""
    rng = np.random.default_rng(n)
    x = rng.normal(0, 0.8, size=n).astype(np.float32)
    scale, zero = np.array([0.011, 0.02, 0.017], np.float32), np.array([0.0, -100.0, -31.5], np.float32)
    ch = (np.arange(n) // 5) % 3
    want = pool_ref.relu(pool_ref.qdq(x.reshape(1, n, 1, 1), scale[ch], zero[ch], 0.0, 255.0)).reshape(n)
    for lead in (0, 1, 2, 3):
        raw = torch.zeros(n + 8, dtype=torch.float32, device=DEV)
        out = raw[lead:lead + n]
        capi.quant_relu(dev(x), capi.requant(dev(scale), dev(zero), 0.0, 255.0, 8, 0), inner=5, out=out)
        assert eq_nan(out.cpu().numpy(), want), lead
        assert float(raw[:lead].abs().sum()) == 0 and float(raw[lead + n:].abs().sum()) == 0


@pytest.mark.parametrize("shape,which", CASES, ids=IDS)
def test_maxpool(shape, which):
    q = pi.module_quantiser(shape, which)
    for nonfinite in (False, True):
        x = pi.module_input(shape, seed=1, nonfinite=nonfinite)
        for kernel, stride, padding in pi.MAX_GEOMETRIES:
            want = pool_ref.quant_maxpool2d(x, *q, kernel, stride, padding)
            got = capi.quant_maxpool2d(dev(x), rq_of(q), kernel, stride, padding)
            assert eq_nan(got.cpu().numpy(), want), (kernel, stride, padding, nonfinite)
            if nonfinite:
                assert np.isnan(want[0, 0, 0, 0]) and np.isnan(want).sum() < want.size // 2
            out = off4(torch.zeros(want.shape, dtype=torch.float32, device=DEV))
            capi.quant_maxpool2d(off4(dev(x)), rq_of(q), kernel, stride, padding, out=out)
            assert eq_nan(out.cpu().numpy(), want), (kernel, stride, padding, "off4")


def test_maxpool_where_max_does_not_commute():
    """A plane whose scale is negative: qdq is non-increasing there, so the kernel goes tap by tap.  The sign of a zero is open."""
    shape = (2, 5, 9, 11)
    scale, zero, lo, hi = pi.module_quantiser(shape, (8, 0, True))
    scale = scale.copy()
    scale[1], scale[4] = -scale[1], -scale[4]
    x = pi.module_input(shape, seed=2, nonfinite=True)
    for kernel, stride, padding in pi.MAX_GEOMETRIES:
        want = pool_ref.quant_maxpool2d(x, scale, zero, lo, hi, kernel, stride, padding)
        got = capi.quant_maxpool2d(dev(x), rq_of((scale, zero, lo, hi)), kernel, stride, padding).cpu().numpy()
        assert eq_nan(got, want, bits=False)
        mono = np.array([0, 2, 3])
        assert eq_nan(np.ascontiguousarray(got[:, mono]), np.ascontiguousarray(want[:, mono]))


def test_unsupported_maxpool_arguments():
    x = dev(pi.module_input((1, 2, 5, 5)))
    rq = rq_of(pi.module_quantiser((1, 2, 5, 5), (8, 0, False)))
    for kw in (dict(dilation=2), dict(return_indices=True), dict(ceil_mode=True)):
        with pytest.raises(capi.QeError, match="not supported"):
            capi.quant_maxpool2d(x, rq, 3, 2, 1, **kw)
    with pytest.raises(capi.QeError, match="invalid argument"):
        capi.quant_maxpool2d(x, rq, 2, 2, 2)                           # 2 * padding > kernel


@pytest.mark.parametrize("shape,which", CASES, ids=IDS)
def test_adaptive_avgpool(shape, which):
    q = pi.module_quantiser(shape, which)
    for nonfinite in (False, True):
        x = pi.module_input(shape, seed=3, nonfinite=nonfinite)
        y64 = pool_ref.qdq(x, *q).astype(np.float64)
        for OH, OW in pi.AVG_SIZES:
            want, cnt, amax = pool_ref.quant_adaptive_avgpool2d(x, *q, OH, OW)
            got = capi.quant_adaptive_avgpool2d(dev(x), rq_of(q), (OH, OW)).cpu().numpy()
            assert eq_nan(got, want), (OH, OW, nonfinite)
            out = off4(torch.zeros(want.shape, dtype=torch.float32, device=DEV))
            capi.quant_adaptive_avgpool2d(off4(dev(x)), rq_of(q), (OH, OW), out=out)
            assert eq_nan(out.cpu().numpy(), want), (OH, OW, "off4")
            if not nonfinite:
                exact = np.empty(want.shape)
                for oh, (h0, h1) in enumerate(pool_ref.windows(shape[2], OH)):
                    for ow, (w0, w1) in enumerate(pool_ref.windows(shape[3], OW)):
                        exact[:, :, oh, ow] = y64[:, :, h0:h1, w0:w1].mean(axis=(2, 3))
                err, bound = np.abs(got - exact), (cnt + 1) * U * amax
                print("%s -> %dx%d: max err %.3g of bound %.3g" % (shape, OH, OW, err.max(), bound[err >= err.max()].min()))
                assert (err <= bound).all(), (OH, OW)
            else:
                assert np.isnan(want[0, 0, 0, 0]) and np.isfinite(want).any()


@pytest.mark.parametrize("shape", [(1, 3, 20, 13), (2, 70, 1, 241), (1, 65, 11, 22), (1, 2, 23, 21)], ids=lambda s: "x".join(map(str, s)))
def test_global_avgpool_in_tiles(shape):
    """(1, 1) on planes of more than one 241-element tile (260, 483: a second and a third, short tile), of exactly one, and of one
    even-sized tile, on more planes than a workgroup takes: the running sum crosses the tiles in the contract's order."""
    q = pi.module_quantiser(shape, (8, 0, True))
    x = pi.module_input(shape, seed=4)
    want = pool_ref.quant_adaptive_avgpool2d(x, *q, 1, 1)[0]
    assert eq_nan(capi.quant_adaptive_avgpool2d(dev(x), rq_of(q), 1).cpu().numpy(), want)
    out = off4(torch.zeros(want.shape, dtype=torch.float32, device=DEV))
    capi.quant_adaptive_avgpool2d(off4(dev(x)), rq_of(q), 1, out=out)
    assert eq_nan(out.cpu().numpy(), want)


def _g13_case(g13, key):
    x = g13._z[str(g13.get(key, "xkey"))]
    sd = {"m.a_quantizer." + f: torch.from_numpy(np.asarray(g13.get(key, "sd_a_quantizer." + f))) for f in ("scale", "zero", "qmin", "qmax")}
    return x, sd, g13.get(key, "y_packed"), [int(v) for v in g13.get(key, "geom")]


def test_g13_through_the_packed_classes(g13):
    assert len(g13.index) == 20
    for key in g13.index:
        x, sd, want, geom = _g13_case(g13, key)
        layer = key.split("_")[1]
        if layer == "relu":
            m = packed.PackedReLU.from_state_dict(sd, "m.")
        elif layer.startswith("maxpool"):
            m = packed.PackedMaxPool2d.from_state_dict(sd, "m.", kernel_size=geom[0], stride=geom[1], padding=geom[2])
        else:
            m = packed.PackedAdaptiveAvgPool2d.from_state_dict(sd, "m.", output_size=tuple(geom))
        got = m.to(DEV)(dev(x)).cpu().numpy()
        if layer.startswith("avg"):
            q = (np.asarray(sd["m.a_quantizer.scale"]), np.asarray(sd["m.a_quantizer.zero"]), m.a_qmin, m.a_qmax)
            _, cnt, amax = pool_ref.quant_adaptive_avgpool2d(x, *q, *geom)
            err = np.abs(got.astype(np.float64) - want.astype(np.float64))
            assert (err <= 2 * (cnt + 1) * U * amax).all(), key
        else:
            assert eq_nan(got, want), key
    # the same layers through the module-level loader, and the in-place ReLU
    x, sd, want, _ = _g13_case(g13, "p_relu_u8ac")
    m = packed.from_state_dict(sd, pool_geometry={"m": ("relu", True)})["m"].to(DEV)
    xd = dev(x)
    assert m(xd) is xd and eq_nan(xd.cpu().numpy(), want)
    # AvgPool2d(2) on an even plane is the adaptive kernel's windows
    x, sd, _, _ = _g13_case(g13, "p_avg57_u8a")
    xe = np.ascontiguousarray(x[:, :, :, :8])
    ap = packed.PackedAvgPool2d.from_state_dict(sd, "m.", kernel_size=2).to(DEV)
    q = (np.asarray(sd["m.a_quantizer.scale"]), np.asarray(sd["m.a_quantizer.zero"]), ap.a_qmin, ap.a_qmax)
    assert eq_nan(ap(dev(xe)).cpu().numpy(), pool_ref.quant_adaptive_avgpool2d(xe, *q, 4, 4)[0])
    with pytest.raises(ValueError):
        ap(dev(x))                                                     # W = 9: no fp32 kernel for it, and nothing in its place
