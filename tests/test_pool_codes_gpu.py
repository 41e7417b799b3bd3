"""GPU: qe_avgpool2d_codes on every row of tests/pool_instances.py x epilogue (out, codes, both) x relu off and on.

Exact regime (scale a power of two, zero' an integer): every step of the header's sequence but the last division is exact, so
`out` is the exact rational s * sum / cnt rounded once -- built here from int64 numerators -- and equals pool_ref bit for bit.
Parity regime (ordinary scale and zero'): `out` equals pool_ref bit for bit: the sequence is the contract.
`codes` equals qe_quantize_pack of the call's own `out` byte for byte, the codes-only call gives the same codes, status is 0."""
import ctypes
import fractions

import numpy as np
import pytest
import torch

import pool_instances as pi
import pool_ref
from quantize_amd import capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def rounded_once(num, den):
    """int64 numerators over float64-exact denominators (cnt * 2^k) -> the nearest float32, ties to even."""
    r64 = num.astype(np.float64) / den                       # correctly rounded: within 2^-53 of num / den
    f = r64.astype(np.float32)
    half = np.spacing(np.abs(f)).astype(np.float64) / 2
    near_tie = np.abs(np.abs(r64 - f.astype(np.float64)) - half) <= np.abs(r64) * 2.0 ** -50
    for i in np.flatnonzero(near_tie.reshape(-1)):           # a float64 quotient this close to a tie decides nothing: exactly
        exact = fractions.Fraction(int(num.reshape(-1)[i])) / fractions.Fraction(float(np.broadcast_to(den, num.shape).reshape(-1)[i]))
        c = [np.float32(f.reshape(-1)[i])]
        c += [np.nextafter(c[0], np.float32(-np.inf)), np.nextafter(c[0], np.float32(np.inf))]
        c.sort(key=lambda v: (abs(fractions.Fraction(float(v)) - exact), int(np.float32(v).view(np.uint32)) & 1))
        f.reshape(-1)[i] = c[0]
    return f


def exact_value(k, relu):
    row = pi.ROWS[k]
    o = pi.operands(k, "exact")
    N, C, H, W = row[1]
    OH, OW = pi.out_hw(row)
    z = np.broadcast_to(o["zx"].astype(np.int64), (C,) if o["zx"].size == C else (1,))
    z = np.full(C, z[0]) if z.size == 1 else z
    s = np.full(C, o["sx"][0], np.float64) if o["sx"].size == 1 else o["sx"].astype(np.float64)
    d = o["q"] - z.reshape(1, C, 1, 1)
    if relu:
        d = np.maximum(d, 0)
    rows = pool_ref.fixed_windows(H, row[2], row[3]) if row[2] else pool_ref.windows(H, OH)
    cols = pool_ref.fixed_windows(W, row[2], row[3]) if row[2] else pool_ref.windows(W, OW)
    num, den = np.empty((N, C, OH, OW), np.int64), np.empty((1, C, OH, OW), np.float64)
    for oh, (h0, h1) in enumerate(rows):
        for ow, (w0, w1) in enumerate(cols):
            num[:, :, oh, ow] = d[:, :, h0:h1, w0:w1].sum(axis=(2, 3))
            den[0, :, oh, ow] = (h1 - h0) * (w1 - w0) / s            # cnt * 2^k: exact in float64
    return rounded_once(num, den)


def run(k, regime, ep, relu, x_off=0, out_off=0, codes_off=0, rq_override=None):
    row = pi.ROWS[k]
    inst, (N, C, H, W), kernel, stride, osize, xs = row[:6]
    o = pi.operands(k, regime)
    OH, OW = pi.out_hw(row)
    n = N * C * OH * OW

    def at(t, off):                       # a copy `off` bytes past a 256-byte boundary
        if not off:
            return t
        raw = torch.empty(t.numel() * t.element_size() + 256, dtype=torch.uint8, device=DEV)
        v = raw[off:off + t.numel() * t.element_size()].view(t.dtype).view(t.shape)
        v.copy_(t)
        return v

    xq = capi.qparam(at(dev(o["x"].reshape(-1)), x_off), 8, xs, dev(o["sx"]), dev(o["zx"]))
    rq = None
    if ep != "out":
        s, z, lo, hi, bits, sign = rq_override or pi.consumer(k, regime)
        rq = capi.requant(dev(s), dev(z), lo, hi, bits, sign)
    out = at(torch.empty((N, C, OH, OW), dtype=torch.float32, device=DEV), out_off) if ep != "codes" else None
    codes = at(torch.empty(capi.packed_nbytes(n, rq.n_bits), dtype=torch.uint8, device=DEV), codes_off) if rq is not None else None
    got = capi.avgpool2d_codes(xq, N, C, H, W, kernel, stride, osize, relu=relu, rq=rq, out=out, codes=codes)
    path = capi.avgpool2d_codes_path(xq, N, C, H, W, kernel, stride, osize, relu=relu, rq=rq, out=0 if out is None else out.data_ptr(),
                                     codes=0 if codes is None else codes.data_ptr())
    return got, rq, path


ROW_IDS = [pi.row_id(k) for k in range(len(pi.ROWS))]


@pytest.mark.parametrize("relu", [False, True], ids=["lin", "relu"])
@pytest.mark.parametrize("k", range(len(pi.ROWS)), ids=ROW_IDS)
def test_every_row_and_epilogue(k, relu):
    row = pi.ROWS[k]
    inner = int(np.prod(pi.out_hw(row)))
    for regime in ("exact", "parity"):
        want = pi.reference(k, regime, relu)
        if regime == "exact":
            assert same_bits(want, exact_value(k, relu)), "pool_ref is not the exact rational rounded once"
        (out, codes, status), rq, path = run(k, regime, "both", relu)
        assert capi.POOL_KERNELS[path] == row[0]
        assert same_bits(out.cpu().numpy(), want), regime
        assert int(status.item()) == 0
        s, z = rq._keep
        packed_out, st = capi.quantize_pack(out, s, z, rq.qmin, rq.qmax, rq.n_bits, rq.sign, inner=inner)
        assert int(st.item()) == 0 and torch.equal(codes, packed_out), regime
        (out1, none, _), _, path1 = run(k, regime, "out", relu)
        assert none is None and same_bits(out1.cpu().numpy(), want)
        (none, codes2, status2), _, path2 = run(k, regime, "codes", relu)
        assert none is None and torch.equal(codes2, codes) and int(status2.item()) == 0 and path2 == path
        if row[7] != "u4":
            assert path1 == path                 # without a sub-8-bit consumer the geometry alone decides


@pytest.mark.parametrize("k", [k for k, r in enumerate(pi.ROWS) if r[0] == "pair"], ids=lambda k: ROW_IDS[k])
def test_pair_is_launched_whatever_the_alignment(k):
    """x at +1 and +7, out at +4, codes at +3: the plan names pair for these very pointers, and the bytes are the aligned call's."""
    for relu in (False, True):
        (out0, codes0, _), _, path0 = run(k, "parity", "both", relu)
        for x_off in (1, 7):
            (out, codes, status), _, path = run(k, "parity", "both", relu, x_off=x_off, out_off=4, codes_off=3)
            assert out.data_ptr() % 16 == 4 and codes.data_ptr() % 16 == 3
            assert capi.POOL_KERNELS[path] == capi.POOL_KERNELS[path0] == "pair"
            assert same_bits(out.cpu().numpy(), out0.cpu().numpy()) and torch.equal(codes, codes0) and int(status.item()) == 0


def test_a_consumer_too_narrow_for_its_clamp_raises_the_flag():
    """4-bit codes under a clamp to [0, 255]: the values reach beyond 15, so the flag must be 1 -- from every instance that can
    be asked (sub-8-bit: plain) and from qe_quantize_pack on the same out alike."""
    for k in (0, 4, 11):
        amax = float(pi.reference(k, "parity", True).max())              # under relu: the largest value is positive
        assert amax > 0
        narrow = (np.array([amax / 200], np.float32), np.array([0.0], np.float32), 0.0, 255.0, 4, 0)
        (out, codes, status), rq, path = run(k, "parity", "both", True, rq_override=narrow)
        assert capi.POOL_KERNELS[path] == "plain" and int(status.item()) == 1
        inner = int(np.prod(pi.out_hw(pi.ROWS[k])))
        assert int(capi.quantize_pack(out, *rq._keep, 0.0, 255.0, 4, 0, inner=inner)[1].item()) == 1
    # and 8-bit codes under a clamp to [0, 300], through the pair instance
    amax = float(pi.reference(0, "parity", True).max())
    wide = (np.array([amax / 290], np.float32), np.array([0.0], np.float32), 0.0, 300.0, 8, 0)
    (out, codes, status), rq, path = run(0, "parity", "both", True, rq_override=wide)
    assert capi.POOL_KERNELS[path] == "pair" and int(status.item()) == 1


def test_unsupported_requests():
    one = dev(np.ones(1, np.float32))
    x = torch.zeros(2 * 32897, dtype=torch.uint8, device=DEV)
    with pytest.raises(capi.QeError, match="not supported"):            # sub-8-bit x
        capi.avgpool2d_codes(capi.qparam(x, 4, 0, one, one), 1, 2, 8, 8, 2)
    with pytest.raises(capi.QeError, match="not supported"):            # 65794 * 255 >= 2^24
        capi.avgpool2d_codes(capi.qparam(x, 8, 0, one, one), 1, 1, 2, 32897, 0, output_size=(1, 1))
    out = torch.empty(16, dtype=torch.float32, device=DEV)
    with pytest.raises(capi.QeError, match="invalid argument"):         # OH / OW that are not the derived ones
        capi.check(capi.lib().qe_avgpool2d_codes(ctypes.byref(capi.qparam(x, 8, 0, one, one)), 1, 1, 8, 8, 2, 2, 4, 3, 0, out.data_ptr(),
                                                 None, None, None, None))
    with pytest.raises(capi.QeError, match="invalid argument"):         # out overlapping x
        xf = torch.zeros(64, dtype=torch.float32, device=DEV)
        capi.avgpool2d_codes(capi.qparam(xf.view(torch.uint8), 8, 0, one, one), 1, 1, 8, 8, 2, out=xf[:16].view(1, 1, 4, 4))
