"""GPU: the residual block end (qe_quantconv2d_residual_prepared) -- out = relu(conv + identity) and the consumer's codes
of out -- equals torch.relu(qe_quantconv2d_prepared(...) + identity) and qe_quantize_pack(out) BIT FOR BIT, on the conv
kernel's own epilogue (path 1: the four ResNet-50 block-end shapes and every RES instance of the resident-tile kernels,
tests/pwr_instances.py) and on the two-pass route (everything else)."""
import numpy as np
import pytest
import torch

import oracle
import pwr_instances
from quantize_amd import capi
from quantize_amd.synthetic import pack_codes
from test_conv_gpu import _assert_conv_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _case(N, IC, H, W, OC, K=1, stride=1, pad=0, x_signed=False, w_signed=True, asym=False, bias=True, seed=0, host=None):
    """host: a dict to receive the operands as host arrays (for the oracle)."""
    rng = np.random.RandomState(seed)
    xlo, xhi = (-128, 128) if x_signed else (0, 256)
    qx = rng.randint(xlo, xhi, size=(N, IC, H, W))
    qw = rng.randint(-128, 128, size=(OC, IC, K, K)) if w_signed else rng.randint(0, 256, size=(OC, IC, K, K))
    sx = _t(np.array([0.02], np.float32))
    zx = _t(np.array([3.0 if asym else (0.0 if x_signed else 0.0)], np.float32))         # kernel convention (q - zero)
    sw = _t(rng.uniform(2e-4, 6e-4, size=OC).astype(np.float32))
    zw = _t((rng.randint(-3, 4, size=OC) if asym else np.zeros(OC) + (0 if w_signed else 128)).astype(np.float32))
    b = _t(rng.normal(0, 0.1, size=OC).astype(np.float32)) if bias else None
    if host is not None:
        host.update(qx=qx, qw=qw, x_signed=x_signed, w_signed=w_signed, sx=sx.cpu().numpy(), zx=zx.cpu().numpy(),
                    sw=sw.cpu().numpy(), zw=zw.cpu().numpy(), b=None if b is None else b.cpu().numpy(), stride=stride, pad=pad)
    sh = capi.conv_shape(N, IC, H, W, OC, K, K, stride, pad)
    xq = capi.qparam(_t(pack_codes(qx, 8, x_signed)), 8, x_signed, sx, zx)
    wq = capi.qparam(_t(pack_codes(qw, 8, w_signed)), 8, w_signed, sw, zw)
    prep = capi.conv_prepare(wq, b, sh, 8)
    y = capi.quantconv2d_prepared(xq, wq, b, sh, prep)
    g = torch.Generator(device="cpu").manual_seed(seed)
    identity = (torch.randn(y.shape, generator=g) * float(y.std())).to(DEV)
    return sh, xq, wq, b, prep, y, identity


def _rq(ref, signed=False, bits=8, per_channel=False, zero=0.0, qmax_over=None):
    qmax = float((1 << (bits - 1)) - 1 if signed else (1 << bits) - 1)
    qmin = float(-(1 << (bits - 1)) if signed else 0)
    if qmax_over is not None:
        qmax = qmax_over
    if per_channel:
        scale = (ref.amax(dim=(0, 2, 3)).clamp(min=1e-3) / qmax).contiguous()
        z = torch.full_like(scale, zero)
    else:
        scale = (ref.max().clamp(min=1e-3) / qmax).reshape(1)
        z = torch.full((1,), zero, device=DEV)
    return capi.requant(scale, z, qmin, qmax, bits, signed)


def _check(sh, xq, wq, b, prep, y, identity, rq, expect_path, out="new"):
    OH, OW = capi.out_hw(sh)
    ref = torch.relu(y + identity)
    assert capi.residual_path(sh, xq, wq, rq) == expect_path
    need = capi.residual_workspace_bytes(sh, xq, wq, rq)
    assert (need == 0) == (expect_path == 1)     # path 1 runs with no workspace: a two-pass call would fail without one
    ident = identity.clone()
    if out == "identity":
        out = ident
    o, codes, st = capi.quantconv2d_residual_prepared(xq, wq, b, sh, prep, ident, rq=rq, out=out)
    torch.cuda.synchronize()
    if o is not None:
        assert torch.equal(o, ref)
    if rq is not None:
        s, z = rq._keep
        ref_codes, ref_st = capi.quantize_pack(ref.contiguous(), s, z, rq.qmin, rq.qmax, rq.n_bits, rq.sign, inner=OH * OW)
        assert int(st.item()) == int(ref_st.item())
        if int(ref_st.item()) == 0:              # codes are unspecified once the range flag is set (as qe_tpack's)
            assert torch.equal(codes, ref_codes)
    return o, codes, st


BLOCK_ENDS = [(2, 64, 56, 56, 256), (2, 128, 28, 28, 512), (2, 256, 14, 14, 1024), (2, 512, 7, 7, 2048)]


@pytest.mark.parametrize("shape", BLOCK_ENDS)
@pytest.mark.parametrize("x_signed,asym,bias", [(False, False, True), (True, True, True), (False, True, False)])
def test_block_end_fused(shape, x_signed, asym, bias):
    c = _case(*shape, x_signed=x_signed, asym=asym, bias=bias, seed=shape[1])
    ref = torch.relu(c[5] + c[6])
    _check(*c, rq=_rq(ref), expect_path=1)                              # fp32 + unsigned codes
    _check(*c, rq=_rq(ref, signed=True), expect_path=1)                 # signed codes
    _check(*c, rq=_rq(ref, zero=-2.0), expect_path=1)                   # non-zero zero point
    _check(*c, rq=None, expect_path=1)                                  # fp32 only
    _check(*c, rq=_rq(ref), expect_path=1, out=None)                    # codes only (stage boundaries)
    _check(*c, rq=_rq(ref), expect_path=1, out="identity")              # in place


def _assert_y_meets_oracle(y, host, n_img, what):
    """The engine's plain conv y (what the block end adds the identity to) on the first n_img images against the oracle."""
    xp, xd = oracle.tpack(host["qx"][:n_img], 8, host["x_signed"])
    wp, wd = oracle.tpack(host["qw"], 8, host["w_signed"])
    args = (xp, xd, host["sx"], host["zx"], wp, wd, host["sw"], host["zw"], host["b"], host["stride"], host["pad"])
    o32, fma = [oracle.quantconv2d(*args, mode=m) for m in ("fp32", "fp32_fma")]
    _, o64 = oracle.quantconv2d(*args, mode="f64", return_f64=True)
    _assert_conv_close(y[:n_img].cpu().numpy(), o64, o32, what, fma)


RES_ROWS = pwr_instances.res_rows()


@pytest.mark.parametrize("k", range(len(RES_ROWS)), ids=["%s-%s" % ("x".join(map(str, r[0][:5])), "g" if r[3] else "")
                                                         for r in RES_ROWS])
def test_block_end_every_instance(k):
    """Every stride-1 row of the instance table through its RES instances (fp32 + codes, fp32 only, codes only, in place;
    signed and unsigned codes, a zero point that is not zero), and the conv y it adds to against the float64 oracle."""
    shp, base, note, env = RES_ROWS[k]
    x_signed, asym, bias = [(False, False, True), (True, True, True), (False, True, False)][k % 3]
    host = {}
    with capi.knobs(**(env or {})):
        c = _case(*shp[:5], x_signed=x_signed, asym=asym, bias=bias, seed=100 + k, host=host)
        ref = torch.relu(c[5] + c[6])
        _check(*c, rq=_rq(ref), expect_path=1)                          # fp32 + unsigned codes
        _check(*c, rq=_rq(ref, signed=True), expect_path=1)             # signed codes
        _check(*c, rq=_rq(ref, zero=-2.0), expect_path=1)               # non-zero zero point
        _check(*c, rq=None, expect_path=1)                              # fp32 only
        _check(*c, rq=_rq(ref, signed=True, zero=1.5), expect_path=1, out=None)    # codes only
        _check(*c, rq=_rq(ref), expect_path=1, out="identity")          # in place
    _assert_y_meets_oracle(c[5], host, min(shp[0], 4), "%s %s (%s)" % (pwr_instances.kernel_name(base + (False, True)), shp,
                                                                        note))


def test_batch_256_block_end_is_batch_independent_196x2():
    """A batch-256 launch of the 64 -> 256 @28x28 block end (<7, 4, 2, 196>, RES): each image's rows equal a batch-2
    launch on that image, and image 255's conv meets the oracle."""
    host = {}
    sh, xq, wq, b, prep, y, identity = _case(256, 64, 28, 28, 256, seed=14, host=host)
    ref = torch.relu(y + identity)
    rq = _rq(ref, signed=True, zero=-1.0)
    assert capi.residual_path(sh, xq, wq, rq) == 1
    o, codes, _ = capi.quantconv2d_residual_prepared(xq, wq, b, sh, prep, identity, rq=rq)
    assert torch.equal(o, ref)
    x_all = xq._keep[0].view(256, -1)
    per = 256 * 784
    for i in (0, 101, 254):
        sh2 = capi.conv_shape(2, 64, 28, 28, 256, 1, 1, 1, 0)
        x2 = capi.qparam(x_all[i:i + 2].contiguous().view(-1), 8, False, xq._keep[1], xq._keep[2])
        o2, c2, _ = capi.quantconv2d_residual_prepared(x2, wq, b, sh2, prep, identity[i:i + 2].contiguous(), rq=rq)
        assert torch.equal(o2, o[i:i + 2])
        assert torch.equal(c2, codes[i * per:(i + 2) * per])
    host["qx"] = host["qx"][255:]
    _assert_y_meets_oracle(y[255:], host, 1, "batch 256, image 255")


@pytest.mark.parametrize("shape", [(3, 512, 7, 7, 2048), (2, 64, 30, 30, 256), (1, 96, 14, 14, 256)])
def test_block_end_fallbacks(shape):
    """odd batch on the 7x7 kernel, a ragged plane, a channel count the resident-tile kernel does not take: two passes"""
    c = _case(*shape, seed=7)
    ref = torch.relu(c[5] + c[6])
    _check(*c, rq=_rq(ref), expect_path=0)
    _check(*c, rq=_rq(ref), expect_path=0, out=None)
    _check(*c, rq=_rq(ref), expect_path=0, out="identity")
    _check(*c, rq=None, expect_path=0)


def test_pwr_disabled_takes_two_passes():
    with capi.knobs(QE_PWR="0"):
        c = _case(2, 128, 28, 28, 512, seed=3)
        ref = torch.relu(c[5] + c[6])
        _check(*c, rq=_rq(ref), expect_path=0)


def test_two_pass_route_basic_block_per_channel_4bit():
    c = _case(2, 64, 14, 14, 64, K=3, stride=1, pad=1, seed=5)          # a BasicBlock's 3x3 block end
    ref = torch.relu(c[5] + c[6])
    _check(*c, rq=_rq(ref), expect_path=0)
    _check(*c, rq=_rq(ref, per_channel=True), expect_path=0)
    _check(*c, rq=_rq(ref, bits=4), expect_path=0)
    _check(*c, rq=_rq(ref, bits=4, signed=True), expect_path=0, out=None)
    c = _case(2, 128, 28, 28, 512, seed=6)                              # a fused-kernel shape with per-channel / 4-bit codes
    ref = torch.relu(c[5] + c[6])
    _check(*c, rq=_rq(ref, per_channel=True), expect_path=0)
    _check(*c, rq=_rq(ref, bits=4), expect_path=0, out="identity")


@pytest.mark.parametrize("shape,path", [((2, 128, 28, 28, 512), 1), ((2, 512, 7, 7, 2048), 1), ((2, 64, 14, 14, 64, 3, 1, 1), 0)])
def test_non_finite_identity(shape, path):
    sh, xq, wq, b, prep, y, identity = _case(*shape, seed=9)
    flat = identity.view(-1)
    idx = torch.randperm(flat.numel(), generator=torch.Generator().manual_seed(1))[:300].to(DEV)
    flat[idx[:100]] = float("nan")
    flat[idx[100:200]] = float("inf")
    flat[idx[200:]] = float("-inf")
    ref = torch.relu(y + identity)
    assert capi.residual_path(sh, xq, wq, None) == path
    o, _, _ = capi.quantconv2d_residual_prepared(xq, wq, b, sh, prep, identity.clone(), rq=None)
    torch.cuda.synchronize()
    assert torch.equal(torch.isnan(o), torch.isnan(ref))
    fin = ~torch.isnan(ref)
    assert torch.equal(o[fin], ref[fin])
    # with codes: NaN trips the range flag as quantize_pack's does
    rq = _rq(torch.relu(y + identity.nan_to_num(0, 0, 0)))
    _, _, st = capi.quantconv2d_residual_prepared(xq, wq, b, sh, prep, identity.clone(), rq=rq)
    assert int(st.item()) == 1


@pytest.mark.parametrize("shape", [(2, 256, 14, 14, 1024), (3, 512, 7, 7, 2048)])
def test_range_flag(shape):
    c = _case(*shape, seed=11)
    ref = torch.relu(c[5] + c[6])
    rq = _rq(ref, qmax_over=300.0)                   # a clamp beyond the 8-bit code range: the largest values do not fit
    _, _, st = _check(*c, rq=rq, expect_path=1 if shape[0] == 2 else 0)
    assert int(st.item()) == 1
    _, _, st = _check(*c, rq=_rq(ref), expect_path=1 if shape[0] == 2 else 0)
    assert int(st.item()) == 0


def test_batch_256_block_end_is_batch_independent():
    """A batch-256 launch of the 256 -> 1024 @14x14 block end: each image's rows equal a batch-2 launch on that image."""
    big = _case(256, 256, 14, 14, 1024, seed=13)
    sh, xq, wq, b, prep, y, identity = big
    ref = torch.relu(y + identity)
    rq = _rq(ref)
    assert capi.residual_path(sh, xq, wq, rq) == 1
    o, codes, _ = capi.quantconv2d_residual_prepared(xq, wq, b, sh, prep, identity, rq=rq)
    assert torch.equal(o, ref)
    x_all = xq._keep[0].view(256, -1)
    per = 1024 * 196
    for i in (0, 77, 254):
        sh2 = capi.conv_shape(2, 256, 14, 14, 1024, 1, 1, 1, 0)
        x2 = capi.qparam(x_all[i:i + 2].contiguous().view(-1), 8, False, xq._keep[1], xq._keep[2])
        o2, c2, _ = capi.quantconv2d_residual_prepared(x2, wq, b, sh2, prep, identity[i:i + 2].contiguous(), rq=rq)
        assert torch.equal(o2, o[i:i + 2])
        assert torch.equal(c2, codes[i * per:(i + 2) * per])


def test_argument_checks():
    sh, xq, wq, b, prep, y, identity = _case(2, 128, 28, 28, 512, seed=2)
    flat = torch.empty(identity.numel() + 64, device=DEV)
    with pytest.raises(capi.QeError):           # partial overlap of out and identity
        capi.quantconv2d_residual_prepared(xq, wq, b, sh, prep, flat[:identity.numel()], out=flat[16:16 + identity.numel()])
    with pytest.raises(capi.QeError):           # neither out nor codes
        capi.quantconv2d_residual_prepared(xq, wq, b, sh, prep, identity, rq=None, out=None)


@pytest.mark.parametrize("ident_off,out_off,codes_off", [(1, 0, 0), (3, 0, 0), (0, 1, 0), (0, 2, 0), (0, 0, 1), (0, 0, 2)])
def test_argument_alignment(ident_off, out_off, codes_off):
    """identity or out not 16-byte aligned, or codes not 4-byte aligned: QE_ERR_ARG (qe_quantconv2d_residual_prepared's
    contract), and neither out nor codes is written.  Offsets in elements: 4 bytes per fp32, 1 per code."""
    sh, xq, wq, b, prep, y, identity = _case(2, 128, 28, 28, 512, seed=2)
    rq = _rq(torch.relu(y + identity))
    n = identity.numel()
    ibuf = torch.zeros(n + 16, device=DEV)
    ident = ibuf[ident_off:ident_off + n].view(identity.shape)
    ident.copy_(identity)
    obuf = torch.full((n + 16,), -7.5, device=DEV)
    cbuf = torch.full((n + 16,), 0xA5, dtype=torch.uint8, device=DEV)
    out = obuf[out_off:out_off + n].view(identity.shape)
    codes = cbuf[codes_off:codes_off + n]
    with pytest.raises(capi.QeError, match="invalid argument"):
        capi.quantconv2d_residual_prepared(xq, wq, b, sh, prep, ident, rq=rq, out=out, codes=codes)
    torch.cuda.synchronize()
    assert bool((obuf == -7.5).all()) and bool((cbuf == 0xA5).all())
    assert torch.equal(ident, identity)
