"""GPU: every row of the operand-type table (tests/quant_instances.py), one test per decode site and regime.

exact   operands on the power-of-two grid of quant_instances.operands(k, "exact"): the kernel must return the numpy float64
        value (tests/quant_ref.py) bit for bit -- np.array_equal, no tolerance -- so one code decoded one LSB wrong at any
        width or sign fails (tests/test_quant_instances_cpu.py shows that it would move an output).  The fused entries are
        held to the same: the consumer's codes of the float64 value (a power-of-two scale: no tie is ambiguous),
        relu(exact + identity), exact + residual, bf16(exact / 2).
parity  the same rows at the headline scales with fractional zero points, under the project's own rule unchanged:
        conftest.conv_tolerance through _assert_conv_close / test_linear_gpu._close with the oracle's two fp32 chains, and
        bit equality with the oracle's fused chain on the order-preserving kernels; the fused entries bit for bit against
        their two-pass forms on the engine's own fp32 result.

A site listed in quant_instances.QUARTER_STEP would be held to |got - exact64| <= lsb / 4 instead (none is)."""
import functools

import numpy as np
import pytest
import torch

import quant_instances as qi
import quant_ref as qr
from conftest import conv_tolerance
from quantize_amd import capi
from test_conv_gpu import DEV, _assert_conv_close, _t, engine  # noqa: F401
from test_linear_gpu import _close
from test_quant_instances_cpu import _oracle

pytestmark = pytest.mark.gpu
SITES = list(qi.SITES)


def _qparam(p):
    return capi.qparam(_t(p["packed"]), p["bits"], p["sign"], _t(p["s"]), _t(p["z"]))


def _des(p):
    return _t(np.array([p["bits"], p["sign"], *p["shape"]], dtype=np.int32))


def _per_channel4(p):
    return _t(p["s"]).reshape(-1, 1, 1, 1), _t(p["z"]).reshape(-1, 1, 1, 1)     # (C,1,1,1) as QuantConv2d stores them


@functools.lru_cache(maxsize=None)
def _want(k, regime):
    """The float64 reference of a row, once."""
    return qi.reference(k, regime)


@functools.lru_cache(maxsize=None)
def _chains(k):
    """The oracle's (fp32 chain, fused fp32 chain, float64) on the parity operands of a row, once."""
    return _oracle(k, "parity", "fp32"), _oracle(k, "parity", "fp32_fma"), _oracle(k, "parity", "f64")


def _plain(k, regime, engine):
    """The plain fp32 call of row k through the C ABI or the torch operator, whichever the row names (the fused rows: the C
    ABI, their two-pass reference).  Returns the device tensor and the call's operands."""
    site, entry, shape, x, w, env, note = qi.ROWS[k]
    o = qi.operands(k, regime)
    op = qi.op_of(qi.ROWS[k])
    W = o["w"]
    bias = None if o["bias"] is None else _t(o["bias"])
    wq = _qparam(W)
    via_torch = entry == "torch"
    ctx = dict(wq=wq, bias=bias)
    if op in ("conv", "conv_f32"):
        N, IC, H, Wd, OC, K, st, p = shape
        sh = capi.conv_shape(N, IC, H, Wd, OC, K, K, st, p)
        ctx["sh"] = sh
        if op == "conv":
            X = o["x"]
            xq = _qparam(X)
            ctx["xq"] = xq
            if via_torch:
                y = engine.quantconv2d(_t(X["packed"]), _des(X), _t(X["s"]), _t(X["z"]), _t(W["packed"]), _des(W),
                                       *_per_channel4(W), bias, st, p)
            elif entry in ("requant", "residual"):
                ctx["prepared"] = capi.conv_prepare(wq, bias, sh, X["bits"])
                y = capi.quantconv2d_prepared(xq, wq, bias, sh, ctx["prepared"])
            else:
                y = capi.quantconv2d(xq, wq, bias, sh)
        else:
            xt = _t(o["xf"])
            if via_torch:
                y = engine.quantconv2d_float_input(xt, _t(W["packed"]), _des(W), *_per_channel4(W), bias, st, p)
            else:
                y = capi.quantconv2d_float_input(xt, wq, bias, sh)
    else:
        B, K, O = shape
        ctx.update(B=B, K=K, O=O)
        if op == "lin":
            X = o["x"]
            xq = _qparam(X)
            ctx["xq"] = xq
            if via_torch:
                y = engine.quantlinear(_t(X["packed"]), _des(X), _t(X["s"]), _t(X["z"]), _t(W["packed"]), _des(W), _t(W["s"]),
                                       _t(W["z"]), bias)
            else:
                y = capi.quantlinear(xq, wq, bias, B, K, O)
        elif op == "lin_f32":
            xt = _t(o["xf"])
            if via_torch:
                y = engine.quantlinear_float_input(xt, _t(W["packed"]), _des(W), _t(W["s"]), _t(W["z"]), bias)
            else:
                y = capi.quantlinear_float_input(xt, wq, bias, O)
        else:
            x16 = _t(o["xf"]).to(torch.bfloat16)
            assert torch.equal(x16.float(), _t(o["xf"]))
            assert capi.quantlinear_bf16_input_path(x16, wq, B, K, O) == 1
            y = capi.quantlinear_bf16_input(x16, wq, bias, O)
    torch.cuda.synchronize()
    return y, ctx


def _what(k, regime):
    return "%s [%s] (%s)" % (qi.row_id(k), regime, qi.SITES[qi.ROWS[k][0]][1])


def _assert_equal(got, want, k, what, lsb=None):
    """Exact equality with the float64 value (or, for a site of QUARTER_STEP, a quarter of the row's LSB)."""
    got64 = np.asarray(got).astype(np.float64)
    assert got64.shape == want.shape, what
    if lsb is not None and qi.ROWS[k][0] in qi.QUARTER_STEP:
        ok = np.abs(got64 - want) <= lsb / 4
    else:
        ok = got64 == want                                # NaN compares false
    bad = np.flatnonzero(~ok)
    if bad.size:
        i = np.unravel_index(bad[0], want.shape)
        step = "" if lsb is None else ", %.6g LSB off" % ((got64[i] - want[i]) / np.broadcast_to(lsb, want.shape)[i])
        raise AssertionError("%s: %d of %d elements wrong, first at %s: got %r, float64 %r%s" % (
            what, bad.size, want.size, tuple(int(v) for v in i), float(got64[i]), float(want[i]), step))


def _stored8(q):
    """Signed 8-bit codes as the engine stores them."""
    return (np.asarray(q, dtype=np.int64) + 128).astype(np.uint8).reshape(-1)


@pytest.mark.parametrize("site", SITES)
def test_exact_regime(engine, site):
    for k in qi.rows_of(site):
        _, entry, shape, x, w, env, note = qi.ROWS[k]
        what = _what(k, "exact")
        want = _want(k, "exact")
        lsb = qi.lsb_of(k, want.shape)
        with capi.knobs(**(env or {})):
            y, c = _plain(k, "exact", engine)
            _assert_equal(y.cpu().numpy(), want, k, what, lsb)
            if entry in ("capi", "torch"):
                continue
            fx = qi.fused_extras(k)
            conv = "sh" in c
            if entry == "requant":
                rq = capi.requant(_t(np.array([fx["rq_scale"]])), _t(np.array([fx["rq_zero"]])), fx["qmin"], fx["qmax"], 8, True)
                if conv:
                    codes, st = capi.quantconv2d_requant_prepared(c["xq"], c["wq"], c["bias"], c["sh"], c["prepared"], rq)
                else:
                    codes, st = capi.quantlinear_requant(c["xq"], c["wq"], c["bias"], c["B"], c["K"], c["O"], rq)
                torch.cuda.synchronize()
                assert int(st.item()) == 0, what
                q64 = qr.codes(want, fx["rq_scale"], fx["rq_zero"], fx["qmin"], fx["qmax"])
                assert fx["qmin"] < q64.min() and q64.max() < fx["qmax"] and np.unique(q64).size > 32, what   # nothing hides in the clamp
                _assert_equal(codes.cpu().numpy(), _stored8(q64).astype(np.float64), k, what + " codes")
            elif entry == "residual":
                ident = _t(fx["identity"])
                if conv:
                    assert capi.residual_path(c["sh"], c["xq"], c["wq"], None) == 1, what
                    out, _, st = capi.quantconv2d_residual_prepared(c["xq"], c["wq"], c["bias"], c["sh"], c["prepared"], ident)
                    wanted = np.maximum(want + fx["identity"].astype(np.float64), 0.0)
                else:
                    out = capi.quantlinear_residual(c["xq"], c["wq"], c["bias"], c["B"], c["K"], c["O"], ident)
                    wanted = want + fx["identity"].astype(np.float64)
                torch.cuda.synchronize()
                _assert_equal(out.cpu().numpy(), wanted, k, what + " + identity", lsb)
            else:
                out = capi.quantlinear_bf16(c["xq"], c["wq"], c["bias"], c["B"], c["K"], c["O"], post_scale=fx["post_scale"])
                torch.cuda.synchronize()
                _assert_equal(out.float().cpu().numpy(), qr.bf16_round(want * fx["post_scale"]), k, what + " bf16")


def _consumer(y, k):
    """The consumer's quantiser as test_conv_instances_gpu draws it: amax / 100 clips a few percent, a zero point off zero."""
    sign = k % 2 == 0
    qmin, qmax = (-128.0, 127.0) if sign else (0.0, 255.0)
    s = torch.tensor([max(float(y.abs().max()) / 100.0, 1e-6)], device=DEV)
    z = torch.tensor([[0.37, -2.0, 5.5][k % 3] if sign else [-117.25, -3.0, -64.5][k % 3]], device=DEV)
    return capi.requant(s, z, qmin, qmax, 8, sign), s, z, qmin, qmax, sign


@pytest.mark.parametrize("site", SITES)
def test_parity_regime(engine, site):
    chain_exact = site in ("generic", "generic_f32", "lin_generic", "lin_generic_f32")
    for k in qi.rows_of(site):
        _, entry, shape, x, w, env, note = qi.ROWS[k]
        what = _what(k, "parity")
        o32, fma, o64 = _chains(k)
        ref = _want(k, "parity")
        assert np.abs(ref - o64).max() <= 1e-12 * max(1.0, float(np.abs(o64).max())), what     # (the CPU suite bounds it tightly)
        with capi.knobs(**(env or {})):
            y, c = _plain(k, "parity", engine)
            got = y.cpu().numpy()
            assert got.shape == o64.shape, what
            err, allowed = conv_tolerance(got, o64, o32, fma)
            bad = np.flatnonzero(~(err <= allowed))
            if bad.size:                                   # the rule's own assertion below fails: say where first
                what += ", first at %s" % (tuple(int(v) for v in np.unravel_index(bad[0], got.shape)),)
            if len(shape) == 3:
                _close(got, o64, o32, what, fma)
            else:
                _assert_conv_close(got, o64, o32, what, fma)
            if chain_exact:
                bad = np.flatnonzero(got != fma)
                assert bad.size == 0, "%s: %d of %d elements differ from the oracle's fused chain, first at %s" % (
                    what, bad.size, got.size, np.unravel_index(bad[0], got.shape))
            if entry in ("capi", "torch"):
                continue
            conv = "sh" in c
            g = torch.Generator(device=DEV).manual_seed(k)
            if entry == "requant":
                rq, s, z, qmin, qmax, sign = _consumer(y, k)
                if conv:
                    codes, st = capi.quantconv2d_requant_prepared(c["xq"], c["wq"], c["bias"], c["sh"], c["prepared"], rq)
                    two_pass, st2 = capi.quantize_pack(y, s, z, qmin, qmax, 8, sign)
                else:
                    codes, st = capi.quantlinear_requant(c["xq"], c["wq"], c["bias"], c["B"], c["K"], c["O"], rq)
                    two_pass, _, st2 = capi.quantize_pack_act(y, s, z, qmin, qmax, 8, sign)
                torch.cuda.synchronize()
                assert int(st.item()) == int(st2.item()) == 0, what
                bad = torch.nonzero(codes != two_pass).flatten()
                assert bad.numel() == 0, "%s: %d of %d codes differ from quantize_pack of the fp32 result, first at %d" % (
                    what, bad.numel(), codes.numel(), int(bad[0]))
            elif entry == "residual":
                res = torch.randn(y.shape, generator=g, device=DEV)
                if conv:
                    out, _, _ = capi.quantconv2d_residual_prepared(c["xq"], c["wq"], c["bias"], c["sh"], c["prepared"], res)
                    want = torch.relu(y + res)
                else:
                    out = capi.quantlinear_residual(c["xq"], c["wq"], c["bias"], c["B"], c["K"], c["O"], res)
                    want = y + res
                torch.cuda.synchronize()
                bad = torch.nonzero(out.flatten() != want.flatten()).flatten()
                assert bad.numel() == 0, "%s: %d of %d elements differ from y + identity, first at %d" % (
                    what, bad.numel(), out.numel(), int(bad[0]))
            else:
                out = capi.quantlinear_bf16(c["xq"], c["wq"], c["bias"], c["B"], c["K"], c["O"], post_scale=0.125)
                torch.cuda.synchronize()
                want = (y * 0.125).to(torch.bfloat16)
                bad = torch.nonzero(out.flatten() != want.flatten()).flatten()
                assert bad.numel() == 0, "%s: %d of %d bf16 values differ from the rounded fp32 result, first at %d" % (
                    what, bad.numel(), out.numel(), int(bad[0]))
