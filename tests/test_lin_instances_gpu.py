"""GPU: every row of tests/lin_instances.py through every epilogue its kernel has, on the kernel the table names.

  * F32 (qe_quantlinear): against the float64 oracle under conv_tolerance, on sampled row tiles (first, interior, last and
    ragged); the fp32 kernel bit for bit against the oracle's fused chain.
  * CODES / CODES_GELU (qe_quantlinear_requant): bit-identical to qe_quantize_pack_act(qe_quantlinear(...)) on every row,
    and on the sampled rows equal to the codes of the float64 value (float64 y, float64 GELU with erf) except for flips of
    one inside the tie band: where the float64 pre-rounding value lies within the operation's fp32 error bound of a
    half-integer.  Both clamp ends occur; a NaN bias sets status.
  * RES (qe_quantlinear_residual): bit-identical to y + residual, out of place and in place (y meets the oracle above).
  * Float-input rows: linear_f32_mfma_kernel against the oracle, its RES instance == y + residual; the fp32 chain kernel bit
    for bit against the oracle's fused chain."""
import math

import numpy as np
import pytest
import torch

import lin_instances as li
import oracle
from conftest import conv_tolerance
from quantize_amd import capi

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
EPS32 = 2.0 ** -23


def _sample_rows(B):
    """All rows of a small problem; else the first, an interior and the last 64 rows (the last row tile is ragged whenever
    the kernel's tile height does not divide B)."""
    if B <= 1024:
        return np.arange(B)
    mid = (B // 2) // 64 * 64 + 37
    return np.concatenate([np.arange(64), np.arange(mid, mid + 64), np.arange(B - 64, B)])


def _operands(i, B, K, O):
    x_sign, per_row, asym = li.XQ[i % 3]
    w_sign = i % 2 == 0
    g = torch.Generator(device=DEV).manual_seed(1000 + i)
    u = lambda *s: torch.randint(0, 256, s, dtype=torch.uint8, generator=g, device=DEV)
    r = lambda n, lo, hi: torch.rand(n, generator=g, device=DEV) * (hi - lo) + lo
    nx = B if per_row else 1
    xs, xz = r(nx, 1e-3, 3e-3), (r(nx, -3, 3) if asym else torch.zeros(nx, device=DEV))
    ws, wz = r(O, 2e-3, 6e-3), (r(O, -2, 2) if asym else torch.zeros(O, device=DEV))
    bias = torch.randn(O, generator=g, device=DEV) * 0.2
    xu, wu = u(B, K), u(O, K)
    return dict(xq=capi.qparam(xu, 8, x_sign, xs, xz), wq=capi.qparam(wu, 8, w_sign, ws, wz), bias=bias,
                xu=xu, wu=wu, xs=xs, xz=xz, ws=ws, wz=wz, x_sign=x_sign, w_sign=w_sign)


def _oracle(op, rows, K, O):
    """The oracle's float64 value and its two fp32 chains (as written, fused) on the sampled rows."""
    n = len(rows)
    idx = torch.from_numpy(rows).to(DEV)
    per_row = op["xs"].numel() > 1
    sx = (op["xs"][idx] if per_row else op["xs"]).cpu().numpy()
    zx = (op["xz"][idx] if per_row else op["xz"]).cpu().numpy()
    args = (op["xu"][idx].cpu().numpy(), np.array([8, int(op["x_sign"]), n, K]), sx, zx,
            op["wu"].cpu().numpy(), np.array([8, int(op["w_sign"]), O, K]), op["ws"].cpu().numpy(), op["wz"].cpu().numpy(),
            op["bias"].cpu().numpy())
    o64 = oracle.quantlinear(*args, mode="f64", return_f64=True)[1]
    return o64, oracle.quantlinear(*args, mode="fp32"), oracle.quantlinear(*args, mode="fp32_fma")


def _gelu64(y):
    return y * 0.5 * (1.0 + np.vectorize(math.erf)(y / math.sqrt(2.0)))


def _codes64(v64, sc, zr, qmin, qmax):
    """Codes of float64 values under q = round(v / sc - zr).clamp(qmin, qmax), and the pre-rounding value."""
    t = v64 / sc - zr
    return np.clip(np.round(t), qmin, qmax), t


def _check_codes_vs_f64(got_q, v64, y_err, act, sc, zr, qmin, qmax, what):
    """got_q: the kernel's codes (as q) on the sampled rows.  A flip of one is allowed only where the pre-rounding value
    lies within the fp32 error bound of a half-integer: |y - y64| <= y_err (the linear's rule), through the activation
    (|GELU'| < 1.13, its fp32 evaluation a few ulp of |y|), then v / sc - zr in fp32 (two roundings of |t|)."""
    q64, t = _codes64(v64, sc, zr, qmin, qmax)
    slope = 1.13 if act == "gelu" else 1.0
    band = (slope * y_err + 4 * EPS32 * np.abs(v64)) / sc + 4 * EPS32 * (np.abs(t) + abs(zr))
    d = np.abs(got_q - q64)
    near_tie = np.abs(np.abs(t - np.floor(t)) - 0.5) <= band
    bad = (d > 1) | ((d == 1) & ~near_tie)
    assert not bad.any(), "%s: %d codes off the float64 codes (worst %d) outside the tie band" % (what, int(bad.sum()), int(d.max()))
    return int((d == 1).sum())


def _consumer(y, act):
    """A per-tensor 8-bit consumer whose clamp both ends of y's codes reach: signed symmetric for plain codes, unsigned
    asymmetric after GELU (as fc2's)."""
    v = torch.nn.functional.gelu(y) if act == "gelu" else y
    flat = v.flatten()
    samp = flat[:: max(1, flat.numel() // (1 << 20))].float()
    lo, hi = float(torch.quantile(samp, 0.1)), float(torch.quantile(samp, 0.9))
    qmin, qmax, sign = (0, 255, False) if act == "gelu" else (-128, 127, True)
    # the 10th and 90th percentiles onto qmin - 1 and qmax + 1: the smallest and the largest value clamp, even among 16
    sc = (hi - lo) / (qmax - qmin + 2)
    zr = lo / sc - (qmin - 1)
    rq = capi.requant(torch.tensor([sc], device=DEV), torch.tensor([zr], device=DEV), qmin, qmax, 8, sign)
    return rq, float(np.float32(sc)), float(np.float32(zr)), qmin, qmax


def _stored_to_q(codes, sign):
    c = codes.to(torch.int32)
    return c - 128 if sign else c


@pytest.mark.parametrize("i", range(len(li.ROWS)), ids=["%dx%dx%d" % r[:3] + ("-" + "-".join(r[3].values()) if r[3] else "")
                                                        for r in li.ROWS])
def test_linear_row_every_epilogue(i):
    B, K, O, env, form, note = li.ROWS[i]
    op = _operands(i, B, K, O)
    xq, wq, bias = op["xq"], op["wq"], op["bias"]
    rows = _sample_rows(B)
    idx = torch.from_numpy(rows).to(DEV)
    with capi.knobs(**(env or {})):
        assert capi.linear_form(xq, wq, B, K, O) == form, note
        assert capi.linear_path(xq, wq, B, K, O) == (form != 0)
        # F32
        y = capi.quantlinear(xq, wq, bias, B, K, O)
        torch.cuda.synchronize()
        ys = y[idx].cpu().numpy()
        o64, c32, cfma = _oracle(op, rows, K, O)
        err, allowed = conv_tolerance(ys, o64, c32, cfma)
        assert (err <= allowed).all(), "%s F32: %d elements off, worst %.3g (allowed %.3g)" % (note, int((err > allowed).sum()),
                                                                                             float(np.nanmax(err)), allowed)
        if form == 0:
            assert np.array_equal(ys, cfma), note
            return
        # CODES / CODES_GELU
        for act in (None, "gelu"):
            rq, sc, zr, qmin, qmax = _consumer(y, act)
            assert capi.linear_requant_path(xq, wq, B, K, O, rq) == 1
            codes, st = capi.quantlinear_requant(xq, wq, bias, B, K, O, rq, act=act)
            ref, _, st_ref = capi.quantize_pack_act(y, rq._keep[0], rq._keep[1], qmin, qmax, 8, rq.sign, act=act)
            torch.cuda.synchronize()
            assert torch.equal(codes, ref), "%s %s: fused codes != two-pass codes" % (note, act)
            assert int(st.item()) == int(st_ref.item()) == 0
            cq = _stored_to_q(codes.view(B, O), rq.sign)
            assert int((cq == qmin).sum()) > 0 and int((cq == qmax).sum()) > 0, (note, act)
            v64 = _gelu64(o64) if act == "gelu" else o64
            _check_codes_vs_f64(cq[idx].cpu().numpy(), v64, allowed, act, sc, zr, qmin, qmax, "%s %s" % (note, act))
        nanb = bias.clone()
        nanb[O // 3] = float("nan")
        _, st = capi.quantlinear_requant(xq, wq, nanb, B, K, O, rq, act="gelu")
        assert int(st.item()) == 1, note
        # RES
        assert capi.linear_residual_path(xq, wq, B, K, O) == 1
        res = torch.randn(B, O, generator=torch.Generator(device=DEV).manual_seed(i), device=DEV)
        ref = y + res
        out = capi.quantlinear_residual(xq, wq, bias, B, K, O, res)
        assert torch.equal(out, ref), note
        capi.quantlinear_residual(xq, wq, bias, B, K, O, res, out=res)
        assert torch.equal(res, ref), note


@pytest.mark.parametrize("i", range(len(li.F_ROWS)), ids=["%dx%dx%d" % r[:3] + ("-chain" if r[3] else "") for r in li.F_ROWS])
def test_float_input_row_every_epilogue(i):
    B, K, O, env, form, note = li.F_ROWS[i]
    g = torch.Generator(device=DEV).manual_seed(2000 + i)
    x = torch.randn(B, K, generator=g, device=DEV)
    wu = torch.randint(0, 256, (O, K), dtype=torch.uint8, generator=g, device=DEV)
    ws = torch.rand(O, generator=g, device=DEV) * 4e-3 + 2e-3
    wz = torch.rand(O, generator=g, device=DEV) * 4 - 2
    bias = torch.randn(O, generator=g, device=DEV) * 0.2
    wq = capi.qparam(wu, 8, True, ws, wz)
    rows = _sample_rows(B)
    idx = torch.from_numpy(rows).to(DEV)
    with capi.knobs(**(env or {})):
        assert capi.linear_float_input_path(x, wq, B, K, O) == form, note
        y = capi.quantlinear_float_input(x, wq, bias, O)
        torch.cuda.synchronize()
        args = (x[idx].cpu().numpy(), wu.cpu().numpy(), np.array([8, 1, O, K]), ws.cpu().numpy(), wz.cpu().numpy(), bias.cpu().numpy())
        o64 = oracle.quantlinear_float_input(*args, mode="f64", return_f64=True)[1]
        cfma = oracle.quantlinear_float_input(*args, mode="fp32_fma")
        ys = y[idx].cpu().numpy()
        err, allowed = conv_tolerance(ys, o64, oracle.quantlinear_float_input(*args, mode="fp32"), cfma)
        assert (err <= allowed).all(), "%s: worst %.3g (allowed %.3g)" % (note, float(np.nanmax(err)), allowed)
        if form == 0:
            assert np.array_equal(ys, cfma), note
            return
        assert capi.linear_float_input_residual_path(x, wq, B, K, O) == 1
        res = torch.randn(B, O, generator=g, device=DEV)
        ref = y + res
        assert torch.equal(capi.quantlinear_float_input_residual(x, wq, bias, O, res), ref), note
        capi.quantlinear_float_input_residual(x, wq, bias, O, res, out=res)
        assert torch.equal(res, ref), note
