"""GPU: qe_quantlinear_bf16_input on every row of tests/lin_bf16in_instances.py.

  * parity: without a residual, against the float64 oracle of qe_quantlinear_float_input on the widened rows under
    conftest.conv_tolerance (chains: the oracle's fp32 and fp32_fma modes) -- the project's parity rule, no headroom factor;
    on a large B the first, an interior and the last (ragged) row tile;
  * residual: entry(residual=r) == entry() + r bit for bit, out of place and in place, on every path-1 row;
  * fallback: on path-0 rows the result equals qe_quantlinear_float_input on x.float() bit for bit (and the residual form
    qe_quantlinear_float_input_residual);
  * row isolation: a NaN and a +inf activation make their own output rows non-finite and leave every other row's bits;
  * rounding bound: against qe_quantlinear_float_input on an unrounded attention context, the bound derived below."""
import numpy as np
import pytest
import torch

import lin_bf16in_instances as bi
import oracle
from conftest import conv_tolerance
from quantize_amd import capi

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _sample_rows(B):
    """All rows of a small problem; else the first row tile (128 rows), an interior one that starts off a tile boundary and
    the last 128 rows (the last tile is ragged whenever 128 does not divide B)."""
    if B <= 1024:
        return np.arange(B)
    mid = (B // 2) // 128 * 128 + 37
    return np.concatenate([np.arange(128), np.arange(mid, mid + 128), np.arange(B - 128, B)])


def _problem(i):
    """Row i of the table in its weight regime: dict(x (bf16, at the row's byte offset), wq, bias, and the host arrays)."""
    B, K, O, w_bits, off, path, note = bi.ROWS[i]
    sign, per_tensor, zero, has_bias, act = bi.REGIMES[i % 4]
    g = torch.Generator(device=DEV).manual_seed(3000 + i)
    xf = torch.randn(B, K, generator=g, device=DEV)
    if act == "abs":
        xf = xf.abs()
    flat = torch.empty(B * K + 8, dtype=torch.bfloat16, device=DEV)
    x = flat[off // 2: off // 2 + B * K].view(B, K)
    x.copy_(xf)
    assert x.is_contiguous() and x.data_ptr() % 16 == off
    n_codes = O * K
    wu = torch.randint(0, 256, (n_codes * w_bits // 8,), dtype=torch.uint8, generator=g, device=DEV)
    no = 1 if per_tensor else O
    ws = torch.rand(no, generator=g, device=DEV) * 4e-3 + 2e-3
    if zero == "none":
        wz = torch.zeros(no, device=DEV)
    elif zero == "mid":                              # the middle code of the unsigned range, a fraction off it
        wz = torch.full((no,), float(1 << (w_bits - 1)) + 0.3, device=DEV)
    else:
        wz = torch.rand(no, generator=g, device=DEV) * 4 - 2
    bias = torch.randn(O, generator=g, device=DEV) * 0.2 if has_bias else None
    return dict(x=x, wq=capi.qparam(wu, w_bits, sign, ws, wz), bias=bias, wu=wu, ws=ws, wz=wz, sign=sign, w_bits=w_bits)


def _oracle(p, xrows, K, O):
    """float64 value and the two fp32 chains of the reference's float-input linear on fp32 rows `xrows` (host)."""
    args = (xrows, p["wu"].cpu().numpy(), np.array([p["w_bits"], int(p["sign"]), O, K]), p["ws"].cpu().numpy(), p["wz"].cpu().numpy(),
            None if p["bias"] is None else p["bias"].cpu().numpy())
    o64 = oracle.quantlinear_float_input(*args, mode="f64", return_f64=True)[1]
    return o64, oracle.quantlinear_float_input(*args, mode="fp32"), oracle.quantlinear_float_input(*args, mode="fp32_fma")


@pytest.mark.parametrize("i", range(len(bi.ROWS)), ids=[bi.row_id(r) for r in bi.ROWS])
def test_row_parity_residual_and_fallback(i):
    B, K, O, w_bits, off, path, note = bi.ROWS[i]
    p = _problem(i)
    x, wq, bias = p["x"], p["wq"], p["bias"]
    assert capi.quantlinear_bf16_input_path(x, wq, B, K, O) == path, note
    y = capi.quantlinear_bf16_input(x, wq, bias, O)
    torch.cuda.synchronize()
    rows = _sample_rows(B)
    idx = torch.from_numpy(rows).to(DEV)
    o64, c32, cfma = _oracle(p, x[idx].float().cpu().numpy(), K, O)
    ys = y[idx].cpu().numpy()
    err, allowed = conv_tolerance(ys, o64, c32, cfma)
    print("%s: worst %.3g, allowed %.3g" % (bi.row_id(bi.ROWS[i]), float(np.nanmax(err)), allowed))
    assert np.isfinite(ys).all(), note
    assert (err <= allowed).all(), "%s: %d elements off, worst %.3g (allowed %.3g)" % (note, int((err > allowed).sum()),
                                                                                      float(np.nanmax(err)), allowed)
    res = torch.randn(B, O, generator=torch.Generator(device=DEV).manual_seed(i), device=DEV)
    ref = y + res
    assert torch.equal(capi.quantlinear_bf16_input(x, wq, bias, O, residual=res), ref), note
    res2 = res.clone()
    assert capi.quantlinear_bf16_input(x, wq, bias, O, residual=res2, out=res2) is res2
    assert torch.equal(res2, ref), note
    if path == 0:
        xw = x.float().contiguous()
        assert torch.equal(y, capi.quantlinear_float_input(xw, wq, bias, O)), note
        assert torch.equal(ref, capi.quantlinear_float_input_residual(xw, wq, bias, O, res)), note


def test_fallback_knob_takes_every_row_to_path_0():
    """QE_LIN_F32_MFMA=0: the widening pass and the order-preserving chain kernel, bit for bit the float-input entry."""
    i = 5
    B, K, O = bi.ROWS[i][:3]
    p = _problem(i)
    with capi.knobs(QE_LIN_F32_MFMA="0"):
        assert capi.quantlinear_bf16_input_path(p["x"], p["wq"], B, K, O) == 0
        y = capi.quantlinear_bf16_input(p["x"], p["wq"], p["bias"], O)
        assert torch.equal(y, capi.quantlinear_float_input(p["x"].float(), p["wq"], p["bias"], O))
    assert capi.quantlinear_bf16_input_path(p["x"], p["wq"], B, K, O) == 1


def test_misaligned_out_takes_path_0():
    """The path query cannot see `out`; an out that is only 4-byte aligned is served by path 0 with the same result bits as
    the float-input entry on the widened rows."""
    i = 5
    B, K, O = bi.ROWS[i][:3]
    p = _problem(i)
    buf = torch.empty(B * O + 4, device=DEV)
    out = buf[1:1 + B * O].view(B, O)
    assert out.data_ptr() % 16 == 4
    capi.quantlinear_bf16_input(p["x"], p["wq"], p["bias"], O, out=out)
    assert torch.equal(out, capi.quantlinear_float_input(p["x"].float(), p["wq"], p["bias"], O))


def test_non_finite_rows_stay_in_their_row():
    i = 5                                            # (130, 64, 40): two row tiles, two stages
    B, K, O, _, _, path, _ = bi.ROWS[i]
    assert (B, K, O, path) == (130, 64, 40, 1)
    p = _problem(i)
    clean = capi.quantlinear_bf16_input(p["x"], p["wq"], p["bias"], O)
    res = torch.randn(B, O, generator=torch.Generator(device=DEV).manual_seed(9), device=DEV)
    x = p["x"].clone()
    x[7, 33] = float("nan")
    x[129, 5] = float("inf")
    bad = torch.zeros(B, dtype=torch.bool, device=DEV)
    bad[7] = bad[129] = True
    for r in (None, res):
        got = capi.quantlinear_bf16_input(x, p["wq"], p["bias"], O, residual=r)
        want = clean if r is None else clean + r
        torch.cuda.synchronize()
        assert not torch.isfinite(got[bad]).any(), "a finite output in a row with a NaN / inf activation"
        assert torch.equal(got[~bad].view(torch.int32), want[~bad].view(torch.int32))


def test_rounding_bound_against_the_float_input_entry():
    """ctx: the fp32 context of a random attention call; y_f = quantlinear_float_input(ctx), y_b = quantlinear_bf16_input(
    bf16(ctx)).  Rounding to nearest even at 8 significant bits moves each context element by at most 2^-9 of itself, so the
    exact results differ by at most 2^-9 (|ctx| |W_deq|^T); each computed result may sit its own parity allowance (a_b, a_f:
    conv_tolerance on its own problem) away from its exact one:
        |y_b - y_f| <= 2^-9 (|ctx| |W_deq|^T) + a_b + a_f      elementwise, in float64."""
    N, L, H, d, O = 3, 17, 2, 64, 96
    E = H * d
    g = torch.Generator(device=DEV).manual_seed(77)
    q, k, v = (torch.randn(N * L, E, generator=g, device=DEV) for _ in range(3))
    ctx = capi.attention(q, k, v, N, L, H)
    wu = torch.randint(0, 256, (O * E,), dtype=torch.uint8, generator=g, device=DEV)
    ws = torch.rand(O, generator=g, device=DEV) * 4e-3 + 2e-3
    wz = torch.rand(O, generator=g, device=DEV) * 4 - 2
    bias = torch.randn(O, generator=g, device=DEV) * 0.2
    p = dict(wu=wu, ws=ws, wz=wz, bias=bias, sign=True, w_bits=8)
    wq = capi.qparam(wu, 8, True, ws, wz)
    ctx16 = ctx.to(torch.bfloat16)
    assert capi.quantlinear_bf16_input_path(ctx16, wq, N * L, E, O) == 1
    y_f = capi.quantlinear_float_input(ctx, wq, bias, O).cpu().numpy()
    y_b = capi.quantlinear_bf16_input(ctx16, wq, bias, O).cpu().numpy()
    f64, f32, ffma = _oracle(p, ctx.cpu().numpy(), E, O)
    b64, b32, bfma = _oracle(p, ctx16.float().cpu().numpy(), E, O)
    err_f, a_f = conv_tolerance(y_f, f64, f32, ffma)
    err_b, a_b = conv_tolerance(y_b, b64, b32, bfma)
    assert (err_f <= a_f).all() and (err_b <= a_b).all()
    w_deq = (wu.view(O, E).cpu().numpy().astype(np.float64) - 128.0 - wz.cpu().numpy().astype(np.float64)[:, None]) \
        * ws.cpu().numpy().astype(np.float64)[:, None]
    bound = 2.0 ** -9 * (np.abs(ctx.cpu().numpy().astype(np.float64)) @ np.abs(w_deq).T) + a_b + a_f
    diff = np.abs(y_b.astype(np.float64) - y_f.astype(np.float64))
    print("worst |y_b - y_f| %.3g, its bound %.3g, a_b %.3g, a_f %.3g" % (float(diff.max()), float(bound.flat[diff.argmax()]), a_b, a_f))
    assert (diff <= bound).all(), "%d elements beyond the bound, worst excess %.3g" % (int((diff > bound).sum()),
                                                                                      float((diff - bound).max()))
    assert diff.max() > 0.0                          # the rounding is there: not the fp32 rows by another road
