"""GPU: qe_quantlinear_bf16 (the LIN_BF16 epilogue of the int8 MFMA linears, and its two-pass form) on every row of
tests/lin_instances.py with B <= 3152, drawn with the row's XQ[i % 3] quantiser as tests/test_lin_instances_gpu.py draws it.

The contract needs no tolerance: out = bf16(y * post_scale) with y the fp32 value qe_quantlinear computes, one fp32
multiply, round to nearest even -- which is what torch's (y * post_scale).to(torch.bfloat16) does to the same y.  So the two
are compared as 16-bit patterns, element for element; a NaN matches a NaN at the same index (the payload is not part of
the contract)."""
import numpy as np
import pytest
import torch

import lin_instances as li
import test_lin_instances_gpu as tl
from quantize_amd import capi

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ROWS = [(i, r) for i, r in enumerate(li.ROWS) if r[0] <= li.BF16_MAX_B]
SCALES = (1.0, 0.125, float(np.float32(48 ** -0.5)))


def test_the_rows_reach_every_form():
    """Forms 1 - 4: the four MFMA instances of the epilogue; form 0: the generic kernel, which has only the two-pass route."""
    assert {r[4] for _, r in ROWS} == {0, 1, 2, 3, 4}
    assert {r[4] for _, r in ROWS if r[2] % 64 == 0} >= {1, 2, 3, 4}
    assert {li.XQ[i % 3] for i, _ in ROWS} == set(li.XQ)


def _same_bits(got, want, what):
    assert got.dtype == torch.bfloat16 and want.dtype == torch.bfloat16 and got.shape == want.shape, what
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn), "%s: NaN at other indices" % what
    g, w = got.view(torch.int16).masked_fill(gn, 0), want.view(torch.int16).masked_fill(wn, 0)
    bad = g != w
    assert not bool(bad.any()), "%s: %d of %d elements differ" % (what, int(bad.sum()), g.numel())


@pytest.mark.parametrize("i,row", ROWS, ids=["%dx%dx%d" % r[:3] + ("-" + "-".join(r[3].values()) if r[3] else "") for _, r in ROWS])
def test_bf16_row_equals_the_rounded_fp32_row(i, row):
    B, K, O, env, form, note = row
    op = tl._operands(i, B, K, O)
    xq, wq, bias = op["xq"], op["wq"], op["bias"]
    env = env or {}
    with capi.knobs(**env):
        assert capi.linear_form(xq, wq, B, K, O) == form, note
        y = capi.quantlinear(xq, wq, bias, B, K, O)
        assert torch.isfinite(y).all(), note
        path = capi.quantlinear_bf16_path(xq, wq, B, K, O)
        if form == 0:
            assert path == 0, note
        elif O % 64 == 0:
            assert path == 1, note
        for ps in SCALES:
            got = capi.quantlinear_bf16(xq, wq, bias, B, K, O, post_scale=ps)
            assert capi.quantlinear_bf16_path(xq, wq, B, K, O, got) == path
            _same_bits(got, (y * ps).to(torch.bfloat16), "%s, post_scale %r, path %d" % (note, ps, path))
        assert (y.to(torch.bfloat16).float() != y).any(), "nothing was rounded"
    with capi.knobs(QE_LIN_EPI="0", **env):
        assert capi.quantlinear_bf16_path(xq, wq, B, K, O) == 0, note
        for ps in SCALES:
            got = capi.quantlinear_bf16(xq, wq, bias, B, K, O, post_scale=ps)
            _same_bits(got, (y * ps).to(torch.bfloat16), "%s, post_scale %r, QE_LIN_EPI=0" % (note, ps))
    torch.cuda.synchronize()


@pytest.mark.parametrize("i", [i for i, r in ROWS if r[:3] in ((197, 768, 768), (100, 256, 256), (64, 100, 40))])
def test_nan_and_inf_bias_columns(i):
    """A NaN and an inf in the bias come out as NaN / inf in exactly those columns (fused and two-pass)."""
    B, K, O, env, form, note = li.ROWS[i]
    op = tl._operands(i, B, K, O)
    bias = op["bias"].clone()
    cn, ci = O // 3, O - 2
    bias[cn], bias[ci] = float("nan"), float("-inf")
    for knobs in (env or {}, dict(env or {}, QE_LIN_EPI="0")):
        with capi.knobs(**knobs):
            got = capi.quantlinear_bf16(op["xq"], op["wq"], bias, B, K, O, post_scale=0.125).float()
        want_nan = torch.zeros(B, O, dtype=torch.bool, device=DEV)
        want_nan[:, cn] = True
        want_inf = torch.zeros_like(want_nan)
        want_inf[:, ci] = True
        assert torch.equal(torch.isnan(got), want_nan), (note, knobs)
        assert torch.equal(got == float("-inf"), want_inf) and not bool((got == float("inf")).any()), (note, knobs)
