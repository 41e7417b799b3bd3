"""GPU: qe_attention_bf16_ctx (capi.attention(..., out_dtype=torch.bfloat16) on torch.bfloat16 q / k / v) against
qe_attention_bf16_stored on the same operands.

The contract is one rounding: each output element is the fp32-out kernel's element rounded to bf16, nearest even.  So
out_bf16 == out_fp32.to(torch.bfloat16), compared as 16-bit patterns with no tolerance, for every instance of the kernel (the
rows of tests/attn_instances.py at N = 2, H = 2, L = 40: 8 head sizes x 14 operand modes) in both layouts.  The output is
pre-filled with a finite sentinel, so an element the kernel leaves unwritten fails."""
import numpy as np
import pytest
import torch

import attention_ref as ar
import attn_bf16_ref as br
import attn_instances as ai
import test_attention_gpu as base
from quantize_amd import capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAYOUTS = ("token", "seq")
# the new table: the operand rows of every attn_bf16_ctx_kernel<D, MODE> instance (the fp32 MFMA kernel's D and MODE sets)
CTX_ROWS = [r for r in ai.ROWS if r[0] == ai.MFMA]
QE_ERR_ARG = 4          # include/quant_engine.h


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bf16_rows(q, k, v, layout):
    return tuple(base._rows(a, layout).to(torch.bfloat16) for a in (q, k, v))


def _pair(q, k, v, layout, **ops):
    """(fp32 context of the stored kernel, bf16 context of the ctx kernel) of host arrays (N, T, H, d), as device rows."""
    N, L, H, d = q.shape
    S = k.shape[1]
    Q, K, V = _bf16_rows(q, k, v, layout)
    kw = dict(S=S, layout=layout, mask=_dev(ops.get("mask")), key_bias=_dev(ops.get("key_bias")), causal=ops.get("causal", False),
              precision="bf16")
    want = capi.attention(Q, K, V, N, L, H, **kw)
    out = torch.full((N * L, H * d), 12345.0, dtype=torch.bfloat16, device=DEV)
    got = capi.attention(Q, K, V, N, L, H, out=out, out_dtype=torch.bfloat16, **kw)
    assert got is out and want.dtype == torch.float32
    torch.cuda.synchronize()
    return want, got


def _same_bits(got, want):
    return torch.equal(got.view(torch.int16), want.to(torch.bfloat16).view(torch.int16))


def test_the_table_reaches_every_instance():
    assert len(CTX_ROWS) == 8 * 14
    assert {ai.row_instance(r)[1:] for r in CTX_ROWS} == {i[1:] for i in ai.dispatchable() if i[0] == ai.MFMA}


@pytest.mark.parametrize("D", ai.MFMA_D)
def test_every_instance_is_the_fp32_context_rounded(D):
    rows = [r for r in CTX_ROWS if r[1] == D]
    assert len(rows) == 14
    for row in rows:
        _, d, S, m, b, c, _ = row
        assert capi.attention_bf16_ctx_path(ai.L, S, ai.H, d, m, b, c) == 2
        q, k, v = (br.bf16(a) for a in base._inputs(ai.N, ai.L, S, ai.H, d, "moderate", seed=d + S))
        ops = ai.operands(row)
        for layout in LAYOUTS:
            want, got = _pair(q, k, v, layout, **ops)
            assert torch.isfinite(want).all(), ai.row_id(row)
            assert _same_bits(got, want), "%s %s: %d elements differ" % (
                ai.row_id(row), layout, int((got.view(torch.int16) != want.to(torch.bfloat16).view(torch.int16)).sum()))


def test_a_row_with_no_visible_key_is_nan_in_both():
    N, L, S, H, d = 2, 40, 45, 3, 64
    q, k, v = (br.bf16(a) for a in base._inputs(N, L, S, H, d, "moderate", seed=3))
    rows = [(1, 2, 5), (0, 1, 0), (0, 1, L - 1), (1, 0, 33)]
    mask = ar.blank_rows(N, H, L, S, rows, np.random.RandomState(4))
    for layout in LAYOUTS:
        want, got = _pair(q, k, v, layout, mask=mask)
        nan = torch.isnan(want)
        assert int(nan.sum()) == len(rows) * d
        assert torch.equal(torch.isnan(got), nan), layout
        assert torch.equal(got[~nan].view(torch.int16), want[~nan].to(torch.bfloat16).view(torch.int16)), layout


def test_callers_out_with_sequence_major_strides():
    """layout "seq": row (t, n) of the caller's (L N, E) bf16 buffer is query t of image n (o_rn = 1, o_rt = N)."""
    N, L, S, H, d = 3, 33, 65, 3, 48
    q, k, v = (br.bf16(a) for a in base._inputs(N, L, S, H, d, "moderate", seed=5))
    want_tok, got_tok = _pair(q, k, v, "token")
    want_seq, got_seq = _pair(q, k, v, "seq", causal=False)
    assert _same_bits(got_seq, want_seq)
    E = H * d
    assert torch.equal(got_seq.view(L, N, E).transpose(0, 1).reshape(N * L, E).view(torch.int16), got_tok.view(torch.int16))


def test_vit_shape_and_prescaled_q():
    """The ViT's use: 197 tokens, 12 heads of 64, q stored already scaled, scale 1."""
    N, L, H, d = 2, 197, 12, 64
    g = torch.Generator(device="cpu").manual_seed(8)
    Q, K, V = (torch.randn(N * L, H * d, generator=g).to(DEV).to(torch.bfloat16) for _ in range(3))
    want = capi.attention(Q, K, V, N, L, H, scale=1.0, precision="bf16")
    got = capi.attention(Q, K, V, N, L, H, scale=1.0, precision="bf16", out_dtype=torch.bfloat16)
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == (N * L, H * d)
    assert _same_bits(got, want)


def test_refusals():
    N, L, H = 2, 40, 2
    f = torch.zeros(N * L, H * 64, device=DEV)
    b = f.to(torch.bfloat16)
    with pytest.raises(ValueError, match="allowed only with torch.bfloat16"):
        capi.attention(f, f.clone(), f.clone(), N, L, H, precision="bf16", out_dtype=torch.bfloat16)
    unsupported = capi.lib().qe_error_string(capi.QE_ERR_UNSUPPORTED).decode()
    for d in (8, 136):
        x = torch.zeros(N * L, H * d, dtype=torch.bfloat16, device=DEV)
        assert capi.attention_bf16_ctx_path(L, L, H, d) == -1
        with pytest.raises(capi.QeError, match=unsupported):
            capi.attention(x, x.clone(), x.clone(), N, L, H, precision="bf16", out_dtype=torch.bfloat16)
    with pytest.raises(capi.QeError, match=capi.lib().qe_error_string(QE_ERR_ARG).decode()):
        capi.attention(b, b.clone(), b.clone(), N, L, H, out=b, precision="bf16", out_dtype=torch.bfloat16)     # out is q
    torch.cuda.synchronize()


def test_bf16_context_makes_no_host_sync():
    N, L, H, d = 2, 77, 4, 64
    g = torch.Generator(device="cpu").manual_seed(0)
    q, k, v = (torch.randn(N * L, H * d, generator=g).to(DEV).to(torch.bfloat16) for _ in range(3))
    out = torch.empty(N * L, H * d, dtype=torch.bfloat16, device=DEV)
    calls = [{}, dict(causal=True), dict(scale=1.0)]
    for kw in calls:                                        # warm-up: module load
        capi.attention(q, k, v, N, L, H, out=out, precision="bf16", out_dtype=torch.bfloat16, **kw)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for kw in calls:
            capi.attention(q, k, v, N, L, H, out=out, precision="bf16", out_dtype=torch.bfloat16, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
