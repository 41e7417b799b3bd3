"""GPU: qe_attention_bf16_stored (capi.attention(..., precision="bf16") on torch.bfloat16 q / k / v) against the fp32-buffer
bf16 core on the same values.

The contract is qe_attention_bf16's with q^ = bf16(fp32(q) scale), k^ = k, v^ = v.  On q, k, v that ARE bf16 values the two
entry points build the same fragments and run the same text after them, so their outputs are compared as int32 bit patterns:
no tolerance.  Against float64 attention on the rounded inputs the bound is the existing one, (2^-8 + 1e-5) max|v^|
(tests/attn_bf16_ref.py).  The output is pre-filled with NaN, so an element the kernel leaves unwritten fails."""
import numpy as np
import pytest
import torch

import attention_ref as ar
import attn_bf16_ref as br
import attn_instances as ai
import test_attention_gpu as base
import test_qkv_bf16_cpu as host
from quantize_amd import capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAYOUTS = ("token", "seq")
MFMA_ROWS = [r for r in ai.ROWS if r[0] == ai.MFMA]
QE_ERR_ARG = 4          # include/quant_engine.h


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(q, k, v, layout, stored, scale=None, mask=None, key_bias=None, causal=False):
    """q, k, v: host fp32 arrays (N, T, H, d).  stored: hand them over as torch.bfloat16 rows (exact for bf16 values)."""
    N, L, H, d = q.shape
    S = k.shape[1]
    Q, K, V = (base._rows(a, layout) for a in (q, k, v))
    if stored:
        for t in (Q, K, V):
            assert torch.equal(t.to(torch.bfloat16).float(), t), "not bf16 values"
        Q, K, V = (t.to(torch.bfloat16) for t in (Q, K, V))
    out = torch.full((N * L, H * d), float("nan"), dtype=torch.float32, device=DEV)
    got = capi.attention(Q, K, V, N, L, H, S=S, layout=layout, scale=scale, out=out, mask=_dev(mask), key_bias=_dev(key_bias),
                         causal=causal, precision="bf16")
    assert got is out
    torch.cuda.synchronize()
    return base._unrows(out, N, L, H, d, layout)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _rounded_inputs(N, L, S, H, d, regime, seed):
    return tuple(br.bf16(a) for a in base._inputs(N, L, S, H, d, regime, seed=seed))


# ---- every instance ----
@pytest.mark.parametrize("D", ai.MFMA_D)
def test_every_instance_equals_its_fp32_buffer_twin(D):
    rows = [r for r in MFMA_ROWS if r[1] == D]
    assert len(rows) == 14
    total = left_out = 0
    for row in rows:
        _, d, S, m, b, c, _ = row
        assert capi.attention_bf16_stored_path(ai.L, S, ai.H, d, m, b, c) == 2
        q, k, v = _rounded_inputs(ai.N, ai.L, S, ai.H, d, "moderate", d + S)
        ops = ai.operands(row)
        twin = _run(q, k, v, "token", False, **ops)
        got = _run(q, k, v, "token", True, **ops)
        assert np.array_equal(_bits(got), _bits(twin)), "%s: %d elements differ" % (ai.row_id(row), int((_bits(got) != _bits(twin)).sum()))
        qh, kh, vh = br.rounded(q, k, v)
        assert np.array_equal(kh, k) and np.array_equal(vh, v)
        ref = br.ref64(qh, kh, vh, **ops)
        total += ref.size
        left_out += int((~np.isfinite(ref)).sum())
        assert np.isfinite(got).all(), ai.row_id(row)
        e, tol = float(np.abs(got - ref).max()), br.bound(vh)
        print("%s: e %.3g, bound %.3g" % (ai.row_id(row), e, tol))
        assert e <= tol, (ai.row_id(row), e, tol)
    assert total > 0 and left_out / total == 0.0


# ---- shapes, both score regimes, both layouts ----
@pytest.mark.parametrize("regime", ["moderate", "peaky"])
@pytest.mark.parametrize("case", br.CASES, ids=lambda c: "N%d-L%d-S%d-H%d-d%d" % c)
def test_shapes_equal_the_fp32_buffer_form(case, regime):
    N, L, S, H, d = case
    q, k, v = _rounded_inputs(N, L, S, H, d, regime, sum(case))
    for ops in ({}, dict(causal=True)):
        for layout in LAYOUTS:
            twin = _run(q, k, v, layout, False, **ops)
            got = _run(q, k, v, layout, True, **ops)
            assert np.isfinite(got).all(), (case, regime, sorted(ops), layout)
            assert np.array_equal(_bits(got), _bits(twin)), (case, regime, sorted(ops), layout, int((_bits(got) != _bits(twin)).sum()))


# ---- the ViT's use: q stored scaled and rounded, scale 1 ----
@pytest.mark.parametrize("case", [(2, 197, 197, 12, 64), (3, 17, 17, 4, 16), (2, 33, 65, 3, 48)], ids=lambda c: "N%d-L%d-S%d-H%d-d%d" % c)
def test_prescaled_q_with_scale_one(case):
    N, L, S, H, d = case
    q, k, v = base._inputs(N, L, S, H, d, "moderate", seed=sum(case))       # q not rounded: the fp32-buffer form rounds q scale
    k, v = br.bf16(k), br.bf16(v)
    qs = br.rounded(q, k, v)[0]                                              # bf16(fp32(q) * fp32(d ** -0.5))
    assert not np.array_equal(qs, br.bf16(q))
    for layout in LAYOUTS:
        twin = _run(q, k, v, layout, False)
        got = _run(qs, k, v, layout, True, scale=1.0)
        assert np.isfinite(got).all()
        assert np.array_equal(_bits(got), _bits(twin)), (case, layout)


# ---- declared behaviours ----
def test_blank_rows_are_nan_and_local():
    N, L, S, H, d = 2, 40, 45, 3, 64
    q, k, v = _rounded_inputs(N, L, S, H, d, "moderate", 3)
    rows = [(1, 2, 5), (0, 1, 0), (0, 1, L - 1), (1, 0, 33)]
    mask = ar.blank_rows(N, H, L, S, rows, np.random.RandomState(4))
    want = np.zeros((N, L, H, d), bool)
    for n, h, t in rows:
        want[n, t, h, :] = True
    qh, kh, vh = br.rounded(q, k, v)
    ref = br.ref64(qh, kh, vh, mask=mask)
    assert np.array_equal(~np.isfinite(ref), want)
    for layout in LAYOUTS:
        got = _run(q, k, v, layout, True, mask=mask)
        assert np.array_equal(np.isnan(got), want), layout
        assert np.isfinite(got[~want]).all(), layout
        e = float(np.abs(got - ref)[~want].max())
        assert e <= br.bound(vh), (layout, e)


def test_nan_key_poisons_its_image_and_head_only():
    N, L, S, H, d = 2, 40, 40, 3, 64
    q, k, v = _rounded_inputs(N, L, S, H, d, "moderate", 3)
    Q, K, V = (base._rows(a, "token").to(torch.bfloat16) for a in (q, k, v))
    K.view(N, S, H, d)[0, 3, 1, 4] = float("nan")
    want = np.zeros((N, L, H, d), bool)
    want[0, :, 1, :] = True
    out = torch.full((N * L, H * d), float("nan"), dtype=torch.float32, device=DEV)
    capi.attention(Q, K, V, N, L, H, out=out, precision="bf16")
    torch.cuda.synchronize()
    assert np.array_equal(~np.isfinite(out.cpu().numpy().reshape(N, L, H, d)), want)


# ---- refusals ----
def test_dtypes_head_sizes_and_overlap():
    N, L, H = 2, 40, 2
    f = torch.zeros(N * L, H * 64, device=DEV)
    b = f.to(torch.bfloat16)
    for q, k, v in ((b, f, f), (f, b, f), (f, f, b)):
        with pytest.raises(ValueError):
            capi.attention(q, k, v, N, L, H, precision="bf16")
    with pytest.raises(ValueError):
        capi.attention(b, b.clone(), b.clone(), N, L, H, precision="fp32")
    with pytest.raises(ValueError):
        capi.attention(b, b.clone(), b.clone(), N, L, H)
    unsupported = capi.lib().qe_error_string(capi.QE_ERR_UNSUPPORTED).decode()
    for d in (8, 136):
        x = torch.zeros(N * L, H * d, dtype=torch.bfloat16, device=DEV)
        assert capi.attention_bf16_stored_path(L, L, H, d) == -1
        with pytest.raises(capi.QeError, match=unsupported):
            capi.attention(x, x.clone(), x.clone(), N, L, H, precision="bf16")
    # out overlapping k: k is the first half of out's bytes
    out = torch.zeros(N * L, H * 64, device=DEV)
    k = out.view(torch.bfloat16).reshape(-1)[:N * L * H * 64].view(N * L, H * 64)
    assert k.data_ptr() == out.data_ptr()
    with pytest.raises(capi.QeError, match=capi.lib().qe_error_string(QE_ERR_ARG).decode()):
        capi.attention(b, k, b.clone(), N, L, H, out=out, precision="bf16")
    torch.cuda.synchronize()


def test_bad_arguments_get_the_bf16_entry_points_answer():
    """Every argument list tests/test_attention_bf16_cpu.py has refused gets qe_attention_bf16's code from
    qe_attention_bf16_stored (the check lives in tests/test_qkv_bf16_cpu.py: nothing is launched)."""
    host.check_stored_refusals()


def test_stored_attention_makes_no_host_sync():
    N, L, H, d = 2, 77, 4, 64
    g = torch.Generator(device="cpu").manual_seed(0)
    q, k, v = (torch.randn(N * L, H * d, generator=g).to(DEV).to(torch.bfloat16) for _ in range(3))
    bias = _dev(ar.pad_tail(N, L, np.random.RandomState(0)))
    out = torch.empty(N * L, H * d, dtype=torch.float32, device=DEV)
    calls = [{}, dict(causal=True), dict(key_bias=bias), dict(scale=1.0)]
    for kw in calls:                                        # warm-up: module load
        capi.attention(q, k, v, N, L, H, out=out, precision="bf16", **kw)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for kw in calls:
            capi.attention(q, k, v, N, L, H, out=out, precision="bf16", **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
