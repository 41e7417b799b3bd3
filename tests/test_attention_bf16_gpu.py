"""GPU: the bf16 attention core (qe_attention_bf16, capi.attention(..., precision="bf16")) against float64 attention on the
rounded inputs q^ = bf16(fp32(q scale)), k^ = bf16(k), v^ = bf16(v) evaluated at scale 1 (tests/attn_bf16_ref.py), in both
row layouts, the output pre-filled with NaN.

Bound: |out - ref| <= (2^-8 + 1e-5) max|v^| -- the rounding of p to bf16 (relative 2^-8 per element, the only error of the
contract that is not fp32-level) plus the fp32 kernel's own 1e-5 max|V|.  tests/test_attention_bf16_cpu.py shows every case
sound and the bound reachable (a numpy emulation of the contract stays within half of it).  A wrong lane map, a missed
tail or truncation instead of rounding lands at 1e-2 .. 1 of max|V|."""
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
MFMA_ROWS = [r for r in ai.ROWS if r[0] == ai.MFMA]
QE_ERR_ARG = 4          # include/quant_engine.h


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(q, k, v, layout, mask=None, key_bias=None, causal=False, precision="bf16"):
    N, L, H, d = q.shape
    S = k.shape[1]
    out = torch.full((N * L, H * d), float("nan"), dtype=torch.float32, device=DEV)
    capi.attention(base._rows(q, layout), base._rows(k, layout), base._rows(v, layout), N, L, H, S=S, layout=layout, out=out,
                   mask=_dev(mask), key_bias=_dev(key_bias), causal=causal, precision=precision)
    torch.cuda.synchronize()
    return base._unrows(out, N, L, H, d, layout)


def _check(got, ref, vh, what, worst):
    assert np.isfinite(got).all(), what
    e = float(np.abs(got - ref).max())
    tol = br.bound(vh)
    print("%s: e %.3g, bound %.3g (%.3f of it)" % (what, e, tol, e / tol))
    assert e <= tol, (what, e, tol)
    worst[0] = max(worst[0], e / float(np.abs(vh).max()))


# ---- (a) every instance ----
@pytest.mark.parametrize("D", ai.MFMA_D)
def test_every_instance_within_the_bound(D):
    worst = [0.0]
    for row in [r for r in MFMA_ROWS if r[1] == D]:
        _, d, S, m, b, c, _ = row
        assert capi.attention_bf16_path(ai.L, S, ai.H, d, m, b, c) == 2
        q, k, v = base._inputs(ai.N, ai.L, S, ai.H, d, "moderate", seed=d + S)
        ops = ai.operands(row)
        qh, kh, vh = br.rounded(q, k, v)
        ref = br.ref64(qh, kh, vh, **ops)
        for layout in LAYOUTS:
            _check(_run(q, k, v, layout, **ops), ref, vh, "%s bf16 %s" % (ai.row_id(row), layout), worst)
    print("worst of d %d: %.3g max|v^|" % (D, worst[0]))


# ---- (b) shapes, both score regimes ----
@pytest.mark.parametrize("regime", ["moderate", "peaky"])
@pytest.mark.parametrize("case", br.CASES, ids=lambda c: "N%d-L%d-S%d-H%d-d%d" % c)
def test_shapes_within_the_bound(case, regime):
    N, L, S, H, d = case
    q, k, v = base._inputs(N, L, S, H, d, regime, seed=sum(case))
    qh, kh, vh = br.rounded(q, k, v)
    worst = [0.0]
    for ops in ({}, dict(causal=True)):
        ref = br.ref64(qh, kh, vh, **ops)
        far = float(np.abs(ar.ref64(q, k, v, **ops) - ref).max()) / float(np.abs(v).max())
        print("%s %s %s: float64 on the unrounded inputs lies %.3g max|V| from the reference" % (case, regime, sorted(ops), far))
        for layout in LAYOUTS:
            _check(_run(q, k, v, layout, **ops), ref, vh, "%s %s %s %s" % (case, regime, sorted(ops), layout), worst)
    print("worst of %s %s: %.3g max|v^|" % (case, regime, worst[0]))


# ---- (c) exact P.V and key order ----
@pytest.mark.parametrize("bias", [False, True], ids=["mask", "mask+pad_front"])
@pytest.mark.parametrize("d", br.EXACT_D)
def test_exact_pv_and_key_order(d, bias):
    """q = 0, v integers, a 0 / -inf mask: every visible p is exactly 1, so the result is float32(sum) / float32(count) bit
    for bit.  A P / V key-order mismatch or a dropped or duplicated tail key cannot survive this."""
    for L, S in br.EXACT_LS:
        q, k, v, ops, want = br.exact_case(d, L, S, bias)
        for layout in LAYOUTS:
            got = _run(q, k, v, layout, **ops)
            assert np.array_equal(got, want), (d, L, S, layout, float(np.abs(got - want).max()))


# ---- (d) bit identities ----
@pytest.mark.parametrize("case", [(2, 40, 45, 2, 48), (2, 64, 64, 2, 64)], ids=["S45-d48", "S64-d64"])
def test_bit_identities(case):
    N, L, S, H, d = case
    q, k, v = base._inputs(N, L, S, H, d, "moderate", seed=5)
    rng = np.random.RandomState(9)
    plain = {layout: _run(q, k, v, layout) for layout in LAYOUTS}
    assert np.isfinite(plain["token"]).all()
    assert np.array_equal(plain["token"], plain["seq"]), "token vs seq"
    for layout in LAYOUTS:
        for name, ops in (("zero mask", dict(mask=np.zeros((L, S), np.float32))),
                          ("zero key_bias", dict(key_bias=np.zeros((N, S), np.float32))),
                          ("zero both", dict(mask=np.zeros((L, S), np.float32), key_bias=np.zeros((N, S), np.float32)))):
            assert np.array_equal(_run(q, k, v, layout, **ops), plain[layout]), (layout, name)
        flag = _run(q, k, v, layout, causal=True)
        assert np.isfinite(flag).all()
        assert np.array_equal(flag, _run(q, k, v, layout, mask=ar.tril_inf(L, S))), (layout, "causal vs tril")
        add = ar.additive2d(L, S, rng)
        wide = np.ascontiguousarray(np.broadcast_to(add, (N * H, L, S)))
        two = _run(q, k, v, layout, mask=add)
        assert np.array_equal(two, _run(q, k, v, layout, mask=wide)), (layout, "2-D vs (N*H, L, S)")
        assert np.array_equal(two, _run(q, k, v, "seq" if layout == "token" else "token", mask=add)), "token vs seq, masked"


@pytest.mark.parametrize("d", [48, 128])
def test_vec4_loads_equal_scalar_loads(d):
    """The same (L, 44) mask once as a 2-D operand (16-byte loads) and once per image through a stride of L*S + 1 floats
    (base 16-byte aligned, image 1's rows not: scalar loads), with a bias and under causal: the same bits."""
    N, H, L, S = ai.N, ai.H, ai.L, ai.S_VEC4
    q, k, v = base._inputs(N, L, S, H, d, "moderate", seed=7)
    rng = np.random.RandomState(8)
    holes = ar.holes3d(1, 1, L, S, rng, keep=np.zeros((1, L), np.int64))[0]          # key 0 visible: survives causal
    Q, K, V = (base._rows(a, "token") for a in (q, k, v))
    for name, ops in (("mask", dict(mask=holes)), ("mask+bias", dict(mask=ar.additive2d(L, S, rng), key_bias=ar.pad_front(N, S, rng))),
                      ("causal+mask", dict(mask=holes, causal=True))):
        vec = _run(q, k, v, "token", **ops)
        assert np.isfinite(vec).all(), name
        wide = torch.zeros(N * (L * S + 1), dtype=torch.float32, device=DEV)
        wide.view(N, L * S + 1)[:, :L * S] = _dev(ops["mask"]).view(1, L * S)
        assert wide.data_ptr() % 16 == 0
        out = torch.full((N * L, H * d), float("nan"), dtype=torch.float32, device=DEV)
        bias = _dev(ops.get("key_bias"))
        capi.check(capi.lib().qe_attention_bf16(Q.data_ptr(), K.data_ptr(), V.data_ptr(), out.data_ptr(), N, L, S, H, d, L, 1, S, 1,
                                                L, 1, float(d ** -0.5), wide.data_ptr(), L * S + 1, 0,
                                                capi._ptr(bias), 1 if ops.get("causal") else 0,
                                                capi._stream(None)))
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().reshape(N, L, H, d), vec), (d, name)


# ---- (e) declared behaviours ----
def test_blank_rows_are_nan_and_local():
    N, L, S, H, d = 2, 40, 45, 3, 64
    q, k, v = base._inputs(N, L, S, H, d, "moderate", seed=3)
    rows = [(1, 2, 5), (0, 1, 0), (0, 1, L - 1), (1, 0, 33)]
    mask = ar.blank_rows(N, H, L, S, rows, np.random.RandomState(4))
    want = np.zeros((N, L, H, d), bool)
    for n, h, t in rows:
        want[n, t, h, :] = True
    qh, kh, vh = br.rounded(q, k, v)
    ref = br.ref64(qh, kh, vh, mask=mask)
    assert np.array_equal(~np.isfinite(ref), want)
    for layout in LAYOUTS:
        got = _run(q, k, v, layout, mask=mask)
        assert np.array_equal(np.isnan(got), want), layout
        assert np.isfinite(got[~want]).all(), layout
        e = float(np.abs(got - ref)[~want].max())
        assert e <= br.bound(vh), (layout, e)


def test_nan_key_poisons_its_image_and_head_only():
    N, L, S, H, d = 2, 40, 40, 3, 64
    q, k, v = base._inputs(N, L, S, H, d, "moderate", seed=3)
    kn = k.copy()
    kn[0, 3, 1, 4] = np.nan
    want = np.zeros((N, L, H, d), bool)
    want[0, :, 1, :] = True
    for layout in LAYOUTS:
        assert np.array_equal(~np.isfinite(_run(q, kn, v, layout)), want), layout


def test_unsupported_head_size_and_overlap():
    N, L, H = 2, 40, 2
    x = torch.zeros(N * L, H * 20, device=DEV)
    assert capi.attention_bf16_path(L, L, H, 20) == -1
    with pytest.raises(capi.QeError, match=capi.lib().qe_error_string(capi.QE_ERR_UNSUPPORTED).decode()):
        capi.attention(x, x.clone(), x.clone(), N, L, H, precision="bf16")
    y = torch.zeros(N * L, H * 64, device=DEV)
    with pytest.raises(capi.QeError, match=capi.lib().qe_error_string(QE_ERR_ARG).decode()):
        capi.attention(y, y.clone(), y.clone(), N, L, H, out=y, precision="bf16")
    torch.cuda.synchronize()


# ---- (f) the fp32 kernel is untouched by the new argument ----
def test_fp32_precision_is_the_default_call():
    N, L, S, H, d = 2, 40, 45, 2, 64
    q, k, v = base._inputs(N, L, S, H, d, "moderate", seed=21)
    ops = dict(mask=ar.holes3d(N, H, L, S, np.random.RandomState(22)))
    Q, K, V = (base._rows(a, "token") for a in (q, k, v))
    for kw in ({}, dict(mask=_dev(ops["mask"]))):
        a = capi.attention(Q, K, V, N, L, H, S=S, **kw)
        b = capi.attention(Q, K, V, N, L, H, S=S, precision="fp32", **kw)
        c = capi.attention(Q, K, V, N, L, H, S=S, precision="bf16", **kw)
        torch.cuda.synchronize()
        assert torch.isfinite(a).all() and torch.equal(a, b), sorted(kw)
        assert not torch.equal(a, c), "bf16 returned the fp32 kernel's bits"


def test_bf16_attention_makes_no_host_sync():
    N, L, H, d = 2, 77, 4, 64
    g = torch.Generator(device="cpu").manual_seed(0)
    q, k, v = (torch.randn(N * L, H * d, generator=g).to(DEV) for _ in range(3))
    bias = _dev(ar.pad_tail(N, L, np.random.RandomState(0)))
    out = torch.empty_like(q)
    calls = [{}, dict(causal=True), dict(key_bias=bias)]
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
