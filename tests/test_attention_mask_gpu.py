"""GPU: the masked attention core (qe_attention_masked) against the float64 yardstick of tests/attention_ref.py, in both row
layouts, on both kernels (the MFMA kernel and the VALU kernel QE_ATTN=0 forces) wherever both apply, output pre-filled
with NaN -- the protocol of tests/test_attention_gpu.py, whose inputs and layout helpers are reused.

Tolerance (the project's rule for the attention core, unchanged): e_q = max |engine - ref64|, e_t = max |torch fp32 SDPA
given the same merged mask - ref64|; e_q <= max(4 e_t, 1e-6 max|V|) and e_q <= 1e-5 max|V|.  Every mask of the accuracy
test leaves each row a visible key (asserted), so every element is compared."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attention_ref as ar
import test_attention_gpu as base
from quantize_amd import capi
from quantize_amd.packed import PackedMultiheadAttention, from_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (N, L, S, H, d): the CLIP text transformer, ViT-B/16, ViT-H/14, S != L, one head at d = 128, the tiny ViT, and the
# VALU-only head sizes
CASES = [(4, 77, 77, 8, 64), (2, 197, 197, 12, 64), (2, 257, 257, 16, 80), (2, 33, 65, 3, 32), (1, 197, 197, 1, 128),
         (3, 17, 17, 4, 16), (2, 37, 45, 3, 20), (1, 40, 70, 2, 136)]
KINDS = ["additive2d", "tril", "causal", "holes3d", "pad_tail", "pad_front", "all"]
_id = lambda c: "N%d-L%d-S%d-H%d-d%d" % c


def _operands(kind, N, L, S, H, rng):
    """dict(mask=, key_bias=, causal=) of host arrays for one mask kind."""
    if kind == "additive2d":
        return dict(mask=ar.additive2d(L, S, rng))
    if kind == "tril":
        return dict(mask=ar.tril_inf(L, S))
    if kind == "causal":
        return dict(causal=True)
    if kind == "holes3d":
        return dict(mask=ar.holes3d(N, H, L, S, rng))
    if kind == "pad_tail":
        return dict(key_bias=ar.pad_tail(N, S, rng))
    if kind == "pad_front":
        return dict(key_bias=ar.pad_front(N, S, rng))
    if kind == "all":           # key 0 stays visible to every row: the tail padding keeps >= 1 key, causal keeps s <= t
        return dict(mask=ar.additive2d(L, S, rng), key_bias=ar.pad_tail(N, S, rng), causal=True)
    raise ValueError(kind)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(q, k, v, layout, mask=None, key_bias=None, causal=False):
    N, L, H, d = q.shape
    S = k.shape[1]
    out = torch.full((N * L, H * d), float("nan"), dtype=torch.float32, device=DEV)
    capi.attention(base._rows(q, layout), base._rows(k, layout), base._rows(v, layout), N, L, H, S=S, layout=layout, out=out,
                   mask=_dev(mask), key_bias=_dev(key_bias), causal=causal)
    torch.cuda.synchronize()
    return base._unrows(out, N, L, H, d, layout)


def _torch_sdpa(q, k, v, m):
    t = lambda a: torch.from_numpy(a).to(DEV).transpose(1, 2)          # (N, H, T, d)
    return F.scaled_dot_product_attention(t(q), t(k), t(v), attn_mask=_dev(m)).transpose(1, 2).cpu().numpy()


def _each_kernel(L, S, H, d):
    for kern in base._kernels(L, S, H, d):
        with capi.knobs(QE_ATTN=None if kern == "mfma" else "0"):
            assert capi.attention_masked_path(L, S, H, d, 1, 1, 1) == (1 if kern == "mfma" else 0)
            for layout in ("token", "seq"):
                yield kern, layout


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_masked_attention_vs_float64(case, kind):
    N, L, S, H, d = case
    q, k, v = base._inputs(N, L, S, H, d, "moderate", seed=sum(case))
    ops = _operands(kind, N, L, S, H, np.random.RandomState(sum(case) + 1))
    m = ar.merged(N, H, L, S, **ops)
    assert ar.visible(m).all()
    ref = ar.ref64(q, k, v, **ops)
    assert np.isfinite(ref).all()
    e_t = float(np.abs(_torch_sdpa(q, k, v, m) - ref).max())
    vmax = float(np.abs(v).max())
    for kern, layout in _each_kernel(L, S, H, d):
        got = _run(q, k, v, layout, **ops)
        assert np.isfinite(got).all(), (kern, layout)
        e_q = float(np.abs(got - ref).max())
        print("%s %s %s %s: e_q %.3g e_t %.3g (max|V| %.3g)" % (case, kind, kern, layout, e_q, e_t, vmax))
        assert e_q <= max(4 * e_t, 1e-6 * vmax), (kern, layout, e_q, e_t)
        assert e_q <= 1e-5 * vmax, (kern, layout, e_q)


@pytest.mark.parametrize("case", [(4, 77, 77, 8, 64), (2, 33, 65, 3, 32), (2, 64, 64, 2, 64), (2, 37, 45, 3, 20)], ids=_id)
def test_bit_identities(case):
    """Finite inputs.  (2, 64, 64, 2, 64) has S % 4 == 0: the 16-byte mask loads."""
    N, L, S, H, d = case
    q, k, v = base._inputs(N, L, S, H, d, "moderate", seed=5)
    rng = np.random.RandomState(9)
    add = ar.additive2d(L, S, rng)
    for kern, layout in _each_kernel(L, S, H, d):
        plain = _run(q, k, v, layout)
        for name, ops in (("zero mask", dict(mask=np.zeros((L, S), np.float32))),
                          ("zero 3-D mask", dict(mask=np.zeros((N * H, L, S), np.float32))),
                          ("zero key_bias", dict(key_bias=np.zeros((N, S), np.float32))),
                          ("zero both", dict(mask=np.zeros((L, S), np.float32), key_bias=np.zeros((N, S), np.float32)))):
            assert np.array_equal(_run(q, k, v, layout, **ops), plain), (kern, layout, name)
        flag = _run(q, k, v, layout, causal=True)
        assert np.array_equal(flag, _run(q, k, v, layout, mask=ar.tril_inf(L, S))), (kern, layout, "causal vs tril")
        assert not np.array_equal(flag, plain)
        two = _run(q, k, v, layout, mask=add)
        wide = np.ascontiguousarray(np.broadcast_to(add, (N * H, L, S)))
        assert np.array_equal(two, _run(q, k, v, layout, mask=wide)), (kern, layout, "2-D vs (N*H, L, S)")
        assert np.array_equal(two, _run(q, k, v, layout, mask=wide.reshape(N, H, L, S))), (kern, layout, "2-D vs 4-D")
        assert np.array_equal(two, _run(q, k, v, layout, mask=wide.reshape(N, H, L, S)[:, 0].copy())), (kern, layout, "(N, L, S)")


@pytest.mark.parametrize("case", [(2, 40, 40, 3, 64), (2, 40, 40, 3, 20), (2, 77, 77, 2, 64)], ids=_id)
def test_fully_masked_rows_are_nan_and_local(case):
    N, L, S, H, d = case
    q, k, v = base._inputs(N, L, S, H, d, "moderate", seed=3)
    rows = [(1, 2, 5), (0, 1, 0), (0, 1, L - 1), (1, 0, 33)]
    rows = [(n, h % H, t) for n, h, t in rows]
    mask = ar.blank_rows(N, H, L, S, rows, np.random.RandomState(4))
    want = np.zeros((N, L, H, d), bool)
    for n, h, t in rows:
        want[n, t, h, :] = True
    ref = ar.ref64(q, k, v, mask=mask)
    assert np.array_equal(~np.isfinite(ref), want)
    ok = ~want
    e_t = float(np.abs(_torch_sdpa(q, k, v, ar.merged(N, H, L, S, mask)) - ref)[ok].max())
    vmax = float(np.abs(v).max())
    for kern, layout in _each_kernel(L, S, H, d):
        got = _run(q, k, v, layout, mask=mask)
        assert np.array_equal(~np.isfinite(got), want), (kern, layout)
        assert np.isnan(got[want]).all(), (kern, layout)
        e_q = float(np.abs(got - ref)[ok].max())
        print("%s blank rows %s %s: e_q %.3g e_t %.3g" % (case, kern, layout, e_q, e_t))
        assert e_q <= max(4 * e_t, 1e-6 * vmax) and e_q <= 1e-5 * vmax, (kern, layout, e_q, e_t)
    # padding every key of one image: that image is NaN, the others are untouched
    bias = np.zeros((N, S), np.float32)
    bias[1, :] = ar.NEG
    for kern, layout in _each_kernel(L, S, H, d):
        got = _run(q, k, v, layout, key_bias=bias)
        assert np.isnan(got[1]).all() and np.array_equal(got[0], _run(q, k, v, layout)[0]), (kern, layout)


def test_masked_attention_makes_no_host_sync():
    N, L, H, d = 4, 77, 8, 64
    g = torch.Generator(device="cpu").manual_seed(0)
    q, k, v = (torch.randn(N * L, H * d, generator=g).to(DEV) for _ in range(3))
    mask, bias = _dev(ar.tril_inf(L, L)), _dev(ar.pad_tail(N, L, np.random.RandomState(0)))
    wide = _dev(ar.holes3d(N, H, L, L, np.random.RandomState(1)))
    out = torch.empty_like(q)
    calls = [dict(mask=mask), dict(key_bias=bias), dict(causal=True), dict(mask=wide, key_bias=bias),
             dict(mask=mask, key_bias=bias, causal=True)]
    for kw in calls:                                        # warm-up: module load
        capi.attention(q, k, v, N, L, H, out=out, **kw)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for kw in calls:
            capi.attention(q, k, v, N, L, H, out=out, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()


def _g10():
    z = np.load(os.path.join(GOLDEN, "g10_mha_masked.npz"), allow_pickle=False)
    for key in [str(k) for k in z["index"]]:
        pre = key + "_sd_"
        sd = {f[len(pre):]: _dev(z[f]) for f in z.files if f.startswith(pre)}
        E, H, KD = [int(v) for v in z[key + "_heads"]]
        mha = from_state_dict({"attn." + k: v for k, v in sd.items()}, num_heads=H)["attn"]
        masks = {n: (_dev(z[key + "_" + n]) if key + "_" + n in z.files else None) for n in ("attn_mask", "key_padding_mask")}
        yield key, mha, _dev(z[key + "_query"]), _dev(z[key + "_key"]), _dev(z[key + "_value"]), masks, z[key + "_y_packed"]


G7_BOUND, G7_YMAX = 2e-5, 0.88          # test_packed_modules_gpu.py / test_g7_engine_attention; max|y_packed| over G7


def test_g10_masked_reference_captures():
    """PackedMultiheadAttention from the G10 state_dicts reproduces the reference's masked packed forward with both cores and
    both operator routes within G7's 2e-5.  Same generator settings as G7; max|y_packed| is 0.75 .. 1.12 in three captures
    (within 2x of G7's 0.88: the bound stays 2e-5) and 2.25 in causal_float (its first rows see one or two keys, so they do
    not average down): there the bound is scaled by that ratio, 2e-5 * 2.25 / 0.88 = 5.1e-5."""
    for key, mha, q, k, v, masks, ref in _g10():
        ymax = float(np.abs(ref).max())
        bound = G7_BOUND * (ymax / G7_YMAX if ymax > 2 * G7_YMAX else 1.0)
        for core in ("torch", "engine"):
            for route in ("packed", "float"):
                y, attn = mha(q, k, v, route=route, need_weights=False, attention=core, **masks)
                assert attn is None and tuple(y.shape) == ref.shape
                err = float(np.abs(y.cpu().numpy() - ref).max())
                print("G10 %s %s %s: %.3g (bound %.3g, max|y| %.3g)" % (key, core, route, err, bound, ymax))
                assert err <= bound, (key, core, route, err)
        with pytest.raises(ValueError):
            mha(q, k, v, need_weights=True, attention="engine", **masks)


def test_packed_mha_bool_masks_equal_their_float_form():
    for key, mha, q, k, v, masks, ref in _g10():
        L, S = q.shape[0], k.shape[0]
        as_float = lambda m: None if m is None else (
            torch.zeros(m.shape, device=DEV).masked_fill_(m, float("-inf")) if m.dtype == torch.bool else m)
        if all(m is None or m.dtype != torch.bool for m in masks.values()):
            continue
        for core in ("torch", "engine"):
            a = mha(q, k, v, need_weights=False, attention=core, **masks)[0]
            b = mha(q, k, v, need_weights=False, attention=core, **{n: as_float(m) for n, m in masks.items()})[0]
            assert torch.isfinite(a).all() and torch.equal(a, b), (key, core)
    # is_causal=True is the tril mask, in both cores
    key, mha, q, k, v, masks, ref = next(_g10())
    L = q.shape[0]
    tril = torch.ones(L, L, dtype=torch.bool, device=DEV).tril().logical_not()
    kk, vv = k[:L].contiguous(), v[:L].contiguous()
    for core in ("torch", "engine"):
        a = mha(q, kk, vv, need_weights=False, attention=core, is_causal=True)[0]
        b = mha(q, kk, vv, need_weights=False, attention=core, attn_mask=tril)[0]
        assert torch.isfinite(a).all() and torch.equal(a, b), core


def _clip_block(rng, E, H):
    """A packed attention block at the CLIP text width on synthetic weights (packed_vit's construction)."""
    from quantize_amd.packed_vit import _lin_entries
    sd = {}
    for i, name in enumerate("qkv"):
        e = _lin_entries(rng, E, E, 8, bias=True)
        sd[name + "_proj_weight"], sd[name + "_proj_des"] = e["weight"], e["w_des"]
        sd[name + "_proj_scale"], sd[name + "_proj_zero"] = e["w_scale"], e["w_zero"]
        sd[name + "_quantizer.scale"] = torch.tensor([4.5 / 127], dtype=torch.float32)      # int8 over |x| <= 4.5
        for f in ("zero", "qmin", "qmax"):
            sd[name + "_quantizer." + f] = e["a_quantizer." + f]
        sd.setdefault("_bias", []).append(e["bias"])
    sd["in_proj_bias"] = torch.cat(sd.pop("_bias"))
    e = _lin_entries(rng, E, E, 8, bias=True)
    sd["out_proj.weight"], sd["out_proj_des"], sd["out_proj_scale"], sd["out_proj_zero"] = \
        e["weight"], e["w_des"], e["w_scale"], e["w_zero"]
    sd["out_proj.bias"] = e["bias"]
    return PackedMultiheadAttention.from_state_dict({k: v.to(DEV) for k, v in sd.items()}, "", H)


def test_causal_stack_engine_vs_torch_context():
    """Two causal attention blocks at the CLIP text shape (L = 77, 8 heads of 64), x <- x + attn(x): on each block's own
    projections the engine's causal context matches the torch core's (bmm scores + tril mask, softmax, bmm) within the
    kernel tolerance, 1e-5 max|V|; the module's two cores are compared on the same block."""
    N, L, E, H = 4, 77, 512, 8
    d = E // H
    rng = np.random.RandomState(12)
    blocks = [_clip_block(rng, E, H) for _ in range(2)]
    x = torch.from_numpy(rng.normal(0, 1, size=(L, N, E)).astype(np.float32)).to(DEV).clamp_(-4.4, 4.4)
    tril = _dev(ar.tril_inf(L, L))
    for i, b in enumerate(blocks):
        Q, K, V = (p(x, "packed").reshape(L * N, E).contiguous() for p in (b.q, b.k, b.v))
        ce = capi.attention(Q, K, V, N, L, H, layout="seq", causal=True)
        heads = lambda t: t.reshape(L, N * H, d).transpose(0, 1)
        p = torch.softmax(torch.bmm(heads(Q) * d ** -0.5, heads(K).transpose(1, 2)) + tril, dim=-1)
        ct = torch.bmm(p, heads(V)).transpose(0, 1).reshape(L * N, E)
        rel = float((ce - ct).abs().max() / V.abs().max())
        print("block %d: causal context engine vs torch %.3g of max|V|" % (i, rel))
        assert torch.isfinite(ce).all() and rel <= 1e-5, (i, rel)
        ye = b(x, x, x, need_weights=False, attention="engine", is_causal=True)[0]
        yt = b(x, x, x, need_weights=False, attention="torch", is_causal=True)[0]
        assert torch.isfinite(ye).all() and tuple(ye.shape) == (L, N, E)
        x = (x + yt).clamp_(-4.4, 4.4)
