"""GPU: the bf16 attention core (attention="engine_bf16") inside the packed ViT and the packed multi-head attention module.

  * Synthetic ViT-B/16 and the ViT-H/14-shaped one-block model (the setup of test_packed_vit_attention_gpu.py): on every
    block's own projections, e_q = max|ctx(engine_bf16) - ctx(torch fp32)| / max|V| against e_t, the same for torch's own
    bf16 SDPA on the bf16-cast projections (result cast back to fp32).  Gate: e_q <= 2 e_t -- torch's kernel rounds the same
    operands and additionally its output, so a correct kernel sits at or below it; the factor 2 covers the sampling noise
    of a maximum over a few hundred thousand elements.
  * Logits of both routes, engine_bf16 against torch: finite, right shape; the relative deviation and the top-1 agreement
    are printed, not gated (the fp32 engine core already moves logits by 2e-2 through flipped int8 codes).
  * G9 (d = 16): the gaps to the reference's simulated logits and block outputs, printed, not gated.
  * G7 and G10 were captured at a head size of 8 (E / H = 32 / 4, 48 / 6, 64 / 8), which the bf16 kernel does not take: the
    module must refuse them with a ValueError that names d, never run another kernel.  Their gap to y_packed therefore
    cannot be printed at the captured head count; it is printed for the 64-wide captures rebuilt with 4 heads (d = 16)
    against the same module's torch core, and the masked call (the float attn_mask + bool key_padding_mask of G10's
    m_float3d_pad, its first 4 heads per image) is checked there: the module's context equals the kernel's on the module's
    own projections bit for bit, lies within (2^-8 + 1e-5) max|v^| of float64 attention on the rounded projections, and
    within the same bound of the module's fp32 engine core.
  * need_weights=True is refused; the fused route with check=False never synchronises."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attn_bf16_ref as br
from quantize_amd import capi
from quantize_amd.packed import from_state_dict
from quantize_amd.packed_vit import CONFIGS, PackedViT, _attention, calibrated_state_dict, pack_vit_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPED = {"vit_b_16": dict(), "vit_h14_shape": dict(width=1280, heads=16, mlp=5120, patch=14, depth=1)}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def models():
    out = {}
    for name, kw in SHAPED.items():
        sd = calibrated_state_dict("vit_b_16", device=DEV, seed=0, **kw)
        out[name] = PackedViT.from_state_dict(sd, kw.get("heads", CONFIGS["vit_b_16"]["heads"]))
    return out


def _images(N, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(N, 3, 224, 224, generator=g).to(DEV)


def _torch_bf16(Q, K, V, N, L, H):
    E = Q.shape[-1]
    q, k, v = (t.reshape(N, L, H, E // H).transpose(1, 2).to(torch.bfloat16) for t in (Q, K, V))
    return F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(N * L, E).to(torch.float32)


@pytest.mark.parametrize("arch", list(SHAPED))
def test_bf16_context_on_model_projections(models, arch):
    m = models[arch]
    N = 2
    x = m.embed(_images(N, 21), "fused", torch.zeros(1, dtype=torch.int32, device=DEV))
    L = x.shape[0] // N
    worst = (0.0, 0.0)
    for b in m.blocks:
        codes = capi.layernorm_quantize_pack(x, b.ln1[0], b.ln1[1], m.eps, [b.q.requant(), b.k.requant(), b.v.requant()])[0]
        Q, K, V = (capi.quantlinear(lin.xq(c), lin.wq(), lin.bias, x.shape[0], lin.K, lin.O)
                   for lin, c in zip((b.q, b.k, b.v), codes))
        ct = _attention(Q, K, V, N, L, m.num_heads, "torch")
        cb = _attention(Q, K, V, N, L, m.num_heads, "engine_bf16")
        vmax = float(V.abs().max())
        e_q = float((cb - ct).abs().max()) / vmax
        e_t = float((_torch_bf16(Q, K, V, N, L, m.num_heads) - ct).abs().max()) / vmax
        print("%s %s: e_q %.3g e_t %.3g of max|V|" % (arch, b.name, e_q, e_t))
        assert torch.isfinite(cb).all(), b.name
        assert e_q <= 2 * e_t, (b.name, e_q, e_t)
        worst = max(worst, (e_q, e_t))
        x = m.block(b, x, N, "fused")
    print("%s: context engine_bf16 vs torch fp32, worst e_q %.3g (torch bf16 SDPA there: %.3g) of max|V|" % ((arch,) + worst))


@pytest.mark.parametrize("arch", list(SHAPED))
def test_bf16_logits(models, arch):
    m = models[arch]
    x = _images(2, 21)
    for route in ("fused", "layers"):
        lt = m(x, route, attention="torch")
        lb = m(x, route, attention="engine_bf16")
        assert lb.shape == lt.shape and torch.isfinite(lb).all(), route
        rel = float((lb - lt).abs().max() / lt.abs().max())
        print("%s %s: engine_bf16 vs torch attention, logits relative %.3g, top-1 agreement %d / %d"
              % (arch, route, rel, int((lb.argmax(-1) == lt.argmax(-1)).sum()), lb.shape[0]))


def test_bf16_check_false_never_syncs(models):
    m = models["vit_b_16"]
    x = _images(2, 7)
    m(x, "fused", check=False, attention="engine_bf16")     # warm-up: kernel attributes, allocator
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        logits = m(x, "fused", check=False, attention="engine_bf16")
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.isfinite(logits).all()


def test_g9_bf16_attention():
    z = np.load(os.path.join(GOLDEN, "g9_vit_module.npz"), allow_pickle=False)
    sd = pack_vit_state_dict({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd_")})
    m = PackedViT.from_state_dict({k: v.to(DEV) for k, v in sd.items()}, int(z["config"][3]))
    assert m.E // m.num_heads == 16
    x = _t(z["images"])
    want = _t(z["logits"])
    for route in ("fused", "layers"):
        logits, blocks = m.forward(x, route, keep_blocks=True, attention="engine_bf16")
        assert logits.shape == want.shape and torch.isfinite(logits).all(), route
        gaps = ["%.3g" % (float((b - _t(z["block_%d" % i])).abs().max()) / float(np.abs(z["block_%d" % i]).max()))
                for i, b in enumerate(blocks)]
        print("G9 engine_bf16 %s: logits gap %.3g (max|logit| %.3g), block gaps relative %s"
              % (route, float((logits - want).abs().max()), float(want.abs().max()), ", ".join(gaps)))
    with pytest.raises(ValueError):
        m(x, "fused", attention="sdpa")


def _captures(name):
    z = np.load(os.path.join(GOLDEN, name), allow_pickle=False)
    for key in [str(k) for k in z["index"]]:
        pre = key + "_sd_"
        sd = {"attn." + f[len(pre):]: _t(z[f]) for f in z.files if f.startswith(pre)}
        E, H, KD = [int(v) for v in z[key + "_heads"]]
        masks = {n: _t(z[key + "_" + n]) for n in ("attn_mask", "key_padding_mask") if key + "_" + n in z.files}
        yield key, sd, E, H, _t(z[key + "_query"]), _t(z[key + "_key"]), _t(z[key + "_value"]), masks, z[key + "_y_packed"]


def test_captured_head_size_is_refused():
    """G7 and G10 run 8-wide heads: engine_bf16 names d and runs nothing; need_weights=True is refused before that."""
    for name in ("g7_mha_module.npz", "g10_mha_masked.npz"):
        for key, sd, E, H, q, k, v, masks, ref in _captures(name):
            assert E // H == 8
            mha = from_state_dict(sd, num_heads=H)["attn"]
            with pytest.raises(ValueError, match="d = 8"):
                mha(q, k, v, need_weights=False, attention="engine_bf16", **masks)
            with pytest.raises(ValueError, match="need_weights"):
                mha(q, k, v, need_weights=True, attention="engine_bf16", **masks)
            with pytest.raises(ValueError):
                mha(q, k, v, need_weights=False, attention="sdpa")


def test_g7_weights_at_16_wide_heads():
    """The 64-wide G7 capture rebuilt with 4 heads: engine_bf16 against the module's own torch core, printed."""
    ran = 0
    for key, sd, E, H, q, k, v, masks, ref in _captures("g7_mha_module.npz"):
        if E != 64:
            continue
        mha = from_state_dict(sd, num_heads=4)["attn"]
        for route in ("packed", "float"):
            y, attn = mha(q, k, v, route=route, need_weights=False, attention="engine_bf16")
            yt = mha(q, k, v, route=route, need_weights=False, attention="torch")[0]
            assert attn is None and tuple(y.shape) == ref.shape and torch.isfinite(y).all()
            print("G7 %s %s at 4 heads: engine_bf16 vs torch core %.3g (max|y| %.3g; y_packed was captured at 8 heads)"
                  % (key, route, float((y - yt).abs().max()), float(yt.abs().max())))
            ran += 1
    assert ran == 2


def test_masked_module_call():
    from quantize_amd.packed import quantlinear_forward
    cap = {c[0]: c for c in _captures("g10_mha_masked.npz")}["m_float3d_pad"]
    key, sd, E, H0, q, k, v, masks, ref = cap
    H, d = 4, 16
    L, N, S = q.shape[0], q.shape[1], k.shape[0]
    am, kp = masks["attn_mask"], masks["key_padding_mask"]
    assert torch.is_floating_point(am) and kp.dtype == torch.bool and tuple(am.shape) == (N * H0, L, S)
    am = am.reshape(N, H0, L, S)[:, :H].reshape(N * H, L, S).contiguous()
    mha = from_state_dict(sd, num_heads=H)["attn"]
    kw = dict(need_weights=False, attn_mask=am, key_padding_mask=kp)
    y_b = mha(q, k, v, attention="engine_bf16", **kw)[0]
    y_f = mha(q, k, v, attention="engine", **kw)[0]
    assert torch.isfinite(y_f).all() and torch.isfinite(y_b).all()
    # the module's own projections, masks and context
    Q, K, V = (p(x, "packed").reshape(-1, E).contiguous() for p, x in ((mha.q, q), (mha.k, k), (mha.v, v)))
    add, bias = mha._additive_masks(am, kp, N, H, L, S)
    run = lambda prec: capi.attention(Q, K, V, N, L, H, S=S, layout="seq", mask=add, key_bias=bias, precision=prec)
    ctx_b, ctx_f = run("bf16"), run("fp32")
    out = quantlinear_forward(ctx_b, (mha.out_weight, mha.out_des, mha.out_scale, mha._neg_out_zero), mha.out_bias)
    assert torch.equal(out.reshape(L, N, E), y_b), "the module ran something else than qe_attention_bf16 on its projections"
    host = lambda t, T: t.cpu().numpy().reshape(T, N, H, d).transpose(1, 0, 2, 3)
    qh, kh, vh = br.rounded(host(Q, L), host(K, S), host(V, S))
    ref64 = br.ref64(qh, kh, vh, mask=add.cpu().numpy(), key_bias=bias.cpu().numpy())
    assert np.isfinite(ref64).all()
    tol = br.bound(vh)
    e_ref = float(np.abs(host(ctx_b, L) - ref64).max())
    e_core = float((ctx_b - ctx_f).abs().max())
    print("masked module call: context vs float64 on the rounded projections %.3g, vs the fp32 engine core %.3g (bound %.3g); "
          "y vs the fp32 core's y %.3g" % (e_ref, e_core, tol, float((y_b - y_f).abs().max())))
    assert e_ref <= tol, (e_ref, tol)
    assert e_core <= tol, (e_core, tol)
