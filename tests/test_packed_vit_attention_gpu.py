"""GPU: the engine's attention core (attention="engine") inside the packed ViT and the packed multi-head attention module.

  * G9 (the reference's own tiny ViT): both routes follow the reference's simulated block outputs and logits within the
    G9 tolerance of test_vit_g9_gpu.py.
  * G7 (the reference's QuantMultiheadAttention captures): with need_weights=False the engine core reproduces y_packed
    within the 2e-5 of test_packed_modules_gpu.py, in both operator routes; need_weights=True is refused.
  * Synthetic ViT-B/16 and the ViT-H/14-shaped model of test_packed_vit_gpu.py: on every block's own projections the engine
    context matches torch's within the kernel tolerance (1e-5 max|V|); the logits keep their top-1 and stay within the
    route-to-route bound of test_packed_vit_gpu.py (5 % of max|logit|: a 1e-7 relative change of the context moves a few
    int8 activation codes of the later blocks, as LayerNorm rounding does between the routes; measured 2e-2 on the
    12-block ViT-B/16); the fused route with check=False still never synchronises."""
import os

import numpy as np
import pytest
import torch

from quantize_amd.packed import from_state_dict
from quantize_amd.packed_vit import CONFIGS, PackedViT, calibrated_state_dict, pack_vit_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
G9_LOGIT_TOL = 1e-4                   # test_vit_g9_gpu.py
SHAPED = {"vit_b_16": dict(), "vit_h14_shape": dict(width=1280, heads=16, mlp=5120, patch=14, depth=1)}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def test_g9_engine_attention():
    z = np.load(os.path.join(GOLDEN, "g9_vit_module.npz"), allow_pickle=False)
    sd = pack_vit_state_dict({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd_")})
    m = PackedViT.from_state_dict({k: v.to(DEV) for k, v in sd.items()}, int(z["config"][3]))
    x = _t(z["images"])
    want = _t(z["logits"])
    for route in ("fused", "layers"):
        logits, blocks = m.forward(x, route, keep_blocks=True, attention="engine")
        for i, b in enumerate(blocks):
            ref = _t(z["block_%d" % i])
            assert float((b - ref).abs().max()) <= G9_LOGIT_TOL * float(ref.abs().max()), (route, i)
        gap = float((logits - want).abs().max())
        print("G9 logits, engine attention, %s route: %.3g" % (route, gap))
        assert gap <= G9_LOGIT_TOL, (route, gap)
    with pytest.raises(ValueError):
        m(x, "fused", attention="sdpa")
    with pytest.raises(ValueError):
        m.block(m.blocks[0], m.embed(x, "layers", None), x.shape[0], "layers", attention="flash")


def test_g7_engine_attention():
    z = np.load(os.path.join(GOLDEN, "g7_mha_module.npz"), allow_pickle=False)
    for key in [str(k) for k in z["index"]]:
        pre = key + "_sd_"
        sd = {f[len(pre):]: _t(z[f]) for f in z.files if f.startswith(pre)}
        E, H, KD = [int(v) for v in z[key + "_heads"]]
        mha = from_state_dict({"attn." + k: v for k, v in sd.items()}, num_heads=H)["attn"]
        q, k, v = _t(z[key + "_query"]), _t(z[key + "_key"]), _t(z[key + "_value"])
        ref = z[key + "_y_packed"]
        for route in ("packed", "float"):
            y, attn = mha(q, k, v, route=route, need_weights=False, attention="engine")
            assert attn is None and tuple(y.shape) == ref.shape
            err = float(np.abs(y.cpu().numpy() - ref).max())
            print("G7 %s %s: engine attention %.3g" % (key, route, err))
            assert err <= 2e-5, (key, route, err)
        with pytest.raises(ValueError):
            mha(q, k, v, need_weights=True, attention="engine")
        with pytest.raises(ValueError):
            mha(q, k, v, need_weights=False, attention="sdpa")


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


@pytest.mark.parametrize("arch", list(SHAPED))
def test_engine_context_on_model_projections(models, arch):
    """Every block's context, engine vs torch, from the same (N L, E) projections of the fused route's codes."""
    from quantize_amd import capi
    from quantize_amd.packed_vit import _attention
    m = models[arch]
    N = 2
    x = m.embed(_images(N, 21), "fused", torch.zeros(1, dtype=torch.int32, device=DEV))
    L = x.shape[0] // N
    worst = 0.0
    for b in m.blocks:
        codes = capi.layernorm_quantize_pack(x, b.ln1[0], b.ln1[1], m.eps, [b.q.requant(), b.k.requant(), b.v.requant()])[0]
        Q, K, V = (capi.quantlinear(lin.xq(c), lin.wq(), lin.bias, x.shape[0], lin.K, lin.O)
                   for lin, c in zip((b.q, b.k, b.v), codes))
        ce = _attention(Q, K, V, N, L, m.num_heads, "engine")
        ct = _attention(Q, K, V, N, L, m.num_heads, "torch")
        rel = float((ce - ct).abs().max() / V.abs().max())
        worst = max(worst, rel)
        assert rel <= 1e-5, (b.name, rel)
        x = m.block(b, x, N, "fused")
    print("%s: context engine vs torch, worst %.3g of max|V|" % (arch, worst))


@pytest.mark.parametrize("arch", list(SHAPED))
def test_engine_vs_torch_logits(models, arch):
    m = models[arch]
    x = _images(2, 21)
    for route in ("fused", "layers"):
        lt = m(x, route, attention="torch")
        le = m(x, route, attention="engine")
        rel = float((le - lt).abs().max() / lt.abs().max())
        print("%s %s: engine vs torch attention, logits relative %.3g" % (arch, route, rel))
        assert rel <= 0.05, (route, rel)
        assert torch.equal(le.argmax(-1), lt.argmax(-1)), route


def test_engine_check_false_never_syncs(models):
    m = models["vit_b_16"]
    x = _images(2, 7)
    m(x, "fused", check=False, attention="engine")     # warm-up: kernel attributes, allocator
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        logits = m(x, "fused", check=False, attention="engine")
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.isfinite(logits).all()
