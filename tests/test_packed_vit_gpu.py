"""GPU: a synthetic packed ViT run end to end.  The fused route (LayerNorm + codes in one pass, GELU + codes and the residual
adds in the linears' epilogues, the patch embedding as a GEMM) gives bit for bit the same logits and block outputs with its
fused epilogues as with their two-pass forms (QE_LIN_EPI=0), follows the layers route (the reference's dataflow with the
engine plugged in) up to LayerNorm / GELU rounding, never synchronises with the host under check=False, and raises on a
NaN image."""
import pytest
import torch
import torch.nn.functional as F

from quantize_amd import capi
from quantize_amd.packed_vit import CONFIGS, PackedViT, calibrated_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ViT-B/16 layouts at other widths (224 x 224 images): ViT-S/16's (E 384: LayerNorm's NV = 2 instance) and ViT-H/14's (E 1280:
# NV = 8; a 14 x 14 patch, so the patch GEMM has K = 588 and runs on the fp32 kernel), at reduced depth
SHAPED = {"vit_s16_shape": dict(width=384, heads=6, mlp=1536, depth=2),
          "vit_h14_shape": dict(width=1280, heads=16, mlp=5120, patch=14, depth=1)}


@pytest.fixture(scope="module")
def models():
    out = {}
    for arch in ("vit_tiny_test", "vit_b_16"):
        sd = calibrated_state_dict(arch, device=DEV, seed=0)
        out[arch] = PackedViT.from_state_dict(sd, CONFIGS[arch]["heads"])
    for name, kw in SHAPED.items():
        sd = calibrated_state_dict("vit_b_16", device=DEV, seed=0, **kw)
        out[name] = PackedViT.from_state_dict(sd, kw["heads"])
    return out


def _images(N, arch, seed):
    s = CONFIGS.get(arch, CONFIGS["vit_b_16"])["image_size"]
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(N, 3, s, s, generator=g).to(DEV)


@pytest.mark.parametrize("arch,N", [("vit_tiny_test", 2), ("vit_tiny_test", 5), ("vit_b_16", 1), ("vit_b_16", 2), ("vit_b_16", 3),
                                    ("vit_s16_shape", 3), ("vit_h14_shape", 2)])
def test_fused_epilogues_equal_two_pass(models, arch, N):
    m = models[arch]
    x = _images(N, arch, N)
    with capi.knobs(QE_LIN_EPI=None):
        l1, b1 = m.forward(x, "fused", keep_blocks=True)
    with capi.knobs(QE_LIN_EPI="0"):
        l0, b0 = m.forward(x, "fused", keep_blocks=True)
    assert torch.isfinite(l1).all() and l1.std() > 0
    assert torch.equal(l1, l0)
    for a, b in zip(b1, b0):
        assert torch.equal(a, b)


# max |fused - layers| / max |layers| over the block outputs, measured on an MI355X when this test was added: 1.5e-3 for
# ViT-B/16 at N = 2 (LayerNorm / GELU rounding moving a code by one), 0 for the small configuration.  The bound leaves a
# 13x margin; a wiring mutation (q and k swapped) moves the small model's logits by 1.57 on a scale of 2.73, where the two
# routes' logits were identical.
BLOCK_REL_TOL = 2e-2


@pytest.mark.parametrize("arch,N", [("vit_tiny_test", 3), ("vit_b_16", 2), ("vit_s16_shape", 2), ("vit_h14_shape", 2)])
def test_block_fused_vs_layers(models, arch, N):
    m = models[arch]
    x = m.embed(_images(N, arch, 11), "layers", None)
    worst = 0.0
    for b in m.blocks:
        # LayerNorm codes: the kernel's vs torch's LayerNorm through quantize_pack
        codes = capi.layernorm_quantize_pack(x, b.ln1[0], b.ln1[1], m.eps, [b.q.requant()])[0][0]
        y = F.layer_norm(x, (m.E,), b.ln1[0], b.ln1[1], m.eps)
        ref = b.q.quantize(y, channel_dim=1)[0]
        d = (codes.to(torch.int16) - ref.to(torch.int16)).abs()
        assert int(d.max()) <= 1 and float((d > 0).float().mean()) <= 1e-3
        fused = m.block(b, x.clone(), N, "fused")
        layers = m.block(b, x.clone(), N, "layers")
        rel = float((fused - layers).abs().max() / layers.abs().max())
        worst = max(worst, rel)
        assert rel <= BLOCK_REL_TOL, rel
        x = layers
    print("block fused vs layers: worst relative difference %.3g (%s, N=%d)" % (worst, arch, N))


def test_logits_fused_vs_layers_and_wiring(models):
    m = models["vit_tiny_test"]
    x = _images(4, "vit_tiny_test", 3)
    lf = m(x, "fused")
    ll = m(x, "layers")
    gap = float((lf - ll).abs().max())
    # a wiring mutation -- q and k swapped in every block -- moves the logits far more than the routes differ
    for b in m.blocks:
        b.q, b.k = b.k, b.q
    try:
        lm = m(x, "fused")
    finally:
        for b in m.blocks:
            b.q, b.k = b.k, b.q
    mut = float((lm - ll).abs().max())
    print("logits: fused vs layers %.3g, q/k swapped %.3g, scale %.3g" % (gap, mut, float(ll.abs().max())))
    assert gap <= 0.05 * float(ll.abs().max())
    assert mut > 5 * gap


@pytest.mark.parametrize("arch", list(SHAPED))
def test_wiring_on_other_widths(models, arch):
    """The q / k swap of test_logits_fused_vs_layers_and_wiring on the ViT-S/16- and ViT-H/14-shaped models: the swap moves the
    logits far more than the fused and layers routes differ."""
    m = models[arch]
    x = _images(2, arch, 5)
    lf, ll = m(x, "fused"), m(x, "layers")
    gap = float((lf - ll).abs().max())
    for b in m.blocks:
        b.q, b.k = b.k, b.q
    try:
        lm = m(x, "fused")
    finally:
        for b in m.blocks:
            b.q, b.k = b.k, b.q
    mut = float((lm - ll).abs().max())
    print("%s logits: fused vs layers %.3g, q/k swapped %.3g, scale %.3g" % (arch, gap, mut, float(ll.abs().max())))
    assert gap <= 0.05 * float(ll.abs().max())
    assert mut > 5 * gap


def test_check_false_never_syncs(models):
    m = models["vit_b_16"]
    x = _images(2, "vit_b_16", 7)
    m(x, "fused", check=False)              # warm-up: kernel attributes, allocator
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        logits = m(x, "fused", check=False)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.isfinite(logits).all()


def test_nan_image_raises(models):
    m = models["vit_tiny_test"]
    x = _images(2, "vit_tiny_test", 8)
    x[1, 2, 5, 5] = float("nan")
    with pytest.raises(RuntimeError, match="out of range"):
        m(x, "fused")
