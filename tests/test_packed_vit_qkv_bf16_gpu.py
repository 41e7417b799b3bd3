"""GPU: PackedViT.forward(route="fused", attention="engine_bf16", qkv="bf16") -- the q / k / v projections written as bf16
rows (qe_quantlinear_bf16, q times d ** -0.5) and read as stored by the attention kernel (qe_attention_bf16_stored, scale 1).

The projections then hold exactly the values the bf16 kernel rounds its fp32 operands to, so logits and every block output
equal those of qkv="fp32" bit for bit: no tolerance.  Two small models: d = 64 (L = 17) and d = 16."""
import pytest
import torch

from quantize_amd import capi
from quantize_amd.packed_vit import PackedViT, calibrated_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODELS = {"d64": dict(width=256, heads=4), "d16": dict(width=128, heads=8)}


@pytest.fixture(scope="module")
def models():
    out = {}
    for name, kw in MODELS.items():
        sd = calibrated_state_dict("vit_b_16", device=DEV, depth=2, mlp=512, image_size=64, patch=16, num_classes=10, **kw)
        out[name] = PackedViT.from_state_dict(sd, kw["heads"])
    return out


def _images(N, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(N, 3, 64, 64, generator=g).to(DEV)


@pytest.mark.parametrize("name", list(MODELS))
def test_qkv_bf16_equals_qkv_fp32_bit_for_bit(models, name):
    m = models[name]
    assert m.E // m.num_heads == int(name[1:])
    x = _images(3, 11)
    kw = dict(route="fused", attention="engine_bf16", keep_blocks=True)
    want, want_blocks = m.forward(x, qkv="fp32", **kw)
    got, got_blocks = m.forward(x, qkv="bf16", **kw)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (3, 10) and torch.isfinite(got).all()
    assert len(got_blocks) == len(want_blocks) == 2 and tuple(got_blocks[0].shape) == (3, 17, m.E)
    for i, (a, b) in enumerate(zip(got_blocks, want_blocks)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "block %d: %d elements differ" % (i, int((a != b).sum()))
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.equal(m(x, attention="engine_bf16", qkv="bf16"), got)          # __call__ passes the option through
    assert torch.equal(m.forward(x, attention="engine_bf16")[0], want)          # the default is qkv="fp32"
    assert not torch.equal(m.forward(x, attention="engine")[0], want), "engine_bf16 returned the fp32 core's bits"


def test_qkv_projection_takes_the_fused_epilogue(models):
    m = models["d64"]
    b = m.blocks[0]
    rows = 3 * 17
    x = torch.zeros(rows * b.q.K, dtype=torch.uint8, device=DEV)
    for lin in (b.q, b.k, b.v):
        assert (lin.K, lin.O) == (256, 256)
        assert capi.quantlinear_bf16_path(lin.xq(x), lin.wq(), rows, lin.K, lin.O) == 1


def test_qkv_bf16_needs_the_fused_route_and_the_bf16_core(models):
    m = models["d64"]
    x = _images(1, 3)
    for kw in (dict(route="fused", attention="torch"), dict(route="fused", attention="engine"),
               dict(route="layers", attention="engine_bf16")):
        with pytest.raises(ValueError, match="qkv='bf16' needs"):
            m.forward(x, qkv="bf16", **kw)
    torch.cuda.synchronize()


def test_qkv_bf16_check_false_never_syncs(models):
    m = models["d64"]
    x = _images(2, 7)
    m(x, "fused", check=False, attention="engine_bf16", qkv="bf16")     # warm-up: kernel attributes, allocator
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        logits = m(x, "fused", check=False, attention="engine_bf16", qkv="bf16")
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.isfinite(logits).all()
