"""GPU: PackedViT.forward(route="fused", attention="engine_bf16", qkv="bf16", ctx="bf16") -- the attention context written
as bf16 rows (qe_attention_bf16_ctx) and read as stored by out_proj (qe_quantlinear_bf16_input, residual add in its epilogue).

The context is rounded once, so the result is not that of ctx="fp32"; what is exact is the composition: a block equals,
bit for bit, the fp32-out attention on the block's own bf16 projections, .to(torch.bfloat16), then quantlinear_bf16_input
with the residual -- public ops only.  Whole-forward logits are finite and of the right shape; their deviation and top-1
agreement against ctx="fp32" are printed, not gated (a flipped int8 code downstream moves logits by more than any core
does).  The two small models of tests/test_packed_vit_qkv_bf16_gpu.py: d = 64 (L = 17) and d = 16."""
import pytest
import torch

from quantize_amd import capi
from quantize_amd.packed_vit import PackedViT, calibrated_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODELS = {"d64": dict(width=256, heads=4), "d16": dict(width=128, heads=8)}
BF16 = dict(route="fused", attention="engine_bf16", qkv="bf16")


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


def _block_by_hand(m, b, x, N):
    """The fused block with ctx="bf16", from public ops: the block's own bf16 projections, the fp32-out stored attention,
    one rounding, out_proj on the bf16 rows with the residual; then the MLP half as block() runs it."""
    E, H = m.E, m.num_heads
    rows = x.shape[0]
    L = rows // N
    status = torch.zeros(1, dtype=torch.int32, device=x.device)
    codes = capi.layernorm_quantize_pack(x, b.ln1[0], b.ln1[1], m.eps, [b.q.requant(), b.k.requant(), b.v.requant()], status=status)[0]
    post = ((E // H) ** -0.5, 1.0, 1.0)
    Q, K, V = (capi.quantlinear_bf16(lin.xq(c), lin.wq(), lin.bias, rows, lin.K, lin.O, post_scale=s)
               for lin, c, s in zip((b.q, b.k, b.v), codes, post))
    ctx = capi.attention(Q, K, V, N, L, H, scale=1.0, precision="bf16").to(torch.bfloat16)
    x = capi.quantlinear_bf16_input(ctx, b.attn.out_wq(), b.attn.out_bias, E, residual=x)
    c1 = capi.layernorm_quantize_pack(x, b.ln2[0], b.ln2[1], m.eps, [b.fc1.requant()], status=status)[0][0]
    c2 = capi.quantlinear_requant(b.fc1.xq(c1), b.fc1.wq(), b.fc1.bias, rows, b.fc1.K, b.fc1.O, b.fc2.requant(), act="gelu",
                                  status=status)[0]
    return capi.quantlinear_residual(b.fc2.xq(c2), b.fc2.wq(), b.fc2.bias, rows, b.fc2.K, b.fc2.O, x)


@pytest.mark.parametrize("name", list(MODELS))
def test_block_equals_the_hand_composition_bit_for_bit(models, name):
    m = models[name]
    assert m.E // m.num_heads == int(name[1:])
    N = 3
    x0 = m.embed(_images(N, 11), "fused", torch.zeros(1, dtype=torch.int32, device=DEV))
    x = x0
    for i, b in enumerate(m.blocks):
        want = _block_by_hand(m, b, x.clone(), N)
        got = m.block(b, x.clone(), N, "fused", attention="engine_bf16", qkv="bf16", ctx="bf16")
        plain = m.block(b, x.clone(), N, "fused", attention="engine_bf16", qkv="bf16")
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), "block %d: %d elements differ" % (i, int((got != want).sum()))
        assert not torch.equal(got, plain), "block %d: ctx='bf16' returned the fp32 context's bits" % i
        x = got


@pytest.mark.parametrize("name", list(MODELS))
def test_whole_forward(models, name):
    m = models[name]
    x = _images(8, 21)
    want, want_blocks = m.forward(x, keep_blocks=True, **BF16)
    got, got_blocks = m.forward(x, keep_blocks=True, ctx="bf16", **BF16)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (8, 10) and torch.isfinite(got).all()
    assert len(got_blocks) == 2 and tuple(got_blocks[0].shape) == (8, 17, m.E)
    rel = float((got - want).norm() / want.norm())
    top1 = float((got.argmax(-1) == want.argmax(-1)).float().mean())
    print("%s: logits relative deviation ctx bf16 vs fp32 %.3g, top-1 agreement %.3f" % (name, rel, top1))
    assert torch.equal(m(x, ctx="bf16", **BF16), got)                                  # __call__ passes the option through
    assert torch.equal(m.forward(x, ctx="fp32", **BF16)[0].view(torch.int32), want.view(torch.int32))   # the default is ctx="fp32"
    assert torch.equal(m(x, **BF16).view(torch.int32), want.view(torch.int32))
    assert not torch.equal(got_blocks[0], want_blocks[0])


def test_out_proj_takes_the_bf16_input_kernel(models):
    m = models["d64"]
    rows = 3 * 17
    ctx = torch.zeros(rows, m.E, dtype=torch.bfloat16, device=DEV)
    assert m.E == 256
    assert capi.quantlinear_bf16_input_path(ctx, m.blocks[0].attn.out_wq(), rows, m.E, m.E) == 1


def test_ctx_bf16_needs_its_prerequisites(models):
    m = models["d64"]
    x = _images(1, 3)
    for kw in (dict(route="fused", attention="engine_bf16", qkv="fp32"), dict(route="fused", attention="engine", qkv="fp32"),
               dict(route="layers", attention="engine_bf16", qkv="fp32")):
        with pytest.raises(ValueError, match="ctx='bf16' needs"):
            m.forward(x, ctx="bf16", **kw)
    torch.cuda.synchronize()


def test_ctx_bf16_check_false_never_syncs(models):
    m = models["d64"]
    x = _images(2, 7)
    m(x, "fused", check=False, attention="engine_bf16", qkv="bf16", ctx="bf16")     # warm-up: kernel attributes, allocator
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        logits = m(x, "fused", check=False, attention="engine_bf16", qkv="bf16", ctx="bf16")
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.isfinite(logits).all()
