"""GPU: the reference anchor of the packed ViT, and the remaining public forms of the packed linear.

  * Both routes of PackedViT, on pack_vit_state_dict of G9's calibrated state_dict (the reference's own tiny ViT), follow
    the reference's simulated forward: block outputs and logits within a measured tolerance, far below what a wiring
    mutation (q and k swapped, a residual dropped) produces.
  * PackedLinear.call_packed: fp32 out, + residual, and the consumer's codes of y / gelu(y), each bit-identical to the
    unfused form.
  * The ragged MFMA epilogue branches: O % 16 != 0 (codes stored byte by byte), and a residual that is an offset view
    (not 16-byte aligned: the per-element residual branch)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from quantize_amd import capi
from quantize_amd.packed import PackedLinear
from quantize_amd.synthetic import pack_codes
from quantize_amd.packed_vit import PackedViT, pack_vit_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G9 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g9_vit_module.npz")

# max |engine - reference simulation| of the logits (scale 1.63), measured on an MI355X when this test was added: 1.2e-7 for
# both routes (the simulation dequantises and calls F.linear / F.conv2d: fp32 summation order is all that differs, and no
# LayerNorm / GELU rounding moved a code).  Wiring mutations measured at the same time: q and k swapped 0.75, the first
# block's residual dropped 0.73.  The bound sits ~800x above the measured gap and ~7000x below the mutations.
G9_LOGIT_TOL = 1e-4


@pytest.fixture(scope="module")
def g9():
    z = np.load(G9, allow_pickle=False)
    sd = pack_vit_state_dict({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd_")})
    m = PackedViT.from_state_dict({k: v.to(DEV) for k, v in sd.items()}, int(z["config"][3]))
    return z, m


def test_g9_logits(g9):
    z, m = g9
    x = torch.from_numpy(z["images"]).to(DEV)
    want = torch.from_numpy(z["logits"]).to(DEV)
    gaps = {}
    for route in ("fused", "layers"):
        logits, blocks = m.forward(x, route, keep_blocks=True)
        gaps[route] = float((logits - want).abs().max())
        for i, b in enumerate(blocks):
            ref = torch.from_numpy(z["block_%d" % i]).to(DEV)
            assert float((b - ref).abs().max()) <= G9_LOGIT_TOL * float(ref.abs().max()), (route, i)
        assert gaps[route] <= G9_LOGIT_TOL, (route, gaps[route])
    # wiring mutations: q and k swapped in every block; the first block's MLP residual dropped
    for b in m.blocks:
        b.q, b.k = b.k, b.q
    try:
        swapped = float((m(x, "fused") - want).abs().max())
    finally:
        for b in m.blocks:
            b.q, b.k = b.k, b.q
    blk = m.blocks[0]
    orig = m.block

    def no_res(b, xx, N, route, status=None):
        y = orig(b, xx.clone(), N, route, status)
        return y - xx if b is blk else y

    m.block = no_res
    try:
        dropped = float((m(x, "layers") - want).abs().max())
    finally:
        m.block = orig
    print("G9 logits: fused %.3g, layers %.3g, q/k swapped %.3g, residual dropped %.3g, scale %.3g" % (
        gaps["fused"], gaps["layers"], swapped, dropped, float(want.abs().max())))
    assert swapped > 10 * G9_LOGIT_TOL and dropped > 10 * G9_LOGIT_TOL


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _packed_linear(rng, O, K, a_signed=True, scale=0.02):
    qw = rng.randint(-127, 128, size=(O, K))
    qmin, qmax = (-128, 127) if a_signed else (0, 255)
    return PackedLinear(weight=_t(pack_codes(qw, 8, True)), w_des=torch.tensor([8, 1, O, K], dtype=torch.int32, device=DEV),
                        w_scale=_t(rng.uniform(1e-3, 3e-3, size=(O, 1)).astype(np.float32)),
                        w_zero=_t(rng.uniform(-1, 1, size=(O, 1)).astype(np.float32)),
                        bias=_t(rng.normal(0, 0.1, size=O).astype(np.float32)),
                        a_scale=_t(np.array([scale], np.float32)), a_zero=_t(np.array([0.0 if a_signed else -20.0], np.float32)),
                        a_qmin=qmin, a_qmax=qmax, a_bits=8, a_signed=a_signed)


@pytest.mark.parametrize("B,K,O", [(333, 256, 320), (197, 128, 200), (64, 256, 1000)])
def test_call_packed(B, K, O):
    rng = np.random.RandomState(B + O)
    lin = _packed_linear(rng, O, K)
    consumer = _packed_linear(rng, 16, O, a_signed=False, scale=0.01)
    x = _t(rng.normal(0, 1, size=(B, K)).astype(np.float32))
    xq, x_des = lin.quantize(x, channel_dim=1)
    y = lin.call_packed(xq, x_des)
    assert torch.equal(y, lin(x, route="packed"))
    res = _t(rng.normal(0, 1, size=(B, O)).astype(np.float32))
    assert torch.equal(lin.call_packed(xq, x_des, residual=res), y + res)
    for act in (None, "gelu"):
        codes, des = lin.call_packed(xq, x_des, consumer=consumer, act=act)
        want, want_des = consumer.quantize(F.gelu(y) if act else y, channel_dim=1)
        assert torch.equal(codes, want) and des.tolist() == want_des.tolist()


@pytest.mark.parametrize("lin8,nj", [(0, 2), (0, 4)])
def test_ragged_epilogue_branches(lin8, nj):
    with capi.knobs(QE_LIN8=lin8, QE_LIN_NJ=nj):
        rng = np.random.RandomState(nj)
        for B, K, O in ((257, 128, 200), (100, 64, 1000)):
            qx, qw = rng.randint(-128, 128, size=(B, K)), rng.randint(-128, 128, size=(O, K))
            xq = capi.qparam(_t(pack_codes(qx, 8, True)), 8, True, _t(rng.uniform(1e-3, 3e-3, size=B).astype(np.float32)),
                             _t(rng.uniform(-2, 2, size=B).astype(np.float32)))
            wq = capi.qparam(_t(pack_codes(qw, 8, True)), 8, True, _t(rng.uniform(2e-3, 6e-3, size=O).astype(np.float32)),
                             _t(rng.uniform(-2, 2, size=O).astype(np.float32)))
            bias = _t(rng.normal(0, 0.2, size=O).astype(np.float32))
            y = capi.quantlinear(xq, wq, bias, B, K, O)
            for act in (None, "gelu"):
                rq = capi.requant(_t(np.array([0.01], np.float32)), _t(np.array([-3.0], np.float32)), -128, 127, 8, True)
                assert capi.linear_requant_path(xq, wq, B, K, O, rq) == 1
                codes, st = capi.quantlinear_requant(xq, wq, bias, B, K, O, rq, act=act)
                want, _, _ = capi.quantize_pack_act(y, rq._keep[0], rq._keep[1], -128, 127, 8, True, act=act)
                assert torch.equal(codes, want)
            # residual and out as offset views: 4-byte but not 16-byte aligned
            base = _t(rng.normal(0, 1, size=B * O + 1).astype(np.float32))
            res = base[1:].view(B, O)
            assert res.data_ptr() % 16 != 0
            ref = y + res
            assert capi.linear_residual_path(xq, wq, B, K, O) == 1
            assert torch.equal(capi.quantlinear_residual(xq, wq, bias, B, K, O, res), ref)
            capi.quantlinear_residual(xq, wq, bias, B, K, O, res, out=res)        # in place, unaligned
            assert torch.equal(res, ref)
