"""GPU: the packed ViT-B/16 at a batch it is benchmarked at (64 images, 12,608 token rows), where the planner puts q / k / v,
fc1 and the patch GEMM on the 4-wave 160 x 256 kernel and fc2 on the 8-wave 320 x 256 kernel: the layers' kernels are asserted
(a planner change fails here instead of quietly testing something else), and the fused route with its fused epilogues gives
bit for bit the logits and block outputs of their two-pass forms (QE_LIN_EPI=0)."""
import pytest
import torch

from quantize_amd import capi
from quantize_amd.packed_vit import CONFIGS, PackedViT, calibrated_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 64


@pytest.fixture(scope="module")
def vit_b():
    sd = calibrated_state_dict("vit_b_16", device=DEV, seed=0)
    return PackedViT.from_state_dict(sd, CONFIGS["vit_b_16"]["heads"])


def test_layer_kernels_at_64_images(vit_b):
    m = vit_b
    codes = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)      # stand-in activation codes: only alignment is read
    rows = N * 197
    c = m.conv
    p = m.patch
    patch_x, patch_w = c.xq(codes, linear=True), c.wq(linear=True)
    assert capi.linear_form(patch_x, patch_w, N * 196, 3 * p * p, m.E) == 4
    for b in m.blocks:
        for lin in (b.q, b.k, b.v, b.fc1):
            assert capi.linear_form(lin.xq(codes), lin.wq(), rows, lin.K, lin.O) == 4, lin.name
        assert capi.linear_form(b.fc2.xq(codes), b.fc2.wq(), rows, b.fc2.K, b.fc2.O) == 3, b.fc2.name
    h = m.head_lin
    assert capi.linear_form(h.xq(codes), h.wq(), N, h.K, h.O) == 1


def test_fused_epilogues_equal_two_pass_at_64_images(vit_b):
    g = torch.Generator(device="cpu").manual_seed(64)
    x = torch.randn(N, 3, 224, 224, generator=g).to(DEV)
    with capi.knobs(QE_LIN_EPI=None):
        l1, b1 = vit_b.forward(x, "fused", keep_blocks=True)
    with capi.knobs(QE_LIN_EPI="0"):
        l0, b0 = vit_b.forward(x, "fused", keep_blocks=True)
    assert torch.isfinite(l1).all() and l1.std() > 0
    assert torch.equal(l1, l0)
    assert len(b1) == len(b0) == 12
    for i, (a, b) in enumerate(zip(b1, b0)):
        assert torch.equal(a, b), "block %d" % i
