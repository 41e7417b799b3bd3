"""GPU: qe_maxpool2d_codes (max pooling on 8-bit stored codes) equals F.max_pool2d on the decoded codes, for signed and
unsigned codes, torchvision's 3x3 / 2 pad 1 stem window and others, and ragged planes; sub-8-bit streams are refused."""
import pytest
import torch
import torch.nn.functional as F

from quantize_amd import capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("N,C,H,W,k,s,p", [(2, 64, 112, 112, 3, 2, 1), (3, 5, 13, 11, 3, 2, 1), (2, 4, 9, 9, 2, 2, 0),
                                            (1, 3, 8, 8, 3, 1, 1), (2, 7, 15, 17, 5, 3, 2), (1, 1, 1, 1, 1, 1, 0),
                                            (5, 3, 7, 7, 3, 2, 1)])
@pytest.mark.parametrize("signed", [False, True])
def test_maxpool_codes_matches_torch(N, C, H, W, k, s, p, signed):
    g = torch.Generator(device="cpu").manual_seed(N * 1000 + C * 10 + k)
    codes = torch.randint(0, 256, (N, C, H, W), generator=g, dtype=torch.uint8).to(DEV)
    q = codes.float() - (128.0 if signed else 0.0)                 # the decoded codes
    ref = F.max_pool2d(q, k, s, p) + (128.0 if signed else 0.0)
    out = capi.maxpool2d_codes(codes.view(-1), 8, N, C, H, W, k, s, p)
    torch.cuda.synchronize()
    assert torch.equal(out.view(ref.shape), ref.to(torch.uint8))


def test_maxpool_codes_of_quantised_relu_equals_quantised_maxpool():
    """maxpool(q(relu(y))) == q(maxpool(relu(y))): the stem's order of operations can be swapped exactly."""
    y = torch.randn(2, 64, 112, 112, device=DEV)
    s, z = torch.tensor([0.013], device=DEV), torch.zeros(1, device=DEV)
    a, _ = capi.quantize_pack(torch.relu(y).contiguous(), s, z, 0, 255, 8, False)
    b, _ = capi.quantize_pack(F.max_pool2d(torch.relu(y), 3, 2, 1).contiguous(), s, z, 0, 255, 8, False)
    assert torch.equal(capi.maxpool2d_codes(a, 8, 2, 64, 112, 112, 3, 2, 1), b)


def test_sub_8_bit_codes_refused():
    x = torch.zeros(2 * 4 * 8 * 8 // 2, dtype=torch.uint8, device=DEV)
    with pytest.raises(capi.QeError, match="not supported"):
        capi.maxpool2d_codes(x, 4, 2, 4, 8, 8, 3, 2, 1)


def test_bad_window_refused():
    x = torch.zeros(64, dtype=torch.uint8, device=DEV)
    with pytest.raises(capi.QeError):
        capi.maxpool2d_codes(x, 8, 1, 1, 8, 8, 3, 2, 2)        # padding above half the window (torch refuses it too)
