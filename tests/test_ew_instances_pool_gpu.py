"""GPU: patchify_quant_kernel (qe_quantize_patchify), maxpool2d_codes_kernel and global_avgpool_kernel at their edges against
tests/ew_ref.py.  The codes of quantize_patchify are ew_ref.quantise's fp32 sequence of the patch matrix bit for bit, on
tie-dense pixels; the pooled codes are the window maxima of the decoded codes; the average is within the fp32 summation
bound of the float64 mean.  Every output sits between guard bands (ew_instances.Guarded).  Cases: tests/ew_instances.py."""
import numpy as np
import pytest
import torch

import ew_instances as ei
import ew_ref
from quantize_amd import capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- quantize_patchify ---------------------------------------------------------------------------------------------------
def _patchify(x, off, p, scale, zero, bits, sign, what):
    qmin, qmax = ew_ref.qrange(bits, sign)
    g = ei.Guarded(capi.packed_nbytes(x.size, bits))
    xd = ei.device_input(x.reshape(-1), "float32", off).view(x.shape)
    _, st = capi.quantize_patchify(xd, p, _t(scale), _t(zero), qmin, qmax, bits, sign, out=g.out)
    return g.result(what), int(st.item())


@pytest.mark.parametrize("bits,sign", ei.PATCHIFY_BITS)
def test_quantize_patchify(bits, sign):
    qmin, qmax = ew_ref.qrange(bits, sign)
    for i, (N, C, H, W, p, off, note) in enumerate(ei.PATCHIFY_CASES):
        for per_ch in (False, True):
            scale, zero = ei.channel_params(C) if per_ch and C > 1 else ei.tensor_params(i)
            n = N * C * H * W
            # quantising is per element, so the reference quantises in NCHW order (channel = (i // (H W)) % C) and moves the
            # integer-valued result into patch-matrix order
            x = ew_ref.tie_dense(np.random.RandomState(i), n, scale, zero, qmin, qmax, H * W)
            what = "quantize_patchify %s (%s) b%d sign %d per-channel %d" % ((N, C, H, W, p), note, bits, sign, per_ch)
            for nan_at in (None, 0, n - 1):
                xx = x.copy()
                if nan_at is not None:
                    if (i + per_ch) % 3 != 0:
                        continue                                # the NaN runs on a third of the cases
                    xx[nan_at] = np.nan
                q = ew_ref.patch_matrix(ew_ref.quantise(xx, scale, zero, qmin, qmax, H * W).reshape(N, C, H, W), p).reshape(-1)
                got, flag = _patchify(xx.reshape(N, C, H, W), off, p, scale, zero, bits, sign, what)
                assert flag == (0 if nan_at is None else 1), what
                ok = ~np.isnan(q)
                assert ok.sum() == n - (nan_at is not None)
                want = ew_ref.stored(q, bits, sign)
                assert np.array_equal(ew_ref.unpack_codes(got, n, bits)[ok], want[ok]), what
                if nan_at is None:
                    assert np.array_equal(got, ew_ref.pack(want, bits)), what      # and the padding of the last byte


# ---- maxpool2d_codes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ei.MAXPOOL_CASES, ids=[c[-1] for c in ei.MAXPOOL_CASES])
def test_maxpool2d_codes(case):
    N, C, H, W, k, s, p, note = case
    rng = np.random.RandomState(H * W + k)
    codes = rng.randint(0, 256, size=(N, C, H, W)).astype(np.uint8)
    codes[0, 0].flat[0], codes[-1, -1].flat[-1] = 255, 0
    codes[N // 2, C // 2] = 0                                   # a plane whose maxima are the lowest code
    OH, OW = ei.maxpool_out_hw(H, W, k, s, p)
    xd = _t(codes)
    for sign in (False, True):
        want = ew_ref.maxpool_codes(codes, sign, k, s, p).reshape(-1)
        for off in ei.MAXPOOL_OUT_OFFSETS:
            g = ei.Guarded(N * C * OH * OW, off)
            capi.maxpool2d_codes(xd, 8, N, C, H, W, k, s, p, out=g.out)
            what = "maxpool2d_codes %s, signed %d, out + %d bytes" % (case, sign, off)
            assert np.array_equal(g.result(what), want), what


# ---- global_avgpool ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", ei.AVGPOOL_P)
def test_global_avgpool(P):
    """|y - mean64| <= (P + 1) * 2^-24 * mean|x| per plane: fp32 summation of P terms in any order is within
    (P - 1) u sum|x| of the exact sum (u = 2^-24), the division by P adds one rounding, and one more u of slack covers the
    second-order terms."""
    rng = np.random.RandomState(P)
    for planes in ei.AVGPOOL_PLANES:
        for mean in (0.0, 1e3):
            x = (rng.normal(0, 1, size=(1, planes, P, 1)) + mean).astype(np.float32)
            ref = ew_ref.avgpool64(x).reshape(-1)
            bound = (P + 1) * 2.0 ** -24 * np.abs(x.astype(np.float64)).mean(axis=(2, 3)).reshape(-1)
            for off in ei.AVGPOOL_OFFSETS:
                xd = ei.device_input(x.reshape(-1), "float32", off).view(x.shape)
                g = ei.Guarded(4 * planes)
                capi.global_avgpool(xd, out=g.view(torch.float32))
                what = "global_avgpool P %d, %d planes, mean %g, x + %d floats" % (P, planes, mean, off)
                y = g.result(what).view(np.float32)
                err = np.abs(y.astype(np.float64) - ref)
                assert (err <= bound).all(), "%s: error %.3g of bound %.3g" % (what, err.max(), bound[err.argmax()])


def test_global_avgpool_refuses_planes_past_its_lds():
    P = ei.AVGPOOL_P_REFUSED
    x = torch.zeros((1, 3, P, 1), device=DEV)
    g = ei.Guarded(12)
    with pytest.raises(capi.QeError, match="not supported"):
        capi.global_avgpool(x, out=g.view(torch.float32))
    g.result("refused global_avgpool")
