"""GPU: the fused ViT forms of the C ABI hold their contracts bit for bit.

  * qe_quantlinear_requant == qe_quantize_pack_act(qe_quantlinear(...), act), on every int8 MFMA form (QE_LIN8 = 0 / 1 / 2,
    QE_LIN_NJ = 2 / 4) and on the two-pass form (QE_LIN_EPI=0, 4-bit or per-channel consumers), each case asserting its path;
  * qe_quantlinear_residual / qe_quantlinear_float_input_residual == the linear + residual (one fp32 add), in place too;
  * qe_quantize_pack_act's GELU is as close to float64 as torch's F.gelu (1 ulp slack);
  * qe_layernorm_quantize_pack: fp32 error at most 2x torch F.layer_norm's, codes == qe_quantize_pack of its own output;
  * qe_quantize_patchify == qe_quantize_pack of the unfolded images, and the patch GEMM computes conv_proj."""
import contextlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from quantize_amd import capi
from quantize_amd.packed import PackedConv2d
from quantize_amd.packed_resnet import pack_codes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@contextlib.contextmanager
def knobs(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        capi.reload_env()
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        capi.reload_env()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _operands(rng, B, K, O, x_sign=True, per_row=True, asym=True):
    """8-bit packed activations (per-row scale, asymmetric, signed or not) and weights (per-column scale, zero)."""
    qx = rng.randint(-128, 128, size=(B, K)) if x_sign else rng.randint(0, 256, size=(B, K))
    qw = rng.randint(-128, 128, size=(O, K))
    xs = _t(rng.uniform(1e-3, 3e-3, size=B if per_row else 1).astype(np.float32))
    xz = _t((rng.uniform(-3, 3, size=B if per_row else 1) if asym else np.zeros(B if per_row else 1)).astype(np.float32))
    ws = _t(rng.uniform(2e-3, 6e-3, size=O).astype(np.float32))
    wz = _t((rng.uniform(-2, 2, size=O) if asym else np.zeros(O)).astype(np.float32))
    bias = _t(rng.normal(0, 0.2, size=O).astype(np.float32))
    xp, wp = _t(pack_codes(qx, 8, x_sign)), _t(pack_codes(qw, 8, True))
    return capi.qparam(xp, 8, x_sign, xs, xz), capi.qparam(wp, 8, True, ws, wz), bias


def _rq(scale, zero, bits=8, signed=True, per=1):
    qmin, qmax = (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if signed else (0, (1 << bits) - 1)
    return capi.requant(_t(np.full(per, scale, np.float32)), _t(np.full(per, zero, np.float32)), qmin, qmax, bits, signed)


def _requant_case(B, K, O, act, rq, seed, x_sign=True, per_row=True, asym=True, expect_path=1):
    rng = np.random.RandomState(seed)
    xq, wq, bias = _operands(rng, B, K, O, x_sign, per_row, asym)
    assert capi.linear_requant_path(xq, wq, B, K, O, rq) == expect_path
    codes, st = capi.quantlinear_requant(xq, wq, bias, B, K, O, rq, act=act)
    y = capi.quantlinear(xq, wq, bias, B, K, O)
    ref, _, st_ref = capi.quantize_pack_act(y, rq._keep[0], rq._keep[1], rq.qmin, rq.qmax, rq.n_bits, rq.sign, act=act, inner=1)
    torch.cuda.synchronize()
    assert torch.equal(codes, ref)
    assert int(st.item()) == int(st_ref.item())
    return codes


# (QE_LIN8, QE_LIN_NJ, B, K, O): the 64-deep kernel at both widths, both 128-deep forms, ragged last row tiles everywhere
FORMS = [(0, 2, 333, 256, 320), (0, 4, 333, 256, 320), (0, 4, 130, 192, 96), (1, None, 700, 256, 512), (2, None, 370, 256, 512)]


@pytest.mark.parametrize("lin8,nj,B,K,O", FORMS)
@pytest.mark.parametrize("act", [None, "gelu"])
def test_requant_every_form(lin8, nj, B, K, O, act):
    with knobs(QE_LIN8=lin8, QE_LIN_NJ=nj):
        codes = _requant_case(B, K, O, act, _rq(0.004, 3.0, 8, False) if act == "gelu" else _rq(0.01, -1.0), seed=B + O)
        _requant_case(B, K, O, act, _rq(0.04, 0.0), seed=B + O + 1, x_sign=False, per_row=False, asym=False)
    # the clamp is exercised at both ends: stored codes 0 and 255 (qmin and qmax of either quantiser) both occur
    assert int((codes == 0).sum()) > 0 and int((codes == 255).sum()) > 0


@pytest.mark.parametrize("act", [None, "gelu"])
def test_requant_two_pass_forms(act):
    with knobs(QE_LIN_EPI=0):
        _requant_case(333, 256, 320, act, _rq(0.05, 1.0), seed=5, expect_path=0)
    _requant_case(333, 256, 320, act, _rq(0.3, 0.0, 4, True), seed=6, expect_path=0)            # 4-bit consumer
    _requant_case(333, 256, 320, act, _rq(0.05, 2.0, 8, True, per=320), seed=7, expect_path=0)  # per-feature consumer
    _requant_case(64, 100, 40, act, _rq(0.05, 0.0), seed=8, expect_path=0)                      # K % 64 != 0: fp32 kernel


def test_requant_nan_sets_status():
    rng = np.random.RandomState(9)
    for lin8, nj, B, K, O in FORMS:
        with knobs(QE_LIN8=lin8, QE_LIN_NJ=nj):
            xq, wq, bias = _operands(rng, B, K, O)
            bias[O // 3] = float("nan")
            rq = _rq(0.05, 0.0)
            assert capi.linear_requant_path(xq, wq, B, K, O, rq) == 1
            _, st = capi.quantlinear_requant(xq, wq, bias, B, K, O, rq, act="gelu")
            assert int(st.item()) == 1
            bias[O // 3] = 0.0
            _, st = capi.quantlinear_requant(xq, wq, bias, B, K, O, _rq(10.0, 0.0))
            assert int(st.item()) == 0


@pytest.mark.parametrize("lin8,nj,B,K,O", FORMS)
def test_residual_every_form(lin8, nj, B, K, O):
    rng = np.random.RandomState(B * 7 + O)
    with knobs(QE_LIN8=lin8, QE_LIN_NJ=nj):
        xq, wq, bias = _operands(rng, B, K, O)
        assert capi.linear_residual_path(xq, wq, B, K, O) == 1
        res = _t(rng.normal(0, 1, size=(B, O)).astype(np.float32))
        ref = capi.quantlinear(xq, wq, bias, B, K, O) + res
        out = capi.quantlinear_residual(xq, wq, bias, B, K, O, res)
        assert torch.equal(out, ref)
        inplace = res.clone()
        capi.quantlinear_residual(xq, wq, bias, B, K, O, inplace, out=inplace)
        assert torch.equal(inplace, ref)
    with knobs(QE_LIN_EPI=0):
        assert capi.linear_residual_path(xq, wq, B, K, O) == 0
        inplace = res.clone()
        capi.quantlinear_residual(xq, wq, bias, B, K, O, inplace, out=inplace)
        assert torch.equal(inplace, ref)


@pytest.mark.parametrize("B,K,O", [(333, 256, 320), (197, 768, 768), (50, 96, 72)])
def test_float_input_residual(B, K, O):
    rng = np.random.RandomState(B + K)
    qw = rng.randint(-128, 128, size=(O, K))
    wq = capi.qparam(_t(pack_codes(qw, 8, True)), 8, True, _t(rng.uniform(2e-3, 6e-3, size=O).astype(np.float32)),
                     _t(rng.uniform(-1, 1, size=O).astype(np.float32)))
    bias = _t(rng.normal(0, 0.2, size=O).astype(np.float32))
    x = _t(rng.normal(0, 1, size=(B, K)).astype(np.float32))
    res = _t(rng.normal(0, 1, size=(B, O)).astype(np.float32))
    ref = capi.quantlinear_float_input(x, wq, bias, O) + res
    assert capi.linear_float_input_residual_path(x, wq, B, K, O) == 1
    out = capi.quantlinear_float_input_residual(x, wq, bias, O, res)
    inplace = res.clone()
    capi.quantlinear_float_input_residual(x, wq, bias, O, inplace, out=inplace)
    with knobs(QE_LIN_EPI=0):
        assert capi.linear_float_input_residual_path(x, wq, B, K, O) == 0
        two = capi.quantlinear_float_input_residual(x, wq, bias, O, res)
    assert torch.equal(out, ref) and torch.equal(inplace, ref) and torch.equal(two, ref)


def test_gelu_accuracy():
    g = torch.Generator(device="cpu").manual_seed(3)
    x = torch.cat([torch.randn(1 << 19, generator=g) * 4,
                   torch.empty(1 << 19).uniform_(-12, 12, generator=g),
                   torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan"), 3.4028235e38, -3.4028235e38,
                                 1.17549435e-38, -1.17549435e-38, 1e-45, -1e-45, 5.0, -5.0, 10.0, -10.0, 0.5])]).to(DEV)
    one = torch.ones(1, device=DEV)
    codes, y, _ = capi.quantize_pack_act(x, one, one * 0, -128, 127, 8, True, act="gelu", y="new")
    tg = F.gelu(x)
    x64 = x.double()
    ref = x64 * 0.5 * (1.0 + torch.special.erf(x64 / np.sqrt(2.0)))
    fin = torch.isfinite(ref)
    ulp = (torch.nextafter(ref.float().abs(), torch.tensor(float("inf"), device=DEV)) - ref.float().abs()).double()
    ulp = torch.where(ulp > 0, ulp, torch.full_like(ulp, 1e-45))
    e_k = (y.double() - ref).abs()[fin]
    e_t = (tg.double() - ref).abs()[fin]
    assert (e_k <= e_t + ulp[fin]).all(), float(((e_k - e_t) / ulp[fin]).max())
    assert torch.equal(torch.isnan(y), torch.isnan(tg))
    assert torch.equal(y[x == float("inf")], tg[x == float("inf")])
    # the codes are quantize_pack's of that fp32 value (status: the NaN trips it)
    ref_codes, st = capi.quantize_pack(torch.nan_to_num(y), one, one * 0, -128, 127, 8, True)
    ok = ~torch.isnan(y)
    assert torch.equal(codes[ok], ref_codes[ok]) and int(st.item()) == 0


@pytest.mark.parametrize("E", [64, 768, 1024])
def test_layernorm_quantize_pack(E):
    g = torch.Generator(device="cpu").manual_seed(E)
    rows = 777
    x = (torch.randn(rows, E, generator=g) * 3 + torch.randn(rows, 1, generator=g) * 20).to(DEV)
    gamma = (1 + 0.2 * torch.randn(E, generator=g)).to(DEV)
    beta = (0.1 * torch.randn(E, generator=g)).to(DEV)
    rqs_all = [_rq(0.03, 0.0, 8, True), _rq(0.05, -100.0, 8, False), _rq(0.4, 1.0, 4, True)]
    x64 = x.double()
    m = x64.mean(-1, keepdim=True)
    ref = (x64 - m) / torch.sqrt(((x64 - m) ** 2).mean(-1, keepdim=True) + 1e-6) * gamma.double() + beta.double()
    e_t = (F.layer_norm(x, (E,), gamma, beta, 1e-6).double() - ref).abs().max()
    for n_out in (1, 2, 3):
        rqs = rqs_all[:n_out] if n_out < 3 else [rqs_all[0], rqs_all[1], _rq(0.02, 0.0)]
        codes, ln, st = capi.layernorm_quantize_pack(x, gamma, beta, 1e-6, rqs, ln_out="new")
        assert capi.layernorm_path(rows, E, rqs, codes) == 1
        e_k = (ln.double() - ref).abs().max()
        assert e_k <= 2 * e_t, (float(e_k), float(e_t))
        for c, r in zip(codes, rqs):
            want, _ = capi.quantize_pack(ln, r._keep[0], r._keep[1], r.qmin, r.qmax, r.n_bits, r.sign)
            assert torch.equal(c, want)
        codes_only, none, _ = capi.layernorm_quantize_pack(x, gamma, beta, 1e-6, rqs)
        assert none is None and all(torch.equal(a, b) for a, b in zip(codes, codes_only))
    # sub-8-bit consumer: the two-pass form, same contract
    codes, ln, _ = capi.layernorm_quantize_pack(x, gamma, beta, 1e-6, rqs_all, ln_out="new")
    assert capi.layernorm_path(rows, E, rqs_all, codes) == 0
    for c, r in zip(codes, rqs_all):
        assert torch.equal(c, capi.quantize_pack(ln, r._keep[0], r._keep[1], r.qmin, r.qmax, r.n_bits, r.sign)[0])
    codes_ws, _, _ = capi.layernorm_quantize_pack(x, gamma, beta, 1e-6, rqs_all)
    assert all(torch.equal(a, b) for a, b in zip(codes, codes_ws))


def test_layernorm_rejects_shapes():
    x = torch.zeros(4, 66, device=DEV)
    with pytest.raises(capi.QeError):
        capi.layernorm_quantize_pack(x, None, None, 1e-6, [_rq(0.1, 0.0)])


def _unfold(x, p):
    N, C, H, W = x.shape
    return x.reshape(N, C, H // p, p, W // p, p).permute(0, 2, 4, 1, 3, 5).reshape(N * (H // p) * (W // p), C * p * p).contiguous()


@pytest.mark.parametrize("N,C,H,W,p", [(2, 3, 224, 224, 16), (3, 3, 32, 32, 8), (1, 5, 12, 18, 6)])
def test_patchify(N, C, H, W, p):
    g = torch.Generator(device="cpu").manual_seed(N * 100 + p)
    x = torch.randn(N, C, H, W, generator=g).to(DEV)
    u = _unfold(x, p)
    for bits, signed, per in ((8, True, 1), (8, False, C), (4, True, 1), (3, False, C)):
        s = torch.linspace(0.01, 0.03, per, device=DEV)
        z = torch.linspace(-2, 1, per, device=DEV) if not signed else torch.zeros(per, device=DEV)
        qmin, qmax = (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if signed else (0, (1 << bits) - 1)
        codes, st = capi.quantize_patchify(x, p, s, z, qmin, qmax, bits, signed)
        if per == 1:
            want, st2 = capi.quantize_pack(u, s, z, qmin, qmax, bits, signed)
        else:   # channel of column k = k // (p p): quantize_pack's (i / inner) % C with inner = p p over the rows
            want, st2 = capi.quantize_pack(u, s, z, qmin, qmax, bits, signed, inner=p * p)
        assert torch.equal(codes, want) and int(st.item()) == int(st2.item())
    nan = x.clone()
    nan[0, 0, 0, 0] = float("nan")
    assert int(capi.quantize_patchify(nan, p, s[:1], z[:1], qmin, qmax, bits, signed)[1].item()) == 1


def test_patch_gemm_is_conv_proj():
    rng = np.random.RandomState(4)
    E, C, p, N = 96, 3, 8, 2           # 8 x 8: the direct convolution has no kernel for 16 x 16 (768 taps)
    qw = rng.randint(-127, 128, size=(E, C, p, p))
    sd = {"weight": _t(pack_codes(qw, 8, True)), "w_des": torch.tensor([8, 1, E, C, p, p], dtype=torch.int32, device=DEV),
          "w_scale": _t(rng.uniform(1e-3, 3e-3, size=(E, 1, 1, 1)).astype(np.float32)),
          "w_zero": _t(np.zeros((E, 1, 1, 1), np.float32)), "bias": _t(rng.normal(0, 0.1, size=E).astype(np.float32)),
          "a_quantizer.scale": _t(np.array([0.02], np.float32)), "a_quantizer.zero": _t(np.array([0.5], np.float32)),
          "a_quantizer.qmin": torch.tensor(-128.0), "a_quantizer.qmax": torch.tensor(127.0)}
    conv = PackedConv2d.from_state_dict(sd, "", stride=p, padding=0)
    x = torch.randn(N, C, 64, 64, generator=torch.Generator().manual_seed(5)).to(DEV)
    ref = conv(x, route="packed").flatten(2).transpose(1, 2).reshape(-1, E)
    codes, _ = capi.quantize_patchify(x, p, conv.a_scale, conv.a_zero, -128, 127, 8, True)
    xq = capi.qparam(codes, 8, True, conv.a_scale, conv.a_zero)
    wq = capi.qparam(conv.weight, 8, True, conv.w_scale.reshape(-1), conv.w_zero.reshape(-1))
    assert capi.linear_path(xq, wq, ref.shape[0], C * p * p, E) == 1
    y = capi.quantlinear(xq, wq, conv.bias, ref.shape[0], C * p * p, E)
    # the GEMM's int32 sum is exact; PackedConv2d's 16x16 kernel runs on the fp32 direct convolution (a 768-term fp32 chain)
    tol = 1e-4 * (1.0 + ref.abs().max())
    assert (y - ref).abs().max() <= tol
