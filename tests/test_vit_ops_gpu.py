"""GPU: the fused ViT forms of the C ABI hold their contracts bit for bit.

  * qe_quantlinear_requant == qe_quantize_pack_act(qe_quantlinear(...), act), on every int8 MFMA form (QE_LIN8 = 0 / 1 / 2,
    QE_LIN_NJ = 2 / 4) and on the two-pass form (QE_LIN_EPI=0, 4-bit or per-channel consumers), each case asserting its path;
  * qe_quantlinear_residual / qe_quantlinear_float_input_residual == the linear + residual (one fp32 add), in place too;
  * qe_quantize_pack_act's GELU is as close to float64 as torch's F.gelu (1 ulp slack);
  * qe_layernorm_quantize_pack: fp32 error at most 2x torch F.layer_norm's, codes == qe_quantize_pack of its own output;
  * qe_quantize_patchify == qe_quantize_pack of the unfolded images, and the patch GEMM computes conv_proj."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from quantize_amd import capi
from quantize_amd.packed import PackedConv2d
from quantize_amd.synthetic import pack_codes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


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
    with capi.knobs(QE_LIN8=lin8, QE_LIN_NJ=nj):
        codes = _requant_case(B, K, O, act, _rq(0.004, 3.0, 8, False) if act == "gelu" else _rq(0.01, -1.0), seed=B + O)
        _requant_case(B, K, O, act, _rq(0.04, 0.0), seed=B + O + 1, x_sign=False, per_row=False, asym=False)
    # the clamp is exercised at both ends: stored codes 0 and 255 (qmin and qmax of either quantiser) both occur
    assert int((codes == 0).sum()) > 0 and int((codes == 255).sum()) > 0


@pytest.mark.parametrize("act", [None, "gelu"])
def test_requant_two_pass_forms(act):
    with capi.knobs(QE_LIN_EPI=0):
        _requant_case(333, 256, 320, act, _rq(0.05, 1.0), seed=5, expect_path=0)
    _requant_case(333, 256, 320, act, _rq(0.3, 0.0, 4, True), seed=6, expect_path=0)            # 4-bit consumer
    _requant_case(333, 256, 320, act, _rq(0.05, 2.0, 8, True, per=320), seed=7, expect_path=0)  # per-feature consumer
    _requant_case(64, 100, 40, act, _rq(0.05, 0.0), seed=8, expect_path=0)                      # K % 64 != 0: fp32 kernel


def test_requant_nan_sets_status():
    rng = np.random.RandomState(9)
    for lin8, nj, B, K, O in FORMS:
        with capi.knobs(QE_LIN8=lin8, QE_LIN_NJ=nj):
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
    with capi.knobs(QE_LIN8=lin8, QE_LIN_NJ=nj):
        xq, wq, bias = _operands(rng, B, K, O)
        assert capi.linear_residual_path(xq, wq, B, K, O) == 1
        res = _t(rng.normal(0, 1, size=(B, O)).astype(np.float32))
        ref = capi.quantlinear(xq, wq, bias, B, K, O) + res
        out = capi.quantlinear_residual(xq, wq, bias, B, K, O, res)
        assert torch.equal(out, ref)
        inplace = res.clone()
        capi.quantlinear_residual(xq, wq, bias, B, K, O, inplace, out=inplace)
        assert torch.equal(inplace, ref)
    with capi.knobs(QE_LIN_EPI=0):
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
    with capi.knobs(QE_LIN_EPI=0):
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


# Every LayerNorm instance (NV = 1, 2, 4, 8 float4 per lane: E up to 256, 512, 1024, 2048), partial float4 groups (E / 4 not a
# multiple of 64), and the row counts of a single row, a few, a ragged last workgroup and ViT-B/16 at 256 images.
LN_E = [4, 64, 100, 260, 384, 516, 768, 1028, 1280, 2044, 2048]
LN_ROWS = [1, 3, 5, 777, 50432]
EPS32 = 2.0 ** -23


def _ln_input(rows, E, seed):
    """Rows of N(0, 9) around a per-row offset N(0, 400); the first rows adversarial: a large mean offset with a small spread,
    a constant row (0.75: its sum and mean are exact, so x - mean is 0 and the row's LayerNorm is beta), a single outlier."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(rows, E, generator=g, device=DEV) * 3 + torch.randn(rows, 1, generator=g, device=DEV) * 20
    gamma = 1 + 0.2 * torch.randn(E, generator=g, device=DEV)
    beta = 0.1 * torch.randn(E, generator=g, device=DEV)
    x[0] = 300.0 + 0.05 * torch.randn(E, generator=g, device=DEV)
    if rows > 1:
        x[1] = 0.75
    if rows > 2:
        x[2] = torch.randn(E, generator=g, device=DEV)
        x[2, E // 3] = 1e4
    return x, gamma, beta


def _ln64(x, gamma, beta, eps):
    x64 = x.double()
    m = x64.mean(-1, keepdim=True)
    y = (x64 - m) / torch.sqrt(((x64 - m) ** 2).mean(-1, keepdim=True) + eps)
    return y if gamma is None else y * gamma.double() + beta.double()


def _ln_bound(ref, x, gamma, beta, eps):
    """Per-row error bound: 2x torch F.layer_norm's error on that row, floored at 8 ulp of the row's largest |LayerNorm|, and
    never looser than today's whole-tensor rule, 2x torch's largest error.  The floor: where torch happens to land within an
    ulp or two on a row, the kernel's different but equally valid reduction order still rounds.  Each output is
    (x - mean) * rstd * gamma + beta: half an ulp for each of the subtraction, the two products and the add, about one for the
    mean, and two to three for rstd (the fp32 sum of squares, the division, the square root): 5 to 6 ulp, 8 with margin."""
    e_t = (F.layer_norm(x, (x.shape[-1],), gamma, beta, eps).double() - ref).abs().amax(-1)
    big = ref.abs().amax(-1).float()
    ulp = (torch.nextafter(big, torch.full_like(big, float("inf"))) - big).double()
    return torch.minimum(torch.maximum(2 * e_t, 8 * ulp), 2 * e_t.max())


def _check_ln_codes_f64(codes, r, ref, bound, what):
    """codes (stored, 8-bit) == the float64 codes of ref, except flips of one where ref / sc - zr is within the fp32 error
    bound (bound on the value, then the division and subtraction) of a half-integer."""
    sc, zr = float(r._keep[0][0]), float(r._keep[1][0])
    t = ref / sc - zr
    q64 = torch.clamp(torch.round(t), r.qmin, r.qmax)
    q = codes.view(ref.shape).to(torch.int32) - (128 if r.sign else 0)
    d = (q.double() - q64).abs()
    band = bound[:, None] / sc + 4 * EPS32 * (t.abs() + abs(zr))
    near_tie = ((t - torch.floor(t)) - 0.5).abs() <= band
    bad = (d > 1) | ((d == 1) & ~near_tie)
    assert not bool(bad.any()), "%s: %d codes off the float64 codes outside the tie band" % (what, int(bad.sum()))


@pytest.mark.parametrize("E", LN_E)
def test_layernorm_vs_float64(E):
    rqs = [_rq(0.02, 0.0, 8, True), _rq(0.03, -120.0, 8, False)]
    for rows in LN_ROWS:
        x, gamma, beta = _ln_input(rows, E, seed=rows * 4096 + E)
        codes, ln, st = capi.layernorm_quantize_pack(x, gamma, beta, 1e-6, rqs, ln_out="new")
        assert capi.layernorm_path(rows, E, rqs, codes) == 1 and int(st.item()) == 0
        ref = _ln64(x, gamma, beta, 1e-6)
        bound = _ln_bound(ref, x, gamma, beta, 1e-6)
        e_k = (ln.double() - ref).abs().amax(-1)
        worst = int(torch.argmax(e_k - bound))
        assert bool((e_k <= bound).all()), "E %d rows %d: row %d error %.3g > %.3g" % (E, rows, worst, float(e_k[worst]), float(bound[worst]))
        if rows > 1:
            assert torch.equal(ln[1], beta)                       # the constant row
        for c, r in zip(codes, rqs):
            assert torch.equal(c, capi.quantize_pack(ln, r._keep[0], r._keep[1], r.qmin, r.qmax, r.n_bits, r.sign)[0])
            _check_ln_codes_f64(c, r, ref, bound, "E %d rows %d" % (E, rows))
    # gamma / beta NULL: the plain normalisation
    codes, ln1, _ = capi.layernorm_quantize_pack(x, None, None, 1e-6, rqs, ln_out="new")
    ref1 = _ln64(x, None, None, 1e-6)
    bound1 = _ln_bound(ref1, x, None, None, 1e-6)
    assert bool(((ln1.double() - ref1).abs().amax(-1) <= bound1).all())
    for c, r in zip(codes, rqs):
        assert torch.equal(c, capi.quantize_pack(ln1, r._keep[0], r._keep[1], r.qmin, r.qmax, r.n_bits, r.sign)[0])
    # n_out = 0, only ln_out: the same fp32 LayerNorm
    none, ln0, _ = capi.layernorm_quantize_pack(x, gamma, beta, 1e-6, [], ln_out="new")
    assert none == [] and torch.equal(ln0, ln)
    # two-pass form with a per-feature consumer (n_param == E) and ln_out NULL (the workspace holds the LayerNorm): the
    # channel of element (row, e) is e
    g = torch.Generator(device=DEV).manual_seed(E)
    s = torch.rand(E, generator=g, device=DEV) * 0.03 + 0.01
    z = torch.rand(E, generator=g, device=DEV) * 6 - 3
    pf = capi.requant(s, z, -128, 127, 8, True)
    assert capi.layernorm_path(x.shape[0], E, [pf], [torch.empty(x.numel(), dtype=torch.uint8, device=DEV)]) == 0
    (cpf,), none, st = capi.layernorm_quantize_pack(x, gamma, beta, 1e-6, [pf])
    assert none is None and int(st.item()) == 0
    want = (torch.clamp(torch.round(ln / s - z), -128, 127).to(torch.int32) + 128).to(torch.uint8).flatten()
    assert torch.equal(cpf, want)


@pytest.mark.parametrize("E", [100, 384, 768, 2048])
def test_layernorm_non_finite_rows(E):
    rows = 37
    x, gamma, beta = _ln_input(rows, E, seed=E + 1)
    rqs = [_rq(0.02, 0.0, 8, True)]
    codes, ln, st = capi.layernorm_quantize_pack(x, gamma, beta, 1e-6, rqs, ln_out="new")
    assert int(st.item()) == 0
    bad_rows = [5, 17, 36]
    for r, v in zip(bad_rows, (float("nan"), float("inf"), float("-inf"))):
        y = x.clone()
        y[r, E // 2] = v
        c2, ln2, st2 = capi.layernorm_quantize_pack(y, gamma, beta, 1e-6, rqs, ln_out="new")
        assert int(st2.item()) == 1, (r, v)
        keep = torch.ones(rows, dtype=torch.bool, device=DEV)
        keep[r] = False
        assert torch.equal(ln2[keep], ln[keep])
        assert torch.equal(c2[0].view(rows, E)[keep], codes[0].view(rows, E)[keep])


def test_layernorm_rejections():
    L = capi.lib()
    E, rows = 64, 8
    x, gamma, beta = _ln_input(rows, E + 4, seed=3)
    xs, gs, bs = x[:, :E].contiguous(), gamma[:E].contiguous(), beta[:E].contiguous()
    rq = _rq(0.02, 0.0, 8, True)
    arr = (capi.QeRequant * 1)(rq)

    def call(xp, n, e, gp, bp, lnp, codes):
        cp = (ctypes.c_void_p * 1)(codes.data_ptr())
        return L.qe_layernorm_quantize_pack(xp, n, e, gp, bp, 1e-6, 1, arr, cp, lnp, None, None, 0, None)

    codes = torch.full((rows * E + 16,), 0xAB, dtype=torch.uint8, device=DEV)
    ln = torch.full((rows * E + 8,), 7.0, device=DEV)
    # rows = 0: a no-op
    assert call(xs.data_ptr(), 0, E, gs.data_ptr(), bs.data_ptr(), ln.data_ptr(), codes) == 0
    # misaligned x, gamma or ln_out (one float off a 16-byte boundary): QE_ERR_ARG, nothing written
    xm = torch.empty(rows * E + 4, device=DEV)
    xm[1:1 + rows * E] = xs.flatten()
    gm = torch.empty(E + 4, device=DEV)
    gm[1:1 + E] = gs
    assert call(xm.data_ptr() + 4, rows, E, gs.data_ptr(), bs.data_ptr(), ln.data_ptr(), codes) == 4
    assert call(xs.data_ptr(), rows, E, gm.data_ptr() + 4, bs.data_ptr(), ln.data_ptr(), codes) == 4
    assert call(xs.data_ptr(), rows, E, gs.data_ptr(), bs.data_ptr(), ln.data_ptr() + 4, codes) == 4
    torch.cuda.synchronize()
    assert bool((codes == 0xAB).all()) and bool((ln == 7.0).all())
    # widths outside E % 4 == 0, 4 <= E <= QE_LN_MAX_E: QE_ERR_UNSUPPORTED
    big = torch.zeros(rows * 2052, device=DEV)
    for e in (2, 66, 2052):
        assert call(big.data_ptr(), rows, e, None, None, None, codes) == 7, e
    # the aligned call itself is accepted and writes both outputs
    assert call(xs.data_ptr(), rows, E, gs.data_ptr(), bs.data_ptr(), ln.data_ptr(), codes) == 0
    torch.cuda.synchronize()
    assert not bool((codes[:rows * E] == 0xAB).all()) and not bool((ln[:rows * E] == 7.0).all())


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
