"""GPU: the fp32 attention core (qe_attention) against a float64 evaluation on the CPU, in both row layouts, on both kernels
(the MFMA kernel and the VALU kernel QE_ATTN=0 forces) wherever both apply.

Tolerance, per case: e_q = max |engine - ref64| and e_t = max |torch fp32 SDPA - ref64| on the same inputs;
e_q <= max(4 e_t, 1e-6 max|V|) and e_q <= 1e-5 max|V|.  Two score regimes: moderate (|scores| <~ 5) and peaky (|scores| up to
~60, each row's maximum in the last, ragged key tile: a missing online-softmax rescale or an exp overflow shows there).
The output is pre-filled with NaN, so every element the kernel leaves unwritten fails the finiteness check."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from quantize_amd import capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (N, L, S, H, d): ViT-B/16, ViT-B/32, ViT-H/14, the tiny test ViT, one token, S != L with a ragged tail on both, one head
# at d = 128, and VALU-only head sizes (d = 20, d = 136)
CASES = [(2, 197, 197, 12, 64), (1, 50, 50, 12, 64), (2, 257, 257, 16, 80), (3, 17, 17, 4, 16), (2, 1, 1, 2, 64),
         (2, 33, 65, 3, 32), (1, 197, 197, 1, 128), (2, 37, 45, 3, 20), (1, 40, 70, 2, 136)]


def _inputs(N, L, S, H, d, regime, seed):
    """q (N, L, H, d), k / v (N, S, H, d) fp32 host arrays."""
    rng = np.random.RandomState(seed)
    k = rng.normal(0, 1, size=(N, S, H, d))
    v = rng.normal(0, 1, size=(N, S, H, d))
    if regime == "moderate":
        q = rng.normal(0, 1, size=(N, L, H, d))                 # scores ~ N(0, 1) at scale d^-0.5
    else:
        # each query row scores 60 on one key of the last (ragged) key tile and 58 on one key of the first tile (the
        # minimum-norm q for the two targets): the row max arrives last, after a large partial sum has to be rescaled;
        # the other keys' scores spread ~ +-60 sqrt(2 / d)
        n_, h_ = np.arange(N)[:, None, None], np.arange(H)[None, None, :]
        j1 = rng.randint(((S - 1) // 32) * 32, S, size=(N, L, H))
        k1 = k[n_, j1, h_]                                                          # (N, L, H, d)
        if S == 1:
            q = k1 * (60.0 / (d ** -0.5 * (k1 ** 2).sum(-1, keepdims=True)))
        else:
            j2 = rng.randint(0, min(32, S), size=(N, L, H))
            j2 = np.where(j2 == j1, (j1 + 1) % S, j2)
            K2 = np.stack([k1, k[n_, j2, h_]], axis=-2)                            # (N, L, H, 2, d)
            G = K2 @ np.swapaxes(K2, -1, -2)
            c = np.linalg.solve(G, np.broadcast_to(np.array([60.0, 58.0]) / d ** -0.5, G.shape[:-1])[..., None])
            q = (np.swapaxes(K2, -1, -2) @ c)[..., 0]
    return q.astype(np.float32), k.astype(np.float32), v.astype(np.float32)


def _ref64(q, k, v):
    d = q.shape[-1]
    q64, k64, v64 = (a.astype(np.float64) for a in (q, k, v))
    s = np.einsum("nlhd,nshd->nhls", q64, k64) * d ** -0.5
    s -= s.max(-1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(-1, keepdims=True)
    return np.einsum("nhls,nshd->nlhd", p, v64)


def _torch_sdpa(q, k, v):
    t = lambda a: torch.from_numpy(a).to(DEV).transpose(1, 2)          # (N, H, T, d)
    return F.scaled_dot_product_attention(t(q), t(k), t(v)).transpose(1, 2).cpu().numpy()


def _rows(a, layout):
    """(N, T, H, d) -> the contiguous device rows of `layout`."""
    N, T, H, d = a.shape
    if layout == "seq":
        a = a.transpose(1, 0, 2, 3)
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1, H * d)).to(DEV)


def _unrows(t, N, T, H, d, layout):
    a = t.cpu().numpy()
    if layout == "seq":
        return a.reshape(T, N, H, d).transpose(1, 0, 2, 3)
    return a.reshape(N, T, H, d)


def _run(q, k, v, layout):
    N, L, H, d = q.shape
    S = k.shape[1]
    out = torch.full((N * L, H * d), float("nan"), dtype=torch.float32, device=DEV)
    capi.attention(_rows(q, layout), _rows(k, layout), _rows(v, layout), N, L, H, S=S, layout=layout, out=out)
    torch.cuda.synchronize()
    return _unrows(out, N, L, H, d, layout)


def _kernels(L, S, H, d):
    return ["mfma", "valu"] if capi.attention_path(L, S, H, d) == 1 else ["valu"]


@pytest.mark.parametrize("regime", ["moderate", "peaky"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "N%d-L%d-S%d-H%d-d%d" % c)
def test_attention_vs_float64(case, regime):
    N, L, S, H, d = case
    q, k, v = _inputs(N, L, S, H, d, regime, seed=sum(case))
    ref = _ref64(q, k, v)
    e_t = float(np.abs(_torch_sdpa(q, k, v) - ref).max())
    vmax = float(np.abs(v).max())
    for kern in _kernels(L, S, H, d):
        with capi.knobs(QE_ATTN=None if kern == "mfma" else "0"):
            assert capi.attention_path(L, S, H, d) == (1 if kern == "mfma" else 0)
            for layout in ("token", "seq"):
                got = _run(q, k, v, layout)
                assert np.isfinite(got).all(), (kern, layout)
                e_q = float(np.abs(got - ref).max())
                print("%s %s %s %s: e_q %.3g e_t %.3g (max|V| %.3g)" % (case, regime, kern, layout, e_q, e_t, vmax))
                assert e_q <= max(4 * e_t, 1e-6 * vmax), (kern, layout, e_q, e_t)
                assert e_q <= 1e-5 * vmax, (kern, layout, e_q)


@pytest.mark.parametrize("case", [(2, 40, 40, 3, 64), (2, 40, 40, 3, 20)], ids=["d64", "d20"])
def test_nan_locality(case):
    N, L, S, H, d = case
    q, k, v = _inputs(N, L, S, H, d, "moderate", seed=3)
    qn = q.copy()
    qn[1, 5, 2, 7] = np.nan
    kn = k.copy()
    kn[0, 3, 1, 4] = np.nan
    for kern in _kernels(L, S, H, d):
        with capi.knobs(QE_ATTN=None if kern == "mfma" else "0"):
            for layout in ("token", "seq"):
                got = _run(qn, k, v, layout)
                bad = ~np.isfinite(got)
                want = np.zeros_like(bad)
                want[1, 5, 2, :] = True
                assert np.array_equal(bad, want), (kern, layout, "query NaN")
                got = _run(q, kn, v, layout)
                bad = ~np.isfinite(got)
                want = np.zeros_like(bad)
                want[0, :, 1, :] = True
                assert np.array_equal(bad, want), (kern, layout, "key NaN")


def test_attention_makes_no_host_sync():
    N, L, H, d = 2, 197, 12, 64
    g = torch.Generator(device="cpu").manual_seed(0)
    q, k, v = (torch.randn(N * L, H * d, generator=g).to(DEV) for _ in range(3))
    out = torch.empty_like(q)
    capi.attention(q, k, v, N, L, H, out=out)               # warm-up: module load
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        capi.attention(q, k, v, N, L, H, out=out)
        capi.attention(q, k, v, N, L, H, out=out, scale=0.1)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
