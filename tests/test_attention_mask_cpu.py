"""CPU: the masked attention entry points are exported and declared, their kernel choice is a host-only answer, every
argument error of qe_attention_masked answers before any device work, the float64 yardstick of the GPU tests
(tests/attention_ref.py) agrees with torch's own masked attention on the CPU -- which pins the bool polarity and the
top-left causal alignment before any GPU is involved -- and PackedMultiheadAttention validates its mask arguments."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attention_ref as ar
from quantize_amd import capi
from quantize_amd.packed import PackedMultiheadAttention

QE_ERR_ARG = 4


def test_masked_symbols_exported_and_declared():
    L = capi.lib()
    for name in ("qe_attention_masked", "qe_attention_masked_path"):
        assert name in capi.SYMBOLS
        assert hasattr(L, name)


OPERANDS = [(m, b, c) for m in (0, 1) for b in (0, 1) for c in (0, 1)]


@pytest.mark.parametrize("L,S,H,d,want", [(197, 197, 12, 64, 1), (257, 257, 16, 80, 1), (17, 17, 4, 16, 1),
                                          (50, 50, 12, 64, 1), (33, 65, 3, 32, 1), (197, 197, 1, 128, 1),
                                          (77, 77, 8, 64, 1),
                                          (17, 17, 4, 20, 0), (9, 9, 2, 136, 0), (9, 9, 2, 7, 0), (9, 9, 2, 256, 0)])
def test_masked_path(L, S, H, d, want):
    for m, b, c in OPERANDS:
        assert capi.attention_masked_path(L, S, H, d, m, b, c) == want, (m, b, c)


@pytest.mark.parametrize("L,S,H,d", [(9, 9, 2, 260), (0, 9, 2, 64), (9, 0, 2, 64), (9, 9, 0, 64), (9, 9, 2, 0)])
def test_masked_path_unsupported(L, S, H, d):
    for m, b, c in OPERANDS:
        assert capi.attention_masked_path(L, S, H, d, m, b, c) < 0, (m, b, c)


def test_masked_path_never_mfma_under_the_knob():
    with capi.knobs(QE_ATTN="0"):
        for shape in ((197, 197, 12, 64), (77, 77, 8, 64), (17, 17, 4, 20)):
            for m, b, c in OPERANDS:
                assert capi.attention_masked_path(*shape, m, b, c) == 0, (shape, m, b, c)
    assert capi.attention_masked_path(197, 197, 12, 64, 1, 1, 1) == 1


def _call(q=4096, k=1 << 20, v=2 << 20, out=3 << 20, N=2, L=5, S=5, H=2, d=16, strides=(5, 1, 5, 1, 5, 1),
          mask=4 << 20, mask_sn=0, mask_sh=0, key_bias=5 << 20, causal=0):
    p = lambda a: None if a is None else ctypes.c_void_p(a)
    return capi.lib().qe_attention_masked(p(q), p(k), p(v), p(out), N, L, S, H, d, *strides, 0.25, p(mask), mask_sn, mask_sh,
                                          p(key_bias), causal, None)


def test_masked_argument_errors_need_no_gpu():
    # what qe_attention refuses, the masked entry point refuses too
    for kw in (dict(N=0), dict(L=0), dict(S=-1), dict(H=0), dict(d=0), dict(N=-3)):
        assert _call(**kw) == QE_ERR_ARG, kw
    for name in ("q", "k", "v", "out"):
        assert _call(**{name: None}) == QE_ERR_ARG, name
    assert _call(strides=(5, -1, 5, 1, 5, 1)) == QE_ERR_ARG
    assert _call(q=4100) == QE_ERR_ARG
    assert _call(out=4096) == QE_ERR_ARG
    assert _call(d=260) == capi.QE_ERR_UNSUPPORTED
    assert _call(d=260, mask=None, key_bias=None, causal=1) == capi.QE_ERR_UNSUPPORTED
    # negative mask strides
    assert _call(mask_sn=-1) == QE_ERR_ARG
    assert _call(mask_sh=-25) == QE_ERR_ARG
    # mask / key_bias not 16-byte aligned
    assert _call(mask=(4 << 20) + 4) == QE_ERR_ARG
    assert _call(key_bias=(5 << 20) + 8) == QE_ERR_ARG
    assert _call(mask=None, key_bias=(5 << 20) + 4) == QE_ERR_ARG
    # strides given without a mask
    assert _call(mask=None, mask_sn=25) == QE_ERR_ARG
    assert _call(mask=None, mask_sh=25) == QE_ERR_ARG
    assert _call(mask=None, key_bias=None, mask_sn=50, mask_sh=25) == QE_ERR_ARG
    # out overlapping the mask: out spans N*L*E = 2*5*32 floats; the mask L*S floats (2-D) or N*H*L*S (3-D)
    ospan = 2 * 5 * 32 * 4
    assert _call(mask=3 << 20) == QE_ERR_ARG
    assert _call(mask=(3 << 20) + ospan - 16) == QE_ERR_ARG
    assert _call(mask=(3 << 20) - 5 * 5 * 4 * 4 + 16, mask_sn=50, mask_sh=25) == QE_ERR_ARG      # its last block reaches out
    # out overlapping key_bias (N*S floats)
    assert _call(key_bias=3 << 20) == QE_ERR_ARG
    assert _call(key_bias=(3 << 20) + ospan - 16) == QE_ERR_ARG
    assert _call(key_bias=(3 << 20) - 32) == QE_ERR_ARG                                          # 2*5 floats = 40 bytes


# ---- the yardstick itself ----
def _qkv(N, L, S, H, d, seed):
    rng = np.random.RandomState(seed)
    return tuple(rng.normal(0, 1, size=(N, T, H, d)) for T in (L, S, S)), rng


def _sdpa64(q, k, v, **kw):
    t = lambda a: torch.from_numpy(a).transpose(1, 2)                  # (N, H, T, d) float64
    return F.scaled_dot_product_attention(t(q), t(k), t(v), **kw).transpose(1, 2).numpy()


@pytest.mark.parametrize("N,L,S,H,d", [(2, 9, 9, 3, 8), (2, 7, 12, 2, 4), (1, 12, 7, 2, 4)])
def test_ref64_against_cpu_sdpa(N, L, S, H, d):
    (q, k, v), rng = _qkv(N, L, S, H, d, 5)
    add = ar.additive2d(L, S, rng)
    cases = {"additive2d": (dict(mask=add), dict(attn_mask=torch.from_numpy(add).double())),
             "causal flag": (dict(causal=True), dict(is_causal=True)),
             "tril additive": (dict(mask=ar.tril_inf(L, S)), dict(is_causal=True)),
             "tril bool": (dict(causal=True), dict(attn_mask=torch.ones(L, S, dtype=torch.bool).tril()))}   # SDPA: True = visible
    holes = ar.holes3d(N, H, L, S, rng)
    cases["holes3d"] = (dict(mask=holes), dict(attn_mask=torch.from_numpy(holes).double().view(N, H, L, S)))
    pad = ar.pad_tail(N, S, rng)
    cases["all three"] = (dict(mask=add, key_bias=pad, causal=True),
                          dict(attn_mask=torch.from_numpy(ar.merged(N, H, L, S, add, pad, True)).double()))
    for name, (mine, theirs) in cases.items():
        assert ar.visible(ar.merged(N, H, L, S, **mine)).all(), name
        got, want = ar.ref64(q, k, v, **mine), _sdpa64(q, k, v, **theirs)
        assert np.isfinite(got).all() and np.abs(got - want).max() <= 1e-12, (name, np.abs(got - want).max())


@pytest.mark.parametrize("N,L,S,H,d", [(3, 6, 6, 2, 4), (2, 5, 11, 4, 4)])
def test_ref64_against_nn_multihead_attention(N, L, S, H, d):
    """nn.MultiheadAttention (fp64, CPU) with identity projections is the bare core: attn_mask 2-D / 3-D, bool (True = NOT
    allowed) and float, key_padding_mask bool (True = ignored) and float."""
    E = H * d
    (q, k, v), rng = _qkv(N, L, S, H, d, 11)
    mha = torch.nn.MultiheadAttention(E, H, bias=False).double()
    with torch.no_grad():
        mha.in_proj_weight.copy_(torch.eye(E, dtype=torch.float64).repeat(3, 1))
        mha.out_proj.weight.copy_(torch.eye(E, dtype=torch.float64))
    seq = lambda a: torch.from_numpy(a.reshape(a.shape[0], a.shape[1], E)).transpose(0, 1)      # (T, N, E)

    def run(**kw):
        with torch.no_grad():
            y, _ = mha(seq(q), seq(k), seq(v), need_weights=True, **kw)
        return y.transpose(0, 1).reshape(N, L, H, d).numpy()

    add = ar.additive2d(L, S, rng)
    holes = ar.holes3d(N, H, L, S, rng)
    pad = ar.pad_tail(N, S, rng)
    front = ar.pad_front(N, S, rng)
    tril = ar.tril_inf(L, S)
    T = torch.from_numpy
    cases = [("float 2-D", dict(mask=add), dict(attn_mask=T(add).double())),
             ("bool 2-D", dict(mask=tril), dict(attn_mask=T(np.isinf(tril)))),
             ("causal flag", dict(causal=True), dict(attn_mask=T(np.isinf(tril)))),
             ("float 3-D", dict(mask=holes), dict(attn_mask=T(holes).double())),
             ("bool 3-D", dict(mask=np.where(np.isinf(holes), ar.NEG, 0).astype(np.float32)), dict(attn_mask=T(np.isinf(holes)))),
             ("bool padding", dict(key_bias=pad), dict(key_padding_mask=T(np.isinf(pad)))),
             ("float padding", dict(key_bias=front), dict(key_padding_mask=T(front).double())),
             ("mask + padding", dict(mask=add, key_bias=pad), dict(attn_mask=T(add).double(), key_padding_mask=T(pad).double()))]
    for name, mine, theirs in cases:
        assert ar.visible(ar.merged(N, H, L, S, **mine)).all(), name
        got, want = ar.ref64(q, k, v, **mine), run(**theirs)
        assert np.isfinite(got).all() and np.abs(got - want).max() <= 1e-12, (name, np.abs(got - want).max())


def test_ref64_blank_row_is_nan_like_torch_softmax():
    (q, k, v), rng = _qkv(2, 5, 5, 2, 4, 3)
    m = ar.blank_rows(2, 2, 5, 5, [(1, 0, 3)], rng)
    bad = ~np.isfinite(ar.ref64(q, k, v, mask=m))
    want = np.zeros_like(bad)
    want[1, 3, 0, :] = True
    assert np.array_equal(bad, want)
    assert torch.isnan(torch.softmax(torch.full((4,), float("-inf")), 0)).all()


# ---- PackedMultiheadAttention's mask validation (raised before any projection runs) ----
def _mha(H=2):
    z = torch.zeros(1)
    return PackedMultiheadAttention(None, None, None, z, z, z, z, None, H)


def test_packed_mha_mask_validation():
    mha, L, S, N, E, H = _mha(), 4, 6, 3, 8, 2
    q, k = torch.zeros(L, N, E), torch.zeros(S, N, E)
    call = lambda **kw: mha(q, k, k, need_weights=False, **kw)
    with pytest.raises(AssertionError, match="only bool and floating types of key_padding_mask are supported"):
        call(key_padding_mask=torch.zeros(N, S, dtype=torch.int64))
    with pytest.raises(ValueError):
        call(key_padding_mask=torch.zeros(S, N, dtype=torch.bool))
    with pytest.raises(ValueError):
        call(key_padding_mask=torch.zeros(N, S + 1))
    with pytest.raises(ValueError):
        call(attn_mask=torch.zeros(L, S, dtype=torch.int32))
    with pytest.raises(ValueError):
        call(attn_mask=torch.zeros(S, L))
    with pytest.raises(ValueError):
        call(attn_mask=torch.zeros(N, L, S))                      # 3-D is (N*H, L, S), as nn.MultiheadAttention
    with pytest.raises(ValueError):
        call(attn_mask=torch.zeros(N, H, L, S))
    with pytest.raises(ValueError):
        mha(q, k, k, need_weights=True, attention="engine", attn_mask=torch.zeros(L, S, dtype=torch.bool))
    add, pad = PackedMultiheadAttention._additive_masks(torch.ones(L, S, dtype=torch.bool).tril().logical_not(),
                                                        torch.arange(S)[None, :].expand(N, S) >= 4, N, H, L, S)
    assert add.dtype == torch.float32 and np.array_equal(add.numpy(), ar.tril_inf(L, S))           # True = NOT allowed
    assert pad.dtype == torch.float32 and bool(torch.isinf(pad[:, 4:]).all()) and bool((pad[:, :4] == 0).all())
