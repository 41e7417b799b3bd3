"""CPU: the attention core's C entry points are exported and declared, the kernel choice is a host-only answer, and
qe_attention's argument checks answer before any device work (no GPU here: a device call would fail)."""
import ctypes

import pytest

from quantize_amd import capi

QE_ERR_ARG = 4


def test_attention_symbols_exported_and_declared():
    L = capi.lib()
    for name in ("qe_attention", "qe_attention_path"):
        assert name in capi.SYMBOLS
        assert hasattr(L, name)


@pytest.mark.parametrize("L,S,H,d,want", [(197, 197, 12, 64, 1), (257, 257, 16, 80, 1), (17, 17, 4, 16, 1),
                                          (50, 50, 12, 64, 1), (33, 65, 3, 32, 1), (197, 197, 1, 128, 1),
                                          (17, 17, 4, 20, 0), (9, 9, 2, 136, 0), (9, 9, 2, 7, 0), (9, 9, 2, 256, 0),
                                          (40, 45, 2, 48, 1), (40, 45, 2, 96, 1), (40, 45, 2, 112, 1), (40, 45, 2, 192, 0),
                                          (40, 45, 2, 193, 0), (300, 300, 2, 64, 1)])
def test_attention_path(L, S, H, d, want):
    assert capi.attention_path(L, S, H, d) == want


@pytest.mark.parametrize("L,S,H,d", [(9, 9, 2, 260), (0, 9, 2, 64), (9, 0, 2, 64), (9, 9, 0, 64), (9, 9, 2, 0)])
def test_attention_path_unsupported(L, S, H, d):
    assert capi.attention_path(L, S, H, d) < 0


def test_attention_knob_forces_the_valu_kernel():
    with capi.knobs(QE_ATTN="0"):
        assert capi.attention_path(197, 197, 12, 64) == 0
        assert capi.attention_path(17, 17, 4, 20) == 0
    assert capi.attention_path(197, 197, 12, 64) == 1


def _call(q=4096, k=1 << 20, v=2 << 20, out=3 << 20, N=2, L=5, S=5, H=2, d=16, strides=(5, 1, 5, 1, 5, 1)):
    p = lambda a: None if a is None else ctypes.c_void_p(a)
    return capi.lib().qe_attention(p(q), p(k), p(v), p(out), N, L, S, H, d, *strides, 0.25, None)


def test_attention_argument_errors_need_no_gpu():
    for kw in (dict(N=0), dict(L=0), dict(S=-1), dict(H=0), dict(d=0), dict(N=-3)):
        assert _call(**kw) == QE_ERR_ARG, kw
    for name in ("q", "k", "v", "out"):
        assert _call(**{name: None}) == QE_ERR_ARG, name
    assert _call(strides=(5, -1, 5, 1, 5, 1)) == QE_ERR_ARG
    assert _call(q=4100) == QE_ERR_ARG                         # not 16-byte aligned
    # out overlapping q, k or v: the spans are N*L*E floats (q, out) and N*S*E (k, v) from their base
    span = 2 * 5 * 32 * 4
    assert _call(out=4096) == QE_ERR_ARG
    assert _call(out=4096 + span - 16) == QE_ERR_ARG
    assert _call(out=(1 << 20) + 64) == QE_ERR_ARG
    assert _call(out=(2 << 20) - span + 16) == QE_ERR_ARG
    # d > 256: no kernel
    assert _call(d=260) == capi.QE_ERR_UNSUPPORTED
