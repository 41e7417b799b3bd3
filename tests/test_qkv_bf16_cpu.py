"""CPU: the host side of the bf16 q / k / v route -- qe_quantlinear_bf16 (LIN_BF16), qe_attention_bf16_stored and PackedViT's
qkv option: the path answers, the argument checks that are made before any device work (pointers are plain integers here,
nothing is launched, so no GPU is needed), and the option's ValueErrors."""
import ctypes

import pytest
import torch

import lin_instances as li
from quantize_amd import capi
from quantize_amd.packed_vit import QKV, PackedViT, synthetic_state_dict

COMBOS = [(m, b, c) for m in (0, 1) for b in (0, 1) for c in (0, 1)]
ARG, UNSUPPORTED = 4, capi.QE_ERR_UNSUPPORTED          # include/quant_engine.h
A, FAR = 1 << 20, 1 << 44                              # 16-byte aligned, far enough apart for any span below
NEW = ["qe_quantlinear_bf16_path", "qe_quantlinear_bf16_workspace_bytes", "qe_quantlinear_bf16",
       "qe_attention_bf16_stored_path", "qe_attention_bf16_stored"]


def test_symbols_exported():
    L = capi.lib()
    for s in NEW:
        assert s in capi.SYMBOLS and hasattr(L, s), s
    assert L.qe_quantlinear_bf16_workspace_bytes.restype is ctypes.c_size_t


def test_stored_path_answers():
    for knob in (None, "0"):                        # QE_ATTN chooses between the fp32 kernels only
        with capi.knobs(QE_ATTN=knob):
            for d in range(16, 129, 16):
                for m, b, c in COMBOS:
                    assert capi.attention_bf16_stored_path(40, 45, 2, d, m, b, c) == 2, (knob, d, m, b, c)
            for d in (8, 136, 20, 72, 144):
                for m, b, c in COMBOS:
                    assert capi.attention_bf16_stored_path(40, 45, 2, d, m, b, c) == -1, (knob, d, m, b, c)
            for L, S, H, d in ((0, 45, 2, 64), (40, 0, 2, 64), (40, 45, 0, 64), (40, 45, 2, 0), (-1, 45, 2, 64), (40, 45, 2, -16)):
                assert capi.attention_bf16_stored_path(L, S, H, d) == -1, (knob, L, S, H, d)


def bad_attention_lists(elem):
    """The 18 argument lists tests/test_attention_bf16_cpu.py refuses, for q / k / v of `elem` bytes per element (4: the
    fp32-buffer entry points, 2: qe_attention_bf16_stored) -- the same broken rule in each: (name, arguments, code)."""
    good = dict(q=A, k=A + FAR, v=A + 2 * FAR, out=A + 3 * FAR, N=2, L=40, S=45, H=2, d=64, q_rn=40, q_rt=1, kv_rn=45, kv_rt=1,
                o_rn=40, o_rt=1, scale=0.125, mask=None, mask_sn=0, mask_sh=0, key_bias=None, causal=0)
    span = 2 * 40 * 128 * 4                   # bytes of out
    bad = [("N = 0", dict(N=0), ARG), ("L < 0", dict(L=-1), ARG), ("d = 0", dict(d=0), ARG), ("negative stride", dict(kv_rt=-1), ARG),
           ("negative out stride", dict(o_rn=-40), ARG), ("null k", dict(k=None), ARG), ("misaligned q", dict(q=A + 4), ARG),
           ("misaligned out", dict(out=A + 3 * FAR + 8), ARG), ("negative mask stride", dict(mask=A + 4 * FAR, mask_sh=-4), ARG),
           ("stride without mask", dict(mask_sn=4), ARG), ("misaligned mask", dict(mask=A + 4 * FAR + 4), ARG),
           ("misaligned key_bias", dict(key_bias=A + 5 * FAR + 4), ARG), ("out is q", dict(out=A), ARG),
           ("out overlaps the end of v", dict(out=A + 2 * FAR + 2 * 45 * 128 * elem - 16), ARG),
           ("out overlaps mask", dict(mask=A + 3 * FAR + span - 16), ARG),
           ("out overlaps key_bias", dict(key_bias=A + 3 * FAR - 2 * 45 * 4 + 16), ARG),
           ("d > 256", dict(d=272), UNSUPPORTED),
           ("more rows than a grid", dict(N=1 << 20, H=1 << 10, L=32, S=32, d=16, q_rn=32, kv_rn=32, o_rn=32), UNSUPPORTED)]
    out = []
    for name, change, want in bad:
        a = dict(good, **change)
        out.append((name, (a["q"], a["k"], a["v"], a["out"], a["N"], a["L"], a["S"], a["H"], a["d"], a["q_rn"], a["q_rt"], a["kv_rn"],
                           a["kv_rt"], a["o_rn"], a["o_rt"], a["scale"], a["mask"], a["mask_sn"], a["mask_sh"], a["key_bias"],
                           a["causal"], None), want))
    return out


def check_stored_refusals():
    """qe_attention_bf16_stored answers every refused argument list as qe_attention_bf16 does (one attn_prepare), the spans
    of q / k / v taken on 2-byte elements; shared with tests/test_attention_bf16_stored_gpu.py."""
    L_ = capi.lib()
    lists4, lists2 = bad_attention_lists(4), bad_attention_lists(2)
    assert len(lists4) == 18
    for (name, args4, want), (_, args2, _) in zip(lists4, lists2):
        bf16, stored = L_.qe_attention_bf16(*args4), L_.qe_attention_bf16_stored(*args2)
        assert bf16 == want and stored == want, (name, bf16, stored, want)
    for d in (8, 136, 20, 72, 144):
        args = (A, A + FAR, A + 2 * FAR, A + 3 * FAR, 2, 40, 45, 2, d, 40, 1, 45, 1, 40, 1, 0.125, None, 0, 0, None, 0, None)
        assert L_.qe_attention_bf16_stored(*args) == UNSUPPORTED, d


def test_stored_bad_arguments_get_the_bf16_entry_points_answer():
    check_stored_refusals()


def test_stored_null_and_misaligned_pointers():
    L_ = capi.lib()
    good = [A, A + FAR, A + 2 * FAR, A + 3 * FAR]
    tail = (2, 40, 45, 2, 64, 40, 1, 45, 1, 40, 1, 1.0, None, 0, 0, None, 0, None)
    for i in range(4):
        for bad in (None, good[i] + 2, good[i] + 8):          # 2-byte aligned is not enough: the rows are read 16 bytes at a time
            p = list(good)
            p[i] = bad
            assert L_.qe_attention_bf16_stored(*p, *tail) == ARG, (i, bad)


def _q(n_param=1, data=A, n_bits=8):
    return capi.QeQParam(data, n_bits, 1, A + FAR, A + 2 * FAR, n_param)


def test_linear_bf16_argument_checks():
    """The checks of the qe_quantlinear_residual trio, and `out` in place of residual / out."""
    L_ = capi.lib()
    x, w = _q(), _q()
    B, K, O = 64, 128, 256
    run = lambda xq, wq, B, K, O, out, ws=None, wsb=0: L_.qe_quantlinear_bf16(ctypes.byref(xq), ctypes.byref(wq), None, B, K, O, 1.0,
                                                                            out, ws, wsb, None)
    assert run(x, w, B, K, O, None) == ARG                                   # null out
    assert run(x, w, B, K, O, A + 3 * FAR + 1) == ARG                        # out not 2-byte aligned
    assert run(x, w, -1, K, O, A + 3 * FAR) == ARG
    assert run(x, w, B, K, -1, A + 3 * FAR) == ARG
    assert run(_q(data=None), w, B, K, O, A + 3 * FAR) == ARG                # null operand stream
    assert run(x, _q(n_param=7), B, K, O, A + 3 * FAR) == ARG                # neither per tensor nor per output feature
    assert run(_q(n_bits=9), w, B, K, O, A + 3 * FAR) == 1                   # QE_ERR_NBITS
    assert L_.qe_quantlinear_bf16(None, ctypes.byref(w), None, B, K, O, 1.0, A + 3 * FAR, None, 0, None) == ARG
    assert run(x, w, 0, K, O, None) == capi.QE_OK and run(x, w, B, K, 0, None) == capi.QE_OK      # empty: nothing to do
    # the two-pass form (here: out only 2-byte aligned) without its workspace is refused before any launch
    out2 = A + 3 * FAR + 2
    need = int(L_.qe_quantlinear_bf16_workspace_bytes(ctypes.byref(x), ctypes.byref(w), B, K, O, out2))
    assert need == B * O * 4 and int(L_.qe_quantlinear_bf16_path(ctypes.byref(x), ctypes.byref(w), B, K, O, out2)) == 0
    assert run(x, w, B, K, O, out2) == 6                                     # QE_ERR_WORKSPACE
    assert run(x, w, B, K, O, out2, A + 4 * FAR, need - 16) == 6             # too small
    assert run(x, w, B, K, O, out2, A + 4 * FAR + 4, need) == 6              # misaligned


@pytest.mark.parametrize("i", range(len(li.ROWS)))
def test_linear_bf16_path_follows_the_plan(i):
    """Fused wherever an MFMA form runs, O % 8 == 0 and out is 16-byte aligned -- every O % 64 == 0 among them; two passes
    (workspace: y in fp32) on the fp32 chain kernel, for any other O, a misaligned out and under QE_LIN_EPI=0.  The kernel
    is the one the F32 call takes."""
    B, K, O, env, form, note = li.ROWS[i]
    L_ = capi.lib()
    x, w = _q(), _q()
    ask = lambda out: (int(L_.qe_quantlinear_bf16_path(ctypes.byref(x), ctypes.byref(w), B, K, O, out)),
                       int(L_.qe_quantlinear_bf16_workspace_bytes(ctypes.byref(x), ctypes.byref(w), B, K, O, out)))
    with capi.knobs(**(env or {})):
        assert int(L_.qe_quantlinear_form(ctypes.byref(x), ctypes.byref(w), B, K, O, 1)) == form, note
        fused = form != 0 and O % 8 == 0
        if form != 0 and O % 64 == 0:
            assert fused
        assert ask(None) == ask(A + 3 * FAR) == ((1, 0) if fused else (0, B * O * 4)), note
        assert ask(A + 3 * FAR + 2) == (0, B * O * 4), note
    with capi.knobs(QE_LIN_EPI="0", **(env or {})):
        assert ask(None) == (0, B * O * 4), note


def _tiny():
    return PackedViT.from_state_dict(synthetic_state_dict("vit_tiny_test"), 4)


def test_vit_qkv_values():
    assert QKV == ("fp32", "bf16")
    m = _tiny()
    x = torch.zeros(1, 3, 32, 32)
    for kw in (dict(route="fused", attention="torch"), dict(route="fused", attention="engine"), dict(route="fused"),
               dict(route="layers", attention="engine_bf16"), dict(route="layers", attention="torch")):
        with pytest.raises(ValueError, match="qkv='bf16' needs"):
            m.forward(x, qkv="bf16", **kw)
        with pytest.raises(ValueError, match="qkv='bf16' needs"):
            m(x, qkv="bf16", **kw)
    for bad in ("fp16", "bfloat16", None):
        with pytest.raises(ValueError, match="qkv must be"):
            m.forward(x, route="fused", attention="engine_bf16", qkv=bad)


def test_vit_qkv_is_refused_before_any_launch(monkeypatch):
    def no_lib():
        raise AssertionError("the library was touched")
    m = _tiny()
    monkeypatch.setattr(capi, "lib", no_lib)
    with pytest.raises(ValueError, match="qkv='bf16' needs"):
        m.forward(torch.zeros(1, 3, 32, 32), route="fused", attention="engine", qkv="bf16")
    with pytest.raises(ValueError, match="qkv='bf16' needs"):
        m.block(m.blocks[0], torch.zeros(5, 64), 1, "layers", attention="engine_bf16", qkv="bf16")


def test_attention_dtypes_are_checked_before_the_library(monkeypatch):
    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(capi, "lib", no_lib)
    f, b = torch.zeros(4, 16), torch.zeros(4, 16, dtype=torch.bfloat16)
    for q, k, v in ((b, f, f), (f, b, f), (f, f, b), (b, b, f)):
        for precision in capi.PRECISIONS:
            with pytest.raises(ValueError, match="all be"):
                capi.attention(q, k, v, 1, 4, 1, precision=precision)
    with pytest.raises(ValueError, match="precision='bf16'"):
        capi.attention(b, b, b, 1, 4, 1, precision="fp32")
    with pytest.raises(ValueError, match="precision='bf16'"):
        capi.attention(b, b, b, 1, 4, 1)
    with pytest.raises(ValueError, match="all be"):
        capi.attention(f.half(), f.half(), f.half(), 1, 4, 1, precision="bf16")
