"""CPU: the host side of the bf16 context route -- qe_quantlinear_bf16_input, qe_attention_bf16_ctx and PackedViT's ctx
option: the exports, the path and workspace answers of the plan, the argument checks that are made before any device work
(pointers are plain integers here, nothing is launched, so no GPU is needed), and the option's ValueErrors."""
import ctypes

import pytest
import torch

import lin_bf16in_instances as bi
import test_qkv_bf16_cpu as host
from quantize_amd import capi
from quantize_amd.packed_vit import CTX, PackedViT, synthetic_state_dict

ARG, UNSUPPORTED = host.ARG, host.UNSUPPORTED
A, FAR = host.A, host.FAR
NEW = {"qe_quantlinear_bf16_input_path": ctypes.c_int, "qe_quantlinear_bf16_input_workspace_bytes": ctypes.c_size_t,
       "qe_quantlinear_bf16_input": ctypes.c_int, "qe_attention_bf16_ctx_path": ctypes.c_int, "qe_attention_bf16_ctx": ctypes.c_int}


def test_symbols_exported():
    L = capi.lib()
    for s, restype in NEW.items():
        assert s in capi.SYMBOLS and hasattr(L, s), s
        assert getattr(L, s).restype is restype, s


# ---- qe_attention_bf16_ctx ----
def test_ctx_path_answers():
    for d in range(16, 129, 16):
        for m, b, c in host.COMBOS:
            assert capi.attention_bf16_ctx_path(40, 45, 2, d, m, b, c) == 2, (d, m, b, c)
    for d in (8, 136, 20, 72, 144):
        assert capi.attention_bf16_ctx_path(40, 45, 2, d) == -1, d
    for L, S, H, d in ((0, 45, 2, 64), (40, 0, 2, 64), (40, 45, 0, 64), (40, 45, 2, 0), (-1, 45, 2, 64)):
        assert capi.attention_bf16_ctx_path(L, S, H, d) == -1, (L, S, H, d)


def _ctx_lists():
    """The 18 refused argument lists of tests/test_qkv_bf16_cpu.py for 2-byte q / k / v.  One of them places the mask 16
    bytes inside the END of out, an address that list computes on fp32 output elements; the same rule on this entry point's
    2-byte output elements is 16 bytes inside the end of a span half as long."""
    lists = host.bad_attention_lists(2)
    out = A + 3 * FAR
    span2 = 2 * 40 * 128 * 2
    fixed = []
    for name, args, want in lists:
        if name == "out overlaps mask":
            args = args[:16] + (out + span2 - 16,) + args[17:]
        fixed.append((name, args, want))
    return fixed


def test_ctx_bad_arguments_get_the_stored_entry_points_answer():
    L_ = capi.lib()
    stored, ctx = host.bad_attention_lists(2), _ctx_lists()
    assert len(stored) == len(ctx) == 18
    for (name, args_s, want), (_, args_c, _) in zip(stored, ctx):
        a, b = L_.qe_attention_bf16_stored(*args_s), L_.qe_attention_bf16_ctx(*args_c)
        assert a == want and b == want, (name, a, b, want)
    for d in (8, 136, 20, 72, 144):
        args = (A, A + FAR, A + 2 * FAR, A + 3 * FAR, 2, 40, 45, 2, d, 40, 1, 45, 1, 40, 1, 0.125, None, 0, 0, None, 0, None)
        assert L_.qe_attention_bf16_ctx(*args) == UNSUPPORTED, d


def test_ctx_out_is_checked_on_two_byte_elements():
    """Null and misaligned pointers (2-byte alignment is not enough: the rows move 16 and 8 bytes at a time), and out
    against q / k / v with every span, out's included, taken on 2-byte elements: the last 16 bytes of each span still count."""
    L_ = capi.lib()
    good = [A, A + FAR, A + 2 * FAR, A + 3 * FAR]
    tail = (2, 40, 45, 2, 64, 40, 1, 45, 1, 40, 1, 1.0, None, 0, 0, None, 0, None)
    for i in range(4):
        for bad in (None, good[i] + 2, good[i] + 8):
            p = list(good)
            p[i] = bad
            assert L_.qe_attention_bf16_ctx(*p, *tail) == ARG, (i, bad)
    out = A + 3 * FAR
    span_out2 = 2 * 40 * 128 * 2                       # N L E 2-byte elements
    span_v2 = 2 * 45 * 128 * 2
    for name, p in (("out is k", [A, out, A + 2 * FAR, out]),
                    ("q starts inside out's last 16 bytes", [out + span_out2 - 16, A + FAR, A + 2 * FAR, out]),
                    ("out starts inside v's last 16 bytes", [A, A + FAR, out - span_v2 + 16, out]),
                    ("out ends inside k", [A, out + span_out2 - 32, A + 2 * FAR, out])):
        assert L_.qe_attention_bf16_ctx(*p, *tail) == ARG, name


def test_attention_out_dtype_is_checked_before_the_library(monkeypatch):
    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(capi, "lib", no_lib)
    f, b = torch.zeros(4, 16), torch.zeros(4, 16, dtype=torch.bfloat16)
    for precision in capi.PRECISIONS:
        with pytest.raises(ValueError, match="allowed only with torch.bfloat16 q / k / v"):
            capi.attention(f, f, f, 1, 4, 1, precision=precision, out_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="allowed only with torch.bfloat16 q / k / v"):
        capi.attention(b, b, f, 1, 4, 1, precision="bf16", out_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="out_dtype must be"):
        capi.attention(b, b, b, 1, 4, 1, precision="bf16", out_dtype=torch.float16)
    with pytest.raises(ValueError, match="precision='bf16'"):
        capi.attention(b, b, b, 1, 4, 1, out_dtype=torch.bfloat16)


# ---- qe_quantlinear_bf16_input ----
def _w(n_param=1, data=A + FAR, n_bits=8):
    return capi.QeQParam(data, n_bits, 1, A + 2 * FAR, A + 3 * FAR, n_param)


X, OUT, RES, WS = A, A + 4 * FAR, A + 5 * FAR, A + 6 * FAR


def _run(x, w, B, K, O, res, out, ws=None, wsb=0):
    return capi.lib().qe_quantlinear_bf16_input(x, None if w is None else ctypes.byref(w), None, B, K, O, res, out, ws, wsb, None)


def test_linear_bf16_input_argument_checks():
    w = _w()
    B, K, O = 64, 128, 256
    assert _run(None, w, B, K, O, None, OUT) == ARG                          # null x
    assert _run(X, w, B, K, O, None, None) == ARG                            # null out
    assert _run(X, None, B, K, O, None, OUT) == ARG                          # null weights
    assert _run(X, _w(data=None), B, K, O, None, OUT) == ARG
    assert _run(X + 1, w, B, K, O, None, OUT) == ARG                         # odd addresses
    assert _run(X, w, B, K, O, None, OUT + 1) == ARG
    assert _run(X, w, B, K, O, RES + 1, OUT) == ARG
    assert _run(X, w, B, K, O, None, OUT + 2) == ARG                         # fp32 out on a 2-byte boundary
    assert _run(X, w, -1, K, O, None, OUT) == ARG
    assert _run(X, w, B, -1, O, None, OUT) == ARG
    assert _run(X, w, B, K, -1, None, OUT) == ARG
    assert _run(X, _w(n_param=7), B, K, O, None, OUT) == ARG                 # neither per tensor nor per output feature
    assert _run(X, _w(n_bits=9), B, K, O, None, OUT) == 1                    # QE_ERR_NBITS
    # overlaps: out with x (2-byte elements), out with a residual that is not out itself
    assert _run(X, w, B, K, O, None, X) == ARG
    assert _run(X, w, B, K, O, None, X + B * K * 2 - 16) == ARG
    assert _run(OUT + B * O * 4 - 16, w, B, K, O, None, OUT) == ARG
    assert _run(X, w, B, K, O, OUT + 16, OUT) == ARG
    assert _run(X, w, B, K, O, OUT - 16, OUT) == ARG
    # empty problems: nothing to do (out == residual in place passes the checks)
    assert _run(X, w, 0, K, O, OUT, OUT) == capi.QE_OK and _run(X, w, B, K, 0, OUT, OUT) == capi.QE_OK
    # path 0 (here: K % 32 != 0) without its workspace is refused before any launch; out == residual is accepted up to there
    K = 100
    need = int(capi.lib().qe_quantlinear_bf16_input_workspace_bytes(X, ctypes.byref(w), B, K, O))
    assert need == B * K * 4 + B * O * 4
    for res, short in ((None, B * K * 4 - 16), (OUT, need - 16), (RES, need - 16)):   # the query sizes for the residual form
        assert _run(X, w, B, K, O, res, OUT) == 6                            # QE_ERR_WORKSPACE
        assert _run(X, w, B, K, O, res, OUT, WS, short) == 6                 # too small
        assert _run(X, w, B, K, O, res, OUT, WS + 4, need) == 6              # misaligned


@pytest.mark.parametrize("row", bi.ROWS, ids=bi.row_id)
def test_linear_bf16_input_path_follows_the_plan(row):
    """Path 1 and no workspace for 8-bit weights, K % 32 == 0 and an aligned x; else path 0 and B K 4 bytes for the widened
    rows plus what the float-input plan of the widened problem asks for.  QE_LIN_F32_MFMA=0 sends every row to path 0."""
    B, K, O, w_bits, off, path, note = row
    L_ = capi.lib()
    w = _w(n_bits=w_bits)
    ask = lambda: (int(L_.qe_quantlinear_bf16_input_path(X + off, ctypes.byref(w), B, K, O)),
                   int(L_.qe_quantlinear_bf16_input_workspace_bytes(X + off, ctypes.byref(w), B, K, O)))
    inner = lambda: int(L_.qe_quantlinear_float_input_residual_workspace_bytes(None, ctypes.byref(w), B, K, O))
    assert (B * K * 4) % 16 == 0
    assert ask() == ((1, 0) if path == 1 else (0, B * K * 4 + inner())), note
    with capi.knobs(QE_LIN_F32_MFMA="0"):
        assert inner() == B * O * 4                     # the chain kernel: the residual form takes two passes
        assert ask() == (0, B * K * 4 + B * O * 4), note
    assert ask()[0] == path


def test_capi_linear_bf16_input_wants_contiguous_bf16_rows(monkeypatch):
    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(capi, "lib", no_lib)
    for x in (torch.zeros(4, 32), torch.zeros(4, 32, dtype=torch.float16), torch.zeros(4, 32, dtype=torch.bfloat16),
              torch.zeros(128, dtype=torch.bfloat16), None):
        with pytest.raises(ValueError, match="contiguous torch.bfloat16"):   # the CPU bf16 tensor: not a device tensor
            capi.quantlinear_bf16_input(x, None, None, 8)


# ---- PackedViT ----
def _tiny():
    return PackedViT.from_state_dict(synthetic_state_dict("vit_tiny_test"), 4)


def test_vit_ctx_values(monkeypatch):
    assert CTX == ("fp32", "bf16")
    m = _tiny()
    x = torch.zeros(1, 3, 32, 32)

    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(capi, "lib", no_lib)
    good = dict(route="fused", attention="engine_bf16", qkv="bf16")
    for change in (dict(route="layers", qkv="fp32"), dict(attention="engine", qkv="fp32"), dict(attention="torch", qkv="fp32"),
                   dict(qkv="fp32")):
        kw = dict(good, **change)
        with pytest.raises(ValueError, match="ctx='bf16' needs"):
            m.forward(x, ctx="bf16", **kw)
        with pytest.raises(ValueError, match="ctx='bf16' needs"):
            m(x, ctx="bf16", **kw)
    with pytest.raises(ValueError, match="ctx='bf16' needs"):
        m.forward(x, ctx="bf16")                                              # the defaults: attention="torch"
    for bad in ("fp16", "bfloat16", None):
        with pytest.raises(ValueError, match="ctx must be"):
            m.forward(x, ctx=bad, **good)
    with pytest.raises(ValueError, match="ctx='bf16' needs"):
        m.block(m.blocks[0], torch.zeros(5, 64), 1, "fused", attention="engine_bf16", qkv="fp32", ctx="bf16")
