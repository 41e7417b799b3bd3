"""CPU: the bf16 attention core's host side (qe_attention_bf16_path, capi.attention's precision argument, the ViT's
attention values), the two lane maps of attn_bf16_kernel emulated lane by lane against float64, and the soundness of every
case tests/test_attention_bf16_gpu.py runs, before a GPU sees it: every query row keeps a visible key, the float64 reference
on the rounded inputs is finite everywhere (0 elements left out), it agrees with torch's float64 SDPA within 1e-12, and a
numpy emulation of the numerics contract (tests/attn_bf16_ref.py: 32-key tiles, online softmax, p through torch.bfloat16)
stays within HALF the GPU bound (2^-8 + 1e-5) max|v^|, so the bound is reachable."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attention_ref as ar
import attn_bf16_ref as br
import attn_instances as ai
import test_attention_gpu as base
from quantize_amd import capi, packed_vit

COMBOS = [(m, b, c) for m in (0, 1) for b in (0, 1) for c in (0, 1)]
MFMA_ROWS = [r for r in ai.ROWS if r[0] == ai.MFMA]


def test_path_answers():
    for knob in (None, "0"):
        with capi.knobs(QE_ATTN=knob):
            for d in range(16, 129, 16):
                for m, b, c in COMBOS:
                    assert capi.attention_bf16_path(40, 45, 2, d, m, b, c) == 2, (knob, d, m, b, c)
            for d in (20, 72, 136, 144):
                for m, b, c in COMBOS:
                    assert capi.attention_bf16_path(40, 45, 2, d, m, b, c) == -1, (knob, d, m, b, c)
            for L, S, H, d in ((0, 45, 2, 64), (40, 0, 2, 64), (40, 45, 0, 64), (40, 45, 2, 0), (-1, 45, 2, 64), (40, 45, 2, -16)):
                assert capi.attention_bf16_path(L, S, H, d) == -1, (knob, L, S, H, d)
            # the fp32 entry points keep their own answers
            assert capi.attention_path(40, 45, 2, 64) == (1 if knob is None else 0)


def test_precision_is_checked_before_the_library(monkeypatch):
    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(capi, "lib", no_lib)
    x = torch.zeros(4, 16)
    for bad in ("fp16", "bfloat16", None, "BF16"):
        with pytest.raises(ValueError, match="precision"):
            capi.attention(x, x, x, 1, 4, 1, precision=bad)


def test_vit_attention_values():
    assert packed_vit.ATTENTION == ("torch", "engine", "engine_bf16")
    assert "engine_bf16" in packed_vit.ATTENTION
    packed_vit._check_attention("engine_bf16")
    for bad in ("sdpa", "flash", "bf16"):
        with pytest.raises(ValueError, match="engine_bf16"):
            packed_vit._check_attention(bad)


def test_bf16_rounds_to_nearest_even():
    x = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.0, 2.0 ** -8], np.float32)
    assert np.array_equal(br.bf16(x), np.array([1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -3.0, 2.0 ** -8], np.float32))


@pytest.mark.parametrize("D", ai.MFMA_D)
def test_lane_maps_against_float64(D):
    """One wave's tile through the fragments as the kernel indexes them and the MFMA's operand layout, on integers (every
    product and sum exact): S^T decodes to q k^T and O to p v, element for element.  Asymmetric operands: a swapped or
    permuted k index on one side changes almost every element."""
    rng = np.random.RandomState(D)
    q, k, v = (rng.randint(-8, 9, size=(32, D)).astype(np.float64) for _ in range(3))
    p = rng.randint(0, 5, size=(32, 32)).astype(np.float64)
    scores, out = br.wave_tile(q, k, v, p)
    assert np.array_equal(scores, q @ k.T)
    assert np.array_equal(out, p @ v)
    # the natural k order on V alone (element j = key 8 h + j of the step) is a different result
    assert not np.array_equal(out, (p[:, np.r_[0:4, 8:12, 4:8, 12:16, 16:20, 24:28, 20:24, 28:32]]) @ v)


def _sdpa64(q, k, v, m):
    t = lambda a: torch.from_numpy(a.astype(np.float64)).transpose(1, 2)                  # (N, H, T, d)
    return F.scaled_dot_product_attention(t(q), t(k), t(v), attn_mask=torch.from_numpy(m).double(),
                                          scale=1.0).transpose(1, 2).numpy()


def _sound(qh, kh, vh, ops, what):
    """The three soundness checks of one case; returns (elements, elements left out, emulation error / bound)."""
    N, L, H, d = qh.shape
    S = kh.shape[1]
    merged = ar.merged(N, H, L, S, **ops)
    assert ar.visible(merged).all(), what
    ref = br.ref64(qh, kh, vh, **ops)
    assert np.isfinite(ref).all(), what
    err = float(np.abs(ref - _sdpa64(qh, kh, vh, merged)).max())
    assert err <= 1e-12, (what, err)
    emu = br.emulate(qh, kh, vh, **ops)
    assert np.isfinite(emu).all(), what
    e = float(np.abs(emu - ref).max()) / br.bound(vh)
    assert e <= 0.5, (what, e)
    return ref.size, int((~np.isfinite(ref)).sum()), e


@pytest.mark.parametrize("D", ai.MFMA_D)
def test_instance_rows_are_sound(D):
    """(a): the 14 rows of one head size, moderate inputs."""
    total = left_out = 0
    worst = 0.0
    rows = [r for r in MFMA_ROWS if r[1] == D]
    assert len(rows) == 14
    for row in rows:
        _, d, S, m, b, c, _ = row
        q, k, v = base._inputs(ai.N, ai.L, S, ai.H, d, "moderate", seed=d + S)
        n, out, e = _sound(*br.rounded(q, k, v), ai.operands(row), ai.row_id(row))
        total, left_out, worst = total + n, left_out + out, max(worst, e)
    print("d %d: emulation within %.3f of the bound" % (D, worst))
    assert total > 0 and left_out == 0


def test_the_table_has_112_rows():
    assert len(MFMA_ROWS) == 112 and {ai.row_instance(r) for r in MFMA_ROWS} == {i for i in ai.dispatchable() if i[0] == ai.MFMA}


@pytest.mark.parametrize("regime", ["moderate", "peaky"])
@pytest.mark.parametrize("case", br.CASES, ids=lambda c: "N%d-L%d-S%d-H%d-d%d" % c)
def test_shape_cases_are_sound(case, regime):
    """(b): the d % 16 == 0 cases of test_attention_gpu.CASES plus two workgroups per head, unmasked and causal."""
    assert set(br.CASES) == {c for c in base.CASES if c[4] % 16 == 0} | {(1, 300, 300, 2, 64)}
    N, L, S, H, d = case
    q, k, v = base._inputs(N, L, S, H, d, regime, seed=sum(case))
    qh, kh, vh = br.rounded(q, k, v)
    left_out = 0
    for ops in ({}, dict(causal=True)):
        n, out, e = _sound(qh, kh, vh, ops, (case, regime, sorted(ops)))
        left_out += out
        print("%s %s %s: emulation within %.3f of the bound" % (case, regime, sorted(ops), e))
    assert left_out == 0


@pytest.mark.parametrize("bias", [False, True], ids=["mask", "mask+pad_front"])
@pytest.mark.parametrize("d", br.EXACT_D)
def test_exact_cases_are_exact_in_the_emulation(d, bias):
    """(c): every visible p is 1, so the contract's arithmetic is exact and the emulation returns float32(sum) /
    float32(count) bit for bit; with pad_front at least one image's whole first key tile is blank."""
    for L, S in br.EXACT_LS:
        q, k, v, ops, want = br.exact_case(d, L, S, bias)
        assert np.isfinite(want).all() and np.abs(v).max() == 8 and np.array_equal(br.bf16(v), v)
        if bias:
            assert np.isinf(ops["key_bias"][:, :32]).all(axis=1).any()
        qh, kh, vh = br.rounded(q, k, v)
        assert np.array_equal(br.emulate(qh, kh, vh, **ops), want), (d, L, S)
        assert float(np.abs(br.ref64(qh, kh, vh, **ops) - want).max()) <= 1e-6


def test_bad_arguments_get_the_fp32_entry_points_answer():
    """qe_attention_bf16 and qe_attention_masked make their argument checks in one function (attn_prepare of
    qe_attention_common.hpp), each with its own path function's answer: for every argument list that is refused before any
    device work, both return the same code.  Pointers are plain integers here; nothing is launched, so no GPU is needed."""
    L_ = capi.lib()
    A, FAR = 1 << 20, 1 << 44                 # 16-byte aligned, far enough apart for any span below
    ARG, UNSUPPORTED = 4, capi.QE_ERR_UNSUPPORTED
    good = dict(q=A, k=A + FAR, v=A + 2 * FAR, out=A + 3 * FAR, N=2, L=40, S=45, H=2, d=64, q_rn=40, q_rt=1, kv_rn=45, kv_rt=1,
                o_rn=40, o_rt=1, scale=0.125, mask=None, mask_sn=0, mask_sh=0, key_bias=None, causal=0)
    span = 2 * 40 * 128 * 4                   # bytes of q / out
    bad = [("N = 0", dict(N=0), ARG), ("L < 0", dict(L=-1), ARG), ("d = 0", dict(d=0), ARG), ("negative stride", dict(kv_rt=-1), ARG),
           ("negative out stride", dict(o_rn=-40), ARG), ("null k", dict(k=None), ARG), ("misaligned q", dict(q=A + 4), ARG),
           ("misaligned out", dict(out=A + 3 * FAR + 8), ARG), ("negative mask stride", dict(mask=A + 4 * FAR, mask_sh=-4), ARG),
           ("stride without mask", dict(mask_sn=4), ARG), ("misaligned mask", dict(mask=A + 4 * FAR + 4), ARG),
           ("misaligned key_bias", dict(key_bias=A + 5 * FAR + 4), ARG), ("out is q", dict(out=A), ARG),
           ("out overlaps the end of v", dict(out=A + 2 * FAR + 2 * 45 * 128 * 4 - 16), ARG),
           ("out overlaps mask", dict(mask=A + 3 * FAR + span - 16), ARG),
           ("out overlaps key_bias", dict(key_bias=A + 3 * FAR - 2 * 45 * 4 + 16), ARG),
           ("d > 256", dict(d=272), UNSUPPORTED),
           ("more rows than a grid", dict(N=1 << 20, H=1 << 10, L=32, S=32, d=16, q_rn=32, kv_rn=32, o_rn=32), UNSUPPORTED)]
    for name, change, want in bad:
        a = dict(good, **change)
        args = (a["q"], a["k"], a["v"], a["out"], a["N"], a["L"], a["S"], a["H"], a["d"], a["q_rn"], a["q_rt"], a["kv_rn"], a["kv_rt"],
                a["o_rn"], a["o_rt"], a["scale"], a["mask"], a["mask_sn"], a["mask_sh"], a["key_bias"], a["causal"], None)
        fp32, bf16 = L_.qe_attention_masked(*args), L_.qe_attention_bf16(*args)
        assert fp32 == want and bf16 == want, (name, fp32, bf16, want)
    # where the two differ on purpose: a head size only the fp32 VALU kernel takes is answered on the host as well
    for d in (20, 72, 136, 144, 8):
        args = (A, A + FAR, A + 2 * FAR, A + 3 * FAR, 2, 40, 45, 2, d, 40, 1, 45, 1, 40, 1, 0.125, None, 0, 0, None, 0, None)
        assert L_.qe_attention_bf16(*args) == UNSUPPORTED, d
