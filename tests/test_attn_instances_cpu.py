"""CPU: the attention instance table (tests/attn_instances.py) reaches every instance attn_run can launch, names them as
the source instantiates them, and its cases are sound before any GPU sees them: every query row keeps a visible key, the
float64 reference is finite everywhere (no element is left out of a comparison), and that reference agrees with torch's own
float64 scaled_dot_product_attention on every row's operands -- the new generators (pad_mid, alibi, holes3d's keep)
included."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attention_ref as ar
import attn_instances as ai
import test_attention_gpu as base
from quantize_amd import capi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_dispatchable_instance_is_covered():
    every = ai.dispatchable()
    assert len(every) == 144
    assert len({i for i in every if i[0] == ai.MFMA}) == 112 and len({i for i in every if i[0] == ai.VALU}) == 32
    missing = every - ai.covered()
    assert not missing, "no row reaches %s" % sorted(ai.kernel_name(i) for i in missing)
    assert ai.covered() == every
    assert len({ai.kernel_name(i) for i in every}) == 144


def test_rows_cover_the_sizes_and_both_mask_kinds():
    assert {r[1] for r in ai.ROWS if r[0] == ai.MFMA} == set(range(16, 129, 16))
    assert {r[1] for r in ai.ROWS if r[0] == ai.VALU} == {20, 72, 136, 256}
    assert {r[2] for r in ai.ROWS} == {44, 45}
    for size in list(ai.MFMA_D) + list(ai.VALU_D):
        rows = ai.rows_of(ai.MFMA if size in ai.MFMA_D else ai.VALU, size)
        assert {r[6] for r in rows} == {None, "additive2d", "holes3d"}, size
        assert len(rows) == (14 if size in ai.MFMA_D else 8)


def test_instance_restates_the_dispatch():
    """kVec4 needs an additive operand, S % 4 == 0 and both strides % 4 == 0; the VALU kernel never carries it."""
    assert ai.instance(ai.MFMA, 64, 44, True, False, False, 0, 0) == (ai.MFMA, 64, ai.kVec4 | ai.kMask)
    assert ai.instance(ai.MFMA, 64, 44, True, False, False, 40 * 44 + 1, 0) == (ai.MFMA, 64, ai.kMask)
    assert ai.instance(ai.MFMA, 64, 44, True, True, True, 0, 40 * 44 + 2) == (ai.MFMA, 64, 7)
    assert ai.instance(ai.MFMA, 64, 45, False, True, False) == (ai.MFMA, 64, ai.kBias)
    assert ai.instance(ai.MFMA, 48, 44, False, False, True) == (ai.MFMA, 48, ai.kCausal)
    assert ai.instance(ai.MFMA, 48, 44, False, False, False) == (ai.MFMA, 48, 0)
    assert ai.instance(ai.VALU, 256, 44, True, True, True) == (ai.VALU, 4, 7)
    assert ai.instance(ai.VALU, 193, 44, False, True, False) == (ai.VALU, 4, ai.kBias)
    assert ai.instance(ai.VALU, 64, 45, False, False, False) == (ai.VALU, 1, 0)


def test_kernel_names_match_the_source():
    """The mode bits and the head sizes of the Python table have their counterpart in the one place the source keeps each:
    the enum and the head-size switch of qe_attention_common.hpp, which both units launch their 32-row kernel through."""
    read = lambda name: open(os.path.join(REPO, "quantize_amd", "csrc", name)).read()
    common, fp32, bf16 = read("qe_attention_common.hpp"), read("qe_attention.hip"), read("qe_attention_bf16.hip")
    assert re.search(r"enum : int \{ kMask = 1, kBias = 2, kCausal = 4, kVec4 = 8 \}", common)
    for D in ai.MFMA_D:
        assert "attn_launch_d<CORE, %d, MODE>" % D in common
    assert "launch_instance<CORE::template kernel<D, MODE>>" in common
    assert re.search(r"kernel = &attn_mfma_kernel<D, MODE>", fp32) and re.search(r"attn_valu_kernel<NO, MODE>", fp32)
    assert re.search(r"kernel = &attn_bf16_kernel<D, MODE>", bf16)
    for src, core in ((fp32, "AttnMfma"), (bf16, "AttnBf16")):
        assert '#include "qe_attention_common.hpp"' in src and "attn_launch_rows32<%s, " % core in src
        assert "attn_dispatch_mode(mode" in src and "enum" not in src      # no mode bits or mode switch of its own
    assert ai.kernel_name((ai.MFMA, 112, 13)) == "attn_mfma_kernel<112, 13>"
    assert ai.kernel_name((ai.VALU, 4, 0)) == "attn_valu_kernel<4, 0>"


def test_rows_take_the_kernel_they_name():
    for row in ai.ROWS:
        kernel, d, S, m, b, c, _ = row
        assert capi.attention_masked_path(ai.L, S, ai.H, d, m, b, c) == (1 if kernel == ai.MFMA else 0), row
        with capi.knobs(QE_ATTN="0"):
            assert capi.attention_masked_path(ai.L, S, ai.H, d, m, b, c) == 0, row


def _sdpa64(q, k, v, m):
    t = lambda a: torch.from_numpy(a.astype(np.float64)).transpose(1, 2)                  # (N, H, T, d)
    return F.scaled_dot_product_attention(t(q), t(k), t(v), attn_mask=torch.from_numpy(m).double()).transpose(1, 2).numpy()


@pytest.mark.parametrize("kernel,size", [(ai.MFMA, D) for D in ai.MFMA_D] + [(ai.VALU, no) for no in ai.VALU_D],
                         ids=lambda v: str(v))
def test_rows_are_sound(kernel, size):
    """Visible key in every query row, finite float64 reference, nothing left out, and ref64 == torch float64 SDPA."""
    left_out = total = 0
    for row in ai.rows_of(kernel, size):
        _, d, S, m, b, c, kind = row
        ops = ai.operands(row)
        assert set(ops) == {n for n, on in (("mask", m), ("key_bias", b), ("causal", c)) if on}, row
        if m:
            assert ops["mask"].shape == ((ai.L, S) if kind == "additive2d" else (ai.N * ai.H, ai.L, S)), row
        merged = ar.merged(ai.N, ai.H, ai.L, S, **ops)
        assert ar.visible(merged).all(), row
        if b:       # the first key tile is blank for at least one image (all but its first a_n <= 7 keys under causal)
            assert np.isinf(ops["key_bias"][:, 7 if c else 0:32]).all(axis=1).any(), row
        q, k, v = base._inputs(ai.N, ai.L, S, ai.H, d, "moderate", seed=d + S)
        ref = ar.ref64(q, k, v, **ops)
        assert np.isfinite(ref).all(), row
        left_out += int((~np.isfinite(ref)).sum())
        total += ref.size
        err = float(np.abs(ref - _sdpa64(q, k, v, merged)).max())
        assert err <= 1e-12, (row, err)
    assert total > 0 and left_out / total == 0.0


@pytest.mark.parametrize("d,S,step", [(16, 44, 32), (48, 45, 32), (64, 44, 32), (128, 45, 32), (20, 76, 64), (256, 77, 64)])
def test_peaky_cases_are_sound(d, S, step):
    """The masked peaky cases.  Unmasked, every |score| is <= 60 and every row reaches it; no operand lifts a score (every
    additive value is <= 0: what the operands add is at most 30 towards the side a -inf entry already lies on), so the
    total score never exceeds 60; alibi's largest magnitude is 30 and, alone or under causal, it moves the maximum of at
    least a quarter of the rows to another key tile (`step` keys: 32 in the MFMA kernel, 64 in the VALU kernel) than the
    unmasked one; the yardstick is finite and agrees with torch's float64 SDPA."""
    q, k, v = ai.peaky_inputs(d, S)
    s = np.einsum("nlhd,nshd->nhls", q.astype(np.float64), k.astype(np.float64)) * d ** -0.5
    assert np.abs(s).max() <= 60.0 * (1 + 1e-6) and (np.abs(s).max(-1) >= 60.0 * (1 - 1e-6)).all()
    q30, _, _ = ai.peaky_inputs(d, S, peak=30.0)
    assert np.allclose(q30, 0.5 * q, rtol=1e-6, atol=0)
    al = ar.alibi(ai.H, ai.L, S)
    assert al.shape == (ai.H, ai.L, S) and al.max() == 0.0 and abs(al.min() + 30.0) < 1e-5
    cases = ai.peaky_operands(S)
    assert set(cases) == {"alibi", "pad_front", "causal+alibi"}
    for name, ops in cases.items():
        merged = ar.merged(ai.N, ai.H, ai.L, S, **ops)
        assert (merged <= 0).all() and ar.visible(merged).all(), name
        assert (s + merged).max() <= 60.0 * (1 + 1e-6)
        ref = ar.ref64(q, k, v, **ops)
        assert np.isfinite(ref).all(), name
        assert float(np.abs(ref - _sdpa64(q, k, v, merged)).max()) <= 1e-12, name
        moved = ((s + merged).argmax(-1) // step != s.argmax(-1) // step).mean()
        print("d %d S %d %s: row maximum in another %d-key tile for %.0f%% of the rows" % (d, S, name, step, 100 * moved))
        if "mask" in ops:
            assert moved >= 0.25, (name, moved)


@pytest.mark.parametrize("S", [35, 40, 44, 45, 300])
def test_pad_mid_keeps_key_0_and_blanks_the_first_tile(S):
    bias = ar.pad_mid(3, S, np.random.RandomState(S))
    assert np.isfinite(bias[:, 0]).all() and np.isinf(bias[:, 7:33]).all() and np.isfinite(bias[:, -1]).all()
    assert ar.visible(ar.merged(3, 2, S, S, key_bias=bias, causal=True)).all()
