"""CPU: tests/arena.py does what the memory-contract tests rely on, and the table of tests/mem_cases.py reaches the kernels
and size queries it is meant to reach (through the host-only plan queries, as the *_instances_cpu tests do)."""
import os
import re

import pytest
import torch

import arena
import lin_instances as li
import mem_cases as mc
from quantize_amd import capi


# ---- arena self-tests on CPU tensors ---------------------------------------------------------------------------------
def _raw_of(a, name):
    return [b for b in a.bufs if b.name == name][0]


@pytest.mark.parametrize("fill", arena.FILLS)
def test_guard_is_a_condition(fill):
    assert arena.GUARD % 256 == 0 and arena.GUARD >= 4096 and arena.GUARD >= 320 * 4 and arena.GUARD >= 256 * 16
    a = arena.Arena("cpu", fill)
    x = a.place(torch.arange(10, dtype=torch.float32), name="x")
    y = a.blank((3, 5), torch.bfloat16, name="y")
    st = a.status()
    assert x.data_ptr() % 256 == 0 and y.data_ptr() % 256 == 0
    assert torch.equal(x, torch.arange(10, dtype=torch.float32)) and x.dtype == torch.float32
    assert y.shape == (3, 5) and bool((y.view(torch.uint8) == fill).all())
    assert int(st.item()) == 0 and st.dtype == torch.int32
    for b in a.bufs:
        assert b.start >= arena.GUARD and b.raw.numel() - b.start - b.nbytes >= arena.GUARD
    a.check("untouched")
    with pytest.raises(AssertionError):
        arena.Arena("cpu", 0xA5)


def test_fills_mean_what_the_tests_assume():
    a = arena.Arena("cpu", 0xFF)
    assert torch.isnan(a.blank(4, torch.float32)).all() and torch.isnan(a.blank(4, torch.bfloat16)).all()
    assert int(a.blank(1, torch.uint8)) == 255 and int(a.blank(1, torch.int8)) == -1
    z = arena.Arena("cpu", 0x00)
    assert bool((z.blank(4, torch.float32) == 0).all()) and int(z.blank(1, torch.uint8)) == 0


@pytest.mark.parametrize("fill", arena.FILLS)
@pytest.mark.parametrize("where", [-1, -arena.GUARD, 40, 40 + arena.GUARD - 1])
def test_flipped_guard_byte_is_reported(fill, where):
    """One byte right before, at the far end of the front guard, right behind and at the far end of the back guard."""
    a = arena.Arena("cpu", fill)
    a.place(torch.zeros(3), name="other")
    a.blank(40, torch.uint8, name="the codes")
    b = _raw_of(a, "the codes")
    front = b.start + where
    if where == -arena.GUARD:                        # the guard's first byte: GUARD plus the alignment pad in front
        front, where = 0, -b.start
    b.raw[front] ^= 0x5A
    with pytest.raises(arena.ArenaError) as e:
        a.check("case 7")
    msg = str(e.value)
    assert "case 7" in msg and "'the codes'" in msg and ("offset %d " % where) in msg
    assert ("front guard" if where < 0 else "back guard") in msg


def test_modified_input_is_reported_unless_in_place():
    a = arena.Arena("cpu", 0xFF)
    x = a.place(torch.ones(7), name="x")
    r = a.place(torch.ones(7), name="residual", inplace=True)
    r += 1
    a.check("in place")
    x[5] = 2.0
    with pytest.raises(arena.ArenaError) as e:
        a.check("case 9")
    assert "input 'x' modified" in str(e.value) and "offset 22" in str(e.value)        # 2.0f differs from 1.0f from byte 2 on


def test_skipped_output_byte_shows_in_the_two_fill_comparison():
    """An op that leaves one output byte alone: whatever the plain result holds there, one of the two pre-fills differs."""
    src = torch.arange(1, 33, dtype=torch.uint8)

    def op(out, skip):
        keep = out[skip].clone()
        out.copy_(src)
        out[skip] = keep

    for legal in (0x00, 0xFF, 0xA5):                 # the plain buffer's left-over at the skipped byte: any value
        plain = torch.full((32,), legal, dtype=torch.uint8)
        op(plain, 13)
        same = []
        for fill in arena.FILLS:
            a = arena.Arena("cpu", fill)
            out = a.blank(32, torch.uint8, name="out")
            op(out, 13)
            a.check("skip")
            same.append(arena.same_bytes(out, plain))
        assert not all(same), legal
    whole = [arena.Arena("cpu", f).blank(32, torch.uint8) for f in arena.FILLS]
    for w in whole:
        w.copy_(src)
    assert arena.same_bytes(whole[0], src) and arena.same_bytes(whole[1], src)


def test_same_bytes_counts_nan_patterns():
    a = torch.tensor([float("nan")])
    b = a.clone()
    assert arena.same_bytes(a, b)
    b.view(torch.int32)[0] ^= 1
    assert torch.isnan(b).all() and not arena.same_bytes(a, b)


@pytest.mark.parametrize("off,dtype", [(0, torch.float32), (1, torch.uint8), (2, torch.bfloat16), (4, torch.float32), (16, torch.uint8)])
def test_off_gives_the_promised_residue(off, dtype):
    a = arena.Arena("cpu", 0x00)
    t = a.place(torch.ones(9, dtype=dtype), off=off)
    o = a.blank(9, dtype, off=off)
    assert t.data_ptr() % 256 == off and o.data_ptr() % 256 == off
    a.check("off")
    if dtype != torch.uint8:
        with pytest.raises(AssertionError):
            a.place(torch.ones(9, dtype=dtype), off=1)


# ---- coverage --------------------------------------------------------------------------------------------------------
def _hosts(family):
    return [(c, c.host()) for c in mc.cases(family)]


def test_linear_entries_reach_every_instance():
    every = li.every_instance()
    assert len(every) == 26
    got = set()
    for c, (inst, ws) in _hosts("linear"):
        got |= inst
    assert not every - got, "no linear entry reaches %s" % sorted(every - got)
    fns = {c.fn for c in mc.cases("linear")}
    assert fns == {"qe_quantlinear", "qe_quantlinear_requant", "qe_quantlinear_residual", "qe_quantlinear_bf16",
                   "qe_quantlinear_float_input", "qe_quantlinear_float_input_residual", "qe_quantlinear_bf16_input"}
    # both packed streams of the odd-tail rows end mid-byte, one of them with per-row scales
    odd = [c for c in mc.cases("linear") if getattr(c, "key", ("", 0))[0] == "odd"]
    assert {c.per_row for c in odd} == {False, True} and all((c.B * c.K * 3) % 8 and (c.O * c.K * 5) % 8 for c in odd)


def test_conv_entries_reach_what_the_instance_table_covers():
    import conv_instances as ci
    got = set()
    for c, (inst, ws) in _hosts("conv"):
        got |= inst
    missing = ci.covered() - got
    assert not missing, "no conv entry reaches %s" % sorted(missing, key=str)
    # every distinct fp32 instance of the table through its cheapest row, in all four entry points where they apply
    assert {c.inst for c in mc.cases("conv")} == {r[4] for r in ci.ROWS}
    assert {c.fn for c in mc.cases("conv")} == {"qe_quantconv2d", "qe_quantconv2d_prepared", "qe_quantconv2d_requant_prepared",
                                                "qe_quantconv2d_residual_prepared"}
    print("conv rows %d of %d, entries %d" % (len(mc._conv_rows()), len(ci.ROWS), len(mc.cases("conv"))))


def test_resident_tile_entries_reach_every_base_instance_in_its_epilogues():
    import pwr_instances as pi
    got = set()
    for c, (inst, ws) in _hosts("pwr"):
        got |= inst
    assert got == pi.covered()                       # fp32, RQ, and RES where has_res, of all 15 base instances
    assert len({c.inst for c in mc.cases("pwr")}) == len({r[1] for r in pi.ROWS}) == 15


def test_float_input_entries_reach_every_instance_and_the_valu_kernel():
    import f32_instances as fi
    for prepared in (False, True):
        got = set()
        for c, (inst, ws) in _hosts("conv_f32"):
            if c.prepared == prepared:
                got |= inst
        assert got == fi.every_instance() | {"VALU"}, prepared


def test_attention_entries_name_both_kernels_of_each_core():
    import attn_instances as ai
    got = set()
    for c, (inst, ws) in _hosts("attention"):
        got |= inst
    kernels = {k[0] for k in got}
    assert kernels == {ai.MFMA, ai.VALU, "attn_bf16_kernel", "attn_bf16_stored_kernel", "attn_bf16_ctx_kernel"}
    fp32 = {k for k in got if k[0] in (ai.MFMA, ai.VALU)}
    assert fp32 <= ai.dispatchable()
    assert {k[1] for k in fp32 if k[0] == ai.MFMA} == {16, 64, 128} and {k[1] for k in fp32 if k[0] == ai.VALU} == {1, 4}
    # the 16-byte mask loads (S = 44) and the scalar ones (S = 45) on the MFMA kernel, both layouts on every entry point
    assert {k[2] & ai.kVec4 for k in fp32 if k[0] == ai.MFMA and k[2] & ai.kMask} == {0, ai.kVec4}
    for fn in mc.ATTN_FN.values():
        assert {c.layout for c in mc.cases("attention") if c.fn == fn} == {"token", "seq"}, fn


def test_ew_entries_are_the_issues_shapes():
    ew = mc.cases("ew")
    ln = [c for c in ew if c.fn == "qe_layernorm_quantize_pack"]
    assert {(c.E, c.with_ln) for c in ln} == {(E, w) for E in (66, 768) for w in (False, True)}
    assert {len(c.rqs) for c in ln} == {0, 1, 3} and all(c.refused == (c.E == 66) for c in ln)
    assert {c.fn for c in ew} == {"qe_layernorm_quantize_pack", "qe_quantize_patchify", "qe_global_avgpool", "qe_maxpool2d_codes"}


def test_case_ids_are_unique_and_the_gpu_file_runs_every_family():
    ids = [c.id for c in mc.all_cases()]
    assert len(ids) == len(set(ids))
    assert set(mc.FAMILIES) == {"linear", "ew", "attention", "conv", "pwr", "conv_f32"}
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_mem_contract_gpu.py")).read()
    assert "mc.all_cases()" in src and "pytest.mark.gpu" in src
    print("memory-contract entries: %s" % {f: len(mc.cases(f)) for f in mc.FAMILIES})


def header_size_queries():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "quant_engine.h")).read()
    return set(re.findall(r"\b(qe_\w*(?:workspace_bytes|prepared_bytes))\s*\(", src))


def test_every_size_query_is_exercised_and_answers_non_zero_somewhere():
    queries = header_size_queries()
    assert len(queries) >= 10 and queries <= set(capi.PROTOTYPES)
    most = {}
    for f in mc.FAMILIES:
        for c, (inst, ws) in _hosts(f):
            for name, n in ws.items():
                most[name] = max(most.get(name, 0), n)
    assert not queries - set(most), "no table entry asks %s" % sorted(queries - set(most))
    assert set(most) <= queries, sorted(set(most) - queries)
    zero = sorted(n for n, v in most.items() if v == 0)
    assert not zero, "no table entry gets a non-zero answer from %s" % zero
