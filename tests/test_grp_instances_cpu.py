"""CPU: the grouped entry points' host side -- symbols, _path, the refusals, the instance table (tests/grp_instances.py)
against qe_quantconv2d_grouped_plan_info, tests/grp_ref.py against torch, and the packed classes' constructors.  No device
work: every operand is a pointer stand-in, so a call that got as far as a kernel launch would come back with a HIP error and
not with the code asserted here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import grp_instances as gi
import grp_ref
from quantize_amd import capi

NAMES = ("qe_quantconv2d_grouped_path", "qe_quantconv2d_grouped_plan_info", "qe_quantconv2d_grouped")
QE_ERR_NBITS, QE_ERR_ARG, QE_ERR_UNSUPPORTED = 1, 4, 7
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "quant_engine.h")
ALL = range(len(gi.rows()))


def test_symbols_are_exported_and_declared():
    text = open(HEADER).read()
    L = capi.lib()
    for name in NAMES:
        assert name in capi.PROTOTYPES and name in capi.SYMBOLS
        assert hasattr(L, name)
        assert re.search(r"\bint %s\(" % name, text), name
    # no workspace and no prepared tables: no such query may exist for these entry points
    assert not re.search(r"qe_\w*grouped\w*(workspace_bytes|prepared_bytes)", text)
    assert not any("grouped" in n and n.endswith(("workspace_bytes", "prepared_bytes")) for n in capi.PROTOTYPES)
    fields = [f[0] for f in capi.QeGrpConvPlan._fields_]
    for f in ("kernel", "slab", "TH", "TW", "tiles", "two_pass", "out16", "codes16", "blocks", "lds"):
        assert f in fields
    m = re.search(r"typedef struct qe_grpconv_plan \{(.*?)\} qe_grpconv_plan;", text, re.S)
    declared = re.findall(r"\b(?!int32_t|int64_t)(\w+)\s*[,;]", m.group(1))
    assert declared == fields
    assert set(re.findall(r"\b(\w+_t)\b", m.group(1))) == {"int32_t", "int64_t"}
    assert len(capi.GRP_KERNELS) == 25 and len(set(capi.GRP_KERNELS)) == 25


def _sh(N=1, C=16, H=9, W=9, OC=None, KH=3, KW=3, stride=1, pad=1):
    return capi.conv_shape(N, C, H, W, C if OC is None else OC, KH, KW, stride, pad)


def test_path_answers():
    x8, w8 = gi.fake_qparam(8, 0), gi.fake_qparam(8, 1, 16)
    for s in (1, 2):
        for g in (4, 2):                                   # Cg 4 and 8
            assert capi.grouped_path(_sh(stride=s), g, x8, w8) == 1
            assert capi.grouped_path(_sh(stride=s), g, x8, w8, gi.fake_requant(8, 0)) == 1
            assert capi.grouped_path(_sh(stride=s), g, x8, w8, gi.fake_requant(4, 0)) == 1   # two passes around the fast kernel
    assert capi.grouped_path(_sh(C=64), 4, x8, gi.fake_qparam(8, 1, 64)) == 1              # Cg 16
    assert capi.grouped_path(_sh(C=64), 2, x8, gi.fake_qparam(8, 1, 64)) == 1              # Cg 32
    assert capi.grouped_path(_sh(C=128), 2, x8, gi.fake_qparam(8, 1, 128)) == 0            # Cg 64
    assert capi.grouped_path(_sh(), 8, x8, w8) == 0                                        # Cg 2
    assert capi.grouped_path(_sh(OC=32), 4, x8, gi.fake_qparam(8, 1, 32)) == 0             # IC / g != OC / g
    assert capi.grouped_path(_sh(), 4, gi.fake_qparam(8, 0, 16), w8) == 0                  # per-input-channel x parameters
    assert capi.grouped_path(_sh(stride=3), 4, x8, w8) == 0
    assert capi.grouped_path(_sh(pad=0), 4, x8, w8) == 0
    assert capi.grouped_path(_sh(KH=5, KW=5, pad=2), 4, x8, w8) == 0
    assert capi.grouped_path(_sh(KH=1, KW=3, pad=0), 4, x8, w8) == 0
    assert capi.grouped_path(_sh(KH=7, KW=7, pad=3), 4, x8, w8) == 0
    assert capi.grouped_path(_sh(), 4, gi.fake_qparam(4, 0), w8) == 0
    assert capi.grouped_path(_sh(), 4, x8, gi.fake_qparam(7, 1, 16)) == 0
    # none: the dense and the depthwise cases, groups that do not divide, a kernel side past 7, padding past half the kernel,
    # an empty output, a bad count
    assert capi.grouped_path(_sh(), 1, x8, w8) == -1
    assert capi.grouped_path(_sh(), 16, x8, w8) == -1
    assert capi.grouped_path(_sh(), 3, x8, w8) == -1
    assert capi.grouped_path(_sh(OC=18), 4, x8, gi.fake_qparam(8, 1, 18)) == -1
    assert capi.grouped_path(_sh(), 0, x8, w8) == -1
    assert capi.grouped_path(_sh(KH=9, KW=9, pad=4, H=20, W=20), 4, x8, w8) == -1
    assert capi.grouped_path(_sh(pad=2), 4, x8, w8) == -1
    assert capi.grouped_path(_sh(H=1, W=1, pad=0), 4, x8, w8) == -1
    assert capi.grouped_path(_sh(), 4, x8, gi.fake_qparam(8, 1, 3)) == -1
    assert capi.grouped_path(_sh(), 4, gi.fake_qparam(8, 0, 4), w8) == -1
    # a depth multiplier with groups == IC is a grouped problem (the depthwise entry refuses it): the plain kernel
    assert capi.grouped_path(_sh(OC=32), 16, x8, gi.fake_qparam(8, 1, 32)) == 0


def _call(sh, x, w, groups=4, bias=4096, relu=0, out=8192, rq=None, codes=None, status=12288):
    return capi.lib().qe_quantconv2d_grouped(ctypes.byref(x), ctypes.byref(w), bias, ctypes.byref(sh), groups, relu, out,
                                             None if rq is None else ctypes.byref(rq), codes, status, None)


def _qp(data, bits, sign, scale, zero, n):
    return capi.QeQParam(data, bits, sign, scale, zero, n)


def _rq(scale, zero, n, bits=8, sign=0):
    lo, hi = grp_ref.code_range(bits, sign)
    return capi.QeRequant(scale, zero, n, lo, hi, bits, sign)


def test_refusals_answer_before_device_work():
    sh = _sh()
    A = 1 << 20                                     # stand-in addresses, 1 MB apart: nothing overlaps unless a case says so
    x, w = _qp(A, 8, 0, 2 * A, 3 * A, 1), _qp(4 * A, 8, 1, 5 * A, 6 * A, 16)
    rq = _rq(7 * A, 8 * A, 1)
    out, codes, st, bias = 9 * A, 10 * A, 11 * A, 12 * A
    ok = dict(bias=bias, out=out, status=st)
    L = capi.lib()
    cases = {
        "groups == 1": (_call(sh, x, w, groups=1, **ok), QE_ERR_UNSUPPORTED),
        "groups == IC == OC": (_call(sh, x, w, groups=16, **ok), QE_ERR_UNSUPPORTED),
        "groups 0": (_call(sh, x, w, groups=0, **ok), QE_ERR_ARG),
        "groups do not divide IC": (_call(sh, x, w, groups=3, **ok), QE_ERR_ARG),
        "groups do not divide OC": (_call(_sh(OC=18), x, _qp(4 * A, 8, 1, 5 * A, 6 * A, 18), **ok), QE_ERR_ARG),
        "x n_param": (_call(sh, _qp(A, 8, 0, 2 * A, 3 * A, 3), w, **ok), QE_ERR_ARG),
        "w n_param": (_call(sh, x, _qp(4 * A, 8, 1, 5 * A, 6 * A, 2), **ok), QE_ERR_ARG),
        "rq n_param": (_call(sh, x, w, rq=_rq(7 * A, 8 * A, 3), codes=codes, **ok), QE_ERR_ARG),
        "x data NULL": (_call(sh, _qp(None, 8, 0, 2 * A, 3 * A, 1), w, **ok), QE_ERR_ARG),
        "x scale NULL": (_call(sh, _qp(A, 8, 0, None, 3 * A, 1), w, **ok), QE_ERR_ARG),
        "w zero NULL": (_call(sh, x, _qp(4 * A, 8, 1, 5 * A, None, 16), **ok), QE_ERR_ARG),
        "rq scale NULL": (_call(sh, x, w, rq=_rq(None, 8 * A, 1), codes=codes, **ok), QE_ERR_ARG),
        "x bits": (_call(sh, _qp(A, 9, 0, 2 * A, 3 * A, 1), w, **ok), QE_ERR_NBITS),
        "out and codes NULL": (_call(sh, x, w, bias=bias, out=None, status=st), QE_ERR_ARG),
        "codes without rq": (_call(sh, x, w, codes=codes, **ok), QE_ERR_ARG),
        "rq without codes": (_call(sh, x, w, rq=rq, **ok), QE_ERR_ARG),
        "out overlaps x": (_call(sh, x, w, bias=bias, out=A + 64, status=st), QE_ERR_ARG),
        "out overlaps w": (_call(sh, x, w, bias=bias, out=4 * A - 8, status=st), QE_ERR_ARG),
        "out overlaps the last weight byte": (_call(sh, x, w, bias=bias, out=4 * A + 16 * 4 * 9 - 4, status=st), QE_ERR_ARG),
        "out overlaps bias": (_call(sh, x, w, bias=bias, out=bias + 4, status=st), QE_ERR_ARG),
        "codes overlap out": (_call(sh, x, w, rq=rq, codes=out + 16, **ok), QE_ERR_ARG),
        "codes overlap x scale": (_call(sh, x, w, rq=rq, codes=2 * A - 3, **ok), QE_ERR_ARG),
        "status inside out": (_call(sh, x, w, bias=bias, out=out, status=out + 8), QE_ERR_ARG),
        "out misaligned": (_call(sh, x, w, bias=bias, out=out + 2, status=st), QE_ERR_ARG),
        "sub-8-bit codes without out": (_call(sh, x, w, bias=bias, out=None, rq=_rq(7 * A, 8 * A, 1, bits=4), codes=codes, status=st),
                                        QE_ERR_UNSUPPORTED),
        "kernel side 9": (_call(_sh(KH=9, KW=9, pad=4, H=20, W=20), x, w, **ok), QE_ERR_UNSUPPORTED),
        "padding past half the kernel": (_call(_sh(pad=2), x, w, **ok), QE_ERR_UNSUPPORTED),
        "shape NULL": (L.qe_quantconv2d_grouped(ctypes.byref(x), ctypes.byref(w), bias, None, 4, 0, out, None, None, st, None), QE_ERR_ARG),
        "x NULL": (L.qe_quantconv2d_grouped(None, ctypes.byref(w), bias, ctypes.byref(sh), 4, 0, out, None, None, st, None), QE_ERR_ARG),
    }
    for name, (got, want) in cases.items():
        assert got == want, "%s: returned %d, expected %d" % (name, got, want)
    info = capi.QeGrpConvPlan()
    assert L.qe_quantconv2d_grouped_plan_info(ctypes.byref(sh), 4, ctypes.byref(x), ctypes.byref(w), None, None, None, None) == QE_ERR_ARG
    for g in (1, 16):
        assert L.qe_quantconv2d_grouped_plan_info(ctypes.byref(sh), g, ctypes.byref(x), ctypes.byref(w), None, None, None,
                                                  ctypes.byref(info)) == QE_ERR_UNSUPPORTED


def test_every_row_names_its_instance():
    for k in ALL:
        row = gi.rows()[k]
        rq = gi.fake_requant(8, 0)
        p_out, p_codes, p_both = gi.plan(row), gi.plan(row, rq), gi.plan(row, rq, out=256)
        assert (p_out.kernel, p_codes.kernel, p_both.kernel) == tuple(gi.expected_kernel(row, e) for e in (0, 1, 2)), gi.row_id(k)
        nx = row[1][1] if "xpc" in row[7] else 1
        assert capi.grouped_path(gi.shape_of(row), row[8], gi.fake_qparam(*row[5], n_param=nx), gi.fake_qparam(*row[6], n_param=row[9])) == \
            (1 if row[0] == "fast" else 0), gi.row_id(k)
        (N, IC, H, W), (KH, KW) = row[1], row[2]
        assert (p_out.OH, p_out.OW) == grp_ref.out_hw(H, W, KH, KW, row[3], row[4])
        if row[0] == "fast":
            assert p_out.TW == p_out.OW and 1 <= p_out.TH <= p_out.OH and p_out.tiles == -(-p_out.OH // p_out.TH)
            # a slab's workgroups share its N * tiles tiles: at least one, at most one per tile
            nslabs = -(-IC // p_out.slab)
            assert p_out.slab % (IC // row[8]) == 0 and p_out.blocks % nslabs == 0 and 1 <= p_out.blocks // nslabs <= N * p_out.tiles
        else:
            assert (p_out.slab, p_out.TH, p_out.TW) == (1, 1, 1)
        p4 = gi.plan(row, gi.fake_requant(4, 0), out=256)
        assert p4.two_pass == 1 and p4.kernel == gi.expected_kernel(row, 0), gi.row_id(k)
        assert not (p_out.two_pass or p_codes.two_pass or p_both.two_pass)
        # the store forms follow the addresses
        assert gi.plan(row, rq, out=256, codes=256).out16 == 1 and gi.plan(row, rq, out=260, codes=256).out16 == 0
        assert gi.plan(row, rq, out=256, codes=256).codes16 == 1 and gi.plan(row, rq, out=256, codes=257).codes16 == 0
        # and nothing else does
        a, b = gi.plan(row, rq, out=256, codes=256), gi.plan(row, rq, out=260, codes=257)
        assert (a.kernel, a.slab, a.TH, a.TW, a.tiles, a.blocks, a.lds) == (b.kernel, b.slab, b.TH, b.TW, b.tiles, b.blocks, b.lds)


def test_no_instance_is_unreached():
    """A condition, not a sample: each of the 24 fast instances and the plain kernel is the plan of at least one row."""
    rq = gi.fake_requant(8, 0)
    seen = set()
    for row in gi.rows():
        seen |= {gi.plan(row).kernel, gi.plan(row, rq).kernel, gi.plan(row, rq, out=256).kernel}
    assert seen == set(range(25)), sorted(set(range(25)) - seen)


def test_rows_reach_every_edge():
    rows = gi.rows()
    fast = [(k, r) for k, r in enumerate(rows) if r[0] == "fast"]
    for cg in gi.FAST_CG:
        slab = gi.probe_slab(cg)
        for s in (1, 2):
            mine = [(k, r, gi.plan(r)) for k, r in fast if r[3] == s and r[1][1] // r[8] == cg]
            for hw in ((1, 1), (2, 2), (3, 3), (7, 7), (14, 14), (56, 56)):
                assert any(r[1][2:] == hw for _, r, p in mine), (cg, s, hw)
            assert {4, 5, 8, 13, 15, 16, 17, 31, 33} <= {r[1][3] for _, r, p in mine if r[1][2] == 5}
            # channels: whole slabs, three of them, a partial last slab where a slab holds more than one group, N = 2
            assert any(r[1][1] == 3 * slab for _, r, p in mine)
            if cg < slab:
                assert any(r[1][1] % slab == cg for _, r, p in mine)
            assert any(r[1][0] == 2 for _, r, p in mine)
            # bands: two and more, and a last band shorter than the others
            TH = gi.probe_TH(cg, s)
            ohs = {p.OH for _, r, p in mine if r[1][3] == 20}
            assert {TH - 1, TH, TH + 1, 2 * TH + 1} <= ohs and TH > 1
            assert any(p.tiles >= 2 and p.OH % p.TH for _, r, p in mine)
            assert any(p.tiles == 1 and p.OH == TH for _, r, p in mine), "the tallest single band"
            assert {(r[5], r[6]) for _, r, p in mine} >= set(gi.SIGN_PAIRS)
            assert {o for _, r, p in mine for o in r[7]} >= {"sym", "intz", "wpt", "neg", "nobias"}
            assert any(not r[7] & {"sym", "intz"} for _, r, p in mine), "non-integer zeros"
            assert any("xpc" in r[7] and r[3] == s and r[1][1] // r[8] == cg for r in rows)
    plain = [r for r in rows if r[0] == "plain"]
    assert {(r[5][0], r[6][0]) for r in plain} >= {(1, 1), (2, 8), (4, 4), (8, 3), (7, 5)}
    assert {(r[2], r[3], r[4]) for r in plain} >= {((5, 5), 3, 2), ((1, 3), 1, 0), ((3, 3), 1, 0), ((7, 7), 1, 3)}
    assert any(r[1][1] // r[8] != r[9] // r[8] for r in plain), "IC / groups != OC / groups"
    assert any(r[1][1] // r[8] == 64 for r in plain), "Cg = 64"
    assert len(set(rows)) == len(rows), "duplicate rows"


def test_exact_operands_stay_on_the_grid():
    """Pass A's choice: power-of-two scales, integer zeros, and sum |a| |b| + |bias units| < 2^24 for every output, so (float)I
    and everything after it is exact in fp32."""
    for k in ALL:
        o = gi.operands(k, "exact")
        for s, z in ((o["sx"], o["zx"]), (o["sw"], o["zw"])):
            assert (np.log2(np.abs(s)) == np.rint(np.log2(np.abs(s)))).all() and (z == np.rint(z)).all()
        bound = grp_ref.int_sums(o["qx"], o["zx"], o["qw"], o["zw"], o["groups"], o["stride"], o["pad"])
        ratio = 8 if o["sx"].size > 1 else 1
        assert bound.max() * ratio + ratio * gi.BIAS_UNITS < 2 ** 24, gi.row_id(k)
        ref = gi.reference(k, "exact")
        m = ref / o["lsb"][None, :, None, None]
        assert (m == np.rint(m)).all() and np.abs(m).max() < 2 ** 24, gi.row_id(k)
        assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
        for name, (bits, sign) in (("x", gi.rows()[k][5]), ("w", gi.rows()[k][6])):
            q = o["q" + name]
            assert np.array_equal(grp_ref.unpack(o[name], q.size, bits, sign).reshape(q.shape), q)
            assert o[name].size == (q.size * bits + 7) // 8


def test_grp_ref_equals_torch_float64():
    for k in list(ALL)[::17] + [len(gi.rows()) - j for j in range(1, 10)]:
        o = gi.operands(k, "parity")
        IC, OC = o["qx"].shape[1], o["qw"].shape[0]
        full = lambda v, C: np.full(C, v[0], np.float64) if v.size == 1 else v.astype(np.float64)
        x = (torch.from_numpy(o["qx"]).double() - torch.from_numpy(full(o["zx"], IC)).view(1, -1, 1, 1)) * \
            torch.from_numpy(full(o["sx"], IC)).view(1, -1, 1, 1)
        w = (torch.from_numpy(o["qw"]).double() - torch.from_numpy(full(o["zw"], OC)).view(-1, 1, 1, 1)) * \
            torch.from_numpy(full(o["sw"], OC)).view(-1, 1, 1, 1)
        b = None if o["bias"] is None else torch.from_numpy(o["bias"]).double()
        want = torch.nn.functional.conv2d(x, w, b, stride=o["stride"], padding=o["pad"], groups=o["groups"]).numpy()
        ref = gi.reference(k, "parity")
        assert ref.shape == want.shape
        assert np.abs(ref - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), gi.row_id(k)


def test_one_lsb_moves_an_output():
    """The float64 reference itself: one code moved by one LSB, at either end of either operand, moves an output by a grid unit."""
    for k in (3, 4, len(gi.rows()) - 3):
        o = gi.operands(k, "exact")
        ref = gi.reference(k, "exact")
        for name in ("qx", "qw"):
            for where in (0, -1):
                q = o[name].copy()
                q.flat[where] += 1 if where == 0 else -1
                args = dict(qx=o["qx"], qw=o["qw"])
                args[name] = q
                moved = grp_ref.conv(args["qx"], o["sx"], o["zx"], args["qw"], o["sw"], o["zw"], o["bias"], o["groups"], o["stride"], o["pad"])
                assert np.abs(moved - ref).max() >= o["lsb"].min(), (gi.row_id(k), name, where)


@pytest.mark.parametrize("stride", [1, 2])
def test_plan_sweep_keeps_what_the_kernel_assumes(stride):
    """For every plan of the cross: the launch fits the default 64 KB LDS limit, the grid is a 1-D grid, every output row of
    every plane belongs to exactly one band, and the regions the kernel lays out (the table, the tile of in_rows x (W + 2) x 32
    bytes, the staged spans of 32 channels) fit the LDS bytes the plan asks for."""
    x8 = gi.fake_qparam(8, 0)
    for cg in gi.FAST_CG:
        for C in (2 * cg, 32 + cg, 1024):
            if C % cg:
                continue
            for N in (1, 256):
                for H in (1, 2, 7, 14, 28, 56, 112, 224, 1000):
                    for W in (1, 7, 14, 20, 56, 112, 224, 1000, 5000):
                        for rq, out in ((None, 0), (gi.fake_requant(8, 0), 0), (gi.fake_requant(8, 0), 260)):
                            sh = capi.conv_shape(N, C, H, W, C, 3, 3, stride, 1)
                            try:
                                p = capi.grouped_plan_info(sh, C // cg, x8, gi.fake_qparam(8, 1, C), rq, out, 257 if rq else 0)
                            except capi.QeError:                # refused, not truncated: a grid of 2^31 workgroups or more
                                OH, OW = grp_ref.out_hw(H, W, 3, 3, stride, 1)
                                assert N * C * OH * OW > (2 ** 31 - 1) * 256 and W >= 1000, (N, C, H, W)
                                continue
                            what = (N, C, H, W, stride, p.kernel, p.slab, p.TH, p.tiles, p.blocks, p.lds)
                            assert 0 < p.blocks < 2 ** 31, what
                            if p.kernel == 0:
                                assert W >= 224, what          # only a row too wide for the budget leaves the fast family
                                continue
                            assert p.lds <= 64 * 1024, what
                            nslabs = -(-C // p.slab)
                            assert p.tiles == -(-p.OH // p.TH) and p.blocks % nslabs == 0 and 1 <= p.blocks // nslabs <= N * p.tiles, what
                            per_out = (1 if rq else 0) + 4          # the fp32 stage is always there
                            in_rows = (p.TH - 1) * stride + 3
                            assert in_rows * (W + 2) * 32 + 32 * max(min(H, in_rows) * W, p.TH * p.OW * per_out) <= p.lds, what
                            assert p.TH * p.OW <= max(256, p.OW), what


def _state(OC=8, ICg=2, K=3):
    return {"weight": torch.zeros(OC * ICg * K * K, dtype=torch.uint8), "w_des": torch.tensor([8, 1, OC, ICg, K, K], dtype=torch.int32),
            "w_scale": torch.ones(OC, 1, 1, 1), "w_zero": torch.zeros(OC, 1, 1, 1), "bias": torch.zeros(OC),
            "a_quantizer.scale": torch.ones(1), "a_quantizer.zero": torch.zeros(1), "a_quantizer.qmin": torch.tensor(0.0),
            "a_quantizer.qmax": torch.tensor(255.0)}


def test_packed_grouped_conv2d_constructor():
    from quantize_amd.packed import PackedGroupedConv2d
    c = PackedGroupedConv2d.from_state_dict(_state(), "", stride=2, padding=1, in_channels=8)
    assert (c.groups, c.IC, c.OC, c.ICg) == (4, 8, 8, 2) and c.out_hw(9, 9) == (5, 5)
    sh = c.shape(2, 9, 9)
    assert (sh.N, sh.IC, sh.OC, sh.stride, sh.padding) == (2, 8, 8, 2, 1)
    with pytest.raises(ValueError, match="no multiple"):
        PackedGroupedConv2d.from_state_dict(_state(), "", in_channels=7)
    with pytest.raises(ValueError, match="PackedConv2d"):
        PackedGroupedConv2d.from_state_dict(_state(), "", in_channels=2)
    with pytest.raises(ValueError, match="PackedDepthwiseConv2d"):
        PackedGroupedConv2d.from_state_dict(_state(ICg=1), "", in_channels=8)
    with pytest.raises(ValueError, match="in_channels"):
        PackedGroupedConv2d.from_state_dict(_state(), "")
    with pytest.raises(ValueError, match="float"):
        c(torch.zeros(1, 8, 4, 4), route="float")
    with pytest.raises(ValueError, match="8"):
        c.call_packed(torch.zeros(64, dtype=torch.uint8), (8, 0, 1, 4, 4, 4))
