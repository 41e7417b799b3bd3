"""CPU: the depthwise entry points' host side -- symbols, _path, the refusals, and the instance table (tests/dw_instances.py)
against qe_quantconv2d_depthwise_plan_info.  No device work: every operand is a pointer stand-in, so a call that got as far
as a kernel launch would come back with a HIP error and not with the code asserted here."""
import ctypes
import os
import re

import numpy as np
import pytest

import dw_instances as di
import dw_ref
from quantize_amd import capi

NAMES = ("qe_quantconv2d_depthwise_path", "qe_quantconv2d_depthwise_plan_info", "qe_quantconv2d_depthwise")
QE_ERR_NBITS, QE_ERR_ARG, QE_ERR_UNSUPPORTED = 1, 4, 7
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "quant_engine.h")


def test_symbols_are_exported_and_declared():
    text = open(HEADER).read()
    L = capi.lib()
    for name in NAMES:
        assert name in capi.PROTOTYPES and name in capi.SYMBOLS
        assert hasattr(L, name)
        assert re.search(r"\bint %s\(" % name, text), name
    # no workspace and no prepared tables: no such query may exist for these entry points
    assert not re.search(r"qe_\w*depthwise\w*(workspace_bytes|prepared_bytes)", text)
    assert not any("depthwise" in n and n.endswith(("workspace_bytes", "prepared_bytes")) for n in capi.PROTOTYPES)
    fields = [f[0] for f in capi.QeDwConvPlan._fields_]
    for f in ("kernel", "symmetric", "G", "TH", "vec", "store16", "codes4", "two_pass", "blocks", "lds"):
        assert f in fields
    m = re.search(r"typedef struct qe_dwconv_plan \{(.*?)\} qe_dwconv_plan;", text, re.S)
    declared = re.findall(r"\b(?!int32_t|int64_t)(\w+)\s*[,;]", m.group(1))
    assert declared == fields
    assert set(re.findall(r"\b(\w+_t)\b", m.group(1))) == {"int32_t", "int64_t"}


def _sh(N=1, C=4, H=9, W=9, OC=None, KH=3, KW=3, stride=1, pad=1):
    return capi.conv_shape(N, C, H, W, C if OC is None else OC, KH, KW, stride, pad)


def test_path_answers():
    x8, w8 = di.fake_qparam(8, 0), di.fake_qparam(8, 1, 4)
    for s in (1, 2):
        assert capi.depthwise_path(_sh(stride=s), x8, w8) == 1
        assert capi.depthwise_path(_sh(stride=s), x8, w8, di.fake_requant(8, 0)) == 1
        assert capi.depthwise_path(_sh(stride=s), x8, w8, di.fake_requant(4, 0)) == 1      # two passes around the fast kernel
    assert capi.depthwise_path(_sh(stride=3), x8, w8) == 0
    assert capi.depthwise_path(_sh(pad=0), x8, w8) == 0
    assert capi.depthwise_path(_sh(KH=5, KW=5, pad=2), x8, w8) == 0
    assert capi.depthwise_path(_sh(KH=1, KW=3, pad=0), x8, w8) == 0
    assert capi.depthwise_path(_sh(KH=7, KW=7, pad=3), x8, w8) == 0
    assert capi.depthwise_path(_sh(), di.fake_qparam(4, 0), w8) == 0
    assert capi.depthwise_path(_sh(), x8, di.fake_qparam(7, 1, 4)) == 0
    # none: a depth multiplier, a kernel side past 7, padding past half the kernel, an empty output, a bad count
    assert capi.depthwise_path(_sh(OC=8), x8, w8) == -1
    assert capi.depthwise_path(_sh(KH=9, KW=9, pad=4, H=20, W=20), x8, w8) == -1
    assert capi.depthwise_path(_sh(pad=2), x8, w8) == -1
    assert capi.depthwise_path(_sh(H=1, W=1, pad=0), x8, w8) == -1
    assert capi.depthwise_path(_sh(), x8, di.fake_qparam(8, 1, 3)) == -1


def _call(sh, x, w, bias=4096, relu=0, out=8192, rq=None, codes=None, status=12288):
    return capi.lib().qe_quantconv2d_depthwise(ctypes.byref(x), ctypes.byref(w), bias, ctypes.byref(sh), relu, out,
                                               None if rq is None else ctypes.byref(rq), codes, status, None)


def _qp(data, bits, sign, scale, zero, n):
    return capi.QeQParam(data, bits, sign, scale, zero, n)


def _rq(scale, zero, n, bits=8, sign=0):
    lo, hi = dw_ref.code_range(bits, sign)
    return capi.QeRequant(scale, zero, n, lo, hi, bits, sign)


def test_refusals_answer_before_device_work():
    sh = _sh()
    A = 1 << 20                                     # stand-in addresses, 64 KB apart: nothing overlaps unless a case says so
    x, w = _qp(A, 8, 0, 2 * A, 3 * A, 1), _qp(4 * A, 8, 1, 5 * A, 6 * A, 4)
    rq = _rq(7 * A, 8 * A, 1)
    out, codes, st, bias = 9 * A, 10 * A, 11 * A, 12 * A
    ok = dict(bias=bias, out=out, status=st)
    cases = {
        "depth multiplier": (_call(_sh(OC=8), x, w, **ok), QE_ERR_UNSUPPORTED),
        "x n_param": (_call(sh, _qp(A, 8, 0, 2 * A, 3 * A, 3), w, **ok), QE_ERR_ARG),
        "w n_param": (_call(sh, x, _qp(4 * A, 8, 1, 5 * A, 6 * A, 2), **ok), QE_ERR_ARG),
        "rq n_param": (_call(sh, x, w, rq=_rq(7 * A, 8 * A, 3), codes=codes, **ok), QE_ERR_ARG),
        "x data NULL": (_call(sh, _qp(None, 8, 0, 2 * A, 3 * A, 1), w, **ok), QE_ERR_ARG),
        "x scale NULL": (_call(sh, _qp(A, 8, 0, None, 3 * A, 1), w, **ok), QE_ERR_ARG),
        "w zero NULL": (_call(sh, x, _qp(4 * A, 8, 1, 5 * A, None, 4), **ok), QE_ERR_ARG),
        "rq scale NULL": (_call(sh, x, w, rq=_rq(None, 8 * A, 1), codes=codes, **ok), QE_ERR_ARG),
        "x bits": (_call(sh, _qp(A, 9, 0, 2 * A, 3 * A, 1), w, **ok), QE_ERR_NBITS),
        "out and codes NULL": (_call(sh, x, w, bias=bias, out=None, status=st), QE_ERR_ARG),
        "codes without rq": (_call(sh, x, w, codes=codes, **ok), QE_ERR_ARG),
        "rq without codes": (_call(sh, x, w, rq=rq, **ok), QE_ERR_ARG),
        "out overlaps x": (_call(sh, x, w, bias=bias, out=A + 64, status=st), QE_ERR_ARG),
        "out overlaps w": (_call(sh, x, w, bias=bias, out=4 * A - 8, status=st), QE_ERR_ARG),
        "out overlaps bias": (_call(sh, x, w, bias=bias, out=bias + 4, status=st), QE_ERR_ARG),
        "codes overlap out": (_call(sh, x, w, rq=rq, codes=out + 16, **ok), QE_ERR_ARG),
        "codes overlap x scale": (_call(sh, x, w, rq=rq, codes=2 * A - 3, **ok), QE_ERR_ARG),
        "status inside out": (_call(sh, x, w, bias=bias, out=out, status=out + 8), QE_ERR_ARG),
        "out misaligned": (_call(sh, x, w, bias=bias, out=out + 2, status=st), QE_ERR_ARG),
        "sub-8-bit codes without out": (_call(sh, x, w, bias=bias, out=None, rq=_rq(7 * A, 8 * A, 1, bits=4), codes=codes, status=st),
                                        QE_ERR_UNSUPPORTED),
        "kernel side 9": (_call(_sh(KH=9, KW=9, pad=4, H=20, W=20), x, w, **ok), QE_ERR_UNSUPPORTED),
        "padding past half the kernel": (_call(_sh(pad=2), x, w, **ok), QE_ERR_UNSUPPORTED),
        "shape NULL": (capi.lib().qe_quantconv2d_depthwise(ctypes.byref(x), ctypes.byref(w), bias, None, 0, out, None, None, st, None),
                       QE_ERR_ARG),
        "x NULL": (capi.lib().qe_quantconv2d_depthwise(None, ctypes.byref(w), bias, ctypes.byref(sh), 0, out, None, None, st, None),
                   QE_ERR_ARG),
    }
    for name, (got, want) in cases.items():
        assert got == want, "%s: returned %d, expected %d" % (name, got, want)
    info = capi.QeDwConvPlan()
    L = capi.lib()
    assert L.qe_quantconv2d_depthwise_plan_info(ctypes.byref(sh), ctypes.byref(x), ctypes.byref(w), None, None, None, None) == QE_ERR_ARG
    assert L.qe_quantconv2d_depthwise_plan_info(ctypes.byref(_sh(OC=8)), ctypes.byref(x), ctypes.byref(w), None, None, None,
                                                ctypes.byref(info)) == QE_ERR_UNSUPPORTED


ALL = range(len(di.rows()))


def _instance(row, e):
    return 0 if row[0] == "plain" else 1 + 3 * (row[3] - 1) + e


def test_every_row_names_its_instance():
    for k in ALL:
        row = di.rows()[k]
        rq = di.fake_requant(8, 0)
        p_out, p_codes, p_both = di.plan(row), di.plan(row, rq), di.plan(row, rq, out=256)
        assert (p_out.kernel, p_codes.kernel, p_both.kernel) == tuple(_instance(row, e) for e in (0, 1, 2)), di.row_id(k)
        assert capi.depthwise_path(di.shape_of(row), di.fake_qparam(*row[5]), di.fake_qparam(*row[6], n_param=row[1][1])) == \
            (1 if row[0] == "fast" else 0), di.row_id(k)
        (N, C, H, W), (KH, KW) = row[1], row[2]
        assert (p_out.OH, p_out.OW) == dw_ref.out_hw(H, W, KH, KW, row[3], row[4])
        assert p_out.symmetric == (1 if row[5][1] and row[6][1] else 0)
        assert p_out.vec == (4 if row[0] == "fast" else 1)
        p4 = di.plan(row, di.fake_requant(4, 0), out=256)
        assert p4.two_pass == 1 and p4.kernel == _instance(row, 0), di.row_id(k)
        assert not (p_out.two_pass or p_codes.two_pass or p_both.two_pass)
        # the store forms follow the addresses
        assert di.plan(row, rq, out=256, codes=256).store16 == 1 and di.plan(row, rq, out=260, codes=256).store16 == 0
        assert di.plan(row, rq, out=256, codes=256).codes4 == 1 and di.plan(row, rq, out=256, codes=257).codes4 == 0
        # and nothing else does
        a, b = di.plan(row, rq, out=256, codes=256), di.plan(row, rq, out=260, codes=257)
        assert (a.kernel, a.G, a.TH, a.bands, a.blocks, a.lds) == (b.kernel, b.G, b.TH, b.bands, b.blocks, b.lds)


def test_rows_reach_every_instance_and_edge():
    rows = di.rows()
    fast = [(k, r) for k, r in enumerate(rows) if r[0] == "fast"]
    for s in (1, 2):
        mine = [(k, r, di.plan(r)) for k, r in fast if r[3] == s]
        # whole planes: one, several, a ragged last workgroup, more than one workgroup
        G = di.probe_G(s)
        nps = {r[1][0] * r[1][1] for _, r, p in mine if r[1][2:] == (7, 7)}
        assert {G - 1, G, G + 1, 2 * G + 1} <= nps and G > 1
        assert any(p.bands == 1 and p.G > 1 and p.blocks > 1 and (r[1][0] * r[1][1]) % p.G for _, r, p in mine)
        assert any(p.bands == 1 and p.G == 1 for _, r, p in mine)
        # bands: two and more, and a last band shorter than the others
        TH = di.probe_TH(s)
        ohs = {p.OH for _, r, p in mine if r[1][3] == 20}
        assert {TH - 1, TH, TH + 1, 2 * TH + 1} <= ohs
        assert any(p.bands >= 2 and p.G == 1 for _, r, p in mine)
        assert any(p.bands >= 2 and p.OH % p.TH for _, r, p in mine)
        assert any(p.bands == 1 and p.OH == TH for _, r, p in mine), "the tallest single band"
        # 49-byte planes on every base residue mod 16, across an image boundary
        assert any(r[1] == (2, 17, 7, 7) for _, r, p in mine) and {(49 * i) % 16 for i in range(17)} == set(range(16))
        # widths around the 4-output vector and the 16-byte chunk; one output; all four sign pairs; the operand sets
        assert {4, 5, 8, 13, 15, 16, 17, 31, 33} <= {r[1][3] for _, r, p in mine if r[1][2] == 5}
        assert any(r[1] == (1, 1, 1, 1) for _, r, p in mine)
        assert {(r[5], r[6]) for _, r, p in mine} >= set(di.SIGN_PAIRS)
        assert {o for _, r, p in mine for o in r[7]} >= {"sym", "intz", "xpc", "wpt", "neg", "nobias"}
        assert any(not r[7] & {"sym", "intz"} for _, r, p in mine), "non-integer zeros"
        for hw in ((14, 14), (28, 28), (56, 56), (112, 112)):
            assert any(r[1][2:] == hw for _, r, p in mine)
    plain = [r for r in rows if r[0] == "plain"]
    assert {(r[5][0], r[6][0]) for r in plain} >= {(1, 1), (2, 8), (4, 4), (8, 3), (7, 5)}
    assert {(r[2], r[3], r[4]) for r in plain} >= {((5, 5), 3, 2), ((1, 3), 1, 0), ((3, 3), 1, 0), ((7, 7), 1, 3)}
    assert any(r[2] == (7, 7) and r[1][2:] == (4, 4) for r in plain)
    assert len(set(rows)) == len(rows), "duplicate rows"


def test_exact_operands_stay_on_the_grid():
    for k in ALL:
        o = di.operands(k, "exact")
        for s, z in ((o["sx"], o["zx"]), (o["sw"], o["zw"])):
            assert (np.log2(np.abs(s)) == np.rint(np.log2(np.abs(s)))).all() and (z == np.rint(z)).all()
        ref = di.reference(k, "exact")
        m = ref / o["lsb"][None, :, None, None]
        assert (m == np.rint(m)).all() and np.abs(m).max() < 2 ** 24, di.row_id(k)
        assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
        for name, (bits, sign) in (("x", di.rows()[k][5]), ("w", di.rows()[k][6])):
            q = o["q" + name]
            assert np.array_equal(dw_ref.unpack(o[name], q.size, bits, sign).reshape(q.shape), q)
            assert o[name].size == (q.size * bits + 7) // 8


def test_one_lsb_moves_an_output():
    """The float64 reference itself: one code moved by one LSB, at either end of either operand, moves an output by a grid unit."""
    for k in (3, 4, len(di.rows()) - 3):      # planes on which every tap is in bounds somewhere
        o = di.operands(k, "exact")
        ref = di.reference(k, "exact")
        for name in ("qx", "qw"):
            for where in (0, -1):
                q = o[name].copy()
                q.flat[where] += 1 if where == 0 else -1
                args = dict(qx=o["qx"], qw=o["qw"])
                args[name] = q
                moved = dw_ref.conv(args["qx"], o["sx"], o["zx"], args["qw"], o["sw"], o["zw"], o["bias"], o["stride"], o["pad"])
                assert np.abs(moved - ref).max() >= o["lsb"].min(), (di.row_id(k), name, where)


@pytest.mark.parametrize("stride", [1, 2])
def test_plan_sweep_keeps_what_the_kernel_assumes(stride):
    """For every plan of the cross: the launch fits the default LDS limit and the budget five workgroups of a CU share, the
    grid is a 1-D grid, in-plane offsets and the whole span of G planes fit 32 bits (they fit the LDS), every output row of
    every plane belongs to exactly one workgroup, and a workgroup's outputs stay below the cap the unit decode relies on."""
    x8 = di.fake_qparam(8, 0)
    for C in (1, 3, 32, 1024):
        for N in (1, 256):
            for H in (1, 2, 7, 14, 28, 56, 112, 224, 1000):
                for W in (1, 7, 14, 20, 112, 224, 1000, 5000):
                    for rq, out in ((None, 0), (di.fake_requant(8, 0), 0), (di.fake_requant(8, 0), 260)):
                        sh = capi.conv_shape(N, C, H, W, C, 3, 3, stride, 1)
                        try:
                            p = capi.depthwise_plan_info(sh, x8, di.fake_qparam(8, 1, C), rq, out, 257 if rq else 0)
                        except capi.QeError:                # refused, not truncated: a grid of 2^31 workgroups or more
                            OH, OW = dw_ref.out_hw(H, W, 3, 3, stride, 1)
                            assert N * C * OH * OW > (2 ** 31 - 1) * 256 and W >= 1000, (N, C, H, W)
                            continue
                        what = (N, C, H, W, stride, p.kernel, p.G, p.TH, p.bands, p.blocks, p.lds)
                        assert 0 < p.blocks < 2 ** 31, what
                        if p.kernel == 0:
                            assert W >= 1000, what          # only a row too wide for the budget leaves the fast kernel
                            continue
                        assert p.lds <= 32 * 1024 < 64 * 1024, what
                        per_out = (1 if rq else 0) + (4 if (rq is None or out) else 0)
                        if p.bands == 1:
                            assert 1 <= p.G <= N * C and p.TH == p.OH, what
                            assert p.blocks == -(-N * C // p.G), what
                            assert p.G * (H * W + p.OH * p.OW * per_out) <= p.lds < 2 ** 31, what
                            assert p.G * p.OH * p.OW <= 4096, what
                        else:
                            assert p.G == 1 and 1 <= p.TH < p.OH, what
                            assert p.bands == -(-p.OH // p.TH) and p.blocks == N * C * p.bands, what
                            assert min(H, (p.TH - 1) * stride + 3) * W + p.TH * p.OW * per_out <= p.lds, what
                            assert p.TH * p.OW <= 4096, what
                        assert H * W < 2 ** 31
