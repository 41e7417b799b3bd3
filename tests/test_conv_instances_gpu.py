"""GPU: every row of the conv instance table (tests/conv_instances.py) -- one small problem per instance of the MFMA
families, the LDS-DMA ring kernel and the pre-passes -- in every epilogue against the float64 oracle.

F32: capi.quantconv2d under the conv rule (conftest.conv_tolerance, both fp32 chains allowed), symmetric and asymmetric
operands on every row; signed / unsigned codes, per-tensor / per-channel weight scales and bias / no bias take turns.
RQ: qe_quantconv2d_requant_prepared; the codes equal quantize_pack of the engine's own fp32 result bit for bit and the
oracle's tpack of the host arithmetic, with the PATCH form and without it (QE_RQ_PATCH=0, codes one byte off a dword).
Every output sits between guard bands inside a larger buffer: the guards stay untouched and every element is written.
Which instance a call runs is read from the host-side plan (capi.conv_plan_info) with the call's own pointers."""
import functools

import numpy as np
import pytest
import torch

import conv_instances as ci
import oracle
from quantize_amd import capi
from test_conv_gpu import DEV, _assert_conv_close, _random_case, _t, engine  # noqa: F401
from test_requant_gpu import _case_tensors, _oracle_chains

pytestmark = pytest.mark.gpu

GUARD = 64               # elements of guard band on either side of an output (fp32: 256 bytes, codes: 64 bytes)
GROUPS = {
    "halo_4x1": lambda e: e[0] == "halo" and e[1] == 0, "halo_2x2": lambda e: e[0] == "halo" and e[1] == 1,
    "halo_1x4": lambda e: e[0] == "halo" and e[1] == 2, "ws": lambda e: e[0] == "ws", "sm2": lambda e: e[0] == "sm2",
    "stem": lambda e: e[0] == "stem", "flat_4x1": lambda e: e[0] == "flat" and e[1] == 0,
    "flat_2x2_1x4": lambda e: e[0] == "flat" and e[1] != 0, "flat_s2_x4": lambda e: e[0] in ("flat_s2", "flat_x4"),
    "flatg": lambda e: e[0] == "flatg", "flatd": lambda e: e[0] == "flatd", "pre": lambda e: e[0] == "pre",
}


def _rows(group):
    return [(i, r) for i, r in enumerate(ci.ROWS) if GROUPS[group](r[4])]


def test_groups_partition_the_table():
    assert sorted(i for g in GROUPS for i, _ in _rows(g)) == list(range(len(ci.ROWS)))


@functools.lru_cache(maxsize=None)
def _case(i, zeros):
    """Operands of row i and the oracle's three evaluations, computed once and shared by every test of the row."""
    shape, xb, wb, env, expected, note = ci.ROWS[i]
    rng = np.random.RandomState(7000 + 2 * i + zeros)
    wsgn = 1 if wb < 8 else i % 2                      # 8-bit weights: signed and unsigned codes take turns
    asgn = (i // 2 + zeros) % 2
    case = _random_case(rng, *shape, wb, wsgn, xb, asgn, w_pc=i % 3 != 0, a_pc=False, zeros=bool(zeros), bias=i % 4 != 3)
    case["o32"], case["fma"], case["o64"] = _oracle_chains(case)
    return case


def _what(i, zeros, extra=""):
    shape, xb, wb, env, expected, note = ci.ROWS[i]
    return "row %d %s A%dW%d %s %s (%s) zeros=%s %s" % (i, shape, xb, wb, env or {}, expected, note, bool(zeros), extra)


def _guarded(n, dtype, fill):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _f32_guarded(xq, wq, bias, sh, what):
    """qe_quantconv2d into a NaN-filled buffer: the result, after checking that the guards are intact and nothing is left
    unwritten.  Also returns the call's plan."""
    OH, OW = capi.out_hw(sh)
    n = sh.N * sh.OC * OH * OW
    buf, out = _guarded(n, torch.float32, float("nan"))
    info = capi.conv_plan_info(sh, xq, wq, None, out.data_ptr(), 0)
    capi.quantconv2d(xq, wq, bias, sh, out=out.view(sh.N, sh.OC, OH, OW))
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    assert np.isnan(b[:GUARD]).all() and np.isnan(b[GUARD + n:]).all(), what + ": written outside out"
    y = b[GUARD:GUARD + n].reshape(sh.N, sh.OC, OH, OW)
    assert not np.isnan(y).any(), "%s: %d elements never written" % (what, int(np.isnan(y).sum()))
    return y, info


def _codes_guarded(xq, wq, bias, sh, prepared, rq, ref, what, off=0):
    """qe_quantconv2d_requant_prepared into a sentinel-filled buffer (`off` bytes past a 16-byte boundary): the codes,
    after checking the guards, the status and that every byte is written (a second sentinel where the first one is a
    code the reference holds)."""
    n = ref.numel()
    got = None
    for fill in (0xA5, 0x5A):
        buf = torch.full((n + 2 * GUARD + 16,), fill, dtype=torch.uint8, device=DEV)
        out = buf[GUARD + off:GUARD + off + n]
        assert out.data_ptr() % 16 == off
        info = capi.conv_plan_info(sh, xq, wq, rq, 0, out.data_ptr())
        _, status = capi.quantconv2d_requant_prepared(xq, wq, bias, sh, prepared, rq, out=out)
        torch.cuda.synchronize()
        assert int(status.item()) == 0, what
        b = buf.cpu().numpy()
        assert (b[:GUARD + off] == fill).all() and (b[GUARD + off + n:] == fill).all(), what + ": written outside codes"
        g = b[GUARD + off:GUARD + off + n]
        r = ref.cpu().numpy()
        bad = np.nonzero(g != r)[0]
        assert bad.size == 0, "%s: %d of %d codes differ from quantize_pack, first at %d (%d vs %d)" % (
            what, bad.size, g.size, bad[0], g[bad[0]], r[bad[0]])
        got = g if got is None else got
        if not (r == fill).any():
            break
    return got, info


def _requant_of(y, i, sign):
    """The consumer's quantiser as test_requant_gpu draws it: amax / 100 clips a few percent, zero points off zero."""
    qmin, qmax = (-128.0, 127.0) if sign else (0.0, 255.0)
    s = torch.tensor([max(float(y.abs().max()) / 100.0, 1e-6)], device=DEV)
    z = torch.tensor([[0.37, -2.0, 5.5][i % 3] if sign else [-117.25, -3.0, -64.5][i % 3]], device=DEV)
    return capi.requant(s, z, qmin, qmax, 8, sign), s, z, qmin, qmax


# ---- F32 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", list(GROUPS))
def test_f32_every_row_vs_oracle(engine, group):
    for i, (shape, xb, wb, env, expected, note) in _rows(group):
        for zeros in (0, 1):
            case = _case(i, zeros)
            sh, xq, wq, bias = _case_tensors(case)
            what = _what(i, zeros)
            with capi.knobs(**(env or {})):
                y, info = _f32_guarded(xq, wq, bias, sh, what)
            assert expected in ci.launched(info), "%s: the plan names %s" % (what, sorted(ci.launched(info), key=str))
            _assert_conv_close(y, case["o64"], case["o32"], what, case["fma"])


# ---- RQ, with and without the LDS byte patch -----------------------------------------------------------------------------
def _rq_row(i, row, off=0):
    """Row i through every re-quantising mode conv_instances.modes lists (at codes offset `off`): returns the instances
    the calls ran."""
    shape, xb, wb, env, expected, note = row
    ran = set()
    for zeros in (0, 1):
        case = _case(i, zeros)
        sh, xq, wq, bias = _case_tensors(case)
        sign = (i + zeros) % 2 == 0
        codes = {}
        for menv, want_rq, _ in ci.modes(row):
            if not want_rq:
                continue
            what = _what(i, zeros, "rq env %s codes + %d" % (menv, off))
            with capi.knobs(**menv):
                prepared = capi.conv_prepare(wq, bias, sh, xb)
                y = capi.quantconv2d_prepared(xq, wq, bias, sh, prepared)
                torch.cuda.synchronize()
                rq, s, z, qmin, qmax = _requant_of(y, i, sign)
                ref, st = capi.quantize_pack(y, s, z, qmin, qmax, 8, sign)
                assert int(st.item()) == 0, what
                assert capi.requant_path(sh, xq, wq, rq) == 1, what
                got, info = _codes_guarded(xq, wq, bias, sh, prepared, rq, ref, what, off)
            assert info.fused == 1, what
            if menv.get("QE_RQ_PATCH") == "0" or off % 4:
                assert info.patch == 0, what
            ran |= ci.launched(info)
            _assert_conv_close(y.cpu().numpy(), case["o64"], case["o32"], what, case["fma"])
            # the same codes from the host arithmetic of the oracle on the engine's fp32 output
            yq = np.clip(np.rint(y.cpu().numpy() / np.float32(s.item()) - np.float32(z.item())), qmin, qmax)
            op, _ = oracle.tpack(yq.astype(np.int64), 8, sign)
            assert np.array_equal(got, op), what
            codes[tuple(sorted(menv.items()))] = got
        first = next(iter(codes.values()))
        assert all(np.array_equal(first, c) for c in codes.values()), _what(i, zeros, "PATCH and non-PATCH codes differ")
    return ran


def _has_rq(row):
    """The row's re-quantising call runs a conv kernel of this table (not a two-pass route, not the resident-tile one)."""
    with capi.knobs(**(row[3] or {})):
        info = ci.plan(row[0], row[1], row[2], rq=True)
    return bool(info.fused) and capi.CONV_ROUTES[info.route] in ("mfma", "flatd")


@pytest.mark.parametrize("group", list(GROUPS))
def test_rq_every_row(engine, group):
    rows = [(i, r) for i, r in _rows(group) if _has_rq(r)]
    assert rows, group
    for i, row in rows:
        ran = _rq_row(i, row)
        assert ran == ci.row_instances(row, rq=True), (row, sorted(ran, key=str))     # what covered() counts did run


@pytest.mark.parametrize("family", ci.LANE_PIXEL + ci.FLAT)
def test_rq_codes_one_byte_off(engine, family):
    """One row per family with the codes one byte past a 16-byte boundary: no PATCH form (it stores dwords), the resident
    and ring kernels step aside, and the codes are the same."""
    rows = [(i, r) for i, r in enumerate(ci.ROWS) if r[4][0] == family and _has_rq(r)]
    # a row whose aligned call takes the PATCH form where the family has one
    patched = [(i, r) for i, r in rows if len(ci.modes(r)) == 3]
    i, row = (patched or rows)[0]
    ran = _rq_row(i, row, off=1)
    assert all(k[0] == "pre" or k[0] == family for k in ran), ran


# ---- pre-passes ------------------------------------------------------------------------------------------------------------
PRE_OFF = {"sub2": {"QE_SUB2": "0"}, "sub_wide": {"QE_SUBSAMPLE": "0"}, "sub_narrow": {"QE_SUBSAMPLE": "0"},
           "sub_x4": {"QE_SUB_X4": "0"}}


def test_prepass_rows_match_the_knob_off(engine):
    """Each pre-pass row against the same problem without the pre-pass: the integer sum and the epilogue are the same, so
    the fp32 results are bit-identical.  The gathers are switched off by their knob; the expansion has none, so its rows
    run again on the same values stored as signed 8-bit codes."""
    for i, (shape, xb, wb, env, expected, note) in _rows("pre"):
        for zeros in (0, 1):
            case = _case(i, zeros)
            sh, xq, wq, bias = _case_tensors(case)
            what = _what(i, zeros)
            with capi.knobs(**(env or {})):
                y, info = _f32_guarded(xq, wq, bias, sh, what)
            assert expected in ci.launched(info), what
            kind = expected[1]
            if kind == "expand":
                xp, xd, sx, zx = case["x"]
                # signed 8-bit codes of the same values, whatever the sign of the narrow codes: what the expansion writes,
                # so a_x = q and zx' = zx in both runs
                q8, _ = oracle.tpack(oracle.tunpack(xp, xd).astype(np.int64), 8, 1)
                xq8 = capi.qparam(_t(q8), 8, 1, _t(sx), _t(zx))
                with capi.knobs(**(env or {})):
                    y2, info2 = _f32_guarded(xq8, wq, bias, sh, what + " as 8-bit codes")
            else:
                with capi.knobs(**dict(env or {}, **PRE_OFF[kind])):
                    y2, info2 = _f32_guarded(xq, wq, bias, sh, what + " knob off")
            assert expected not in ci.launched(info2), what
            assert np.array_equal(y, y2), "%s: %d elements differ without the pre-pass, worst %.3g" % (
                what, int((y != y2).sum()), float(np.abs(y - y2).max()))
