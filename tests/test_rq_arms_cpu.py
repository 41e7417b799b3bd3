"""No GPU: the table of tests/rq_arms.py drives every fused re-quantising epilogue body into every arm of the quantiser.

The numpy restatement of rq_setup / rq_bounded says which arm a (row, setting, wave) takes; the host-only plan queries say
which body a row runs.  So this proves, without a device, that the GPU test's settings land where the table says, and that
every body listed in rq_arms.BODIES meets every arm it has, at the ragged edges where a padded lane could raise the flag."""
import numpy as np
import pytest

import conv_instances as ci
import dw_instances as di
import ew_ref
import grp_instances as gi
import pwr_instances as pi
import rq_arms as ra
from quantize_amd import capi

F32 = np.float32
SCALAR_ARMS = {"markstein", "markstein+range", "division"}


def _y(seed, n=4001):
    rng = np.random.RandomState(seed)
    y = (rng.normal(0.3, 1.0, size=n) * 2.5).astype(F32)
    y[:3] = 0.0
    return y


@pytest.mark.parametrize("sign", [False, True])
@pytest.mark.parametrize("i", range(3))
def test_each_setting_lands_in_its_arm(i, sign):
    y = _y(10 * i + sign)
    lo, hi = ra.lohi(sign)
    for qid in ra.Q_ALL:
        sc, z, qmin, qmax = ra.quantiser(qid, y, i, sign)
        got = ra.arm("dw", False, ra.slow(sc, z, qmin, qmax), ra.chk(qmin, qmax, sign), True)
        assert got == ra.Q_ARM[qid], (qid, got)
        codes, n_bad = ra.expectation(y, sc, z, qmin, qmax, sign)
        assert (n_bad > 0) == bool(ra.Q_STATUS[qid]), (qid, n_bad)
        if qid == "Q7":
            assert 1 <= n_bad <= 8
        if qid == "Q8":
            assert n_bad == y.size
    # what singles the arms out
    s1 = ra.quantiser("Q1", y, i, sign)[0]
    s0 = ra.base_quantiser(y, i, sign)[0]
    assert int(s1.view(np.uint32)) & 0x7fffff == 0x7fffff and s0 <= s1 < 2 * s0
    assert ra.slow(F32(2.0 ** -60), 0.0, lo, hi) is False and ra.slow(F32(2.0 ** 60), 0.0, lo, hi) is False
    assert ra.slow(np.nextafter(F32(2.0 ** -60), F32(0)), 0.0, lo, hi) and ra.slow(np.nextafter(F32(2.0 ** 60), F32(np.inf)), 0.0, lo, hi)
    assert not ra.slow(s0, F32(2.0 ** 30 - 512), lo, hi) and ra.slow(s0, F32(2.0 ** 30), lo, hi)      # span = max|q| + |z| + 2
    assert not ra.slow(F32(-s0), 0.37, lo, hi) and not ra.chk(lo, hi, sign) and ra.chk(lo - 1, hi, sign) and ra.chk(lo, hi + 1, sign)
    # Q6 is tight: one ulp less and something leaves the code range
    s6, z6 = ra.quantiser("Q6", y, i, sign)[:2]
    assert ra.offenders(y, s6, z6, sign) == 0 and ra.offenders(y, np.nextafter(s6, F32(0)), z6, sign) > 0
    s7 = ra.quantiser("Q7", y, i, sign)[0]
    assert s7 < s6 and ra.offenders(y, s7, z6, sign) == ra.expectation(y, s7, z6, lo - ra.OVER, hi + ra.OVER, sign)[1]


@pytest.mark.parametrize("sign", [False, True])
def test_contract_gives_the_constant_codes(sign):
    y = _y(77)
    i = 1
    lo, hi = ra.lohi(sign)
    code = lambda v: ew_ref.stored(np.array([v], F32), 8, sign)[0]
    z = ra.base_quantiser(y, i, sign)[1]
    c4, n4 = ra.expectation(y, *ra.quantiser("Q4", y, i, sign), sign)
    assert n4 == 0 and (c4 == code(-10.0 if sign else 50.0)).all()                 # qmin > qmax: always qmax
    c5a, n5a = ra.expectation(y, *ra.quantiser("Q5a", y, i, sign), sign)
    c5b, n5b = ra.expectation(y, *ra.quantiser("Q5b", y, i, sign), sign)
    assert n5a == n5b == 0 and (c5a == code(lo)).all() and (c5b == code(hi)).all()
    c3a, n3a = ra.expectation(y, *ra.quantiser("Q3a", y, i, sign), sign)
    mid = code(min(max(np.rint(-z), lo), hi))
    assert n3a == 0 and (c3a[y > 0] == code(hi)).all() and (c3a[y < 0] == code(lo)).all() and (c3a[y == 0] == mid).all()
    c3b, n3b = ra.expectation(y, *ra.quantiser("Q3b", y, i, sign), sign)
    assert n3b == 0 and (c3b == mid).all()


# ---- the constants of every row -------------------------------------------------------------------------------------------------
def _cases():
    """(name, body per mode, constants, full) of every conv and resident-tile row, both twins."""
    for i, row, modes in ra.conv_rows():
        bodies = sorted({ra.conv_body(ra.conv_plan(row, m)) for m in modes})
        for zeros in (0, 1):
            yield "conv row %d zeros=%d" % (i, zeros), bodies, ra.constants(ra.conv_case(i, zeros)), zeros == 0, row
    for k, (shp, base, note, env) in enumerate(pi.ROWS):
        yield "pwr row %d" % k, ["pwr7" if base[0] == pi.PWR7 else "pwr"], ra.constants(ra.pwr_cases()[k]), k % 3 != 1, None


def test_constant_settings_break_rq_bounded_where_they_should():
    """B3 / B4 turn exactly the waves they name out of the packed form, B2 / B3 leave the other waves' constants bounded,
    and alpha f stays below half an ulp of 2^51, so the fp32 value of the changed channel is the bias itself."""
    n = 0
    for name, bodies, k, full, row in _cases():
        OC = k["alpha"].size
        assert ra.bounded(k["alpha"], k["cst"], k["bias"], k["zwp"]).all(), name       # the control keeps every wave bounded
        assert float(np.abs(k["alpha"]).max()) * k["f_max"] < 2.0 ** 26, name           # half an ulp below 2^51 is 2^26
        for c in (0, OC - 1):
            for bid in ra.B_ALL:
                kb = ra.with_bias(k, c, ra.bias_value(bid))
                ok = ra.bounded(kb["alpha"], kb["cst"], kb["bias"], kb["zwp"])
                assert not ok[c] and ok[np.arange(OC) != c].all(), (name, bid, c)
        k4 = ra.times_2_31(k)
        assert (np.abs(k4["alpha"]) > 2.0 ** 10).all(), name
        assert not ra.bounded(k4["alpha"], k4["cst"], k4["bias"], k4["zwp"]).any(), name
        n += 1
    assert n >= 2 * len(ra.conv_rows()) + len(pi.ROWS)


def test_every_body_meets_every_arm():
    """Per epilogue body: the arms its rows reach under the table's settings.  Q0 / Q2 stand for a scale in the normal
    range (0.01 here; the GPU test asserts the arm of the scale it draws), the other settings do not depend on y."""
    reached = {b: set() for b in ra.BODIES}
    mixed = set()                                   # bodies with a launch that runs packed and scalar waves side by side
    q6_patch = {True: set(), False: set()}
    for name, bodies, k, full, row in _cases():
        OC = k["alpha"].size
        sign = True
        lo, hi = ra.lohi(sign)
        for body in bodies:
            for qid in (ra.Q_ALL if full else ra.Q_ASYM):
                y = _y(1)
                sc, z, qmin, qmax = ra.quantiser(qid, y, 0, sign)
                reached[body] |= set(ra.wave_arms(body, k, sc, z, qmin, qmax, sign))
                if qid in ("Q6", "Q7") and body.startswith("lane_pixel"):
                    q6_patch[body.endswith("patch")].add(qid)
            for c in (0, OC - 1):
                for bid in (ra.B_ALL if full else ra.B_ASYM):
                    arms = ra.wave_arms(body, ra.with_bias(k, c, ra.bias_value(bid)), F32(0.01), 0.37, lo, hi, sign)
                    reached[body] |= set(arms)
                    if "packed" in arms and "markstein" in arms:
                        mixed.add(body)
                    if body.startswith("lane_pixel"):
                        q6_patch[body.endswith("patch")].add(bid)
            if full:
                assert "packed" not in ra.wave_arms(body, ra.times_2_31(k), F32(0.01), 0.37, lo, hi, sign), name
    # the scalar-only bodies: every row runs every scalar arm (their rows are listed in rq_arms.dw_rows / grp_rows / res_rows)
    for body, n_rows in (("res", len(pi.res_rows())), ("dw", len(ra.dw_rows())), ("grp", len(ra.grp_rows()))):
        assert n_rows >= 1
        reached[body] |= {ra.Q_ARM[q] for q in ra.Q_ALL}
    for body in ra.BODIES:
        want = SCALAR_ARMS | ({"packed"} if body in ra.PACKS else set())
        assert reached[body] >= want, "%s reaches only %s" % (body, sorted(reached[body]))
        assert "packed" in reached[body] or body not in ra.PACKS
    # one launch that mixes both forms: a bias out of bounds on one channel of a row with several 32-channel strips
    assert mixed >= set(ra.PACKS), sorted(mixed)
    # PATCH and non-PATCH both meet the range test with nothing to report, with something to report, and a NaN
    for patch in (True, False):
        assert q6_patch[patch] >= {"Q6", "Q7", "B1"}, (patch, q6_patch[patch])


def test_rows_cover_the_edges_where_padding_could_raise_the_flag():
    """Q6 / Q7 run on every fused row; per family at least one of them has lanes that compute on padding: a ragged OC tile
    and a partial pixel tile (flat families), a partial image group (flatg), a ragged OC tile (lane = pixel families)."""
    seen = {}
    for i, row, modes in ra.conv_rows():
        for m in modes:
            info = ra.conv_plan(row, m)
            if capi.CONV_ROUTES[info.route] != "mfma":
                continue
            fam = capi.CONV_FAMILIES[info.family]
            seen.setdefault(fam, []).append(ci.edges(row[0], row[1], row[2], info))
    for fam in ("flat", "flat_s2", "flat_x4"):
        assert any({"partial pixel tile", "ragged OC tile"} <= e for e in seen[fam]), fam
    assert any({"partial image group", "ragged OC tile"} <= e for e in seen["flatg"])
    for fam in ci.LANE_PIXEL:
        assert any("ragged OC tile" in e for e in seen[fam]), fam
    # every family of the table, the ring kernel and both resident-tile kernels have a fused row
    bodies = {ra.conv_body(ra.conv_plan(row, m)) for i, row, modes in ra.conv_rows() for m in modes}
    assert bodies == {"lane_pixel", "lane_pixel_patch", "flat", "flatg", "flatd"}, bodies
    assert set(seen) == set(ci.LANE_PIXEL + ci.FLAT)
    assert {b[0] for _, b, _, _ in pi.ROWS} == {pi.PWR, pi.PWR7} and pi.res_rows()


def test_span_rows_name_one_row_per_code_storing_kernel():
    """dw: fast stride 1, fast stride 2, plain; grp: each group width at both strides, plain -- by the plan of the
    codes-only call, with the consumer's parameters per tensor and per channel."""
    for mod, rows, fake in ((di, ra.dw_rows(), di.fake_requant), (gi, ra.grp_rows(), gi.fake_requant)):
        kernels = set()
        for k in rows:
            row = mod.rows()[k]
            C = mod.shape_of(row).OC
            for n_param in (1, C):
                p = mod.plan(row, rq=fake(8, k % 2, n_param), out=0, codes=256)
                assert p.two_pass == 0
                kernels.add(p.kernel)
            assert row[1][0] * C >= 3 and "nobias" not in row[7]
        if mod is di:
            assert kernels == {0, 2, 5}
        else:
            assert kernels == {0} | {1 + 6 * c + 3 * s + 1 for c in range(len(gi.FAST_CG)) for s in (0, 1)}
