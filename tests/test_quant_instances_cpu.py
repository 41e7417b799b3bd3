"""CPU: the operand-type table (tests/quant_instances.py) against the host-side plan queries, the C oracle and itself; no
device work.

Reach        every row lands on the decode site it names (plan queries, with the row's knobs).
Coverage     every site sees the settings listed for it here, spelled out and not derived from the rows.
Bound        every exact-regime row keeps its integers below 2^24 (the issue's figure; the four rows of TIGHT the tight one).
Cross-check  the numpy reference equals the oracle's float64 result on every row in both regimes, and in the exact regime
             the oracle's two fp32 chains equal it too.
Sensitivity  one LSB on the first or on the last code of either operand moves an output by at least sx min(sw)."""
import numpy as np
import pytest

import oracle
import quant_instances as qi
import quant_ref as qr

ALL16, SUB8, PAIRS = qi.ALL16, qi.SUB8, qi.SIGN_PAIRS
EIGHT = frozenset(("s8", "u8"))
MID = frozenset(("s5", "u5", "s6", "u6", "s7", "u7"))
X4 = frozenset(("s4", "u4"))
X4_W = frozenset(("s8", "u8", "s4", "u3", "s7"))
# site -> what its plain fp32 rows (entries "capi" and "torch") must show: ("w", settings), ("x", settings), ("xw", pairs)
EXPECTED = {
    "prep": [("w", ALL16), ("x", EIGHT)],
    "prep_smallic": [("w", ALL16), ("x", EIGHT)],
    "wraw_flat": [("xw", PAIRS)], "wraw_flat_s2": [("xw", PAIRS)], "wraw_flatg": [("xw", PAIRS)],
    "pwr": [("xw", PAIRS)], "pwr7": [("xw", PAIRS)], "flatd": [("xw", PAIRS)],
    "generic": [("x", ALL16), ("w", ALL16)],
    "expand_3x3": [("x", SUB8)],
    "expand_1x1": [("x", SUB8), ("xw", frozenset((x, w) for x in X4 for w in X4_W))],
    "expand_gather": [("x", frozenset(("s3", "u3", "s5", "u5")) | X4)],
    "sub_x4": [("x", X4)],
    "flat_x4": [("xw", frozenset((x, w) for x in X4 for w in X4_W))],
    "f32_prep": [("w", MID)], "f32_prep_stem": [("w", MID)], "generic_f32": [("w", ALL16)],
    "lin_generic": [("x", ALL16), ("w", ALL16)],
    "lin_generic_f32": [("w", ALL16)],
    "lin_f32_mfma": [("w", EIGHT)], "lin_bf16in": [("w", EIGHT)],
    "lin_mfma1": [("xw", PAIRS)], "lin_mfma2": [("xw", PAIRS)], "lin_mfma3": [("xw", PAIRS)], "lin_mfma4": [("xw", PAIRS)],
}
# the fused entries: (site, entry) -> number of rows
FUSED = {("expand_3x3", "requant"): 1, ("expand_1x1", "requant"): 1, ("expand_gather", "requant"): 1, ("sub_x4", "requant"): 1,
         ("flat_x4", "requant"): 1, ("pwr", "requant"): 1, ("pwr", "residual"): 1,
         ("lin_generic", "requant"): 1, ("lin_generic", "residual"): 1, ("lin_generic", "bf16"): 1}
ALL = range(len(qi.ROWS))


def test_rows_reach_their_site():
    for k, row in enumerate(qi.ROWS):
        got = qi.planned_sites(row)
        assert row[0] in got, "%s: the plan names %s" % (qi.row_id(k), sorted(got, key=str))
        assert "?" not in got, qi.row_id(k)
        assert qi.macs(row) <= 400000 or row[0] in ("pwr", "pwr7", "flatd", "wraw_flat_s2", "lin_mfma3", "lin_mfma4"), (
            "%s: %d multiply-adds" % (qi.row_id(k), qi.macs(row)))      # those kernels take nothing smaller
    assert len({(r[0], r[1], r[2], r[3], r[4], str(r[5])) for r in qi.ROWS}) == len(qi.ROWS), "duplicate rows"


def test_every_site_sees_its_settings():
    assert set(EXPECTED) == set(qi.SITES)
    for site, wants in EXPECTED.items():
        rows = [r for r in qi.ROWS if r[0] == site and r[1] in ("capi", "torch")]
        seen = {"x": {qi.tag(r[3]) for r in rows}, "w": {qi.tag(r[4]) for r in rows},
                "xw": {(qi.tag(r[3]), qi.tag(r[4])) for r in rows}}
        for what, want in wants:
            assert want <= seen[what], "%s %s: no row with %s" % (site, what, sorted(want - seen[what]))
    # the pairing rule on the two kernels that decode both operands: every setting of each operand against two partners
    for site in ("generic", "lin_generic"):
        rows = [r for r in qi.ROWS if r[0] == site and r[1] in ("capi", "torch")]
        for q in qi.SETTINGS:
            assert len({r[4] for r in rows if r[3] == q}) >= 2 and len({r[3] for r in rows if r[4] == q}) >= 2, (site, q)
        for i, q in enumerate(qi.SETTINGS):
            assert any(r[3] == q and r[4] == qi.partner(i) for r in rows) and any(r[4] == q and r[3] == qi.partner(i) for r in rows)
    fused = {}
    for r in qi.ROWS:
        if r[1] not in ("capi", "torch"):
            fused[(r[0], r[1])] = fused.get((r[0], r[1]), 0) + 1
    assert fused == FUSED
    # both entry points on every site without knobs
    for site in EXPECTED:
        rows = [r for r in qi.ROWS if r[0] == site and r[5] is None and r[3] != qi.BF16X and r[1] in ("capi", "torch")]
        assert not rows or {r[1] for r in rows} == {"capi", "torch"}, site


def test_streams_end_inside_a_byte():
    """Element count x bits is no multiple of 8, and odd for the widths that straddle bytes, wherever the site's planner
    conditions allow an odd count (quant_instances.EVEN_X lists the rest)."""
    for k, row in enumerate(qi.ROWS):
        o = qi.operands(k, "exact")
        for name, q in (("x", row[3]), ("w", row[4])):
            if name not in o or q[0] == 8:
                continue
            n = o[name]["q"].size
            if name == "x" and row[2] in qi.EVEN_X:
                continue
            assert n % 2 == 1, "%s %s: %d elements" % (qi.row_id(k), name, n)
            assert (n * q[0]) % 8 != 0 or q[0] == 8, "%s %s: %d elements of %d bits" % (qi.row_id(k), name, n, q[0])
            assert o[name]["packed"].size == (n * q[0] + 7) // 8


def test_data_rule_and_exact_grid():
    for k, row in enumerate(qi.ROWS):
        for regime in ("exact", "parity"):
            o = qi.operands(k, regime)
            for name, q in (("x", row[3]), ("w", row[4])):
                if name not in o:
                    continue
                lo, hi = qr.code_range(*q)
                c = o[name]["q"]
                assert c.flat[0] == lo and c.flat[-1] == hi and c.min() == lo and c.max() == hi, qi.row_id(k)
                assert np.array_equal(qr.unpack(o[name]["packed"], c.size, *q).reshape(c.shape), c)
        o = qi.operands(k, "exact")
        for name in ("x", "w"):
            if name in o:
                z, s = o[name]["z"], o[name]["s"]
                assert (z != 0).all() and (z == np.rint(z)).all() and np.abs(z).max() <= (1 << o[name]["bits"]) // 4 + 1, qi.row_id(k)
                assert (np.log2(s) == np.rint(np.log2(s))).all()
        if "xf" in o:
            m = o["xf"].astype(np.float64) * 16
            assert (m == np.rint(m)).all() and np.abs(m).max() == 255
            assert np.array_equal(qr.bf16_round(o["xf"]), o["xf"].astype(np.float64))
        if o["bias"] is not None:
            m = o["bias"].astype(np.float64) / o["lsb"]
            assert (m == np.rint(m)).all()
        assert (o["w"]["s"] >= 2.0 ** -7).all() and (o["w"]["s"] <= 2.0 ** -3).all()
        assert (o["w"]["s"].size == 1) == (k % 3 == 0)


def test_exact_rows_stay_below_2_24():
    tight = []
    for k in ALL:
        if qi.bound(k) < 2 ** 24:
            continue
        tight.append(k)
        assert qi.tight_bound(k) < 2 ** 24, "%s: %.0f" % (qi.row_id(k), qi.tight_bound(k))
    # only the unsigned x unsigned 8-bit rows of the four kernels whose shortest reduction is K = 128 miss the loose figure
    assert tuple(tight) == qi.TIGHT and len(tight) == 4
    for k in tight:
        assert qi.reduction(qi.ROWS[k]) == 128 and 128 * 385 * 385 > 2 ** 24


def _oracle(k, regime, mode):
    row = qi.ROWS[k]
    o = qi.operands(k, regime)
    op = qi.op_of(row)
    W = o["w"]
    wd = np.array([W["bits"], W["sign"], *W["shape"]], dtype=np.int32)
    kw = dict(mode=mode, return_f64=mode == "f64")
    if op == "conv":
        X = o["x"]
        xd = np.array([X["bits"], X["sign"], *X["shape"]], dtype=np.int32)
        r = oracle.quantconv2d(X["packed"], xd, X["s"], X["z"], W["packed"], wd, W["s"], W["z"], o["bias"], o["stride"], o["pad"], **kw)
    elif op == "conv_f32":
        r = oracle.quantconv2d_float_input(o["xf"], W["packed"], wd, W["s"], W["z"], o["bias"], o["stride"], o["pad"], **kw)
    elif op == "lin":
        X = o["x"]
        xd = np.array([X["bits"], X["sign"], *X["shape"]], dtype=np.int32)
        r = oracle.quantlinear(X["packed"], xd, X["s"], X["z"], W["packed"], wd, W["s"], W["z"], o["bias"], **kw)
    else:
        r = oracle.quantlinear_float_input(o["xf"], W["packed"], wd, W["s"], W["z"], o["bias"], **kw)
    return r[1] if mode == "f64" else r


@pytest.mark.parametrize("regime", ["exact", "parity"])
def test_numpy_reference_equals_the_oracle(regime):
    for k in ALL:
        ref = qi.reference(k, regime)
        o64 = _oracle(k, regime, "f64")
        assert ref.shape == o64.shape, qi.row_id(k)
        if regime == "exact":
            assert np.array_equal(ref, o64), qi.row_id(k)
            assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref), "%s: not an fp32 number" % qi.row_id(k)
            m = ref / qi.lsb_of(k, ref.shape)
            assert (m == np.rint(m)).all() and np.abs(m).max() < 2 ** 24, qi.row_id(k)
            for mode in ("fp32", "fp32_fma"):
                assert np.array_equal(_oracle(k, regime, mode).astype(np.float64), ref), "%s: the oracle's %s chain" % (qi.row_id(k), mode)
        else:
            # two float64 sums of the same K + 1 terms in different orders: each within (K + 2) 2^-53 of the exact sum
            # of magnitudes, which max |x| max |w| K + max |bias| bounds
            K = qi.reduction(qi.ROWS[k])
            mag = K * _amax(k, "x") * _amax(k, "w") + (0.0 if qi.operands(k, regime)["bias"] is None else 1.0)
            assert np.abs(ref - o64).max() <= 2 * (K + 2) * 2.0 ** -53 * mag, qi.row_id(k)


def _amax(k, name):
    o = qi.operands(k, "parity")
    if name == "x" and "xf" in o:
        return float(np.abs(o["xf"]).max())
    p = o[name]
    return float((np.abs(p["q"]).max() + np.abs(p["z"]).max()) * np.abs(p["s"]).max())


def _bump(k, name, where):
    """operands(k, "exact") with one code of operand `name` moved by one LSB: the first goes up, the last comes down."""
    o = dict(qi.operands(k, "exact"))
    if name == "x" and "xf" in o:
        xf = o["xf"].copy()
        xf[where] += -1 / 16.0 if xf[where] > 0 else 1 / 16.0
        o["xf"] = xf
        return o
    p = dict(o[name])
    c = p["q"].copy()
    lo, hi = qr.code_range(p["bits"], p["sign"])
    c[where] += -1 if c[where] == hi else 1
    p["q"], p["packed"] = c, qr.pack(c, p["bits"], p["sign"])
    o[name] = p
    return o


def test_one_lsb_at_either_end_of_each_operand_moves_an_output():
    for k, row in enumerate(qi.ROWS):
        o = qi.operands(k, "exact")
        ref = qi.reference(k, "exact")
        step = float(o["lsb"].min())
        for name in ("x", "w"):
            arr = o["xf"] if (name == "x" and "xf" in o) else o[name]["q"]
            first = (0,) * arr.ndim
            last = o["x_last"] if (name == "x" and o["x_last"] is not None) else tuple(d - 1 for d in arr.shape)
            for where in (first, last):
                moved = np.abs(qi.reference(k, "exact", _bump(k, name, where)) - ref).max()
                assert moved >= step, "%s: one LSB on %s%s moves the output by %g < %g" % (qi.row_id(k), name, where, moved, step)
