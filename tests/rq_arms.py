"""Which arithmetic a fused re-quantising conv epilogue runs: the table behind tests/test_rq_arms_{cpu,gpu}.py.

Every packed conv kernel that stores the consumer's 8-bit codes itself ends in the quantiser of qe_conv_common.hpp, which
has four forms ("arms") and picks one at run time:

    packed            rq_fast2, two values per instruction, no NaN test, no range flag: rq_fast_ok(c) and a wave-wide ballot of
                      rq_bounded(alpha, cst, bias, zw') -- only the bodies that have it (PACKS), the lane = pixel one only on
                      symmetric operands
    markstein         rq_value, !slow, !chk: NaN test, +-B clamp, two fmas on a reciprocal
    markstein+range   ... with the range test: qmin / qmax reach outside the code range (chk)
    division          rq_value, slow: |scale| outside [2^-60, 2^60], a significand of all ones, span > 2^30 or qmin > qmax

The rows are the existing per-instance problems (conv_instances, pwr_instances, dw_instances, grp_instances) with their own
seeds; the settings below (quantiser settings Q*, constant settings B*) are what drives each of them into each arm.  The
expectation of every fused call is exact: ew_ref.quantise / ew_ref.range_bad (the fp32 operation sequence that is the
quantiser's contract) on the engine's own fp32 output of the same operands, and equalities that hold bit for bit in fp32.

slow / chk / bounded restate rq_setup and rq_bounded in numpy, constants() the epilogue constants alpha, cst, bias, zw' of a
problem the way the kernels' comments define them, arm() the choice."""
import functools

import numpy as np

import conv_instances as ci
import dw_instances as di
import ew_ref
import grp_instances as gi
import pwr_instances as pi
from quantize_amd import capi

F32 = np.float32
TWO31 = F32(2.0 ** 31)
TWO51 = F32(2.0 ** 51)
OVER = 1000.0             # Q6 / Q7: how far qmin / qmax reach outside the code range

# the epilogue bodies ("Why" of the table): which have a packed form, and whether it also serves asymmetric operands
BODIES = ("lane_pixel", "lane_pixel_patch", "flat", "flatg", "flatd", "pwr", "pwr7", "res", "dw", "grp")
PACKS = {"lane_pixel": "sym", "lane_pixel_patch": "sym", "flat": "any", "flatd": "any", "pwr": "any", "pwr7": "any"}

Q_ALL = ("Q0", "Q1", "Q2", "Q3a", "Q3b", "Q4", "Q5a", "Q5b", "Q6", "Q7", "Q8")
Q_ASYM = ("Q1", "Q6", "Q7")                  # the asymmetric twin of a row (zeros = 1)
B_ALL = ("B1", "B2", "B3p", "B3m")           # one channel's bias; B4 (power-of-two invariance) has no channel
B_ASYM = ("B1",)
# the arm a setting must reach where the body has no packed form (or the operands keep it out), and the status it leaves
Q_ARM = {"Q0": "markstein", "Q1": "division", "Q2": "markstein", "Q3a": "division", "Q3b": "division", "Q4": "division",
         "Q5a": "division", "Q5b": "division", "Q6": "markstein+range", "Q7": "markstein+range", "Q8": "division"}
Q_STATUS = {q: 0 for q in Q_ALL}
Q_STATUS.update(Q7=1, Q8=1)
# conv_instances rows whose largest value repeats: 1x1 taps at stride 3 over a padded border leave output pixels that see
# padding only, all equal to their channel's bias.  No scale puts between 1 and 8 elements outside the code range there; Q7
# takes the smallest group that leaves (every offender holds the same value) and the GPU test asserts exactly that.
Q7_TIED_ROWS = (12, 28, 38, 61, 64)


def lohi(sign):
    lo, hi = ew_ref.qrange(8, sign)
    return float(lo), float(hi)


# ---- rq_setup / rq_bounded in numpy --------------------------------------------------------------------------------------
def slow(scale, zero, qmin, qmax):
    sc, zr, qmin, qmax = F32(scale), F32(zero), F32(qmin), F32(qmax)
    asc = np.abs(sc)
    with np.errstate(all="ignore"):
        span = F32(F32(np.fmax(np.abs(qmin), np.abs(qmax)) + np.abs(zr)) + F32(2.0))
        in_range = bool(asc >= F32(2.0 ** -60)) and bool(asc <= F32(2.0 ** 60))
    ones = (int(sc.view(np.uint32)) & 0x7fffff) == 0x7fffff
    return (not in_range) or ones or not bool(span <= F32(2.0 ** 30)) or not bool(qmin <= qmax)


def chk(qmin, qmax, sign):
    lo, hi = lohi(sign)
    return not (F32(qmin) >= F32(lo) and F32(qmax) <= F32(hi))


def bounded(alpha, cst, bias, zwp):
    """rq_bounded per channel (NaN fails every comparison)."""
    with np.errstate(invalid="ignore"):
        return ((np.abs(np.asarray(alpha, F32)) <= F32(2.0 ** 10)) & (np.abs(np.asarray(cst, F32)) <= F32(2.0 ** 40)) &
                (np.abs(np.asarray(bias, F32)) <= F32(2.0 ** 50)) & (np.abs(np.asarray(zwp, F32)) <= F32(2.0 ** 20)))


def arm(body, symmetric, slow_, chk_, wave_bounded):
    """The form one wave of `body` runs."""
    packs = PACKS.get(body)
    if packs and (packs == "any" or symmetric) and not slow_ and not chk_ and wave_bounded:
        return "packed"
    return "division" if slow_ else ("markstein+range" if chk_ else "markstein")


def wave_arms(body, k, scale, zero, qmin, qmax, sign):
    """The arm of each 32-channel strip (one wave's channels in every MFMA body) of a problem with constants k."""
    s, c = slow(scale, zero, qmin, qmax), chk(qmin, qmax, sign)
    if body in ("lane_pixel", "lane_pixel_patch"):     # the symmetric branch tests rq_bounded(alpha, 0, bias, 0)
        ok = bounded(k["alpha"], 0.0, k["bias"], 0.0)
    else:
        ok = bounded(k["alpha"], k["cst"], k["bias"], k["zwp"])
    OC = ok.size
    return [arm(body, k["symmetric"], s, c, bool(ok[w:w + 32].all())) for w in range(0, OC, 32)]


# ---- quantiser settings ----------------------------------------------------------------------------------------------------
def base_quantiser(y, i, sign):
    """(s0, z, qmin, qmax) as test_conv_instances_gpu._requant_of draws them."""
    lo, hi = lohi(sign)
    amax = float(np.abs(np.asarray(y, F32)).max())
    s0 = F32(max(amax / 100.0, 1e-6))
    z = F32([0.37, -2.0, 5.5][i % 3] if sign else [-117.25, -3.0, -64.5][i % 3])
    return s0, z, lo, hi


def _extremes(y, k=64):
    """The k smallest and k largest values: the quantiser is monotone in y, so what leaves the code range is among them."""
    f = np.asarray(y, F32).reshape(-1)
    return f if f.size <= 2 * k else np.concatenate([np.partition(f, k)[:k], np.partition(f, f.size - k)[-k:]])


def offenders(y, scale, zero, sign):
    lo, hi = lohi(sign)
    q = ew_ref.quantise(y, [scale], [zero], lo - OVER, hi + OVER)
    return int(ew_ref.range_bad(q, 8, sign).sum())


def q6_scale(y, zero, sign):
    """The smallest fp32 scale at which every element of y quantises inside the code range."""
    lo, hi = lohi(sign)
    e = _extremes(y)
    z = float(zero)
    assert lo + z < 0.0 < hi + z
    # rint keeps a value in range up to half a step past the last code
    s = F32(max(float(e.max()) / (hi + 0.5 + z), float(e.min()) / (lo - 0.5 + z), 1e-30))
    for _ in range(4096):
        if offenders(e, s, zero, sign) == 0:
            break
        s = np.nextafter(s, F32(np.inf))
    for _ in range(4096):
        t = np.nextafter(s, F32(0.0))
        if offenders(e, t, zero, sign) != 0:
            return s
        s = t
    raise AssertionError("no Q6 scale found")


def q7_scale(y, zero, sign):
    """The largest fp32 scale below q6_scale at which some element leaves the code range (bisection over the bit patterns)."""
    e = _extremes(y)
    good = q6_scale(y, zero, sign)
    bad = F32(good / F32(4.0))
    assert offenders(e, bad, zero, sign) > 0, "no element leaves the code range at a quarter of the Q6 scale"
    a, b = int(bad.view(np.uint32)), int(good.view(np.uint32))
    while b - a > 1:
        m = (a + b) // 2
        if offenders(e, np.uint32(m).view(F32), zero, sign) > 0:
            a = m
        else:
            b = m
    return np.uint32(a).view(F32)


def quantiser(qid, y, i, sign):
    """(scale, zero, qmin, qmax) of setting qid for fp32 output y of row i."""
    s0, z, lo, hi = base_quantiser(y, i, sign)
    if qid == "Q0":
        return s0, z, lo, hi
    if qid == "Q1":                                  # significand of all ones
        return np.nextafter(F32(2.0 ** np.ceil(np.log2(float(s0)))), F32(0.0)), z, lo, hi
    if qid == "Q2":
        return F32(-s0), z, lo, hi
    if qid in ("Q3a", "Q3b"):
        return F32(2.0 ** (-70 if qid == "Q3a" else 70)), z, lo, hi
    if qid == "Q4":                                  # qmin > qmax
        return (s0, z, 10.0, -10.0) if sign else (s0, z, 200.0, 50.0)
    if qid in ("Q5a", "Q5b"):                        # span > 2^30
        return s0, F32((1.5 if qid == "Q5a" else -1.5) * 2.0 ** 30), lo, hi
    if qid == "Q6":
        return q6_scale(y, z, sign), z, lo - OVER, hi + OVER
    if qid == "Q7":
        return q7_scale(y, z, sign), z, lo - OVER, hi + OVER
    if qid == "Q8":
        return F32(np.nan), z, lo, hi
    raise ValueError(qid)


def expectation(y, scale, zero, qmin, qmax, sign, inner=1):
    """(stored codes, number of elements that fail the range test) by the contract; scale / zero scalars or per channel."""
    q = ew_ref.quantise(y, np.atleast_1d(scale), np.atleast_1d(zero), qmin, qmax, inner)
    return ew_ref.stored(q, 8, sign), int(ew_ref.range_bad(q, 8, sign).sum())


def bias_value(bid):
    return {"B1": F32(np.nan), "B2": F32(np.inf), "B3p": TWO51, "B3m": F32(-TWO51)}[bid]


# ---- rows --------------------------------------------------------------------------------------------------------------------
def conv_body(info):
    route = capi.CONV_ROUTES[info.route]
    if route == "flatd":
        return "flatd"
    if route in ("pwr", "pwr7"):
        return route
    fam = capi.CONV_FAMILIES[info.family]
    if fam in ci.LANE_PIXEL:
        return "lane_pixel_patch" if info.patch else "lane_pixel"
    return "flatg" if fam == "flatg" else "flat"


@functools.lru_cache(maxsize=None)
def conv_rows():
    """[(i, row, [mode env, ...])]: every conv_instances row whose re-quantising call runs a fused MFMA-family or ring
    kernel, in each re-quantising mode conv_instances.modes lists (the PATCH form, and again under QE_RQ_PATCH=0)."""
    out = []
    for i, row in enumerate(ci.ROWS):
        with capi.knobs(**(row[3] or {})):
            info = ci.plan(row[0], row[1], row[2], rq=True)
        if info.fused and capi.CONV_ROUTES[info.route] in ("mfma", "flatd"):
            out.append((i, row, tuple(tuple(sorted(m[0].items())) for m in ci.modes(row) if m[1])))
    return tuple(out)


def conv_plan(row, menv):
    with capi.knobs(**dict(menv)):
        return ci.plan(row[0], row[1], row[2], rq=True)


def conv_signs(i, zeros):
    """(weight sign, activation sign, sign of the consumer's codes) of row i as the instance tests draw them."""
    return (1 if ci.ROWS[i][2] < 8 else i % 2), (i // 2 + zeros) % 2, (i + zeros) % 2 == 0


@functools.lru_cache(maxsize=None)
def conv_case(i, zeros):
    """Operands of conv row i: test_conv_instances_gpu._case without the oracle's evaluations (same seed, same draws)."""
    from test_conv_gpu import _random_case
    shape, xb, wb, env, expected, note = ci.ROWS[i]
    rng = np.random.RandomState(7000 + 2 * i + zeros)
    wsgn, asgn, _ = conv_signs(i, zeros)
    return _random_case(rng, *shape, wb, wsgn, xb, asgn, w_pc=i % 3 != 0, a_pc=False, zeros=bool(zeros), bias=i % 4 != 3)


@functools.lru_cache(maxsize=None)
def pwr_cases():
    """Operands of every pwr_instances row as test_requant_every_pwr_instance draws them (one stream over the rows)."""
    from test_conv_gpu import _random_case
    rng = np.random.RandomState(4343)
    out = []
    for i, (shp, base, note, env) in enumerate(pi.ROWS):
        zeros, has_bias = i % 3 == 1, i % 4 != 3
        out.append(_random_case(rng, *shp, 8, 1, 8, 0 if zeros else 1, w_pc=True, a_pc=False, zeros=zeros, bias=has_bias))
    return tuple(out)


def pwr_sign(i):
    return i % 2 == 0


def _zero_shift(bits, sign):
    return 128.0 if (not sign and bits == 8) else 0.0


def constants(case):
    """alpha, cst, bias, zw' per output channel (fp32) of a _random_case, as the kernels' comments define them:
    alpha = sx sw, zx' = zx - d_x, zw' = zw - d_w (d = 128 for unsigned 8-bit codes), cst = IC zx' zw' - zx' S_w with S_w the
    channel's sum of weight operands a_w = q - d_w (all taps: the flat bodies are 1x1).  `symmetric`: zx' and every zw' zero."""
    import oracle
    wp, wd, sw, zw = case["w"]
    xp, xd, sx, zx = case["x"]
    qw = np.asarray(oracle.tunpack(wp, wd)).astype(np.int64)
    OC = qw.shape[0]
    dw_, dx_ = _zero_shift(int(wd[0]), int(wd[1])), _zero_shift(int(xd[0]), int(xd[1]))
    swv = np.full(OC, sw[0], F32) if sw.size == 1 else sw.astype(F32)
    zwv = np.full(OC, zw[0], F32) if zw.size == 1 else zw.astype(F32)
    zxp = F32(F32(zx[0]) - F32(dx_))
    zwp = (zwv - F32(dw_)).astype(F32)
    IC = qw.shape[1]
    sw_sum = (qw.reshape(OC, -1).sum(axis=1) - int(dw_) * qw[0].size).astype(F32)
    cst = (F32(IC) * zxp * zwp - zxp * sw_sum).astype(F32)
    bias = np.zeros(OC, F32) if case["bias"] is None else case["bias"].astype(F32)
    # |sum over taps and channels of (a_x - zx')(a_w - zw')|: what alpha multiplies, whatever the order of the terms
    f_max = float(qw[0].size) * (128.0 + abs(float(zxp))) * (128.0 + float(np.abs(zwp).max()))
    return dict(alpha=(F32(sx[0]) * swv).astype(F32), cst=cst, bias=bias, zwp=zwp, zxp=zxp,
                symmetric=bool(zxp == 0 and not zwp.any()), f_max=f_max)


def with_bias(k, c, value):
    out = dict(k)
    out["bias"] = k["bias"].copy()
    out["bias"][c] = value
    return out


def times_2_31(k):
    out = dict(k)
    out["alpha"], out["bias"] = (k["alpha"] * TWO31).astype(F32), (k["bias"] * TWO31).astype(F32)
    return out


# ---- depthwise and grouped rows ------------------------------------------------------------------------------------------------
def _first(rows, pred):
    for k, r in enumerate(rows):
        if pred(r):
            return k
    raise AssertionError("no such row")


def _plain_ops(r):
    return not r[7] & {"nobias", "wpt", "xpc", "neg", "sym"}


@functools.lru_cache(maxsize=None)
def dw_rows():
    """One depthwise row per kernel number that stores codes alone (fast stride 1 and 2, plain): several planes per
    workgroup, an odd plane, per-channel weight scales and a bias."""
    rows = di.rows()
    out = [_first(rows, lambda r, s=s: r[0] == "fast" and r[3] == s and r[1] == (2, 17, 7, 7) and _plain_ops(r)) for s in (1, 2)]
    out.append(_first(rows, lambda r: r[0] == "plain" and r[5][0] == 8 and r[6][0] == 8 and _plain_ops(r)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def grp_rows():
    """One grouped row per kernel number that stores codes alone: each group width of the fast family at stride 1 and 2 (two
    images, a partial last slab), and the plain kernel."""
    rows = gi.rows()
    out = []
    for cg in gi.FAST_CG:
        for s in (1, 2):
            out.append(_first(rows, lambda r, cg=cg, s=s: r[0] == "fast" and r[3] == s and r[1][1] // r[8] == cg and
                              r[1][0] == 2 and r[1][2:] == (9, 11) and _plain_ops(r)))
    out.append(_first(rows, lambda r: r[0] == "plain" and r[5][0] == 8 and r[6][0] == 8 and _plain_ops(r)))
    return tuple(out)
