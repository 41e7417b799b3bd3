"""GPU: every fused re-quantising conv epilogue in each arithmetic arm of its quantiser (tests/rq_arms.py).

The rows are the per-instance problems of the instance tables with their own seeds; per (row, mode, setting) the fused call
writes into a sentinel-filled, guarded buffer and must leave exactly what the contract says: ew_ref.quantise /
ew_ref.range_bad -- the fp32 operation sequence -- on the engine's own fp32 output y of the same operands (which the instance
tests hold against float64), the library's own two-pass qe_quantize_pack of that y, and equalities that hold bit for bit in
fp32 (an infinite or huge bias pins one channel to a clamp code and changes no other; scaling weights, bias and the
consumer's scale by 2^31 changes no code).  With the status flag up only the flag and the guards are asserted: the codes
are unspecified then.

Where the table of the settings and the contract disagree the contract rules: an infinite or 2^51 bias under Q6 (clamp
bounds 1000 outside the code range) quantises to a value outside the code range, so the flag must come up there."""
import numpy as np
import pytest
import torch

import conv_instances as ci
import dw_instances as di
import ew_ref
import grp_instances as gi
import pwr_instances as pi
import rq_arms as ra
from quantize_amd import capi
from test_conv_gpu import DEV, _t, engine  # noqa: F401
from test_conv_instances_gpu import GROUPS, GUARD

pytestmark = pytest.mark.gpu
F32 = np.float32


def _dev1(v):
    return torch.from_numpy(np.atleast_1d(np.asarray(v, F32)).copy()).to(DEV)


class Problem:
    """One row in one mode: its operands, the fp32 call, the fused call.  ops = (sw, bias) as host arrays (bias None: none)."""
    n_param = 1                       # elements of the consumer's scale / zero
    q7_tied = False                   # rq_arms.Q7_TIED_ROWS
    relu_identity = None

    def base_ops(self):
        raise NotImplementedError

    def y(self, ops):                 # fp32 result of the same operands (device tensor N x OC x OH x OW)
        raise NotImplementedError

    def fused(self, ops, rq, codes):  # -> status tensor
        raise NotImplementedError

    def check_plan(self, ops, rq, codes_ptr):
        raise NotImplementedError


class ConvProblem(Problem):
    def __init__(self, i, zeros, menv, case=None, sign=None, off=0):
        self.i, self.zeros, self.menv, self.off = i, zeros, dict(menv), off
        self.case = ra.conv_case(i, zeros) if case is None else case
        self.sign = ra.conv_signs(i, zeros)[2] if sign is None else sign
        wp, wd, sw, zw = self.case["w"]
        xp, xd, sx, zx = self.case["x"]
        N, IC, H, W = [int(v) for v in xd[2:6]]
        self.sh = capi.conv_shape(N, IC, H, W, int(wd[2]), int(wd[4]), int(wd[5]), self.case["stride"], self.case["pad"])
        self.xb = int(xd[0])
        self.xq = capi.qparam(_t(xp), int(xd[0]), int(xd[1]), _t(sx), _t(zx))
        self._w = (_t(wp), int(wd[0]), int(wd[1]), _t(zw))
        self.OC = self.sh.OC
        OH, OW = capi.out_hw(self.sh)
        self.inner, self.n = OH * OW, N * self.OC * OH * OW
        self._prep = {}
        self.q7_tied = case is None and i in ra.Q7_TIED_ROWS

    def base_ops(self):
        return self.case["w"][2].astype(F32), self.case["bias"]

    def _dev(self, ops):
        key = (ops[0].tobytes(), None if ops[1] is None else ops[1].tobytes())
        if key not in self._prep:
            wq = capi.qparam(self._w[0], self._w[1], self._w[2], _t(ops[0]), self._w[3])
            bias = None if ops[1] is None else _t(ops[1])
            with capi.knobs(**self.menv):
                self._prep[key] = (wq, bias, capi.conv_prepare(wq, bias, self.sh, self.xb))
        return self._prep[key]

    def y(self, ops):
        wq, bias, prepared = self._dev(ops)
        with capi.knobs(**self.menv):
            return capi.quantconv2d_prepared(self.xq, wq, bias, self.sh, prepared)

    def fused(self, ops, rq, codes):
        wq, bias, prepared = self._dev(ops)
        with capi.knobs(**self.menv):
            return capi.quantconv2d_requant_prepared(self.xq, wq, bias, self.sh, prepared, rq, out=codes)[1]

    def check_plan(self, ops, rq, codes_ptr):
        wq = self._dev(ops)[0]
        with capi.knobs(**self.menv):
            info = capi.conv_plan_info(self.sh, self.xq, wq, rq, 0, codes_ptr)
            assert capi.requant_path(self.sh, self.xq, wq, rq) == 1
        assert info.fused == 1
        if self.menv.get("QE_RQ_PATCH") == "0":
            assert info.patch == 0
        return info


class ResProblem(ConvProblem):
    """The residual block end: codes of relu(conv + identity); codes only (out NULL)."""

    def __init__(self, k):
        import test_residual_gpu as tr
        shp, base, note, env = pi.res_rows()[k]
        self.i, self.zeros, self.menv, self.off = k, 0, dict(env or {}), 0
        x_signed, asym, bias = [(False, False, True), (True, True, True), (False, True, False)][k % 3]
        self.host = {}
        with capi.knobs(**self.menv):
            self.sh, self.xq, wq, b, prep, y, self.identity = tr._case(*shp[:5], x_signed=x_signed, asym=asym, bias=bias,
                                                                      seed=100 + k, host=self.host)
        self._w = (wq._keep[0], 8, 1, wq._keep[2])
        self.xb, self.sign, self.OC = 8, k % 2 == 0, self.sh.OC
        OH, OW = capi.out_hw(self.sh)
        self.inner, self.n = OH * OW, self.sh.N * self.OC * OH * OW
        self._prep = {}

    def base_ops(self):
        return self.host["sw"].astype(F32), self.host["b"]

    def y(self, ops):
        wq, bias, prepared = self._dev(ops)
        with capi.knobs(**self.menv):
            return capi.quantconv2d_residual_prepared(self.xq, wq, bias, self.sh, prepared, self.identity.clone(), rq=None)[0]

    def fused(self, ops, rq, codes):
        wq, bias, prepared = self._dev(ops)
        with capi.knobs(**self.menv):
            return capi.quantconv2d_residual_prepared(self.xq, wq, bias, self.sh, prepared, self.identity.clone(), rq=rq, out=None,
                                                      codes=codes)[2]

    def check_plan(self, ops, rq, codes_ptr):
        with capi.knobs(**self.menv):
            assert capi.residual_path(self.sh, self.xq, self._dev(ops)[0], rq) == 1
        return None


class SpanProblem(Problem):
    """A depthwise (groups None) or grouped row, codes only, the consumer's parameters per tensor or per channel."""

    def __init__(self, mod, k, per_channel):
        self.mod, self.k, self.row = mod, k, mod.rows()[k]
        self.grouped = mod is gi
        self.o = mod.operands(k, "parity")
        row = self.row
        self.sh = mod.shape_of(row)
        self.OC = self.sh.OC
        self.n_param = self.OC if per_channel else 1
        self.xq = capi.qparam(_t(self.o["x"]), row[5][0], row[5][1], _t(self.o["sx"]), _t(self.o["zx"]))
        OH, OW = capi.out_hw(self.sh)
        self.inner, self.n = OH * OW, self.sh.N * self.OC * OH * OW
        self.sign, self.i, self.off = k % 2 == 0, k, 0
        self.head = (self.o["groups"],) if self.grouped else ()

    def base_ops(self):
        return self.o["sw"].astype(F32), self.o["bias"]

    def _dev(self, ops):
        wq = capi.qparam(_t(self.o["w"]), self.row[6][0], self.row[6][1], _t(ops[0]), _t(self.o["zw"]))
        return wq, (None if ops[1] is None else _t(ops[1]))

    def _call(self, ops, rq, out, codes):
        wq, bias = self._dev(ops)
        fn = capi.quantconv2d_grouped if self.grouped else capi.quantconv2d_depthwise
        return fn(self.xq, wq, bias, self.sh, *self.head, rq=rq, out=out, codes=codes)

    def y(self, ops):
        return self._call(ops, None, "new", None)[0]

    def fused(self, ops, rq, codes):
        return self._call(ops, rq, None, codes)[2]

    def check_plan(self, ops, rq, codes_ptr):
        wq = self._dev(ops)[0]
        if self.grouped:
            p = capi.grouped_plan_info(self.sh, self.o["groups"], self.xq, wq, rq, 0, codes_ptr)
            assert p.kernel == gi.expected_kernel(self.row, 1) and p.two_pass == 0
        else:
            p = capi.depthwise_plan_info(self.sh, self.xq, wq, rq, 0, codes_ptr)
            assert p.kernel == (0 if self.row[0] == "plain" else 1 + 3 * (self.row[3] - 1) + 1) and p.two_pass == 0
        return p


# ---- one fused call inside guards ---------------------------------------------------------------------------------------------
def _fused_guarded(pb, ops, rqt, ref, n_bad, what):
    """The fused call of problem pb with quantiser rqt = (scale, zero, qmin, qmax) (scalars or per channel) into a sentinel-
    filled buffer: status == (n_bad > 0); the guards intact; with the flag down every byte written and equal to ref (a second
    sentinel where the first is a code the reference holds).  Returns (codes or None, plan)."""
    scale, zero, qmin, qmax = rqt
    s, z = _dev1(scale), _dev1(zero)
    rq = capi.requant(s, z, qmin, qmax, 8, pb.sign)
    n, off = pb.n, pb.off
    got = info = None
    for fill in (0xA5, 0x5A):
        buf = torch.full((n + 2 * GUARD + 16,), fill, dtype=torch.uint8, device=DEV)
        out = buf[GUARD + off:GUARD + off + n]
        assert out.data_ptr() % 16 == off
        info = pb.check_plan(ops, rq, out.data_ptr())
        status = pb.fused(ops, rq, out)
        torch.cuda.synchronize()
        st = int(status.item())
        assert st == (1 if n_bad else 0), "%s: status %d with %d elements outside the code range" % (what, st, n_bad)
        b = buf.cpu().numpy()
        assert (b[:GUARD + off] == fill).all() and (b[GUARD + off + n:] == fill).all(), what + ": written outside codes"
        if n_bad:
            return None, info
        g = b[GUARD + off:GUARD + off + n]
        bad = np.nonzero(g != ref)[0]
        assert bad.size == 0, "%s: %d of %d codes differ from the contract, first at %d (%d vs %d)" % (
            what, bad.size, g.size, bad[0], g[bad[0]], ref[bad[0]])
        got = g
        if not (ref == fill).any():
            break
    return got, info


def _per_param(pb, base, special, cstar, uniform):
    """A per-tensor value, or for a per-channel consumer the vector: `special` everywhere (uniform) or on channel cstar."""
    if pb.n_param == 1:
        return F32(special)
    v = np.full(pb.n_param, special if uniform else base, F32)
    v[cstar] = special
    return v


def _same(a, b):
    """fp32 arrays equal as values (NaN in the same places)"""
    return np.array_equal(a, b, equal_nan=True)


def run_arms(pb, what, full):
    """Every setting of the table on one problem; returns the plans of its fused calls."""
    plans = []
    ops0 = pb.base_ops()
    yd = pb.y(ops0)
    torch.cuda.synchronize()
    y0 = yd.cpu().numpy()
    assert np.isfinite(y0).all(), what
    lo, hi = ra.lohi(pb.sign)
    OC, inner = pb.OC, pb.inner
    s0, z0, _, _ = ra.base_quantiser(y0, pb.i, pb.sign)
    base = {}

    def quantiser(qid):
        sc, z, qmin, qmax = ra.quantiser(qid, y0, pb.i, pb.sign)
        uniform = qid in ("Q0", "Q4", "Q6", "Q7")
        return _per_param(pb, s0, sc, OC - 1, uniform), _per_param(pb, z0, z, OC - 1, uniform), qmin, qmax

    # ---- quantiser settings ----
    for qid in (ra.Q_ALL if full else ra.Q_ASYM):
        w = "%s %s" % (what, qid)
        rqt = quantiser(qid)
        sc1, z1 = np.atleast_1d(rqt[0])[-1], np.atleast_1d(rqt[1])[-1]
        want_arm = ra.arm("none", False, ra.slow(sc1, z1, rqt[2], rqt[3]), ra.chk(rqt[2], rqt[3], pb.sign), True)
        assert want_arm == ra.Q_ARM[qid], "%s: the setting lands in %s" % (w, want_arm)
        ref, n_bad = ra.expectation(y0, *rqt, pb.sign, inner)
        # preconditions, by the contract on y
        assert (n_bad > 0) == bool(ra.Q_STATUS[qid]), "%s: %d offenders" % (w, n_bad)
        if qid == "Q7" and not 1 <= n_bad <= 8:
            assert pb.q7_tied, "%s: %d offenders" % (w, n_bad)
            q = ew_ref.quantise(y0, np.atleast_1d(rqt[0]), np.atleast_1d(rqt[1]), rqt[2], rqt[3], inner)
            out = y0.reshape(-1)[ew_ref.range_bad(q, 8, pb.sign)]
            assert (out == out[0]).all() and out[0] in (y0.max(), y0.min()), "%s: %d offenders, not one tied value" % (w, n_bad)
        if qid == "Q6":
            q = ew_ref.quantise(y0, np.atleast_1d(rqt[0]), np.atleast_1d(rqt[1]), rqt[2], rqt[3], inner)
            assert q.max() >= hi - 1 or q.min() <= lo + 1, w
        if qid == "Q4":
            assert (ref == ew_ref.stored(np.array([rqt[3]]), 8, pb.sign)[0]).all(), w
        got, info = _fused_guarded(pb, ops0, rqt, ref, n_bad, w)
        plans.append(info)
        if not n_bad:
            two, st2 = capi.quantize_pack(yd.contiguous(), _dev1(rqt[0]), _dev1(rqt[1]), rqt[2], rqt[3], 8, pb.sign, inner=inner)
            assert int(st2.item()) == 0 and np.array_equal(two.cpu().numpy(), got), w + ": quantize_pack disagrees"
            base[qid] = got

    # ---- constant settings ----
    if pb.relu_identity is not None:
        return plans
    sw0, b0 = ops0
    bz = np.zeros(OC, F32) if b0 is None else b0.astype(F32)
    if b0 is None:      # a row without a bias: the base of the B settings is a zero bias, which changes no value
        assert _same(pb.y((sw0, bz)).cpu().numpy(), y0), what + ": a zero bias changes y"
    y4 = y0.reshape(-1, OC, inner)
    rqts = {rqid: quantiser(rqid) for rqid in ("Q0", "Q6")}
    for cstar in (0, OC - 1):
        for bid in (ra.B_ALL if full else ra.B_ASYM):
            bb = bz.copy()
            bb[cstar] = ra.bias_value(bid)
            ops = (sw0, bb)
            yb = pb.y(ops).cpu().numpy().reshape(-1, OC, inner)
            others = np.arange(OC) != cstar
            w = "%s %s channel %d" % (what, bid, cstar)
            assert _same(yb[:, others], y4[:, others]), w + ": another channel's fp32 value changed"
            if bid == "B1":
                assert np.isnan(yb[:, cstar]).all(), w
            else:
                assert (yb[:, cstar] == ra.bias_value(bid)).all(), w
            for rqid, rqt in rqts.items():
                w = "%s %s %s channel %d" % (what, rqid, bid, cstar)
                ref, n_bad = ra.expectation(yb, *rqt, pb.sign, inner)
                want_bad = bid == "B1" or rqid == "Q6"          # Q6: the clamp bound itself is outside the code range
                assert (n_bad > 0) == want_bad, "%s: %d offenders" % (w, n_bad)
                if not n_bad:
                    r3 = ref.reshape(-1, OC, inner)
                    end = rqt[2] if bid == "B3m" else rqt[3]
                    assert (r3[:, cstar] == ew_ref.stored(np.array([end]), 8, pb.sign)[0]).all(), w
                    assert np.array_equal(r3[:, others], base[rqid].reshape(-1, OC, inner)[:, others]), w
                plans.append(_fused_guarded(pb, ops, rqt, ref, n_bad, w)[1])
    if full:
        # B4: weights' scale, bias and the consumer's scale times 2^31 -- every quotient is unchanged
        per = pb.n_param > 1
        m = np.ones(OC, F32)
        m[[OC - 1] if per else slice(None)] = ra.TWO31
        assert sw0.size == OC or not per
        ops = ((sw0 * (m if sw0.size == OC else ra.TWO31)).astype(F32), None if b0 is None else (b0 * m).astype(F32))
        y31 = pb.y(ops).cpu().numpy().reshape(-1, OC, inner)
        assert np.array_equal((y4 * m[None, :, None]).view(np.int32), y31.view(np.int32)), what + " B4: y is not y * 2^31 bit for bit"
        for rqid, rqt in rqts.items():
            sc = np.atleast_1d(rqt[0]).astype(F32)
            rq4 = ((sc * m).astype(F32) if per else F32(sc[0] * ra.TWO31), rqt[1], rqt[2], rqt[3])
            plans.append(_fused_guarded(pb, ops, rq4, base[rqid], 0, "%s %s B4" % (what, rqid))[1])
    return plans


# ---- the MFMA families and the ring kernel -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", list(GROUPS))
def test_conv_rows_in_every_arm(engine, group):
    rows = [(i, row, modes) for i, row, modes in ra.conv_rows() if GROUPS[group](row[4])]
    assert rows, group
    for i, row, modes in rows:
        for menv in modes:
            want = ra.conv_body(ra.conv_plan(row, menv))
            for zeros in (0, 1):
                what = "row %d %s %s zeros=%d" % (i, row[0], dict(menv), zeros)
                for info in run_arms(ConvProblem(i, zeros, menv), what, full=zeros == 0):
                    assert ra.conv_body(info) == want, what
                    assert ci.launched(info) == ci.launched(ra.conv_plan(row, menv)), what


# ---- the resident-tile kernels ---------------------------------------------------------------------------------------------------------
PWR_IDS = ["%d-%s" % (k, "x".join(map(str, r[0][:5]))) for k, r in enumerate(pi.ROWS)]


@pytest.mark.parametrize("k", range(len(pi.ROWS)), ids=PWR_IDS)
def test_pwr_rows_in_every_arm(engine, k):
    shp, base, note, env = pi.ROWS[k]
    pb = ConvProblem(k, int(k % 3 == 1), env or {}, case=ra.pwr_cases()[k], sign=ra.pwr_sign(k))
    what = "%s %s" % (pi.kernel_name(pi.full(base, True, False)), shp)
    for info in run_arms(pb, what, full=k % 3 != 1):
        assert capi.CONV_ROUTES[info.route] == ("pwr7" if base[0] == pi.PWR7 else "pwr"), what


RES_IDS = ["%d-%s" % (k, "x".join(map(str, r[0][:5]))) for k, r in enumerate(pi.res_rows())]


@pytest.mark.parametrize("k", range(len(pi.res_rows())), ids=RES_IDS)
def test_res_rows_in_every_arm(engine, k):
    """The block end quantises relu(conv + identity) and has the element-by-element forms only: every quantiser setting on
    every row.  (A value that is not finite reaches it through the identity: test_residual_gpu.test_non_finite_identity.)"""
    shp, base, note, env = pi.res_rows()[k]
    pb = ResProblem(k)
    pb.relu_identity = True
    run_arms(pb, "%s %s" % (pi.kernel_name(pi.full(base, True, True)), shp), full=True)


# ---- depthwise and grouped ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_channel", [False, True], ids=["rq1", "rqC"])
@pytest.mark.parametrize("k", ra.dw_rows(), ids=[di.row_id(k) for k in ra.dw_rows()])
def test_dw_rows_in_every_arm(k, per_channel):
    run_arms(SpanProblem(di, k, per_channel), "dw %s n_param %s" % (di.row_id(k), "C" if per_channel else "1"), full=True)


@pytest.mark.parametrize("per_channel", [False, True], ids=["rq1", "rqC"])
@pytest.mark.parametrize("k", ra.grp_rows(), ids=[gi.row_id(k) for k in ra.grp_rows()])
def test_grp_rows_in_every_arm(k, per_channel):
    run_arms(SpanProblem(gi, k, per_channel), "grp %s n_param %s" % (gi.row_id(k), "C" if per_channel else "1"), full=True)
