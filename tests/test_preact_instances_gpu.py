"""GPU: qe_affine_relu_quantize_pack against tests/preact_ref.py, bit for bit on the codes, sum_out, act_out and the status flag,
on every row of tests/preact_instances.py in every output form: n_out 0, 1 and 2; with and without identity; sum_out off, distinct,
in place on identity and in place on x; act_out on and off; every buffer aligned, and every fp32 buffer off by one element with
every code stream off by one byte.  Then the tie-dense input (the affine is not contracted), NaN and infinities, the range flag
from the first, a middle and the last element (and not from what lies behind a ragged group), and one tensor beyond the capped
grid of the plain instance.

fp32 outputs are compared as bits, except that a NaN counts as equal to a NaN (the payload an addition hands on is the
hardware's); the code of an element whose value is NaN is unspecified (include/quant_engine.h), the flag is not."""
import numpy as np
import pytest
import torch

import preact_instances as pi
import preact_ref
from quantize_amd import capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.array(a, copy=True)).to(DEV)          # the shared operands are read-only


def _off(a, mis, fill=None):
    """a on the device; mis: inside a larger buffer, one element past its (256-byte aligned) start.  fill: what surrounds it."""
    a = np.ascontiguousarray(a)
    if not mis:
        return _t(a)
    buf = np.full(a.size + 8, 0 if fill is None else fill, a.dtype)
    buf[1:1 + a.size] = a.reshape(-1)
    return _t(buf)[1:1 + a.size].view(a.shape)


def _blank(n, dtype, mis):
    buf = torch.empty(n + 8, dtype=dtype, device=DEV)
    return buf[1:1 + n] if mis else buf[:n]


def _rq(q):
    scale, zero, qmin, qmax, bits, sign = q
    return capi.requant(_t(scale), _t(zero), qmin, qmax, bits, sign)


def run(o, rqs, form, mis=False, fill=None):
    """One call on operands o (x, identity, alpha, shift as (N, C, P) / (C,) arrays).  Returns (codes [np.uint8], s, a, flag, x after,
    identity after) with None for what was not requested."""
    ident, smode, act = form
    N, C, P = o["x"].shape
    x = _off(o["x"].reshape(N, C, 1, P), mis, fill)
    identity = _off(o["identity"].reshape(N, C, 1, P), mis, fill) if ident else None
    sum_out = {None: None, "new": _blank(N * C * P, torch.float32, mis).view(N, C, 1, P), "identity": identity, "x": x}[smode]
    act_out = _blank(N * C * P, torch.float32, mis).view(N, C, 1, P) if act else None
    codes = [_blank(capi.packed_nbytes(N * C * P, q[4]), torch.uint8, mis) for q in rqs]
    keep = [_rq(q) for q in rqs]
    got, s, a, status = capi.affine_relu_quantize_pack(x, _off(o["alpha"], mis), _off(o["shift"], mis), identity=identity, rqs=keep,
                                                       sum_out=sum_out, act_out=act_out, codes=codes)
    np_ = lambda t: None if t is None else t.cpu().numpy().reshape(N, C, P)
    return [c.cpu().numpy() for c in got], np_(s), np_(a), int(status.item()), np_(x), np_(identity)


def same_f32(got, want):
    """bit for bit, a NaN equal to any NaN"""
    nan = np.isnan(want)
    return got.dtype == want.dtype == np.float32 and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def check(what, res, ref, rqs, form, o):
    codes, s, a, flag, x_after, id_after = res
    ident, smode, act = form
    n = ref["a"].size
    assert flag == int(ref["flag"]), what
    for i, (c, q) in enumerate(zip(codes, rqs)):
        g, w = preact_ref.unpack_codes(c, n, q[4]), preact_ref.unpack_codes(ref["codes"][i], n, q[4])
        ok = ~np.isnan(ref["q"][i]).reshape(-1)
        assert np.array_equal(g[ok], w[ok]), "%s: codes of consumer %d" % (what, i)
        assert c.size == ref["codes"][i].size
        if ok.all():
            assert np.array_equal(c, ref["codes"][i]), "%s: the stream of consumer %d, padding bits included" % (what, i)
    assert (s is None) == (smode is None) and (a is None) == (not act), what
    if s is not None:
        assert same_f32(s, ref["s"]), "%s: sum_out" % what
    if a is not None:
        assert same_f32(a, ref["a"]), "%s: act_out" % what
    if smode != "x":
        assert same_f32(x_after, o["x"]), "%s: x changed" % what
    if ident and smode != "identity":
        assert same_f32(id_after, o["identity"]), "%s: identity changed" % what


@pytest.mark.parametrize("k", range(len(pi.ROWS)), ids=[pi.row_id(k) for k in range(len(pi.ROWS))])
def test_every_form_is_the_reference_bit_for_bit(k):
    o, cons = pi.operands(k), pi.consumers(k)
    for form in pi.FORMS:
        ref = pi.reference(k, form[0])
        for n_out in (0, 1, 2):
            if n_out == 0 and form[1] is None and not form[2]:
                continue
            rqs = cons[:n_out]
            sub = dict(ref, q=ref["q"][:n_out], codes=ref["codes"][:n_out], flag=False)
            assert not ref["flag"]
            for mis in (False, True):
                what = "%s %s n_out %d %s" % (pi.row_id(k), pi.form_id(form), n_out, "off by one" if mis else "aligned")
                check(what, run(o, rqs, form, mis), sub, rqs, form, o)


@pytest.mark.parametrize("P,inst", [(64, "fast"), (63, "plain")])
def test_the_affine_is_not_contracted(P, inst):
    t = pi.tie_dense(P=P)
    assert capi.PREACT_KERNELS[capi.affine_relu_quantize_pack_path(*t["x"].shape, [pi.fake_rq("u8", 3)])] == inst
    o = dict(x=t["x"], identity=t["x"], alpha=t["alpha"], shift=t["shift"])
    ref = preact_ref.forward(t["x"], None, t["alpha"], t["shift"], [t["rq"]])
    fma = preact_ref.forward(t["x"], None, t["alpha"], t["shift"], [t["rq"]], mode="fma")
    assert (ref["q"][0] != fma["q"][0]).sum() >= t["x"].size // 20
    for mis in (False, True):
        check("tie-dense %s" % inst, run(o, [t["rq"]], (False, None, True), mis), ref, [t["rq"]], (False, None, True), o)


@pytest.mark.parametrize("k", [0, 2, 6, 9, 11], ids=lambda k: pi.row_id(k))
def test_nan_and_infinities(k):
    inst, (N, C, P), _ = pi.ROWS[k]
    base, cons = pi.operands(k), pi.consumers(k)
    n = N * C * P
    for where in ("x", "identity"):
        for vals, flagged in (((np.inf, -np.inf), False), ((np.nan, np.inf, -np.inf), True)):
            o = {f: v.copy() for f, v in base.items()}
            for j, v in enumerate(vals):
                o[where].reshape(-1)[(j * (n - 1)) // max(len(vals) - 1, 1)] = v
            form = (True, "new", True)
            ref = preact_ref.forward(o["x"], o["identity"], o["alpha"], o["shift"], cons)
            assert ref["flag"] == flagged and np.isinf(ref["s"]).any()
            for mis in (False, True):
                check("%s %s in %s" % (pi.row_id(k), vals, where), run(o, cons, form, mis), ref, cons, form, o)


@pytest.mark.parametrize("shape,inst", [((2, 3, 64), "fast"), ((2, 3, 17), "plain"), ((1, 5, 1), "plain")])
def test_the_range_flag_from_any_position_and_not_from_padding(shape, inst):
    """qmax = 300 on 8-bit unsigned codes: a value whose q exceeds 255 fails tpack's range test without being a NaN."""
    N, C, P = shape
    n = N * C * P
    rq = (np.array([0.5], np.float32), np.zeros(1, np.float32), 0.0, 300.0, 8, 0)
    assert capi.PREACT_KERNELS[capi.affine_relu_quantize_pack_path(N, C, P, [capi.requant(pi._Fake(1), pi._Fake(1), 0, 300, 8, 0)])] == inst
    rng = np.random.default_rng(5)
    base = dict(x=rng.uniform(0.0, 50.0, size=shape).astype(np.float32), identity=np.zeros(shape, np.float32),
                alpha=np.ones(C, np.float32), shift=np.zeros(C, np.float32))
    form = (False, None, False)
    for name, pos in (("clean", None), ("first", 0), ("middle", n // 2), ("last", n - 1)):
        o = {f: v.copy() for f, v in base.items()}
        if pos is not None:
            o["x"].reshape(-1)[pos] = 140.0                      # q = 280
        ref = preact_ref.forward(o["x"], None, o["alpha"], o["shift"], [rq])
        assert ref["flag"] == (pos is not None)
        for mis, fill in ((False, None), (True, np.nan), (True, 1e30)):
            # behind the tensor's last (ragged) group lie NaNs or huge values: the lanes that would read them compute nothing
            codes, _, _, flag, _, _ = run(o, [rq], form, mis, fill)
            assert flag == int(ref["flag"]), (shape, name, mis, fill)
            ok = np.ones(n, bool)
            if pos is not None:
                ok[pos] = False
            assert np.array_equal(preact_ref.unpack_codes(codes[0], n, 8)[ok], preact_ref.unpack_codes(ref["codes"][0], n, 8)[ok])


def test_a_tensor_beyond_the_grid_cap():
    N, C, P = pi.beyond_the_grid_cap()
    o = pi.draw(77, N, C, P)
    amax = float(preact_ref.activated(o["x"], o["identity"], o["alpha"], o["shift"])[1].max())
    rqs = [pi.quantiser("u8z", C, amax, seed=1)]
    assert capi.affine_relu_quantize_pack_path(N, C, P, [pi.fake_rq("u8z", C)]) == 0
    ref = preact_ref.forward(o["x"], o["identity"], o["alpha"], o["shift"], rqs)
    form = (True, "new", False)
    check("beyond the grid cap", run(o, rqs, form), ref, rqs, form, o)
