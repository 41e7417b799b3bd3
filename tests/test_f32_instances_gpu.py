"""GPU: every instance of the float-input conv kernels (tests/f32_instances.py: conv_f32_mfma_kernel x 8,
conv_f32_stem_kernel x 3, with both prepare kernels) against float64, through the C ABI with the row's own shape, the
output pre-filled with NaN.

A  integer grid, bit-exact.  Integer activations |x| <= xmax, integer zero points |z_w| <= 3, s_w = 2^-k (k = 8 .. 11),
   bias = m 2^-10, and xmax such that IC KH KW xmax (max|q| + 3) < 2^22: every product, every partial sum in any order, the
   zero-point correction and the final multiply-add are exact in fp32, so the kernel has to return the float64 value bit
   for bit.  A dropped tap, a wrong code, channel, pixel or zero point changes an integer and cannot hide in a tolerance.
B  three-split exact (rows with IC KH KW <= 64).  Odd 17-bit integers: x = x1 + x2 + x3 with all three bf16 parts non-zero
   on most elements; 2-bit or 1-bit codes, so every partial sum of S_xq stays below 2^24 and of S_x below 2^23: bit-equal
   to float64 again.  A kernel that drops or misplaces a split part fails here (and nowhere in a tolerance test: the third
   part is 2^-16 of a product).
C  random normal activations at the headline weight scales, zero points up to +-3: the project's rule
   conftest.conv_tolerance, unchanged.  err / allowed is printed per row (DESIGN.md quotes the worst per instance).
D  identities on the A inputs: prepare + run on kept tables == the one-call form; x as a view at +1, +2, +3 floats and out
   as a view at +1 float (no 16-byte store possible) == the aligned run, all bit for bit.
E  both sides of each planner boundary: the VALU kernel (path 0) is bit-identical to the reference's fmaf chain, the MFMA
   side meets C's rule.
F  non-finite locality (include/quant_engine.h): an output whose KH x KW window holds a +-inf / NaN activation is non-finite,
   every other output is finite and bit-equal to the run with those activations zeroed."""
import functools
import zlib

import numpy as np
import pytest
import torch

import f32_instances as fi
import oracle
from conftest import conv_tolerance
from quantize_amd import capi
from test_conv_gpu import _t, engine  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROW_IDS = [fi.row_id(r) for r in fi.ROWS]
B_ROWS = [r for r in fi.ROWS if r.IC * r.KH * r.KW <= 64]
FIRST_OF = [fi.rows_of(i)[0] for i in capi.F32_KERNELS]


def _rng(r, salt):
    return np.random.RandomState(zlib.crc32(("%s/%s" % (fi.row_id(r), salt)).encode()) & 0x7fffffff)


def _codes(rng, r, bits, signed):
    lo, hi = (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if signed else (0, (1 << bits) - 1)
    return rng.randint(lo, hi + 1, size=(r.OC, r.IC, r.KH, r.KW)), max(-lo, hi)


def _weights(r, rng, exact, bits=None, signed=None):
    """The row's weights (fi.weights_of): packed codes, scales, zero points, bias.  exact: s_w = 2^-k, integer z_w, bias on
    the 2^-10 grid; otherwise the headline scales of test_conv_gpu._random_case with real zero points in +-3."""
    rb, rs, per_tensor, has_bias, zmode = fi.weights_of(r)
    bits, signed = (rb, rs) if bits is None else (bits, signed)
    qw, qmax = _codes(rng, r, bits, signed)
    n = 1 if per_tensor else r.OC
    if exact:
        sw = (2.0 ** -rng.randint(8, 12, size=n)).astype(np.float32)
        zw = rng.choice([-3, -2, -1, 1, 2, 3], size=n).astype(np.float32)
        bias = (rng.randint(-512, 513, size=r.OC) * 2.0 ** -10).astype(np.float32)
    else:
        sw = rng.uniform(2.5e-4, 7.5e-4, size=n).astype(np.float32)
        zw = rng.uniform(-3, 3, size=n).astype(np.float32)
        bias = rng.normal(0, 0.1, size=r.OC).astype(np.float32)
    if zmode == "zero":
        zw[:] = 0
    elif zmode == "tile_mix":
        assert not per_tensor and r.OC > fi.mt(r.instance)
        zw[:fi.mt(r.instance)] = 0                # need_sx is decided per output-channel tile
    wp, wd = oracle.tpack(qw, bits, signed)
    return dict(wp=wp, wd=wd, sw=sw, zw=zw, bias=bias if has_bias else None, bits=bits, signed=signed, qw=qw, qmax=qmax)


def _oracle(r, x, w, mode):
    if mode == "f64":
        return oracle.quantconv2d_float_input(x, w["wp"], w["wd"], w["sw"], w["zw"], w["bias"], r.stride, r.pad, mode="f64",
                                              return_f64=True)[1]
    return oracle.quantconv2d_float_input(x, w["wp"], w["wd"], w["sw"], w["zw"], w["bias"], r.stride, r.pad, mode=mode)


def _operands(r, w):
    sh = capi.conv_shape(*fi.shape_of(r))
    wq = capi.qparam(_t(w["wp"]), w["bits"], w["signed"], _t(w["sw"]), _t(w["zw"]))
    return sh, wq, None if w["bias"] is None else _t(w["bias"])


def _nan_out(r, shift=0):
    """The output tensor, NaN everywhere; shift: floats off the allocation's 16-byte boundary."""
    p = capi.conv_f32_plan_info(capi.conv_shape(*fi.shape_of(r)))
    OH, OW = capi.out_hw(capi.conv_shape(*fi.shape_of(r)))
    assert not p.ok or (p.OH, p.OW) == (OH, OW)
    n = r.N * r.OC * OH * OW
    buf = torch.full((n + 4,), float("nan"), dtype=torch.float32, device=DEV)
    out = buf[shift:shift + n].view(r.N, r.OC, OH, OW)
    assert out.data_ptr() % 16 == 4 * shift
    return out


def _shifted(x, shift):
    buf = torch.empty(x.numel() + 4, dtype=torch.float32, device=DEV)
    v = buf[shift:shift + x.numel()].view(x.shape)
    v.copy_(x)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * shift
    return v


def _run(r, x, w, x_shift=0, out_shift=0, prepared=False, expect_path=1):
    sh, wq, bias = _operands(r, w)
    assert capi.float_input_path(sh, wq) == expect_path, fi.shape_of(r)
    xt = _shifted(_t(x), x_shift)
    out = _nan_out(r, out_shift)
    if prepared:
        tables = capi.conv_f32_prepare(wq, bias, sh)
        assert tables.numel() == capi.conv_f32_plan_info(sh).total > 0
        capi.quantconv2d_float_input_prepared(xt, wq, bias, sh, tables, out=out)
    else:
        capi.quantconv2d_float_input(xt, wq, bias, sh, out=out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _assert_fp32_exact(o64, what):
    assert np.array_equal(o64.astype(np.float32).astype(np.float64), o64), "%s: the float64 result is not an fp32 number" % what


# ---- A: integer grid ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _grid_case(r):
    """Inputs, float64 result and the aligned one-call run of pass A (shared with pass D)."""
    rng = _rng(r, "grid")
    w = _weights(r, rng, exact=True)
    K = r.IC * r.KH * r.KW
    xmax = ((1 << 22) - 1) // (K * (w["qmax"] + 3))
    assert xmax >= 1 and K * xmax * (w["qmax"] + 3) < 1 << 22, (K, xmax)
    x = rng.randint(-xmax, xmax + 1, size=(r.N, r.IC, r.H, r.W)).astype(np.float32)
    o64 = _oracle(r, x, w, "f64")
    _assert_fp32_exact(o64, fi.row_id(r))
    return x, w, o64, _run(r, x, w)


@pytest.mark.parametrize("r", fi.ROWS, ids=ROW_IDS)
def test_integer_grid_bit_exact(r):
    x, w, o64, y = _grid_case(r)
    want = o64.astype(np.float32)
    bad = ~(y == want)                         # NaN (an element the kernel did not write) compares unequal
    assert not bad.any(), "%s: %d of %d elements differ, %d of them NaN; first at %s: got %r, float64 says %r" % (
        fi.row_id(r), int(bad.sum()), bad.size, int(np.isnan(y).sum()), tuple(np.argwhere(bad)[0]), y[bad][0], want[bad][0])
    assert np.array_equal(y, want)


@pytest.mark.parametrize("r", FIRST_OF, ids=[fi.row_id(r) for r in FIRST_OF])
def test_torch_module_runs_the_same_kernel(r, engine):  # noqa: F811
    """engine.quantconv2d_float_input (the torch binding: its own plan call, workspace and stream) on one row per instance."""
    x, w, o64, y = _grid_case(r)
    wd = _t(w["wd"])
    bias = None if w["bias"] is None else _t(w["bias"])
    ye = engine.quantconv2d_float_input(_t(x), _t(w["wp"]), wd, _t(w["sw"]).reshape(-1, 1, 1, 1), _t(w["zw"]).reshape(-1, 1, 1, 1),
                                        bias, r.stride, r.pad)
    assert ye.dtype == torch.float32 and tuple(ye.shape) == y.shape and ye.is_contiguous()
    assert np.array_equal(ye.cpu().numpy(), y)


# ---- B: three non-zero bf16 parts -----------------------------------------------------------------------------------
def _bf16_trunc(a):
    return (a.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)


def _split_case(r):
    rng = _rng(r, "split")
    bits, signed = ((1, fi.weights_of(r)[1]) if fi.weights_of(r)[0] == 1 else (2, True))
    w = _weights(r, rng, exact=True, bits=bits, signed=signed)
    if w["bias"] is not None:
        # s_w V + bias = 2^-k V + m 2^-10 with |V| up to 2^24 is an fp32 number when the bias is a multiple of s_w as well
        # (k <= 10: bias = m 2^-k, still on the 2^-10 grid) or s_w of the bias's grid (k = 11: 2^-11 (V + 2 m))
        k = np.broadcast_to(-np.log2(w["sw"]), (r.OC,))
        w["bias"] = (rng.randint(-512, 513, size=r.OC) * 2.0 ** -np.minimum(k, 10)).astype(np.float32)
    K = r.IC * r.KH * r.KW
    shape = (r.N, r.IC, r.H, r.W)
    # 17 significant bits, odd; bit 8 set on 7 of 8 elements: then x1 = bits 16..9, x2 = bits 8..1, x3 = bit 0
    mag = (1 << 16) + (rng.randint(0, 128, size=shape) << 9) + ((rng.randint(0, 8, size=shape) > 0).astype(np.int64) << 8) \
        + (rng.randint(0, 128, size=shape) << 1) + 1
    x = (mag * rng.choice([-1, 1], size=shape)).astype(np.float32)
    assert np.array_equal(np.abs(x).astype(np.int64), mag) and (mag % 2 == 1).all() and (mag < 1 << 17).all()
    x1 = _bf16_trunc(x)
    x2 = _bf16_trunc(x - x1)
    x3 = x - x1 - x2
    assert np.array_equal((x1.astype(np.float64) + x2) + x3, x) and np.array_equal(_bf16_trunc(x3), x3)
    third = float((x3 != 0).mean())
    assert (x1 != 0).all() and (x2 != 0).all() and third > 0.75, third
    # S_xq: any partial sum is below sum |x| |q| < K 2^17 max|q| <= 2^24; S_x below K 2^17 <= 2^23: integers, exact
    assert K <= 64 and w["qmax"] <= 2 and K * (1 << 17) * w["qmax"] <= 1 << 24
    o64 = _oracle(r, x, w, "f64")
    # acc - z_w S_x is rounded once (fmaf): exact when the integer sum x (q - z_w) fits 24 bits, and so is s_w v + bias then
    sw = np.broadcast_to(w["sw"], (r.OC,)).astype(np.float64).reshape(1, -1, 1, 1)
    b = np.zeros(r.OC) if w["bias"] is None else w["bias"].astype(np.float64)
    v = (o64 - b.reshape(1, -1, 1, 1)) / sw
    assert np.array_equal(v, np.round(v)) and np.abs(v).max() < (1 << 24) - (1 << 11), np.abs(v).max()
    _assert_fp32_exact(o64, fi.row_id(r))
    return x, w, o64, third


@pytest.mark.parametrize("r", B_ROWS, ids=[fi.row_id(r) for r in B_ROWS])
def test_three_split_bit_exact(r):
    x, w, o64, third = _split_case(r)
    y = _run(r, x, w)
    want = o64.astype(np.float32)
    bad = ~(y == want)
    assert not bad.any(), "%s: %d of %d elements differ (third part non-zero on %.0f%% of x); first: got %r, float64 says %r" % (
        fi.row_id(r), int(bad.sum()), bad.size, 100 * third, y[bad][0], want[bad][0])


def test_three_split_rows_reach_every_instance():
    assert {r.instance for r in B_ROWS} == fi.every_instance()


# ---- C: the project's tolerance rule on random activations ------------------------------------------------------------
@pytest.mark.parametrize("r", fi.ROWS, ids=ROW_IDS)
def test_random_activations_within_the_conv_rule(r):
    rng = _rng(r, "normal")
    w = _weights(r, rng, exact=False)
    x = rng.normal(0, 1, size=(r.N, r.IC, r.H, r.W)).astype(np.float32)
    y = _run(r, x, w)
    o64, o32, fma = _oracle(r, x, w, "f64"), _oracle(r, x, w, "fp32"), _oracle(r, x, w, "fp32_fma")
    err, allowed = conv_tolerance(y, o64, o32, fma)
    print("C %s %s: worst err %.3g, allowed %.3g, ratio %.3f" % (r.instance, fi.row_id(r), float(np.nanmax(err)), allowed,
                                                                  float(np.nanmax(err)) / allowed))
    ok = err <= allowed                          # NaN compares false
    assert ok.all(), "%s: %d elements off, worst err %.3g (allowed %.3g)" % (fi.row_id(r), int((~ok).sum()),
                                                                             float(np.nanmax(err)), allowed)


# ---- D: identities ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", fi.ROWS, ids=ROW_IDS)
def test_prepared_and_unaligned_views_match_bit_for_bit(r):
    x, w, o64, y = _grid_case(r)
    assert np.array_equal(_run(r, x, w, prepared=True), y), "prepare + run on kept tables"
    for shift in (1, 2, 3):
        assert np.array_equal(_run(r, x, w, x_shift=shift), y), "x at +%d floats" % shift
    assert np.array_equal(_run(r, x, w, out_shift=1), y), "out at +1 float"


# ---- E: both sides of each planner boundary -----------------------------------------------------------------------------
@pytest.mark.parametrize("f", fi.FALLBACK, ids=["%s-%s" % (f[10], f[11].replace(" ", "_")) for f in fi.FALLBACK])
def test_planner_boundaries(f):
    r = fi.Row(*f[:9], f[10], "")
    rng = _rng(r, "boundary")
    w = _weights(r, rng, exact=False)
    x = rng.normal(0, 1, size=(r.N, r.IC, r.H, r.W)).astype(np.float32)
    with capi.knobs(**(f[9] or {})):
        p = capi.conv_f32_plan_info(capi.conv_shape(*f[:9]))
        assert (capi.F32_KERNELS[p.kernel] if p.ok else None) == f[10]
        y = _run(r, x, w, expect_path=int(f[10] is not None))
    fma = _oracle(r, x, w, "fp32_fma")
    if f[10] is None:
        assert np.array_equal(y, fma), f[11]              # the order-preserving kernel's contract
    else:
        o64 = _oracle(r, x, w, "f64")
        err, allowed = conv_tolerance(y, o64, _oracle(r, x, w, "fp32"), fma)
        assert (err <= allowed).all(), (f[11], float(np.nanmax(err)), allowed)


# ---- F: non-finite locality ---------------------------------------------------------------------------------------------
INF, NAN = float("inf"), float("nan")
NONFINITE = [
    # shape (N, IC, H, W, OC, KH, KW, stride, pad), [(n, c, h, w, value)], dependents expected, note
    ((1, 3, 20, 24, 8, 7, 7, 2, 3), [(0, 1, 5, 6, INF), (0, 0, 11, 10, -INF), (0, 2, 15, 14, NAN)], True,
     "stem 7x7/2 pad 3, even columns >= 4: column w is the zero-weight eighth tap of output column (w - 4) / 2"),
    ((1, 3, 20, 120, 8, 7, 7, 2, 3), [(0, 0, 2, 4, INF), (0, 1, 9, 118, -INF), (0, 2, 19, 60, NAN)], True,
     "stem 7x7/2 pad 3 on 14 column slots, two row tiles"),
    ((2, 4, 12, 12, 16, 5, 5, 1, 2), [(0, 3, 4, 5, INF), (1, 0, 7, 2, -INF), (1, 2, 11, 9, NAN)], True, "stem 5x5/1: 3 columns overhang"),
    ((1, 3, 10, 12, 70, 3, 3, 1, 1), [(0, 0, 2, 6, INF), (0, 1, 5, 9, -INF), (0, 2, 8, 3, NAN)], True,
     "stem 3x3/1, 128-channel tiles: 5 columns overhang"),
    ((1, 3, 6, 40, 8, 1, 1, 1, 0), [(0, 0, 1, 9, INF), (0, 1, 3, 20, -INF), (0, 2, 5, 39, NAN)], True, "stem 1x1, IC 3: 7 columns overhang"),
    ((1, 2, 9, 30, 64, 3, 3, 3, 0), [(0, 0, 2, 5, INF), (0, 1, 4, 16, -INF), (0, 1, 7, 28, NAN)], True, "stem 3x3/3, IC 2"),
    ((3, 16, 6, 6, 16, 3, 3, 1, 1), [(1, 3, 2, 2, INF), (1, 9, 0, 5, -INF), (1, 15, 5, 0, NAN)], True,
     "three images in one tile, the bad values in the middle one"),
    ((2, 16, 9, 9, 16, 1, 1, 2, 0), [(0, 3, 1, 4, INF), (1, 9, 4, 3, -INF), (1, 15, 7, 7, NAN)], False,
     "strided 1x1, the bad values at pixels no output samples"),
    ((2, 64, 9, 9, 16, 1, 1, 2, 0), [(0, 3, 2, 4, INF), (1, 9, 4, 3, -INF), (1, 63, 8, 8, NAN)], True,
     "strided 1x1 on a two-group instance, two sampled pixels and one that is not"),
    ((1, 16, 9, 11, 16, 3, 3, 1, 1), [(0, 3, 0, 10, INF), (0, 9, 4, 10, -INF), (0, 15, 8, 10, NAN)], True, "W % 4 = 3, the last column"),
    ((1, 21, 9, 9, 16, 3, 3, 1, 1), [(0, 20, 2, 2, INF), (0, 20, 5, 8, -INF), (0, 20, 8, 0, NAN)], True,
     "IC % 16 = 5, the last real channel"),
    ((2, 75, 7, 7, 130, 1, 1, 1, 0), [(0, 74, 2, 2, INF), (1, 74, 5, 6, -INF), (1, 64, 6, 0, NAN)], True,
     "IC % 16 = 11 on 128-channel tiles, the last real channel and the first of its group"),
]


@pytest.mark.parametrize("zeros", [False, True], ids=["zw0", "zw"])
@pytest.mark.parametrize("case", NONFINITE, ids=["case%d" % i for i in range(len(NONFINITE))])
def test_non_finite_locality(case, zeros):
    shape, bad, expect, note = case
    sh = capi.conv_shape(*shape)
    p = capi.conv_f32_plan_info(sh)
    assert p.ok, shape
    r = fi.Row(*shape, capi.F32_KERNELS[p.kernel], "" if zeros else "zw0")
    N, IC, H, W, OC, KH, KW, s, pad = shape
    rng = _rng(r, "nonfinite")
    w = _weights(r, rng, exact=False)
    x = rng.normal(0, 1, size=(N, IC, H, W)).astype(np.float32)
    xb, xc = x.copy(), x.copy()
    hit = np.zeros((N, p.OH, p.OW), bool)
    for (n, c, h, wc, v) in bad:
        xb[n, c, h, wc] = v
        xc[n, c, h, wc] = 0.0
        for oh in range(p.OH):
            for ow in range(p.OW):
                if 0 <= h - (oh * s - pad) < KH and 0 <= wc - (ow * s - pad) < KW:
                    hit[n, oh, ow] = True
    yb, yc = _run(r, xb, w), _run(r, xc, w)
    assert np.isfinite(yc).all()
    hit = np.broadcast_to(hit[:, None], yb.shape)
    assert hit.any() == expect, note
    print("F %s (%s): %d dependent outputs, %d non-finite" % (r.instance, note, int(hit.sum()), int((~np.isfinite(yb)).sum())))
    assert not np.isfinite(yb[hit]).any(), "%s: a dependent output is finite" % note
    leak = ~np.isfinite(yb) & ~hit
    assert not leak.any(), "%s (%s): %d outputs that do not depend on a bad activation are non-finite, first at %s" % (
        note, r.instance, int(leak.sum()), tuple(np.argwhere(leak)[0]))
    assert np.array_equal(yb[~hit], yc[~hit]), note
