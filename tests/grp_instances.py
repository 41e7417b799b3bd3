"""The grouped kernel instances (quantize_amd/csrc/qe_conv_grp.hip) as a table of problems, and their operands.  A plain
helper module for tests/test_grp_instances_{cpu,gpu}.py and tests/test_grp_mem_contract_gpu.py.

A row is (kernel, (N, IC, H, W), (KH, KW), stride, pad, x, w, ops, groups, OC): kernel "fast" or "plain", x / w = (bits,
sign), ops a set of operand-set words (below).  The rows that depend on the plan's tiling (the slab width, the TH rows of a
band) read them from qe_quantconv2d_grouped_plan_info on a probe problem: nothing here names a number the kernel chose.
A fast tile is a band of whole rows (TW == OW), so the tile-edge rows vary the height; the widths are covered by the
H = 5 rows.

Operand-set words (the parity regime; the exact regime always uses power-of-two scales and integer zeros):
    sym      zeros 0 on both operands            intz    integer zeros          (default: non-integer zeros)
    xpc      per-input-channel x scale / zero    wpt     per-tensor w scale / zero   (default: x per tensor, w per channel)
    neg      a negative scale on each operand    nobias  bias None
Per-input-channel activation parameters do not factor out of the channel sum, so the xpc rows are the plain kernel's."""
import functools

import numpy as np

import grp_ref

S8, U8 = (8, 1), (8, 0)
SIGN_PAIRS = ((S8, S8), (S8, U8), (U8, S8), (U8, U8))
FAST_CG = (4, 8, 16, 32)
TWO24 = 1 << 24
BIAS_UNITS = 2000


def _row(kernel, shape, cg, k=(3, 3), stride=1, pad=1, x=U8, w=S8, ops=(), OC=None):
    """cg: input channels of a group."""
    N, IC, H, W = shape
    assert IC % cg == 0
    if "xpc" in ops:
        kernel = "plain"
    return (kernel, tuple(shape), tuple(k), stride, pad, x, w, frozenset(ops), IC // cg, IC if OC is None else OC)


def shape_of(row):
    from quantize_amd import capi
    (N, IC, H, W), (KH, KW) = row[1], row[2]
    return capi.conv_shape(N, IC, H, W, row[9], KH, KW, row[3], row[4])


class _Fake:
    """Pointer stand-in: the host-side queries look at formats and counts only."""

    def __init__(self, n):
        self._n = n

    def data_ptr(self):
        return 256

    def numel(self):
        return self._n


def fake_qparam(bits, sign, n_param=1):
    from quantize_amd import capi
    return capi.qparam(_Fake(1), bits, sign, _Fake(n_param), _Fake(n_param))


def fake_requant(bits=8, sign=0, n_param=1):
    from quantize_amd import capi
    lo, hi = grp_ref.code_range(bits, sign)
    return capi.requant(_Fake(n_param), _Fake(n_param), lo, hi, bits, sign)


def plan(row, rq=None, out=0, codes=0):
    from quantize_amd import capi
    IC, OC = row[1][1], row[9]
    return capi.grouped_plan_info(shape_of(row), row[8], fake_qparam(*row[5], n_param=1 if "xpc" not in row[7] else IC),
                                  fake_qparam(*row[6], n_param=OC if "wpt" not in row[7] else 1), rq, out, codes)


def probe_slab(cg):
    return plan(_row("fast", (1, 8 * cg, 8, 8), cg)).slab


def probe_TH(cg, stride):
    """TH of a plane too tall for one band, at W = 20."""
    return plan(_row("fast", (1, 2 * cg, 4096, 20), cg, stride=stride)).TH


@functools.lru_cache(maxsize=None)
def rows():
    out = []
    for cg in FAST_CG:
        slab = probe_slab(cg)
        one = max(slab, 2 * cg)               # one slab, or the two groups a grouped layer has at least
        for s in (1, 2):
            for hw in ((1, 1), (2, 2), (3, 3), (7, 7), (14, 14)):
                out.append(_row("fast", (1, one) + hw, cg, stride=s))
            for W in (4, 5, 8, 13, 15, 16, 17, 31, 33):
                out.append(_row("fast", (1, one, 5, W), cg, stride=s))
            out.append(_row("fast", (1, one, 56, 56), cg, stride=s, ops=("intz",)))
            # one slab plus one group (a partial last slab), three slabs, N = 2
            out.append(_row("fast", (1, slab + cg, 6, 9), cg, stride=s))
            out.append(_row("fast", (1, 3 * slab, 6, 9), cg, stride=s))
            out.append(_row("fast", (2, slab + cg, 9, 11), cg, stride=s))
            # bands: the output rows of a plane too tall for one workgroup, around multiples of TH
            TH = probe_TH(cg, s)
            for OH in (TH - 1, TH, TH + 1, 2 * TH + 1):
                if OH < 1:
                    continue
                H = OH if s == 1 else 2 * OH - 1
                out.append(_row("fast", (1, 2 * cg, H, 20), cg, stride=s, ops=("intz",)))
            # operand sets
            out.append(_row("fast", (2, slab + cg, 5, 7), cg, stride=s, x=S8, w=S8, ops=("sym",)))
            out.append(_row("fast", (2, slab + cg, 5, 7), cg, stride=s, ops=("intz",)))
            for xq, wq in SIGN_PAIRS:
                out.append(_row("fast", (1, 2 * cg, 6, 10), cg, stride=s, x=xq, w=wq))
            out.append(_row("fast", (2, 2 * cg, 5, 7), cg, stride=s, ops=("xpc",)))
            out.append(_row("fast", (2, slab + cg, 5, 7), cg, stride=s, ops=("wpt",)))
            out.append(_row("fast", (2, slab + cg, 5, 7), cg, stride=s, ops=("neg",)))
            out.append(_row("fast", (2, slab + cg, 5, 7), cg, stride=s, ops=("nobias",)))
    for xq, wq in (((1, 0), (1, 1)), ((2, 1), (8, 0)), ((4, 0), (4, 1)), ((8, 1), (3, 0)), ((7, 0), (5, 1))):
        out.append(_row("plain", (1, 6, 5, 7), 2, stride=1, x=xq, w=wq))
    out.append(_row("plain", (1, 6, 5, 7), 3, OC=4))                         # 6 -> 4 channels in 2 groups
    out.append(_row("plain", (2, 4, 6, 5), 2, OC=6, ops=("xpc", "neg")))
    out.append(_row("plain", (1, 6, 11, 13), 3, k=(5, 5), stride=3, pad=2))
    out.append(_row("plain", (2, 6, 4, 9), 2, k=(1, 3), stride=1, pad=0))
    out.append(_row("plain", (1, 6, 6, 7), 3, k=(3, 3), stride=1, pad=0))
    out.append(_row("plain", (1, 4, 4, 4), 2, k=(7, 7), stride=1, pad=3))
    out.append(_row("plain", (1, 128, 5, 6), 64))                             # Cg = 64
    out.append(_row("plain", (1, 128, 5, 6), 64, stride=2))
    return tuple(out)


def row_id(k):
    kernel, sh, kk, s, p, x, w, ops, g, OC = rows()[k]
    return "%d-%s-%s-g%d-oc%d-k%dx%d-s%d-p%d-%s%d%s%d%s" % (k, kernel, "x".join(map(str, sh)), g, OC, kk[0], kk[1], s, p,
                                                          "su"[1 - x[1]], x[0], "su"[1 - w[1]], w[0],
                                                          "".join("-" + o for o in sorted(ops)))


def expected_kernel(row, e):
    """The plan's instance number of a row with epilogue e (0 fp32 out, 1 codes, 2 both)."""
    if row[0] == "plain":
        return 0
    cg = row[1][1] // row[8]
    return 1 + 6 * FAST_CG.index(cg) + 3 * (row[3] - 1) + e


@functools.lru_cache(maxsize=None)
def operands(k, regime):
    """regime "exact": power-of-two scales, integer zeros, bias an integer number of grid units, and weight codes kept so close
    to their zero point that K max|qx - zx| max|qw - zw| + |bias units| < 2^24 (K = KH KW IC / groups): every intermediate,
    (float)I included, is an integer below 2^24 grid units and exact in fp32.  "parity": ordinary fp32 scales and (by default
    non-integer) zeros over the full code ranges."""
    kernel, (N, IC, H, W), (KH, KW), stride, pad, (xb, xs), (wb, ws), ops, groups, OC = rows()[k]
    rng = np.random.default_rng(2000 + k)
    ICg = IC // groups
    nx, nw = (IC if "xpc" in ops else 1), (1 if "wpt" in ops else OC)
    xlo, xhi = grp_ref.code_range(xb, xs)
    wlo, whi = grp_ref.code_range(wb, ws)
    qx = rng.integers(xlo, xhi + 1, size=(N, IC, H, W), dtype=np.int64)
    qx.flat[0], qx.flat[-1] = xlo, xhi          # both ends of the code range, at both ends of the stream
    if regime == "exact":
        sx = 2.0 ** -rng.integers(2, 6, size=nx)
        sw = 2.0 ** -rng.integers(3, 8, size=nw)
        zx = np.rint(rng.uniform(xlo, xhi, size=nx) / 2)
        zw = np.rint(rng.uniform(wlo, whi, size=nw) / 4) + 1
    else:
        sx = rng.uniform(0.01, 0.05, size=nx)
        sw = rng.uniform(0.002, 0.01, size=nw)
        zx = rng.uniform(xlo, xhi, size=nx) / 2 + 0.37
        zw = rng.uniform(wlo, whi, size=nw) / 4 + 0.21
        if "intz" in ops:
            zx, zw = np.rint(zx), np.rint(zw) + 1
    if "sym" in ops:
        zx, zw = np.zeros(nx), np.zeros(nw)
    qw = rng.integers(wlo, whi + 1, size=(OC, ICg, KH, KW), dtype=np.int64)
    if regime == "exact":
        a_max = int(max(np.abs(xlo - zx).max(), np.abs(xhi - zx).max()))
        ratio = 8 if nx > 1 else 1          # per-channel x scales span 2^-2 .. 2^-5: the budget in units of the finest
        cap = (TWO24 - 1 - ratio * BIAS_UNITS) // (KH * KW * ICg * a_max * ratio)
        assert cap >= 1
        zwc = np.full(OC, zw[0]) if nw == 1 else zw
        lo = np.maximum(wlo, zwc - cap)[:, None, None, None]
        hi = np.minimum(whi, zwc + cap)[:, None, None, None]
        qw = np.clip(qw, lo, hi).astype(np.int64)
    else:
        qw.flat[0], qw.flat[-1] = wlo, whi
    if "neg" in ops:
        sx, sw = sx.copy(), sw.copy()
        sx[0], sw[-1] = -sx[0], -sw[-1]
    sx, sw, zx, zw = (v.astype(np.float32) for v in (sx, sw, zx, zw))
    # the grid of an output: its group's finest x scale times its w scale; an exact bias sits on the coarsest (a multiple)
    sxa = np.abs(np.full(IC, sx[0]) if nx == 1 else sx).astype(np.float64).reshape(groups, ICg)
    swa = np.abs(np.full(OC, sw[0]) if nw == 1 else sw).astype(np.float64)
    lsb = np.repeat(sxa.min(axis=1), OC // groups) * swa
    bias_lsb = np.repeat(sxa.max(axis=1), OC // groups) * swa
    if "nobias" in ops:
        bias = None
    elif regime == "exact":
        bias = (rng.integers(-BIAS_UNITS, BIAS_UNITS + 1, size=OC) * bias_lsb).astype(np.float32)
    else:
        bias = rng.uniform(-1, 1, size=OC).astype(np.float32)
    return dict(qx=qx, qw=qw, x=grp_ref.pack(qx, xb, xs), w=grp_ref.pack(qw, wb, ws), sx=sx, zx=zx, sw=sw, zw=zw, bias=bias, lsb=lsb,
                stride=stride, pad=pad, groups=groups)


@functools.lru_cache(maxsize=None)
def reference(k, regime, relu=False):
    o = operands(k, regime)
    return grp_ref.conv(o["qx"], o["sx"], o["zx"], o["qw"], o["sw"], o["zw"], o["bias"], o["groups"], o["stride"], o["pad"], relu=relu)


@functools.lru_cache(maxsize=None)
def chain(k):
    o = operands(k, "parity")
    return grp_ref.chain(o["qx"], o["sx"], o["zx"], o["qw"], o["sw"], o["zw"], o["bias"], o["groups"], o["stride"], o["pad"])


def consumer(k, which, regime="exact"):
    """A consumer quantiser for row k's output: (scale, zero, qmin, qmax, bits, sign) with scale / zero fp32 arrays.
    which: "u8" per tensor unsigned, "s8c" per channel signed, "u4" / "s3c" the sub-8-bit ones."""
    C = rows()[k][9]
    ref = reference(k, regime, relu=False)
    amax = max(float(np.nanmax(np.abs(ref))), 1e-3)
    bits, sign, per_channel = {"u8": (8, 0, False), "s8c": (8, 1, True), "u4": (4, 0, False), "s3c": (3, 1, True)}[which]
    lo, hi = grp_ref.code_range(bits, sign)
    n = C if per_channel else 1
    if regime == "exact":
        step = 2.0 ** np.ceil(np.log2(2 * amax / (hi - lo)))
        scale = np.full(n, step) * (2.0 ** (np.arange(n) % 2))
        zero = np.full(n, float(-(lo + hi + 1) // 2 if not sign else 0)) + (np.arange(n) % 3)
    else:
        scale = np.full(n, 2 * amax / (hi - lo) * 0.9) * (1 + 0.1 * (np.arange(n) % 3))
        zero = np.full(n, -(lo + hi) / 2.0 + 0.3) + (np.arange(n) % 3)
    return scale.astype(np.float32), zero.astype(np.float32), float(lo), float(hi), bits, sign
