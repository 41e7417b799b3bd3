"""The depthwise kernel instances (quantize_amd/csrc/qe_conv_dw.hip) as a table of problems, and their operands.  A plain
helper module for tests/test_dw_instances_{cpu,gpu}.py and tests/test_dw_mem_contract_gpu.py.

A row is (kernel, (N, C, H, W), (KH, KW), stride, pad, x, w, ops): kernel "fast" or "plain", x / w = (bits, sign), ops a set
of operand-set words (below).  The rows that depend on the plan's tiling (G planes per workgroup, TH rows per band) read G
and TH from qe_quantconv2d_depthwise_plan_info on a probe problem: nothing here names a number the kernel chose.

Operand-set words (the parity regime; the exact regime always uses power-of-two scales and integer zeros):
    sym      zeros 0 on both operands            intz    integer zeros          (default: non-integer zeros)
    xpc      per-channel x scale / zero          wpt     per-tensor w scale / zero   (default: x per tensor, w per channel)
    neg      a negative scale on each operand    nobias  bias None"""
import functools

import numpy as np

import dw_ref

S8, U8 = (8, 1), (8, 0)
SIGN_PAIRS = ((S8, S8), (S8, U8), (U8, S8), (U8, U8))


def _row(kernel, shape, k=(3, 3), stride=1, pad=1, x=U8, w=S8, ops=()):
    return (kernel, tuple(shape), tuple(k), stride, pad, x, w, frozenset(ops))


def shape_of(row):
    from quantize_amd import capi
    (N, C, H, W), (KH, KW) = row[1], row[2]
    return capi.conv_shape(N, C, H, W, C, KH, KW, row[3], row[4])


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
    lo, hi = dw_ref.code_range(bits, sign)
    return capi.requant(_Fake(n_param), _Fake(n_param), lo, hi, bits, sign)


def plan(row, rq=None, out=0, codes=0):
    from quantize_amd import capi
    C = row[1][1]
    return capi.depthwise_plan_info(shape_of(row), fake_qparam(*row[5], n_param=1 if "xpc" not in row[7] else C),
                                    fake_qparam(*row[6], n_param=C if "wpt" not in row[7] else 1), rq, out, codes)


def probe_TH(stride):
    """TH of the band plan at W = 20: the tallest plane is one band, so ask for a plane too tall for one."""
    H = 4096
    return plan(_row("fast", (1, 1, H, 20), stride=stride)).TH


def probe_G(stride):
    return plan(_row("fast", (64, 64, 7, 7), stride=stride)).G


@functools.lru_cache(maxsize=None)
def rows():
    out = []
    for s in (1, 2):
        shapes = [(1, 1, 1, 1), (2, 3, 2, 2), (1, 5, 3, 3), (2, 17, 7, 7), (1, 4, 14, 14)]
        shapes += [(1, 2, 5, W) for W in (4, 5, 8, 13, 15, 16, 17, 31, 33)]
        shapes += [(1, 2, 7, 8), (1, 2, 9, 6), (1, 2, 8, 8), (1, 2, 28, 28), (1, 2, 56, 56), (1, 1, 112, 112)]
        for sh in shapes:
            out.append(_row("fast", sh, stride=s))
        # bands: the output rows of a plane too tall for one workgroup, around multiples of TH
        TH = probe_TH(s)
        for OH in (TH - 1, TH, TH + 1, 2 * TH + 1):
            H = OH if s == 1 else 2 * OH - 1
            out.append(_row("fast", (1, 1, H, 20), stride=s, ops=("intz",)))
        G = probe_G(s)
        for NP in (G - 1, G, G + 1, 2 * G + 1):
            out.append(_row("fast", (1, NP, 7, 7), stride=s, ops=("xpc",)))
        # operand sets
        out.append(_row("fast", (2, 5, 9, 11), stride=s, x=S8, w=S8, ops=("sym",)))
        out.append(_row("fast", (2, 5, 9, 11), stride=s, ops=("intz",)))
        for xq, wq in SIGN_PAIRS:
            out.append(_row("fast", (1, 3, 6, 10), stride=s, x=xq, w=wq))
        out.append(_row("fast", (2, 5, 9, 11), stride=s, ops=("xpc",)))
        out.append(_row("fast", (2, 5, 9, 11), stride=s, ops=("wpt",)))
        out.append(_row("fast", (2, 5, 9, 11), stride=s, ops=("neg",)))
        out.append(_row("fast", (2, 5, 9, 11), stride=s, ops=("nobias",)))
    for xq, wq in (((1, 0), (1, 1)), ((2, 1), (8, 0)), ((4, 0), (4, 1)), ((8, 1), (3, 0)), ((7, 0), (5, 1))):
        out.append(_row("plain", (1, 3, 5, 7), stride=1, x=xq, w=wq))
    out.append(_row("plain", (1, 3, 11, 13), k=(5, 5), stride=3, pad=2))
    out.append(_row("plain", (2, 3, 4, 9), k=(1, 3), stride=1, pad=0))
    out.append(_row("plain", (1, 3, 6, 7), k=(3, 3), stride=1, pad=0))
    out.append(_row("plain", (1, 2, 4, 4), k=(7, 7), stride=1, pad=3))
    out.append(_row("plain", (1, 3, 6, 7), k=(3, 3), stride=3, pad=1, ops=("xpc", "neg")))
    return tuple(out)


def row_id(k):
    kernel, sh, kk, s, p, x, w, ops = rows()[k]
    return "%d-%s-%s-k%dx%d-s%d-p%d-%s%d%s%d%s" % (k, kernel, "x".join(map(str, sh)), kk[0], kk[1], s, p, "su"[1 - x[1]], x[0],
                                                 "su"[1 - w[1]], w[0], "".join("-" + o for o in sorted(ops)))


def _codes(rng, shape, bits, sign):
    lo, hi = dw_ref.code_range(bits, sign)
    q = rng.integers(lo, hi + 1, size=shape, dtype=np.int64)
    q.flat[0], q.flat[-1] = lo, hi           # both ends of the code range, at both ends of the stream
    return q


@functools.lru_cache(maxsize=None)
def operands(k, regime):
    """regime "exact": power-of-two scales, integer zeros, bias an integer number of grid units -- every sum an integer far
    below 2^24 grid units (49 * 255 * 255 < 2^22).  "parity": ordinary fp32 scales and (by default non-integer) zeros."""
    kernel, (N, C, H, W), (KH, KW), stride, pad, (xb, xs), (wb, ws), ops = rows()[k]
    rng = np.random.default_rng(1000 + k)
    qx = _codes(rng, (N, C, H, W), xb, xs)
    qw = _codes(rng, (C, KH, KW), wb, ws)
    nx, nw = (C if "xpc" in ops else 1), (1 if "wpt" in ops else C)
    xlo, xhi = dw_ref.code_range(xb, xs)
    wlo, whi = dw_ref.code_range(wb, ws)
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
    if "neg" in ops:
        sx, sw = sx.copy(), sw.copy()
        sx[0], sw[-1] = -sx[0], -sw[-1]
    sx, sw, zx, zw = (v.astype(np.float32) for v in (sx, sw, zx, zw))
    lsb = np.abs((np.full(C, sx[0]) if nx == 1 else sx).astype(np.float64) * (np.full(C, sw[0]) if nw == 1 else sw))
    if "nobias" in ops:
        bias = None
    elif regime == "exact":
        bias = (rng.integers(-2000, 2001, size=C) * lsb).astype(np.float32)
    else:
        bias = rng.uniform(-1, 1, size=C).astype(np.float32)
    return dict(qx=qx, qw=qw, x=dw_ref.pack(qx, xb, xs), w=dw_ref.pack(qw, wb, ws), sx=sx, zx=zx, sw=sw, zw=zw, bias=bias, lsb=lsb,
                stride=stride, pad=pad)


@functools.lru_cache(maxsize=None)
def reference(k, regime, relu=False):
    o = operands(k, regime)
    return dw_ref.conv(o["qx"], o["sx"], o["zx"], o["qw"], o["sw"], o["zw"], o["bias"], o["stride"], o["pad"], relu=relu)


@functools.lru_cache(maxsize=None)
def chain(k):
    """The reference's packed forward on the parity operands: fp32 F.conv2d(groups=C) on the dequantised tensors, on the CPU."""
    import torch
    import torch.nn.functional as F
    o = operands(k, "parity")
    C = o["qx"].shape[1]

    def deq(q, s, z, shape):
        s, z = (torch.from_numpy(np.full(C, v[0], np.float32) if v.size == 1 else v).reshape(shape) for v in (s, z))
        return (torch.from_numpy(q.astype(np.float32)) - z) * s

    x = deq(o["qx"], o["sx"], o["zx"], (1, C, 1, 1))
    w = deq(o["qw"], o["sw"], o["zw"], (C, 1, 1)).unsqueeze(1)
    b = None if o["bias"] is None else torch.from_numpy(o["bias"])
    return F.conv2d(x, w, b, stride=o["stride"], padding=o["pad"], groups=C).numpy()


def consumer(k, which, regime="exact"):
    """A consumer quantiser for row k's output: (scale, zero, qmin, qmax, bits, sign) with scale / zero fp32 arrays.
    which: "u8" per tensor unsigned, "s8c" per channel signed, "u4" / "s3c" the sub-8-bit ones."""
    C = rows()[k][1][1]
    ref = reference(k, regime, relu=False)
    amax = max(float(np.nanmax(np.abs(ref))), 1e-3)
    bits, sign, per_channel = {"u8": (8, 0, False), "s8c": (8, 1, True), "u4": (4, 0, False), "s3c": (3, 1, True)}[which]
    lo, hi = dw_ref.code_range(bits, sign)
    n = C if per_channel else 1
    if regime == "exact":
        step = 2.0 ** np.ceil(np.log2(2 * amax / (hi - lo)))
        scale = np.full(n, step) * (2.0 ** (np.arange(n) % 2))
        zero = np.full(n, float(-(lo + hi + 1) // 2 if not sign else 0)) + (np.arange(n) % 3)
    else:
        scale = np.full(n, 2 * amax / (hi - lo) * 0.9) * (1 + 0.1 * (np.arange(n) % 3))
        zero = np.full(n, -(lo + hi) / 2.0 + 0.3) + (np.arange(n) % 3)
    return scale.astype(np.float32), zero.astype(np.float32), float(lo), float(hi), bits, sign
