"""The instances of qe_avgpool2d_codes (quantize_amd/csrc/qe_pool.hip) as a table of problems, their operands, and the
module-form cases.  A plain helper module for tests/test_pool_*.py.

A row is (instance, (N, C, H, W), kernel, stride, output_size, x_sign, xpc, rq): instance "pair" | "plane" | "plain" is what the
host-side plan must answer for it; kernel 0 = adaptive to output_size; xpc = per-channel x scale / zero'; rq = the consumer the
row's codes epilogues use: "u8" 8-bit per tensor, "s8c" 8-bit per channel signed, "u4" 4-bit per tensor (the plain instance,
whatever the geometry)."""
import functools

import numpy as np

import pool_ref

EPILOGUES = ("out", "codes", "both")


def _row(inst, shape, kernel=0, stride=None, osize=None, x_sign=0, xpc=False, rq="u8"):
    return (inst, tuple(shape), kernel, kernel if stride is None else stride, osize, x_sign, xpc, rq)


ROWS = (
    # pair: kernel == stride == 2 (CLIP).  8x8; a 17-output row (one chunk and a ragged one); 33-output rows (two chunks and a
    # ragged one) on more than one workgroup's worth of rows; odd H and W, where the last row and column drop
    _row("pair", (2, 3, 8, 8), 2),
    _row("pair", (1, 2, 6, 34), 2, x_sign=1, rq="s8c"),
    _row("pair", (2, 5, 10, 66), 2, xpc=True),
    _row("pair", (1, 3, 9, 11), 2, rq="s8c"),
    # plane: the whole plane, P = 49, 64 (as a fixed 8 x 8 window: wrn_40_2), 241, 3136
    _row("plane", (2, 3, 7, 7), 0, osize=(1, 1), rq="s8c"),
    _row("plane", (2, 4, 8, 8), 8, x_sign=1),
    _row("plane", (1, 2, 1, 241), 0, osize=(1, 1), xpc=True),
    _row("plane", (1, 2, 56, 56), 0, osize=(1, 1)),
    _row("plane", (3, 70, 7, 7), 0, osize=(1, 1), xpc=True, rq="s8c"),          # more planes than a workgroup takes
    # plain: every other problem
    _row("plain", (2, 4, 16, 16), 8, 8, rq="s8c"),
    _row("plain", (1, 3, 9, 11), 3, 2, x_sign=1),
    _row("plain", (2, 6, 8, 9), 0, osize=(5, 7), xpc=True),
    # sub-8-bit consumers take the plain instance on any geometry
    _row("plain", (2, 3, 8, 8), 2, rq="u4"),
    _row("plain", (2, 3, 7, 7), 0, osize=(1, 1), rq="u4"),
    _row("plain", (2, 6, 8, 9), 0, osize=(5, 7), x_sign=1, rq="u4"),
)

RQ_KINDS = {"u8": (8, 0, False), "s8c": (8, 1, True), "u4": (4, 0, False)}


def row_id(k):
    inst, sh, kernel, stride, osize, xs, xpc, rq = ROWS[k]
    geo = "k%ds%d" % (kernel, stride) if kernel else "a%dx%d" % osize
    return "%d-%s-%s-%s-%s%s-%s" % (k, inst, "x".join(map(str, sh)), geo, "su"[1 - xs], "-xpc" if xpc else "", rq)


def out_hw(row):
    _, (N, C, H, W), kernel, stride, osize = row[:5]
    return ((H - kernel) // stride + 1, (W - kernel) // stride + 1) if kernel else osize


class _Fake:
    """Pointer stand-in for the host-side query."""

    def __init__(self, n, ptr=256):
        self._n, self._p = n, ptr

    def data_ptr(self):
        return self._p

    def numel(self):
        return self._n


def path(k, ep="both", relu=False, x_ptr=256, out_ptr=256, codes_ptr=256):
    """qe_avgpool2d_codes_path of row k in epilogue ep, with the operands at the given addresses."""
    from quantize_amd import capi
    inst, (N, C, H, W), kernel, stride, osize, xs, xpc, rqk = ROWS[k]
    bits, sign, pc = RQ_KINDS[rqk]
    xq = capi.qparam(_Fake(1, x_ptr), 8, xs, _Fake(C if xpc else 1), _Fake(C if xpc else 1))
    lo, hi = pool_ref.code_range(bits, sign)
    rq = capi.requant(_Fake(C if pc else 1), _Fake(C if pc else 1), lo, hi, bits, sign) if ep != "out" else None
    return capi.avgpool2d_codes_path(xq, N, C, H, W, kernel, stride, osize, relu=relu, rq=rq, out=0 if ep == "codes" else out_ptr,
                                     codes=codes_ptr)


@functools.lru_cache(maxsize=None)
def operands(k, regime):
    """regime "exact": scale a power of two and zero' an integer (every value an exact rational rounded once); "parity": ordinary
    fp32 scales and non-integer zero'."""
    inst, (N, C, H, W), kernel, stride, osize, xs, xpc, rqk = ROWS[k]
    rng = np.random.default_rng(7000 + k)
    stored = rng.integers(0, 256, size=(N, C, H, W), dtype=np.int64).astype(np.uint8)
    stored.flat[0], stored.flat[-1] = 0, 255
    n = C if xpc else 1
    lo, hi = pool_ref.code_range(8, xs)
    if regime == "exact":
        sx = 2.0 ** -rng.integers(2, 7, size=n).astype(np.float64)
        zx = np.rint(rng.uniform(lo, hi, size=n) / 2)
    else:
        sx = rng.uniform(0.01, 0.05, size=n)
        zx = rng.uniform(lo, hi, size=n) / 2 + 0.37
    return dict(x=stored, q=pool_ref.decode(stored, xs), sx=sx.astype(np.float32), zx=zx.astype(np.float32))


@functools.lru_cache(maxsize=None)
def reference(k, regime, relu):
    """pool_ref's value of row k: computed once, shared, never written to."""
    row = ROWS[k]
    o = operands(k, regime)
    OH, OW = out_hw(row)
    y = pool_ref.avgpool2d_codes(o["q"], o["sx"], o["zx"], row[2], row[3], OH, OW, relu_taps=relu)
    y.setflags(write=False)
    return y


def consumer(k, regime):
    """The row's consumer quantiser: (scale, zero, qmin, qmax, bits, sign), sized so that no code leaves its range."""
    C = ROWS[k][1][1]
    bits, sign, pc = RQ_KINDS[ROWS[k][7]]
    amax = max(max(float(np.abs(reference(k, regime, r)).max()) for r in (False, True)), 1e-3)
    lo, hi = pool_ref.code_range(bits, sign)
    n = C if pc else 1
    if regime == "exact":
        scale = np.full(n, 2.0 ** np.ceil(np.log2(2 * amax / (hi - lo)))) * (2.0 ** (np.arange(n) % 2))
        zero = np.full(n, float(-(lo + hi + 1) // 2)) + (np.arange(n) % 3)
    else:
        scale = np.full(n, 2 * amax / (hi - lo) * 1.1) * (1 + 0.1 * (np.arange(n) % 3))
        zero = np.full(n, -(lo + hi) / 2.0 + 0.3) + (np.arange(n) % 3) * 0.5
    return scale.astype(np.float32), zero.astype(np.float32), float(lo), float(hi), bits, sign


# ---- module forms ------------------------------------------------------------------------------------------------------------
SHAPES = ((2, 3, 7, 7), (1, 2, 5, 33), (2, 5, 9, 11), (3, 17, 8, 8))
MAX_GEOMETRIES = ((3, 2, 1), (2, 2, 0), (3, 1, 1), (2, 1, 1))          # (kernel, stride, padding)
AVG_SIZES = ((1, 1), (5, 7), (2, 3))
# (bits, signed, per channel)
QUANTISERS = ((8, 1, False), (8, 0, False), (4, 0, False), (8, 0, True), (4, 1, True))


def module_quantiser(shape, which, seed=0):
    """(scale, zero, qmin, qmax) of a module-form case, module convention; the data below spans a little more than its range."""
    bits, sign, pc = which
    C = shape[1]
    rng = np.random.default_rng(900 + seed)
    lo, hi = pool_ref.code_range(bits, sign)
    n = C if pc else 1
    scale = (3.0 / (hi - lo)) * rng.uniform(0.8, 1.25, size=n)
    zero = np.zeros(n) if sign else -rng.uniform(0.2, 0.45, size=n) * (hi - lo)
    return scale.astype(np.float32), zero.astype(np.float32), float(lo), float(hi)


def module_input(shape, seed=0, nonfinite=False):
    rng = np.random.default_rng(500 + seed)
    x = rng.normal(0.0, 0.8, size=shape).astype(np.float32)
    if nonfinite:                         # known windows: the first plane's corner, a middle element, the last element
        x[0, 0, 0, 0] = np.nan
        x[0, -1, shape[2] // 2, shape[3] // 2] = np.inf
        x[-1, -1, -1, -1] = -np.inf
        x[-1, 0, 0, -1] = np.nan
    return x
