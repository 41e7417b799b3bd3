"""The instances of qe_affine_relu_quantize_pack (quantize_amd/csrc/qe_preact.hip) as a table of problems, their operands and
their references.  A plain helper module for tests/test_preact_*.py.

A row is (instance, (N, C, P), rqs): instance "fast" | "plain" is what the host-side plan must answer for the row with its
consumers; rqs names up to two consumer quantisers (RQ_KINDS).  FORMS are the output forms every row runs in: (identity, sum,
act) with sum None | "new" | "identity" (in place on identity) | "x" (in place on x).  n_out 0, 1 and 2 are the row's rqs[:n]."""
import functools

import numpy as np

import preact_ref

GRID_CAP = 256 * 8                # PREACT_MAX_BLOCKS of qe_preact.hpp: kNumCU * 8
THREADS, PLAIN_VEC, FAST_VEC = 256, 8, 16

# kind -> (bits, signed, per channel, negative scale, non-zero zero point)
RQ_KINDS = {"u8": (8, 0, False, False, False), "u8z": (8, 0, False, False, True), "s8": (8, 1, False, False, False),
            "s8c": (8, 1, True, False, True), "u8c": (8, 0, True, False, True), "n8": (8, 1, False, True, True),
            "u4": (4, 0, False, False, False), "s4c": (4, 1, True, False, True), "u1": (1, 0, False, False, False),
            "s1": (1, 1, False, False, False)}

ROWS = (
    # fast: 8-bit consumers on planes of 16, 64 and 256 elements (WideResNet's 8x8 and 16x16 maps), C = 3 and 5
    ("fast", (2, 3, 16), ("u8", "s8c")),
    ("fast", (2, 5, 64), ("u8c", "u8z")),
    ("fast", (2, 3, 256), ("n8", "s8")),
    ("fast", (2, 5, 16), ("s8c", "u8c")),
    # plain: ragged planes, from one element to one that is no multiple of 8
    ("plain", (2, 3, 1), ("u8", "s8c")),
    ("plain", (2, 5, 7), ("u8z", "u8c")),
    ("plain", (2, 3, 15), ("s8c", "n8")),
    ("plain", (2, 5, 17), ("u8c", "s8")),
    ("plain", (2, 3, 63), ("n8", "u8z")),
    ("plain", (2, 5, 1000), ("s8", "u8c")),
    # plain: a sub-8-bit consumer moves a 16-multiple plane there too; 4-bit and 1-bit codes, alone and beside an 8-bit consumer
    ("plain", (2, 3, 64), ("u4", "s8c")),
    ("plain", (2, 5, 16), ("s4c", "u1")),
    ("plain", (2, 3, 17), ("s1", "u4")),
    ("plain", (2, 5, 63), ("u1", "s4c")),
)

FORMS = tuple((ident, s, act) for ident in (True, False) for s in (None, "new", "identity", "x") for act in (False, True)
              if not (s == "identity" and not ident))


def row_id(k):
    inst, (N, C, P), rqs = ROWS[k]
    return "%d-%s-%dx%dx%d-%s" % (k, inst, N, C, P, "+".join(rqs))


def form_id(form):
    ident, s, act = form
    return "%s-sum_%s-%s" % ("id" if ident else "noid", s or "off", "act" if act else "noact")


class _Fake:
    """Pointer stand-in for the host-side query."""

    def __init__(self, n, ptr=256):
        self._n, self._p = n, ptr

    def data_ptr(self):
        return self._p

    def numel(self):
        return self._n


def fake_rq(kind, C):
    from quantize_amd import capi
    bits, sign, pc = RQ_KINDS[kind][:3]
    lo, hi = preact_ref.code_range(bits, sign)
    return capi.requant(_Fake(C if pc else 1), _Fake(C if pc else 1), lo, hi, bits, sign)


def path(k, n_out, sum_ptr=256, act_ptr=0):
    """qe_affine_relu_quantize_pack_path of row k with its first n_out consumers and the outputs at the given addresses."""
    from quantize_amd import capi
    inst, (N, C, P), rqs = ROWS[k]
    return capi.affine_relu_quantize_pack_path(N, C, P, [fake_rq(r, C) for r in rqs[:n_out]], sum_out=sum_ptr, act_out=act_ptr)


def expected_instance(k, n_out):
    inst, (N, C, P), rqs = ROWS[k]
    return "fast" if P % FAST_VEC == 0 and all(RQ_KINDS[r][0] == 8 for r in rqs[:n_out]) else "plain"


def draw(seed, N, C, P):
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 1.0, size=(N, C, P)).astype(np.float32)
    identity = rng.normal(0.0, 1.0, size=(N, C, P)).astype(np.float32)
    alpha = (rng.uniform(0.5, 1.5, size=C) * np.where(np.arange(C) % 3 == 1, -1.0, 1.0)).astype(np.float32)
    shift = rng.normal(0.2, 0.5, size=C).astype(np.float32)
    return dict(x=x, identity=identity, alpha=alpha, shift=shift)


@functools.lru_cache(maxsize=None)
def operands(k):
    inst, (N, C, P), rqs = ROWS[k]
    o = draw(8100 + k, N, C, P)
    for v in o.values():
        v.setflags(write=False)
    return o


def quantiser(kind, C, amax, seed=0):
    """(scale, zero, qmin, qmax, bits, sign) of a consumer whose codes of values in [0, amax] stay in range (a is post-ReLU)."""
    bits, sign, pc, neg, nz = RQ_KINDS[kind]
    lo, hi = preact_ref.code_range(bits, sign)
    n = C if pc else 1
    rng = np.random.default_rng(300 + seed)
    span = max(hi - lo, 1)
    scale = (max(amax, 1e-3) / span) * 1.07 * rng.uniform(1.0, 1.3, size=n)
    if not nz:
        # q = a / scale - zero over [0, amax / scale]: put it at the bottom of the range
        zero = np.full(n, float(-lo))
    else:
        zero = np.full(n, float(-lo)) - rng.uniform(0.1, 0.4, size=n)
    if bits <= 1:
        zero = np.full(n, float(-lo))
    if neg:                          # a negative scale mirrors q: the values sit at the top of the range instead
        scale, zero = -scale, -(zero + (hi + lo))
    return scale.astype(np.float32), zero.astype(np.float32), float(lo), float(hi), bits, sign


@functools.lru_cache(maxsize=None)
def consumers(k):
    inst, (N, C, P), rqs = ROWS[k]
    o = operands(k)
    amax = max(float(preact_ref.activated(o["x"], ident, o["alpha"], o["shift"])[1].max()) for ident in (o["identity"], None))
    return tuple(quantiser(r, C, amax, seed=7 * k + i) for i, r in enumerate(rqs))


@functools.lru_cache(maxsize=None)
def reference(k, with_identity):
    """preact_ref's answer for row k with both consumers: computed once, shared, never written to."""
    o = operands(k)
    ref = preact_ref.forward(o["x"], o["identity"] if with_identity else None, o["alpha"], o["shift"], consumers(k))
    for v in [ref["s"], ref["a"]] + ref["q"] + ref["codes"]:
        v.setflags(write=False)
    return ref


# ---- the tie-dense input -----------------------------------------------------------------------------------------------------
def tie_dense(N=2, C=3, P=64, seed=11):
    """x, alpha, shift and a per-tensor unsigned 8-bit quantiser (scale 1/4, zero 0) such that a / scale sits on or next to a .5
    tie: alpha and shift have full 24-bit significands, so s * alpha is inexact and rounding it before the addition (the
    contract) or after (an FMA) or not at all (float64) lands on different sides of the tie for a good share of the elements.
    Built backwards: pick the target t = (k + 0.5) * scale, then x = fp32((t - shift) / alpha)."""
    rng = np.random.default_rng(seed)
    alpha = (rng.uniform(1.0, 2.0, size=C)).astype(np.float32)
    shift = rng.uniform(-1.0, 1.0, size=C).astype(np.float32)
    scale = np.float32(0.25)
    k = rng.integers(0, 250, size=(N, C, P)).astype(np.float64)
    t = (k + 0.5) * float(scale)
    x = ((t - shift.astype(np.float64).reshape(1, C, 1)) / alpha.astype(np.float64).reshape(1, C, 1)).astype(np.float32)
    rq = (np.array([scale], np.float32), np.zeros(1, np.float32), 0.0, 255.0, 8, 0)
    return dict(x=x, identity=None, alpha=alpha, shift=shift, rq=rq)


# ---- the grid cap --------------------------------------------------------------------------------------------------------------
def beyond_the_grid_cap():
    """(N, C, P) of the smallest two-plane-per-image tensor whose plain groups exceed one sweep of the capped grid, with a ragged
    P (so the plan takes the plain instance whatever the consumer) and a ragged last group."""
    per_sweep = GRID_CAP * THREADS * PLAIN_VEC
    P = 1031                                        # prime: no multiple of 16, and N * C * P is no multiple of 8
    C = 3
    N = per_sweep // (C * P) + 1
    assert N * C * P > per_sweep and (N * C * P) % PLAIN_VEC != 0 and N * C * P < 2 * per_sweep
    return N, C, P
