"""numpy reference of qe_affine_relu_quantize_pack's contract (include/quant_engine.h), written from the header alone: every fp32
operation of the sequence is its own np.float32 operation, one per line, in the header's order.  Independent of the engine and of
oracle/.  A plain helper module for tests/test_preact_*.py and tests/test_packed_wrn_*.py.

`mode` selects the two nearly-right evaluations a tie-dense input has to tell from the contract: "fma" rounds s * alpha + shift
once (what a contracted kernel computes), "f64" evaluates the whole chain in float64."""
import numpy as np

F = np.float32


def code_range(bits, sign):
    return (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if sign else (0, (1 << bits) - 1)


def _bc(v, C):
    """1 or C values against (N, C, P)."""
    v = np.asarray(v).reshape(-1)
    return (np.full(C, v[0], v.dtype) if v.size == 1 else v).reshape(1, C, 1)


def bn_affine(gamma, beta, mean, var, eps):
    """(alpha, shift) of an eval-mode BatchNorm, in fp32 on the host: invstd = 1 / sqrt(var + eps); alpha = gamma * invstd;
    shift = beta - mean * alpha."""
    gamma, beta, mean, var = (np.asarray(v, F) for v in (gamma, beta, mean, var))
    ve = var + F(eps)
    sd = np.sqrt(ve)
    invstd = F(1.0) / sd
    alpha = gamma * invstd
    ma = mean * alpha
    shift = beta - ma
    assert alpha.dtype == F and shift.dtype == F
    return alpha, shift


def relu(t):
    return np.where((t > 0) | np.isnan(t), t, t.dtype.type(0)).astype(t.dtype)


def activated(x, identity, alpha, shift, mode="contract"):
    """(s, a) of (N, C, P) inputs.  mode "contract": fp32, one operation per line; "fma": the affine rounded once; "f64"."""
    T = np.float64 if mode == "f64" else F
    x = np.asarray(x, F).astype(T)
    C = x.shape[1]
    al, sh = _bc(np.asarray(alpha, F).astype(T), C), _bc(np.asarray(shift, F).astype(T), C)
    with np.errstate(all="ignore"):
        s = x if identity is None else x + np.asarray(identity, F).astype(T)
        if mode == "fma":
            t = (s.astype(np.float64) * al.astype(np.float64) + sh.astype(np.float64)).astype(F)     # the product is exact in float64
        else:
            m = s * al
            t = m + sh
        a = relu(t)
    assert s.dtype == T and a.dtype == T
    return s, a


def pre_round(a, scale, zero):
    """a / scale - zero in a's own precision: what the quantiser rounds."""
    T = a.dtype.type
    C = a.shape[1]
    sc, zr = _bc(np.asarray(scale, F).astype(T), C), _bc(np.asarray(zero, F).astype(T), C)
    with np.errstate(all="ignore"):
        d = a / sc
        t = d - zr
    assert t.dtype == a.dtype
    return t


def quantise(a, scale, zero, qmin, qmax):
    """q = clamp(rint(a / scale - zero), qmin, qmax), a NaN passing the clamp; in a's own precision."""
    T = a.dtype.type
    t = pre_round(a, scale, zero)
    r = np.rint(t)
    with np.errstate(invalid="ignore"):
        c = np.minimum(np.maximum(r, T(qmin)), T(qmax))
    return np.where(np.isnan(r), r, c).astype(a.dtype)


def stored(q, bits, sign):
    """stored code = (int(q) + offset) & mask per element (a NaN reads as 0: callers mask those elements)."""
    off = (1 << (bits - 1)) if sign else 0
    qi = np.trunc(np.where(np.isnan(q), 0, q)).astype(np.int64)
    return ((qi + off) & ((1 << bits) - 1)).astype(np.uint8).reshape(-1)


def pack(codes, bits):
    """element i at bits [i b, (i + 1) b) of the stream, LSB first, zero padding in the last byte"""
    b = np.unpackbits(np.ascontiguousarray(codes, np.uint8).reshape(-1)[:, None], axis=1, bitorder="little")[:, :bits]
    return np.packbits(b.reshape(-1), bitorder="little")


def unpack_codes(packed, n, bits):
    b = np.unpackbits(np.ascontiguousarray(packed, np.uint8), bitorder="little")[:n * bits].reshape(n, bits)
    return np.packbits(b, axis=1, bitorder="little").reshape(-1)


def flag(q, bits, sign):
    """tpack's range test on the quantised values: any outside the code range, or NaN."""
    lo, hi = code_range(bits, sign)
    with np.errstate(invalid="ignore"):
        return bool((~((q >= lo) & (q <= hi))).any())


def forward(x, identity, alpha, shift, rqs=(), mode="contract"):
    """The whole call.  rqs: (scale, zero, qmin, qmax, bits, sign) per consumer.  Returns dict(s, a, q=[...], codes=[packed
    streams], flag)."""
    s, a = activated(x, identity, alpha, shift, mode)
    qs = [quantise(a, sc, zr, qmin, qmax) for sc, zr, qmin, qmax, bits, sign in rqs]
    codes = [pack(stored(q, r[4], r[5]), r[4]) for q, r in zip(qs, rqs)]
    return dict(s=s, a=a, q=qs, codes=codes, flag=any(flag(q, r[4], r[5]) for q, r in zip(qs, rqs)))


def tie_excused(x, identity, alpha, shift, scale, zero):
    """Elements whose pre-round value, evaluated in float64, lies within fp32 rounding of a .5 tie: the only ones where two
    correct fp32 evaluations of the chain may round to different codes.  The margin is the first-order bound of the five fp32
    roundings (u = 2^-24 relative each: add, multiply, add, divide, subtract) carried through the chain, doubled for the second
    order."""
    u = 2.0 ** -24
    x64 = np.asarray(x, F).astype(np.float64)
    C = x64.shape[1]
    al, sh = _bc(np.asarray(alpha, F).astype(np.float64), C), _bc(np.asarray(shift, F).astype(np.float64), C)
    sc, zr = _bc(np.asarray(scale, F).astype(np.float64), C), _bc(np.asarray(zero, F).astype(np.float64), C)
    with np.errstate(all="ignore"):
        s = x64 if identity is None else x64 + np.asarray(identity, F).astype(np.float64)
        m = s * al
        ta = m + sh
        e = (0.0 if identity is None else u * np.abs(s)) * np.abs(al) + u * np.abs(m) + u * np.abs(ta)      # error of the affine
        a = relu(ta)
        d = a / sc
        t = d - zr
        e = e / np.abs(sc) + u * np.abs(d) + u * np.abs(t)
        dist = np.abs(t - (np.floor(t) + 0.5))
        return dist <= 2 * e
