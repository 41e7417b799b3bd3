"""numpy references of the elementwise kernels (qe_tpack.hip, patchify_quant_kernel, maxpool2d_codes_kernel,
global_avgpool_kernel): independent of the engine and of the C oracle (tests/test_ew_instances_cpu.py compares the packer
with both).

The quantiser's contract is an fp32 operation SEQUENCE, not a real-valued function: q = clamp(rint(x / scale - zero)) with
an IEEE fp32 division, an fp32 subtraction and round-half-even.  On inputs that sit on `.5` ties of x / scale - zero a
reciprocal multiply or a float64 evaluation changes a fifth to a half of the codes, so `quantise` below does exactly those
fp32 operations, and `quantise_reciprocal` / `quantise_f64` are the two nearly-right variants a test input has to tell
from it (`tie_dense` makes such inputs; the CPU test measures that they do)."""
import math

import numpy as np

F32 = np.float32


def qrange(bits, sign):
    """(lowest, highest) code of a width: what tpack's range test admits."""
    return (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if sign else (0, (1 << bits) - 1)


def channels(n, n_ch, inner):
    """channel of element i = (i // inner) % n_ch"""
    return (np.arange(n, dtype=np.int64) // int(inner)) % int(n_ch)


def _params(n, scale, zero, inner):
    scale = np.asarray(scale, F32).reshape(-1)
    zero = np.asarray(zero, F32).reshape(-1)
    assert scale.size == zero.size and scale.size >= 1
    if scale.size == 1:
        return scale[0], zero[0]
    ch = channels(n, scale.size, inner)
    return scale[ch], zero[ch]


def _clamp(r, qmin, qmax):
    """fminf(fmaxf(r, qmin), qmax) with NaN passing through"""
    with np.errstate(invalid="ignore"):
        c = np.minimum(np.maximum(r, F32(qmin)), F32(qmax))
    return np.where(np.isnan(r), r, c).astype(F32)


def quantise(x, scale, zero, qmin, qmax, inner=1):
    """The contract: fp32 division, fp32 subtraction, np.rint (half to even), clamp; NaN passes through."""
    x = np.ascontiguousarray(x, F32).reshape(-1)
    s, z = _params(x.size, scale, zero, inner)
    with np.errstate(all="ignore"):
        t = (x / s).astype(F32)
        r = np.rint((t - z).astype(F32)).astype(F32)
    return _clamp(r, qmin, qmax)


def quantise_reciprocal(x, scale, zero, qmin, qmax, inner=1):
    """WRONG on purpose: x * (1 / scale) in place of the division."""
    x = np.ascontiguousarray(x, F32).reshape(-1)
    s, z = _params(x.size, scale, zero, inner)
    with np.errstate(all="ignore"):
        t = (x * (F32(1.0) / s).astype(F32)).astype(F32)
        r = np.rint((t - z).astype(F32)).astype(F32)
    return _clamp(r, qmin, qmax)


def quantise_f64(x, scale, zero, qmin, qmax, inner=1):
    """WRONG on purpose: the same formula evaluated in float64."""
    x = np.ascontiguousarray(x, F32).reshape(-1)
    s, z = _params(x.size, scale, zero, inner)
    with np.errstate(all="ignore"):
        r = np.rint(x.astype(np.float64) / np.float64(s) - np.float64(z)).astype(F32)
    return _clamp(r, qmin, qmax)


def tie_distance_ulp(x, scale, zero, inner=1):
    """Distance of x / scale - zero (float64) from the nearest k + 0.5, in fp32 ulps of that value."""
    x = np.ascontiguousarray(x, F32).reshape(-1)
    s, z = _params(x.size, scale, zero, inner)
    t = x.astype(np.float64) / np.float64(s) - np.float64(z)
    d = np.abs(t - (np.floor(t) + 0.5))
    return d / np.spacing(np.abs(t).astype(F32)).astype(np.float64)


def tie_dense(rng, n, scale, zero, qmin, qmax, inner=1, fraction=0.6):
    """n floats of which `fraction` are fp32((k + 0.5 + zero) * scale) for integers k over [qmin - 2, qmax + 2] (on or within
    an ulp or two of a tie of x / scale - zero, both sides of each clamp), the rest normals over the same range."""
    s, z = _params(n, scale, zero, inner)
    k = rng.randint(int(qmin) - 2, int(qmax) + 2, size=n).astype(np.float64)
    ties = ((k + 0.5 + np.float64(z)) * np.float64(s)).astype(F32)
    if fraction >= 1.0:
        return ties
    mid, half = 0.5 * (qmin + qmax), 0.5 * (qmax - qmin) + 1.0
    other = ((rng.normal(0.0, 0.6, size=n) * half + mid + np.float64(z)) * np.float64(s)).astype(F32)
    return np.where(rng.uniform(size=n) < fraction, ties, other).astype(F32)


def stored(q, bits, sign):
    """Stored code of an in-range integer-valued float: (int(q) + (sign ? 2^(b-1) : 0)) & (2^b - 1).  NaN -> 0 (callers mask)."""
    q = np.asarray(q)
    if q.dtype.kind == "f":
        q = np.where(np.isnan(q), 0, q)
    off = (1 << (bits - 1)) if sign else 0
    return ((np.trunc(q).astype(np.int64) + off) & ((1 << bits) - 1)).astype(np.uint8).reshape(-1)


def pack(codes, bits):
    """Element i at bits [i*b, (i+1)*b) of the stream, LSB first, zero padding in the last byte."""
    codes = np.ascontiguousarray(codes, np.uint8).reshape(-1)
    b = np.unpackbits(codes[:, None], axis=1, bitorder="little")[:, :bits]
    return np.packbits(b.reshape(-1), bitorder="little")


def unpack_codes(packed, n, bits):
    """The stored codes (uint8) of the first n elements of a stream."""
    b = np.unpackbits(np.ascontiguousarray(packed, np.uint8), bitorder="little")[:n * bits].reshape(n, bits)
    return np.packbits(b, axis=1, bitorder="little").reshape(-1)


def unpack(packed, n, bits, sign):
    """Inverse of pack(stored(q)): int8 when signed, uint8 otherwise."""
    c = unpack_codes(packed, n, bits).astype(np.int64) - ((1 << (bits - 1)) if sign else 0)
    return c.astype(np.int8 if sign else np.uint8)


def range_bad(v, bits, sign):
    """tpack's range test on the value as float: out of [lo, hi], or NaN."""
    lo, hi = qrange(bits, sign)
    f = np.asarray(v).astype(F32)
    with np.errstate(invalid="ignore"):
        return ~((f >= F32(lo)) & (f <= F32(hi)))


_erf = np.vectorize(math.erf, otypes=[np.float64])


def gelu64(x):
    """x * 0.5 * (1 + erf(x / sqrt(2))) in float64"""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        return x * 0.5 * (1.0 + _erf(x / math.sqrt(2.0)))


def maxpool_codes(codes, sign, k, stride, pad):
    """Max pool of 8-bit stored codes (N, C, H, W) -> (N, C, OH, OW): decode, take each window's maximum by explicit loops
    (padding taps do not take part), encode again."""
    codes = np.asarray(codes, np.uint8)
    N, C, H, W = codes.shape
    off = 128 if sign else 0
    q = codes.astype(np.int64) - off
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    out = np.empty((N, C, OH, OW), np.int64)
    for oh in range(OH):
        for ow in range(OW):
            best = None
            for kh in range(k):
                for kw in range(k):
                    ih, iw = oh * stride - pad + kh, ow * stride - pad + kw
                    if 0 <= ih < H and 0 <= iw < W:
                        best = q[:, :, ih, iw] if best is None else np.maximum(best, q[:, :, ih, iw])
            assert best is not None, "a window of padding only"
            out[:, :, oh, ow] = best
    return (out + off).astype(np.uint8)


def avgpool64(x):
    """(N, C, H, W) -> (N, C) mean in float64"""
    return np.asarray(x, np.float64).mean(axis=(2, 3))


def patch_matrix(x, p):
    """(N, C, H, W) -> (N * (H/p) * (W/p), C * p * p): row = (image, patch row, patch column), column = (c, kh, kw)."""
    N, C, H, W = x.shape
    assert H % p == 0 and W % p == 0
    return np.ascontiguousarray(x.reshape(N, C, H // p, p, W // p, p).transpose(0, 2, 4, 1, 3, 5)).reshape(
        N * (H // p) * (W // p), C * p * p)
