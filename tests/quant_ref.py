"""Plain numpy float64 reference of the packed operations, independent of the engine and of the C oracle.

The packed format, from its definition: element i of a tensor (row-major) occupies bits [i b, i b + b) of the byte stream,
least significant bit first (bit k of the stream is bit k % 8 of byte k / 8), so an element may straddle two bytes; the b
bits hold the code q itself when the codes are unsigned (0 .. 2^b - 1) and q + 2^(b-1) when they are signed
(-2^(b-1) .. 2^(b-1) - 1).  A stream of n elements has ceil(n b / 8) bytes, the unused high bits of the last one zero.

The operations: out = sum (q_x - z_x) s_x (q_w - z_w) s_w + bias, over (ic, kh, kw) for conv2d -- taps outside the image
contribute nothing (the padding is the real value zero, not the code zero) -- and over k for linear.  x scales and zero
points are per tensor or per input channel (conv) / per batch row (linear), w's per tensor or per output channel / column.
quantlinear alone ADDS its zero points (the packed Linear module's convention): `add_zero=True`."""
import numpy as np


def pack(q, n_bits, sign):
    """Integer codes -> uint8 stream."""
    q = np.asarray(q, dtype=np.int64).reshape(-1)
    lo, hi = code_range(n_bits, sign)
    assert q.min() >= lo and q.max() <= hi
    u = q + (1 << (n_bits - 1)) if sign else q
    bits = ((u[:, None] >> np.arange(n_bits)) & 1).astype(np.uint8).reshape(-1)
    return np.packbits(bits, bitorder="little")


def unpack(packed, n, n_bits, sign):
    """uint8 stream -> int64 codes (n of them)."""
    packed = np.asarray(packed, dtype=np.uint8).reshape(-1)
    assert packed.size == (n * n_bits + 7) // 8
    bits = np.unpackbits(packed, bitorder="little")[:n * n_bits].reshape(n, n_bits).astype(np.int64)
    u = (bits << np.arange(n_bits)).sum(axis=1)
    return u - (1 << (n_bits - 1)) if sign else u


def code_range(n_bits, sign):
    return (-(1 << (n_bits - 1)), (1 << (n_bits - 1)) - 1) if sign else (0, (1 << n_bits) - 1)


def _per(v, n, axis_shape):
    """A scale / zero array of 1 or n elements, shaped to broadcast along one axis."""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    assert v.size in (1, n)
    return v.reshape(axis_shape) if v.size == n else v.reshape([1] * len(axis_shape))


def dequant(packed, shape, n_bits, sign, scale, zero, axis, add_zero=False):
    """(q -+ z) s as float64, scale / zero per tensor or along `axis`."""
    n = int(np.prod(shape))
    q = unpack(packed, n, n_bits, sign).reshape(shape).astype(np.float64)
    ax = [1] * len(shape)
    ax[axis] = shape[axis]
    s, z = _per(scale, shape[axis], ax), _per(zero, shape[axis], ax)
    return (q + z if add_zero else q - z) * s


def conv2d(x, w, bias, stride, pad):
    """float64 NCHW convolution of real values, zero padding."""
    N, IC, H, W = x.shape
    OC, IC2, KH, KW = w.shape
    assert IC == IC2
    OH, OW = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
    xp = np.pad(x.astype(np.float64), ((0, 0), (0, 0), (pad, pad), (pad, pad)))
    out = np.zeros((N, OC, OH, OW), dtype=np.float64)
    for kh in range(KH):
        for kw in range(KW):
            win = xp[:, :, kh:kh + stride * (OH - 1) + 1:stride, kw:kw + stride * (OW - 1) + 1:stride]
            out += np.einsum("nchw,oc->nohw", win, w[:, :, kh, kw].astype(np.float64))
    if bias is not None:
        out += np.asarray(bias, dtype=np.float64).reshape(1, OC, 1, 1)
    return out


def quantconv2d(xp, x_shape, x_bits, x_sign, sx, zx, wp, w_shape, w_bits, w_sign, sw, zw, bias, stride, pad):
    x = dequant(xp, x_shape, x_bits, x_sign, sx, zx, axis=1)
    w = dequant(wp, w_shape, w_bits, w_sign, sw, zw, axis=0)
    return conv2d(x, w, bias, stride, pad)


def quantconv2d_float_input(x, wp, w_shape, w_bits, w_sign, sw, zw, bias, stride, pad):
    return conv2d(np.asarray(x, dtype=np.float64), dequant(wp, w_shape, w_bits, w_sign, sw, zw, axis=0), bias, stride, pad)


def linear(x, w, bias):
    out = x.astype(np.float64) @ w.astype(np.float64).T
    return out if bias is None else out + np.asarray(bias, dtype=np.float64).reshape(1, -1)


def quantlinear(xp, x_shape, x_bits, x_sign, sx, zx, wp, w_shape, w_bits, w_sign, sw, zw, bias):
    """The packed linear: (q + z) on both operands, x scale / zero per batch row, w's per output column."""
    x = dequant(xp, x_shape, x_bits, x_sign, sx, zx, axis=0, add_zero=True)
    w = dequant(wp, w_shape, w_bits, w_sign, sw, zw, axis=0, add_zero=True)
    return linear(x, w, bias)


def quantlinear_float_input(x, wp, w_shape, w_bits, w_sign, sw, zw, bias):
    """fp32 / bf16 rows times packed weights: (q - z) s on the weight."""
    return linear(np.asarray(x, dtype=np.float64), dequant(wp, w_shape, w_bits, w_sign, sw, zw, axis=0), bias)


def bf16_round(v):
    """float64 values that are fp32 numbers -> their bf16 rounding (nearest even) as float64."""
    f = np.asarray(v, dtype=np.float64).astype(np.float32)
    u = f.view(np.uint32).astype(np.uint64)
    u = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def codes(v, scale, zero, qmin, qmax):
    """The consumer's quantiser q = round(v / scale - zero).clamp(qmin, qmax) (ties to even) on float64 values."""
    return np.clip(np.rint(np.asarray(v, dtype=np.float64) / float(scale) - float(zero)), qmin, qmax).astype(np.int64)
