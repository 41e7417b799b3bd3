"""numpy float64 reference of the depthwise packed convolution (qe_quantconv2d_depthwise).  A plain helper module: it shares no
code with the engine, the window loops are explicit and the streams are unpacked with np.unpackbits(bitorder="little").

    y[n, c, oh, ow] = bias[c] + sum over in-bounds taps of ((qx - zx[c]) sx[c]) ((qw - zw[c]) sw[c])
    relu: max(y, 0) with NaN passing;  codes: round(y / s - z).clamp(qmin, qmax), stored as qe_tpack stores them."""
import numpy as np


def code_range(bits, sign):
    return (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if sign else (0, (1 << bits) - 1)


def pack(q, bits, sign):
    """Codes -> the packed little-endian bit stream: element i in bits [i * bits, (i + 1) * bits), stored q + 2^(bits-1) when signed."""
    stored = (np.asarray(q, dtype=np.int64).reshape(-1) + ((1 << (bits - 1)) if sign else 0)).astype(np.uint8)
    b = np.unpackbits(stored[:, None], axis=1, bitorder="little")[:, :bits].reshape(-1)
    return np.packbits(b, bitorder="little")


def unpack(stream, n, bits, sign):
    b = np.unpackbits(np.asarray(stream, dtype=np.uint8), bitorder="little")[:n * bits].reshape(n, bits)
    stored = (b.astype(np.int64) << np.arange(bits, dtype=np.int64)).sum(axis=1)
    return stored - ((1 << (bits - 1)) if sign else 0)


def out_hw(H, W, KH, KW, stride, pad):
    return (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1


def _per_channel(v, C):
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    return np.full(C, v[0]) if v.size == 1 else v


def conv(qx, sx, zx, qw, sw, zw, bias, stride, pad, relu=False):
    """qx (N, C, H, W) and qw (C, KH, KW) integer codes; scales / zeros of 1 or C elements (fp32 values, widened exactly).
    Returns float64 (N, C, OH, OW)."""
    N, C, H, W = qx.shape
    _, KH, KW = qw.shape
    OH, OW = out_hw(H, W, KH, KW, stride, pad)
    sx, zx, sw, zw = (_per_channel(v, C) for v in (sx, zx, sw, zw))
    x = (qx.astype(np.float64) - zx[None, :, None, None]) * sx[None, :, None, None]
    w = (qw.astype(np.float64) - zw[:, None, None]) * sw[:, None, None]
    y = np.zeros((N, C, OH, OW), dtype=np.float64)
    for oh in range(OH):
        for ow in range(OW):
            acc = np.zeros((N, C), dtype=np.float64)
            for kh in range(KH):
                ih = oh * stride - pad + kh
                if ih < 0 or ih >= H:
                    continue
                for kw in range(KW):
                    iw = ow * stride - pad + kw
                    if iw < 0 or iw >= W:
                        continue
                    acc += x[:, :, ih, iw] * w[None, :, kh, kw]
            y[:, :, oh, ow] = acc
    if bias is not None:
        y = y + np.asarray(bias, dtype=np.float64)[None, :, None, None]
    if relu:
        y = np.where((y > 0) | np.isnan(y), y, 0.0)
    return y


def quantize(y, scale, zero, qmin, qmax):
    """The consumer's quantiser on fp32 values, in fp32 as the module does it: round(y / s - z).clamp(qmin, qmax).  y is
    (N, C, OH, OW); scale / zero 1 or C elements."""
    C = y.shape[1]
    s = _per_channel(scale, C).astype(np.float32)[None, :, None, None]
    z = _per_channel(zero, C).astype(np.float32)[None, :, None, None]
    q = np.rint(y.astype(np.float32) / s - z)
    return np.clip(q, np.float32(qmin), np.float32(qmax)).astype(np.int64)
