"""numpy float64 reference of the grouped packed convolution (qe_quantconv2d_grouped).  A plain helper module: it shares no
code with the engine or the C oracle, the window and group loops are explicit and the streams are unpacked with
np.unpackbits(bitorder="little").

    y[n, oc, oh, ow] = bias[oc] + sum over the IC/g channels ic of oc's group and the in-bounds taps of
                       ((qx - zx[ic]) sx[ic]) ((qw - zw[oc]) sw[oc])
    relu: max(y, 0) with NaN passing;  codes: round(y / s - z).clamp(qmin, qmax), stored as qe_tpack stores them.

chain() is the reference's packed forward, fp32 F.conv2d(groups=g) on the dequantised tensors on the CPU: the yardstick of
conftest.conv_tolerance."""
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


def conv(qx, sx, zx, qw, sw, zw, bias, groups, stride, pad, relu=False):
    """qx (N, IC, H, W) and qw (OC, IC / groups, KH, KW) integer codes; x scales / zeros of 1 or IC elements, w scales /
    zeros of 1 or OC (fp32 values, widened exactly).  Returns float64 (N, OC, OH, OW)."""
    N, IC, H, W = qx.shape
    OC, ICg, KH, KW = qw.shape
    assert IC == ICg * groups and OC % groups == 0
    OCg = OC // groups
    OH, OW = out_hw(H, W, KH, KW, stride, pad)
    sx, zx = (_per_channel(v, IC) for v in (sx, zx))
    sw, zw = (_per_channel(v, OC) for v in (sw, zw))
    x = (qx.astype(np.float64) - zx[None, :, None, None]) * sx[None, :, None, None]
    w = (qw.astype(np.float64) - zw[:, None, None, None]) * sw[:, None, None, None]
    y = np.zeros((N, OC, OH, OW), dtype=np.float64)
    for g in range(groups):
        xg = x[:, g * ICg:(g + 1) * ICg]                  # (N, ICg, H, W)
        wg = w[g * OCg:(g + 1) * OCg]                     # (OCg, ICg, KH, KW)
        for oh in range(OH):
            for ow in range(OW):
                acc = np.zeros((N, OCg), dtype=np.float64)
                for kh in range(KH):
                    ih = oh * stride - pad + kh
                    if ih < 0 or ih >= H:
                        continue
                    for kw in range(KW):
                        iw = ow * stride - pad + kw
                        if iw < 0 or iw >= W:
                            continue
                        acc += xg[:, :, ih, iw] @ wg[:, :, kh, kw].T
                y[:, g * OCg:(g + 1) * OCg, oh, ow] = acc
    if bias is not None:
        y = y + np.asarray(bias, dtype=np.float64)[None, :, None, None]
    if relu:
        y = np.where((y > 0) | np.isnan(y), y, 0.0)
    return y


def int_sums(qx, zx, qw, zw, groups, stride, pad):
    """max over the outputs of |I| = |sum (qx - zx)(qw - zw)| bounds: the sum of |a| |b| over the in-bounds taps and the group's
    channels, per output, as int64 (N, OC, OH, OW).  zx / zw integer-valued."""
    N, IC, H, W = qx.shape
    OC, ICg, KH, KW = qw.shape
    a = np.abs(qx.astype(np.int64) - np.rint(_per_channel(zx, IC)).astype(np.int64)[None, :, None, None]).astype(np.float64)
    b = np.abs(qw.astype(np.int64) - np.rint(_per_channel(zw, OC)).astype(np.int64)[:, None, None, None]).astype(np.float64)
    ones = np.ones(1)
    return conv(a, ones, np.zeros(1), b, ones, np.zeros(1), None, groups, stride, pad)


def chain(qx, sx, zx, qw, sw, zw, bias, groups, stride, pad):
    """The reference's packed forward: fp32 F.conv2d(groups=g) on the dequantised tensors, on the CPU."""
    import torch
    import torch.nn.functional as F
    IC, OC = qx.shape[1], qw.shape[0]

    def deq(q, s, z, C, shape):
        s, z = (torch.from_numpy(np.full(C, v[0], np.float32) if v.size == 1 else v.astype(np.float32)).reshape(shape) for v in (s, z))
        return (torch.from_numpy(q.astype(np.float32)) - z) * s

    x = deq(qx, np.asarray(sx), np.asarray(zx), IC, (1, IC, 1, 1))
    w = deq(qw, np.asarray(sw), np.asarray(zw), OC, (OC, 1, 1, 1))
    b = None if bias is None else torch.from_numpy(np.asarray(bias, np.float32))
    return F.conv2d(x, w, b, stride=stride, padding=pad, groups=groups).numpy()


def quantize(y, scale, zero, qmin, qmax):
    """The consumer's quantiser on fp32 values, in fp32 as the module does it: round(y / s - z).clamp(qmin, qmax).  y is
    (N, C, OH, OW); scale / zero 1 or C elements."""
    C = y.shape[1]
    s = _per_channel(scale, C).astype(np.float32)[None, :, None, None]
    z = _per_channel(zero, C).astype(np.float32)[None, :, None, None]
    q = np.rint(y.astype(np.float32) / s - z)
    return np.clip(q, np.float32(qmin), np.float32(qmax)).astype(np.int64)
