"""numpy reference of the quantised ReLU / pooling contracts of include/quant_engine.h, written from the header alone: every fp32
operation of a sequence is its own np.float32 operation, in the header's order.  Independent of the engine and of oracle/.
A plain helper module for tests/test_pool_*.py."""
import numpy as np

F = np.float32


def _bc(v, C):
    """scale / zero (1 or C elements) against NCHW."""
    v = np.asarray(v, F).reshape(-1)
    return (np.full(C, v[0], F) if v.size == 1 else v).reshape(1, C, 1, 1)


def qdq(x, scale, zero, qmin, qmax):
    """(clamp(rint(x / scale - zero), qmin, qmax) + zero) * scale, NaN passing the clamp."""
    x = np.asarray(x, F)
    s, z = _bc(scale, x.shape[1]), _bc(zero, x.shape[1])
    with np.errstate(all="ignore"):
        t = x / s
        t = t - z
        r = np.rint(t)
        c = np.where(np.isnan(r), r, np.minimum(np.maximum(r, F(qmin)), F(qmax))).astype(F)
        d = c + z
        y = d * s
    assert y.dtype == F
    return y


def relu(y):
    return np.where((y > 0) | np.isnan(y), y, F(0)).astype(F)


def quant_relu(x, scale, zero, qmin, qmax):
    return relu(qdq(x, scale, zero, qmin, qmax))


def quant_maxpool2d(x, scale, zero, qmin, qmax, kernel, stride, padding):
    """The tap-wise form: max over the in-bounds taps of qdq(tap); np.max hands a NaN on."""
    y = qdq(x, scale, zero, qmin, qmax)
    N, C, H, W = y.shape
    OH, OW = (H + 2 * padding - kernel) // stride + 1, (W + 2 * padding - kernel) // stride + 1
    out = np.empty((N, C, OH, OW), F)
    for oh in range(OH):
        h0, h1 = max(oh * stride - padding, 0), min(oh * stride - padding + kernel, H)
        for ow in range(OW):
            w0, w1 = max(ow * stride - padding, 0), min(ow * stride - padding + kernel, W)
            with np.errstate(all="ignore"):
                out[:, :, oh, ow] = np.max(y[:, :, h0:h1, w0:w1], axis=(2, 3))
    return out


def windows(n_in, n_out):
    """torch's adaptive windows of one axis: [(lo, hi)] with lo = floor(o * in / out), hi = ceil((o + 1) * in / out)."""
    return [((o * n_in) // n_out, -((-(o + 1) * n_in) // n_out)) for o in range(n_out)]


def fixed_windows(n_in, kernel, stride):
    return [(o * stride, o * stride + kernel) for o in range((n_in - kernel) // stride + 1)]


def quant_adaptive_avgpool2d(x, scale, zero, qmin, qmax, OH, OW):
    """sum from +0, tap by tap (rows outer, columns inner), then one division by the tap count.  Returns (out, cnt, max|qdq(tap)|
    per output) -- the last two for the float64 bound."""
    y = qdq(x, scale, zero, qmin, qmax)
    N, C, H, W = y.shape
    out, cnt, amax = np.empty((N, C, OH, OW), F), np.empty((OH, OW), np.int64), np.empty((N, C, OH, OW), np.float64)
    for oh, (h0, h1) in enumerate(windows(H, OH)):
        for ow, (w0, w1) in enumerate(windows(W, OW)):
            s = np.zeros((N, C), F)
            with np.errstate(all="ignore"):
                for ih in range(h0, h1):
                    for iw in range(w0, w1):
                        s = s + y[:, :, ih, iw]
                n = (h1 - h0) * (w1 - w0)
                out[:, :, oh, ow] = s / F(n)
                amax[:, :, oh, ow] = np.abs(y[:, :, h0:h1, w0:w1].astype(np.float64)).max(axis=(2, 3))
            cnt[oh, ow] = n
            assert s.dtype == F
    return out, cnt, amax


def decode(stored, sign):
    """stored codes (uint8) -> q."""
    return stored.astype(np.int64) - (128 if sign else 0)


def avgpool2d_codes(q, scale, zero_p, kernel, stride, OH, OW, relu_taps=False):
    """qe_avgpool2d_codes' value rule on decoded codes q (N, C, H, W); scale / zero' of 1 or C elements, kernel convention."""
    N, C, H, W = q.shape
    s, z = _bc(scale, C)[:, :, 0, 0], _bc(zero_p, C)[:, :, 0, 0]
    rows = fixed_windows(H, kernel, stride) if kernel else windows(H, OH)
    cols = fixed_windows(W, kernel, stride) if kernel else windows(W, OW)
    assert (len(rows), len(cols)) == (OH, OW)
    out = np.empty((N, C, OH, OW), F)
    with np.errstate(all="ignore"):
        for oh, (h0, h1) in enumerate(rows):
            for ow, (w0, w1) in enumerate(cols):
                fc = F((h1 - h0) * (w1 - w0))
                if not relu_taps:
                    S = q[:, :, h0:h1, w0:w1].sum(axis=(2, 3))
                    t = fc * z
                    d = S.astype(F) - t
                else:
                    d = np.zeros((N, C), F)
                    for ih in range(h0, h1):
                        for iw in range(w0, w1):
                            t = q[:, :, ih, iw].astype(F) - z
                            d = d + relu(t)
                m = s * d
                out[:, :, oh, ow] = m / fc
                assert m.dtype == F
    return out


def code_range(bits, sign):
    return (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if sign else (0, (1 << bits) - 1)
