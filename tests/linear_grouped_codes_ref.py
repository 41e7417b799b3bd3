"""numpy float64 reference of qe_quantlinear_grouped's contract (include/quant_engine.h), written from the header: decode both
streams, then a plain double loop over groups.  Both operands in the kernel convention (q - zero).  A plain helper module."""
import numpy as np

from awq_cases import decoded


def _operands(c):
    """The decoded codes and the parameters of a case dict, in float64: qx (B, K), qw (O, K), sx / zx (B, 1), sw / zw (O, NG)."""
    B, K, O = c["B"], c["K"], c["O"]
    qx, qw, sw, zw = decoded(c, (B, K), (O, K), K // c["G"])
    sx, zx = (np.broadcast_to(np.asarray(c[k], np.float64).reshape(-1, 1), (B, 1)) for k in ("sx", "zx"))
    return qx, qw, sx, zx, sw, zw


def forward(c, terms=False):
    """out[b,o] = bias[o] + sx[b] sum_g sw[o,g] sum_{k in g} (qx[b,k] - zx[b]) (qw[o,k] - zw[o,g]) in float64.  terms=True: also
    sum_k |sx sw (qx - zx) (qw - zw)| + |bias| per output, the bound on every partial sum."""
    qx, qw, sx, zx, sw, zw = _operands(c)
    G, O = c["G"], c["O"]
    acc, mag = np.zeros((c["B"], O)), np.zeros((c["B"], O))
    for o in range(O):
        for g in range(c["K"] // G):
            ks = slice(g * G, (g + 1) * G)
            d = qw[o, ks] - zw[o, g]
            acc[:, o] += sw[o, g] * ((qx[:, ks] - zx) @ d)
            mag[:, o] += abs(sw[o, g]) * (np.abs(qx[:, ks] - zx) @ np.abs(d))
    bias = np.zeros(O) if c["bias"] is None else np.asarray(c["bias"], np.float64)
    out = bias[None, :] + sx * acc
    return (out, np.abs(bias)[None, :] + np.abs(sx) * mag) if terms else out


def dequantised(c):
    """The fp32 operands (q - zero) * scale, x (B, K) and w (O, K): what the fp32 F.linear chain of the parity rule multiplies."""
    qx, qw, sx, zx, sw, zw = (v.astype(np.float32) for v in _operands(c))
    G = c["G"]
    return (qx - zx) * sx, (qw - np.repeat(zw, G, axis=1)) * np.repeat(sw, G, axis=1)
