"""numpy float64 reference of qe_quantlinear_grouped_float_input's contract (include/quant_engine.h), written from the header:
decode the codes from the packed stream, then a plain double loop over groups.  A plain helper module."""
import numpy as np


def decode(stream, n, n_bits, signed):
    """The n integer codes of a little-endian n_bits stream (stored value q + 2^(n_bits-1) when signed)."""
    bits = np.unpackbits(np.asarray(stream, np.uint8), bitorder="little")[:n * n_bits].reshape(n, n_bits)
    stored = (bits.astype(np.int64) << np.arange(n_bits)).sum(1)
    return stored - ((1 << (n_bits - 1)) if signed else 0)


def xprime(x, x_mul):
    """x' = x * x_mul: ONE fp32 multiply (the contract), then exact in float64."""
    x = np.asarray(x, np.float32)
    return (x if x_mul is None else x * np.asarray(x_mul, np.float32)[None, :]).astype(np.float64)


def forward(x, x_mul, stream, n_bits, signed, scale, zero, group_size, bias, O, terms=False):
    """out[b,o] = bias[o] + sum_g sw[o,g] sum_{k in g} x'[b,k] (q[o,k] - zw[o,g]) in float64; scale / zero in (o, g) order, kernel
    convention.  terms=True: also sum_k |sw x' (q - zw)| + |bias| per output, the bound on every partial sum."""
    B, K = x.shape
    NG = K // group_size
    q = decode(stream, O * K, n_bits, signed).reshape(O, K).astype(np.float64)
    xp = xprime(x, x_mul)
    sw, zw = np.asarray(scale, np.float64).reshape(O, NG), np.asarray(zero, np.float64).reshape(O, NG)
    out = np.zeros((B, O)) if bias is None else np.tile(np.asarray(bias, np.float64), (B, 1))
    mag = np.abs(out)
    for o in range(O):
        for g in range(NG):
            ks = slice(g * group_size, (g + 1) * group_size)
            d = q[o, ks] - zw[o, g]
            out[:, o] += sw[o, g] * (xp[:, ks] @ d)
            mag[:, o] += abs(sw[o, g]) * (np.abs(xp[:, ks]) @ np.abs(d))
    return (out, mag) if terms else out


def dequantised(stream, n_bits, signed, scale, zero, group_size, O, K):
    """The fp32 weight (q - zw) * sw, (O, K): what the fp32 F.linear chain of the parity rule multiplies."""
    q = decode(stream, O * K, n_bits, signed).reshape(O, K // group_size, group_size).astype(np.float32)
    sw, zw = (np.asarray(v, np.float32).reshape(O, K // group_size, 1) for v in (scale, zero))
    return ((q - zw) * sw).reshape(O, K)


def g15_layer(path, layer):
    """A G15 layer through PackedGroupedLinear.from_awq: (the fixture, the layer, the contract's float64 output on pre_act)."""
    import torch
    from quantize_amd.packed import PackedGroupedLinear
    g = np.load(path)
    K, O, G, bits, _ = (int(v) for v in g["config"])
    t = lambda k: torch.from_numpy(g["%s_%s" % (layer, k)])
    qmin, qmax, signed = (int(v) for v in g[layer + "_qrange"])
    lin = PackedGroupedLinear.from_awq(t("weight"), (t("scale"), t("zero"), qmin, qmax, t("awq_scale")), bits, signed, G, bias=t("bias"))
    exact = forward(g[layer + "_pre_act"], lin.x_mul.numpy(), lin.weight.numpy(), lin.w_bits, lin.w_signed, lin.w_scale.numpy(),
                    lin._neg_w_zero.numpy(), G, lin.bias.numpy(), O)
    return g, lin, exact
