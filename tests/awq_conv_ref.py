"""numpy float64 reference of qe_quantconv2d_awq's contract (include/quant_engine.h), written from the header: decode both
streams, then tap by tap and group by group.  Both operands in the kernel convention (q - zero); a tap in the padding
contributes nothing.  A plain helper module."""
import numpy as np

from awq_cases import decoded


def out_hw(c):
    return ((c["H"] + 2 * c["padding"] - c["KH"]) // c["stride"] + 1, (c["W"] + 2 * c["padding"] - c["KW"]) // c["stride"] + 1)


def _operands(c):
    """Decoded codes and parameters of a case dict, float64: qx (N, IC, H, W), qw (OC, IC, KH, KW), sx, zx scalars, sw / zw (OC, NG)."""
    qx, qw, sw, zw = decoded(c, (c["N"], c["IC"], c["H"], c["W"]), (c["OC"], c["IC"], c["KH"], c["KW"]), c["IC"] // c["G"])
    return qx, qw, float(np.asarray(c["sx"]).reshape(-1)[0]), float(np.asarray(c["zx"]).reshape(-1)[0]), sw, zw


def forward(c, terms=False):
    """The contract in float64, (N, OC, OH, OW).  terms=True: also sum |sx sw (qx - zx) (qw - zw)| + |bias| per output, the bound
    on every partial sum (of the value before the activation)."""
    qx, qw, sx, zx, sw, zw = _operands(c)
    G, S, pad = c["G"], c["stride"], c["padding"]
    OH, OW = out_hw(c)
    xz = np.pad(qx - zx, ((0, 0), (0, 0), (pad, pad), (pad, pad)))          # (q - zx) inside the image, 0 in the padding
    acc, mag = np.zeros((c["N"], c["OC"], OH, OW)), np.zeros((c["N"], c["OC"], OH, OW))
    for g in range(c["IC"] // G):
        cs = slice(g * G, (g + 1) * G)
        d = qw[:, cs] - zw[:, g, None, None, None]
        for kh in range(c["KH"]):
            for kw in range(c["KW"]):
                tap = xz[:, cs, kh:kh + S * (OH - 1) + 1:S, kw:kw + S * (OW - 1) + 1:S]
                acc += sw[None, :, g, None, None] * np.einsum("nchw,oc->nohw", tap, d[:, :, kh, kw])
                mag += np.abs(sw)[None, :, g, None, None] * np.einsum("nchw,oc->nohw", np.abs(tap), np.abs(d[:, :, kh, kw]))
    bias = np.zeros(c["OC"]) if c.get("bias") is None else np.asarray(c["bias"], np.float64)
    out = bias[None, :, None, None] + sx * acc
    if c.get("relu"):
        out = np.where(out < 0, 0.0, out)
    return (out, np.abs(bias)[None, :, None, None] + abs(sx) * mag) if terms else out


def dequantised(c):
    """The fp32 operands (q - zero) * scale, x (N, IC, H, W) and w (OC, IC, KH, KW): what the fp32 F.conv2d chain multiplies."""
    qx, qw, sx, zx, sw, zw = _operands(c)
    f = np.float32
    rep = lambda v: np.repeat(v.astype(f), c["G"], axis=1)[:, :, None, None]
    return (qx.astype(f) - f(zx)) * f(sx), (qw.astype(f) - rep(zw)) * rep(sw)


def g16_layer(path, name):
    """A layer of tests/golden/g16_awq_conv.npz: (fixture arrays of the layer, the PackedAwqConv2d from_awq builds, the fp32 pre_act batch)."""
    import torch
    from quantize_amd import packed
    z = np.load(path)
    g = {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "_")}
    n_bits, G, pad, qmin, qmax, signed = (int(v) for v in g["config"])
    w = torch.from_numpy(g["weight_i8"].astype(np.float32) * z["steps"][0])
    cfgs = (torch.from_numpy(g["scale"]), torch.from_numpy(g["zero"]), qmin, qmax, torch.from_numpy(g["awq_scale"]))
    conv = packed.PackedAwqConv2d.from_awq(w, cfgs, n_bits, signed, G, bias=torch.from_numpy(g["bias"]), padding=pad)
    return g, conv, g["pre_act_i8"].astype(np.float32) * z["steps"][1]
