#!/usr/bin/env python3
"""G10: the reference's QuantMultiheadAttention run through its packed forward WITH masks -> tests/golden/g10_mha_masked.npz.

Made on the CPU the way oracle/gen_golden.py makes G7 (its import_ref_modules loads the reference's module package at run
time; nothing of it is stored here): the separate-projection form (kdim != embed_dim, the only one whose pack() works),
calibrated, packed, reloaded, then called with
  (a) causal_float   a float (L, L) mask, -inf above the diagonal (the CLIP text transformer's build_attention_mask)
  (b) bool2d         a bool (L, S) mask, True = not allowed
  (c) padding        a bool key_padding_mask (N, S) with ragged lengths
  (d) float3d_pad    a float (N*H, L, S) mask with -inf holes, plus a bool key_padding_mask
Every row keeps at least one visible key.  Keys as in G7 (m_<name>_query / _key / _value / _heads / _sd_* / _y_packed) plus
_attn_mask and _key_padding_mask where the case has one.
usage: python tools/gen_golden_mha_masked.py     (needs the reference checkout oracle/gen_golden.py points at)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "g10_mha_masked.npz")

W8 = dict(n_bits=8, symmetric=True, signed=True, granularity="channel", range={"name": "minmax"})
A8 = dict(n_bits=8, symmetric=True, signed=True, granularity="layer", range={"name": "minmax"})
W8U = dict(n_bits=8, symmetric=False, signed=False, granularity="channel", range={"name": "minmax"})
A8U = dict(n_bits=8, symmetric=False, signed=False, granularity="layer", range={"name": "minmax"})


def _masks(kind, N, H, L, S, g):
    """(attn_mask or None, key_padding_mask or None); every (n, h, t) row keeps a visible key."""
    attn_mask = kpm = None
    if kind == "causal_float":
        attn_mask = torch.full((L, S), float("-inf")).triu_(1)
    elif kind == "bool2d":
        attn_mask = torch.rand(L, S, generator=g) < 0.4
        attn_mask[torch.arange(L), torch.arange(L) % S] = False
    elif kind == "padding":
        lengths = [max(1, S - 2 * n - 1) for n in range(N)]
        kpm = torch.arange(S)[None, :] >= torch.tensor(lengths)[:, None]
    elif kind == "float3d_pad":
        attn_mask = torch.randn(N * H, L, S, generator=g)
        attn_mask[torch.rand(N * H, L, S, generator=g) < 0.3] = float("-inf")
        attn_mask[:, torch.arange(L), torch.arange(L) % (S - 2)] = 0.0        # a visible key below every padded tail
        kpm = torch.arange(S)[None, :] >= torch.tensor([S - (n % 3) for n in range(N)])[:, None]
    else:
        raise ValueError(kind)
    return attn_mask, kpm


def main():
    from oracle import gen_golden
    mm = gen_golden.import_ref_modules()
    out, index = {}, []
    torch.manual_seed(23)
    g = torch.Generator().manual_seed(29)
    # name, E, H, kdim, L, S, N, weight / activation settings, mask kind
    cfgs = [("causal_float", 32, 4, 24, 9, 9, 3, W8, A8, "causal_float"),
            ("bool2d", 48, 6, 40, 6, 11, 2, W8U, A8U, "bool2d"),
            ("padding", 32, 4, 24, 5, 12, 4, W8, A8, "padding"),
            ("float3d_pad", 64, 8, 48, 7, 10, 2, W8, A8, "float3d_pad")]
    for (name, E, H, KD, L, S, N, w_set, a_set, kind) in cfgs:
        ref = torch.nn.MultiheadAttention(E, H, kdim=KD, vdim=KD, bias=True)

        def make():
            return mm.QuantMultiheadAttention(
                E, H, kdim=KD, vdim=KD, w_setting=dict(w_set), a_setting=dict(a_set),
                _parameters={k: (v.detach().clone() if v is not None else None) for k, v in ref._parameters.items()},
                _modules={"out_proj": ref.out_proj})

        q, k, v = torch.randn(L, N, E), torch.randn(S, N, KD), torch.randn(S, N, KD)
        if not a_set["symmetric"]:
            q, k, v = torch.relu(q), torch.relu(k), torch.relu(v)
        attn_mask, kpm = _masks(kind, N, H, L, S, g)
        m = make()
        with torch.no_grad():
            m.calibrating = True
            m(q, k, v)
            m.calibrating = False
            for mod in m.modules():
                if isinstance(mod, mm.Quantizer):
                    mod.quant(True)
            m.pack()
            sd = {kk: vv.clone() for kk, vv in m.state_dict().items()}
            m2 = make()
            m2.load_state_dict(sd)
            for mod in m2.modules():
                if isinstance(mod, mm.Quantizer):
                    mod.quant(True)
            y_packed, _ = m2(q, k, v, key_padding_mask=kpm, need_weights=False, attn_mask=attn_mask)
            y_plain, _ = m2(q, k, v, need_weights=False)
        assert torch.isfinite(y_packed).all(), name
        key = "m_" + name
        out[key + "_query"], out[key + "_key"], out[key + "_value"] = q.numpy(), k.numpy(), v.numpy()
        out[key + "_heads"] = np.array([E, H, KD], np.int32)
        for kk, vv in sd.items():
            out[key + "_sd_" + kk] = vv.numpy()
        out[key + "_y_packed"] = y_packed.numpy()
        if attn_mask is not None:
            out[key + "_attn_mask"] = attn_mask.numpy()
        if kpm is not None:
            out[key + "_key_padding_mask"] = kpm.numpy()
        index.append(key)
        print("G10 %s: max|y| %.3g, max|masked - unmasked| %.3g" % (
            name, float(y_packed.abs().max()), float((y_packed - y_plain).abs().max())))
    out["index"] = np.array(index)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
