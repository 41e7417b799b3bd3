"""A packed torchvision ViT run end to end on the engine.

torchvision's VisionTransformer with the reference's quant modules in it: conv_proj a QuantConv2d (kernel = stride = patch),
each EncoderBlock x = x + attn(ln_1(x)); x = x + mlp(ln_2(x)) with a QuantMultiheadAttention (separate q / k / v projections
after pack()) and mlp = QuantLinear, GELU, QuantLinear; the final LayerNorm on the class token and a QuantLinear head.
PackedViT takes the state_dict of such a model after pack() and runs it two ways:

  route="layers"  the reference's dataflow with the engine plugged in: conv_proj as quantize_pack of the unfolded image
                  + quantlinear, torch F.layer_norm,
                  PackedLinear for q / k / v, the attention core, quantlinear_float_input for out_proj, torch `+`, F.gelu
                  and PackedLinear for the two MLP linears, the final LayerNorm and the head;
  route="fused"   the image quantiser and the unfold in one pass (qe_quantize_patchify) and the patch embedding as a GEMM
                  on the int8 matrix cores; per block one pass of LayerNorm + the q / k / v codes
                  (qe_layernorm_quantize_pack), the three projections, the attention core, out_proj with the residual
                  add in its epilogue, LayerNorm + fc1's codes, fc1 with GELU + fc2's codes in its epilogue
                  (qe_quantlinear_requant) and fc2 with the residual add in its epilogue (qe_quantlinear_residual).

Both routes call the same attention core, _attention: by default fp32 F.scaled_dot_product_attention on (N, H, L, d) --
what F.multi_head_attention_forward runs for need_weights=False; with attention="engine" the fp32 qe_attention kernel,
which reads the three projections in their (N L, E) buffers and writes the context straight into out_proj's input; with
attention="engine_bf16" the same, its two products on the bf16 matrix cores (qe_attention_bf16: not fp32-exact).
qkv="bf16" (fused route with attention="engine_bf16" only) has the three projections write bf16 rows (qe_quantlinear_bf16,
q already multiplied by d ** -0.5) that the attention kernel reads as stored (qe_attention_bf16_stored, scale 1): the values
the bf16 kernel would have rounded to anyway, so logits and block outputs are bit-identical to qkv="fp32".
ctx="bf16" (on top of qkv="bf16") has the attention kernel write its context as bf16 rows as well (qe_attention_bf16_ctx: the
fp32 context rounded once) and out_proj read them as stored (qe_quantlinear_bf16_input, residual add in its epilogue): one
rounding of the context to 8 significant bits, so NOT bit-identical to ctx="fp32".
The C entry points take their two-pass form wherever the fused form is not eligible (sub-8-bit or per-channel consumer codes, non-MFMA shapes, QE_LIN_EPI=0), so every step of
the fused route exists for every model the layers route runs.  With check=False the fused route makes no device -> host
copy or synchronisation: every range flag accumulates in one device int32, read once at the end when check=True.
"""
import re

import numpy as np
import torch
import torch.nn.functional as F

from . import capi, synthetic
from .packed import OUT_OF_RANGE, PackedConv2d, PackedLinear, PackedMultiheadAttention, quantizer_bits
from .synthetic import pack_codes


ATTENTION = ("torch", "engine", "engine_bf16")
QKV = ("fp32", "bf16")
CTX = ("fp32", "bf16")


def _check_attention(attention):
    if attention not in ATTENTION:
        raise ValueError("attention must be 'torch', 'engine' or 'engine_bf16'")


def _check_qkv(qkv, route, attention):
    if qkv not in QKV:
        raise ValueError("qkv must be 'fp32' or 'bf16'")
    if qkv == "bf16" and (route != "fused" or attention != "engine_bf16"):
        raise ValueError("qkv='bf16' needs route='fused' and attention='engine_bf16' (the bf16 attention core reads the rows)")


def _check_ctx(ctx, route, attention, qkv):
    if ctx not in CTX:
        raise ValueError("ctx must be 'fp32' or 'bf16'")
    if ctx == "bf16" and (route != "fused" or attention != "engine_bf16" or qkv != "bf16"):
        raise ValueError("ctx='bf16' needs route='fused', attention='engine_bf16' and qkv='bf16' (the bf16 attention core on "
                         "bf16 rows writes the context)")


def _attention(Q, K, V, N, L, H, attention="torch", ctx="fp32"):
    """(N L, E) fp32 projections -> (N L, E) context: softmax(Q K^T / sqrt(d)) V per head, fp32.  bf16 projections (Q
    already scaled; "engine_bf16" only) are read as stored, with scale 1; with ctx "bf16" their context is bf16 rows too."""
    if Q.dtype == torch.bfloat16:
        return capi.attention(Q, K, V, N, L, H, scale=1.0, precision="bf16", out_dtype=torch.bfloat16 if ctx == "bf16" else None)
    if attention == "engine":
        return capi.attention(Q, K, V, N, L, H)
    if attention == "engine_bf16":
        return capi.attention(Q, K, V, N, L, H, precision="bf16")
    E = Q.shape[-1]
    d = E // H
    q, k, v = (t.reshape(N, L, H, d).transpose(1, 2) for t in (Q, K, V))
    ctx = F.scaled_dot_product_attention(q, k, v)
    return ctx.transpose(1, 2).reshape(N * L, E).contiguous()


def _run(layer, t, observe):
    """layer(t) on the `layers` route; observe(layer, its fp32 input) is called in front of it (calibration)."""
    if observe is not None:
        observe(layer, t)
    return layer(t, route="packed")


class _Block:
    def __init__(self, name, ln1, attn, ln2, fc1, fc2):
        self.name, self.ln1, self.attn, self.ln2, self.fc1, self.fc2 = name, ln1, attn, ln2, fc1, fc2
        self.q, self.k, self.v = attn.q, attn.k, attn.v


class PackedViT:
    """A packed torchvision ViT (B/16, L/16, ... or any depth / width / patch) on the engine."""

    def __init__(self, conv, class_token, pos, blocks, ln, head, num_heads, eps):
        self.conv, self.class_token, self.pos, self.blocks = conv, class_token, pos, blocks
        self.ln, self.head, self.num_heads, self.eps = ln, head, int(num_heads), float(eps)
        self.E, self.C, self.patch = conv.OC, conv.IC, conv.KH
        if conv.KH != conv.KW:
            raise ValueError("conv_proj: a %dx%d kernel; a ViT's patch embedding is square" % (conv.KH, conv.KW))
        for lin in self.linears():
            if lin.a_scale.numel() != 1:
                raise ValueError("%s: a per-channel activation quantiser (%d scales) on a linear: the packed x packed kernel "
                                 "scales by batch row, so only a per-tensor quantiser is supported" % (lin.name, lin.a_scale.numel()))
        if conv.a_scale.numel() != 1:
            raise ValueError("conv_proj: a per-channel image quantiser (%d scales): the patch embedding runs as a GEMM whose "
                             "activations are scaled by row, so only a per-tensor image quantiser is supported" % conv.a_scale.numel())

    @classmethod
    def from_state_dict(cls, sd, num_heads, eps=1e-6, prefix=""):
        sd = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}

        def need(k):
            if k not in sd:
                raise KeyError("packed ViT state_dict: missing %s%s" % (prefix, k))
            return sd[k]

        need("conv_proj.w_des")
        kh = int(sd["conv_proj.w_des"][4])
        conv = PackedConv2d.from_state_dict(sd, "conv_proj.", stride=kh, padding=0)
        idx = sorted({int(m.group(1)) for k in sd for m in [re.match(r"encoder\.layers\.encoder_layer_(\d+)\.", k)] if m})
        if not idx or idx != list(range(len(idx))):
            raise KeyError("packed ViT state_dict: encoder layers encoder_layer_0.. not found (have %s)" % idx)
        blocks = []
        for i in idx:
            pre = "encoder.layers.encoder_layer_%d." % i
            need(pre + "self_attention.q_proj_des")
            need(pre + "mlp.0.w_des")
            need(pre + "mlp.3.w_des")
            attn = PackedMultiheadAttention.from_state_dict(sd, pre + "self_attention.", num_heads)
            ln1 = (need(pre + "ln_1.weight"), need(pre + "ln_1.bias"))
            ln2 = (need(pre + "ln_2.weight"), need(pre + "ln_2.bias"))
            blocks.append(_Block(pre[:-1], ln1, attn, ln2, PackedLinear.from_state_dict(sd, pre + "mlp.0."),
                                 PackedLinear.from_state_dict(sd, pre + "mlp.3.")))
        ln = (need("encoder.ln.weight"), need("encoder.ln.bias"))
        need("heads.head.w_des")
        head = PackedLinear.from_state_dict(sd, "heads.head.")
        return cls(conv, need("class_token"), need("encoder.pos_embedding"), blocks, ln, head, num_heads, eps)

    # ---- introspection ----
    head_lin = property(lambda self: self.head)       # the head under its earlier name

    @property
    def depth(self):
        return len(self.blocks)

    @property
    def mlp_dim(self):
        return self.blocks[0].fc1.O

    def linears(self):
        out = []
        for b in self.blocks:
            out += [b.q, b.k, b.v, b.fc1, b.fc2]
        return out + [self.head]

    # ---- the two routes ----
    def __call__(self, images, route="fused", check=True, attention="torch", qkv="fp32", ctx="fp32"):
        return self.forward(images, route, check, attention=attention, qkv=qkv, ctx=ctx)[0]

    def forward(self, images, route="fused", check=True, keep_blocks=False, attention="torch", qkv="fp32", ctx="fp32"):
        """(logits, [block outputs (N, L, E)] if keep_blocks else None).  attention: "torch" (F.scaled_dot_product_attention)
        "engine" (the fp32 qe_attention kernel) or "engine_bf16" (qe_attention_bf16), in either route.  qkv: "fp32", or
        "bf16" (route "fused" with attention "engine_bf16" only; ValueError otherwise, before any launch): the q / k / v
        projections as bf16 rows, bit-identical results.  ctx: "fp32", or "bf16" (with qkv "bf16" only; ValueError otherwise,
        before any launch): the attention context as bf16 rows that out_proj reads in place -- the context rounded once."""
        if route not in ("fused", "layers"):
            raise ValueError("route must be 'fused' or 'layers'")
        _check_attention(attention)
        _check_qkv(qkv, route, attention)
        _check_ctx(ctx, route, attention, qkv)
        kw = {} if attention == "torch" else {"attention": attention}    # the default keeps block()'s five-argument call
        if qkv != "fp32":
            kw["qkv"] = qkv
        if ctx != "fp32":
            kw["ctx"] = ctx
        images = images.contiguous()
        N = images.shape[0]
        status = torch.zeros(1, dtype=torch.int32, device=images.device)
        x = self.embed(images, route, status)
        outs = [] if keep_blocks else None
        for b in self.blocks:
            x = self.block(b, x, N, route, status, **kw)
            if keep_blocks:
                outs.append(x.reshape(N, -1, self.E).clone())
        cls_rows = x.reshape(N, -1, self.E)[:, 0].contiguous()
        y = F.layer_norm(cls_rows, (self.E,), self.ln[0], self.ln[1], self.eps)
        if route == "layers":
            logits = self.head(y, route="packed")
        else:
            logits = self.head.call_packed(*self.head.quantize_codes(y, status), status=status)
            if check and int(status.item()) != 0:
                raise RuntimeError(OUT_OF_RANGE)
        return logits, outs

    def embed(self, images, route, status, observe=None):
        """Patch embedding + class token + position embedding: (N L, E) fp32 rows.  observe: see _run (`layers` route)."""
        N, C, H, W = images.shape
        p = self.patch
        c = self.conv
        rows = N * (H // p) * (W // p)
        if route == "layers":
            # the Quantizer on the unfolded image, then the conv as the GEMM it is (the engine's direct convolution has
            # no kernel for a 16 x 16 filter of 768 taps)
            if observe is not None:
                observe(c, images)
            u = images.reshape(N, C, H // p, p, W // p, p).permute(0, 2, 4, 1, 3, 5).reshape(rows, C * p * p).contiguous()
            codes = capi.quantize_pack(u, c.a_scale, c.a_zero, c.a_qmin, c.a_qmax, c.a_bits, c.a_signed)[0]
        else:
            codes = capi.quantize_patchify(images, p, c.a_scale, c.a_zero, c.a_qmin, c.a_qmax, c.a_bits, c.a_signed,
                                           status=status)[0]
        # quantlinear's convention: (q + zero) with the module's zero -- the conv's (q - zero') with zero' = -zero
        xq, wq = c.xq(codes, linear=True), c.wq(linear=True)
        t = capi.quantlinear(xq, wq, c.bias, rows, C * p * p, self.E).reshape(N, -1, self.E)
        x = torch.cat([self.class_token.expand(N, -1, -1), t], dim=1) + self.pos
        return x.reshape(-1, self.E).contiguous()

    def block(self, b, x, N, route, status=None, attention="torch", observe=None, qkv="fp32", ctx="fp32"):
        """One encoder block on (N L, E) fp32 rows -> (N L, E).  The fused route updates x in place.  observe: see _run
        (`layers` route).  qkv, ctx: see forward."""
        _check_attention(attention)
        _check_qkv(qkv, route, attention)
        _check_ctx(ctx, route, attention, qkv)
        E, H = self.E, self.num_heads
        L = x.shape[0] // N
        if route == "layers":
            y = F.layer_norm(x, (E,), b.ln1[0], b.ln1[1], self.eps)
            Q, K, V = (_run(lin, y, observe) for lin in (b.q, b.k, b.v))
            c = _attention(Q, K, V, N, L, H, attention)
            x = x + capi.quantlinear_float_input(c, b.attn.out_wq(), b.attn.out_bias, E)
            y = F.layer_norm(x, (E,), b.ln2[0], b.ln2[1], self.eps)
            h = F.gelu(_run(b.fc1, y, observe))
            return x + _run(b.fc2, h, observe)
        if status is None:
            status = torch.zeros(1, dtype=torch.int32, device=x.device)
        rows = x.shape[0]
        codes = capi.layernorm_quantize_pack(x, b.ln1[0], b.ln1[1], self.eps, [b.q.requant(), b.k.requant(), b.v.requant()],
                                             status=status)[0]
        if qkv == "bf16":       # q carries the score scale, the fp32 value capi.attention would pass: the kernel's own q^
            post = ((E // H) ** -0.5, 1.0, 1.0)
            Q, K, V = (capi.quantlinear_bf16(lin.xq(c), lin.wq(), lin.bias, rows, lin.K, lin.O, post_scale=s)
                       for lin, c, s in zip((b.q, b.k, b.v), codes, post))
        else:
            Q, K, V = (capi.quantlinear(lin.xq(c), lin.wq(), lin.bias, rows, lin.K, lin.O) for lin, c in zip((b.q, b.k, b.v), codes))
        c = _attention(Q, K, V, N, L, H, attention, ctx)
        if ctx == "bf16":
            x = capi.quantlinear_bf16_input(c, b.attn.out_wq(), b.attn.out_bias, E, residual=x, out=x)
        else:
            x = capi.quantlinear_float_input_residual(c, b.attn.out_wq(), b.attn.out_bias, E, x, out=x)
        c1 = capi.layernorm_quantize_pack(x, b.ln2[0], b.ln2[1], self.eps, [b.fc1.requant()], status=status)[0][0]
        c2 = capi.quantlinear_requant(b.fc1.xq(c1), b.fc1.wq(), b.fc1.bias, rows, b.fc1.K, b.fc1.O, b.fc2.requant(), act="gelu",
                                      status=status)[0]
        return capi.quantlinear_residual(b.fc2.xq(c2), b.fc2.wq(), b.fc2.bias, rows, b.fc2.K, b.fc2.O, x, out=x)

    # ---- calibration (synthetic models, tests, tools) ----
    def calibrate(self, images):
        """Set every activation quantiser from what reaches it in one `layers` pass: signed ones max|x| / qmax, the
        unsigned ones (fc2's, after the GELU) asymmetric over [min, max] with zero = round(min / scale)."""
        def set_q(m, t):
            if m.a_signed:
                m.a_scale = torch.clamp(t.abs().max() / m.a_qmax, min=1e-8).reshape(1)
            else:
                lo, hi = t.min(), t.max()
                s = torch.clamp((hi - lo) / (m.a_qmax - m.a_qmin), min=1e-8)
                m.a_scale = s.reshape(1)
                m.a_zero = torch.round(lo / s).reshape(1)
        with torch.no_grad():
            N = images.shape[0]
            x = self.embed(images, "layers", None, observe=set_q)
            for b in self.blocks:
                x = self.block(b, x, N, "layers", observe=set_q)
            set_q(self.head, F.layer_norm(x.reshape(N, -1, self.E)[:, 0], (self.E,), self.ln[0], self.ln[1], self.eps))
        return self

    def state_dict_quantizers(self):
        """{key: tensor} of every activation quantiser's scale and zero, in the state_dict's key layout."""
        out = {}

        def put(prefix, m):
            out[prefix + "scale"], out[prefix + "zero"] = m.a_scale, m.a_zero
        put("conv_proj.a_quantizer.", self.conv)
        for b in self.blocks:
            for n, lin in (("q", b.q), ("k", b.k), ("v", b.v)):
                put(b.name + ".self_attention.%s_quantizer." % n, lin)
            put(b.name + ".mlp.0.a_quantizer.", b.fc1)
            put(b.name + ".mlp.3.a_quantizer.", b.fc2)
        put("heads.head.a_quantizer.", self.head)
        return out


# ---------------------------------------------------------------------------------------------
# From a calibrated reference ViT to this engine
# ---------------------------------------------------------------------------------------------
def _pack_weight(w, scale, zero, qmin, qmax, static_scale=None):
    """Quantizer.pack() of a weight (quantizer.py:228-250) + tpack: round(w / scale - zero).clamp(qmin, qmax) in fp32, the
    stored b-bit stream, des [n_bits, sign, *shape], and (scale * static_scale, zero)."""
    n_bits, signed = quantizer_bits(qmin, qmax)
    w = w.detach().float().cpu()
    scale, zero = scale.detach().float().cpu(), zero.detach().float().cpu()
    q = (w / scale - zero).round().clamp(float(qmin), float(qmax))
    packed = torch.from_numpy(pack_codes(q.numpy().astype(np.int64), n_bits, signed))
    des = torch.tensor([n_bits, 1 if signed else 0] + list(w.shape), dtype=torch.int32)
    s = scale if static_scale is None else scale * static_scale.detach().float().cpu()
    return packed, des, s, zero


def pack_vit_state_dict(sd):
    """The state_dict a calibrated (unpacked) reference ViT would have after pack() -- which the reference cannot produce
    itself: QuantMultiheadAttention.pack() reads the None q_proj_weight when kdim == embed_dim (its in_proj_weight form).
    QuantConv2d / QuantLinear: weight -> packed stream, w_des, w_scale = scale * static_scale, w_zero
    (quantconv2d.py:187-192, quantlinear.py:123-148); QuantMultiheadAttention: in_proj_weight packed per chunk with the
    q / k / v projection quantisers, out_proj.weight with out_proj_quantizer (quantmultiheadattention.py:165-223).
    Activation quantisers, biases, LayerNorms, class token and position embedding pass through.  Every key of `sd` is
    consumed: an unknown key raises ValueError.  Returns host tensors in PackedViT.from_state_dict's layout."""
    sd = {k: v for k, v in sd.items()}
    out, used = {}, set()

    def take(k):
        used.add(k)
        return sd[k]

    def wq(prefix):
        st = sd.get(prefix + "_static_scale")
        if st is not None:
            used.add(prefix + "_static_scale")
        return take(prefix + "scale"), take(prefix + "zero"), take(prefix + "qmin"), take(prefix + "qmax"), st

    for k in sorted(sd):
        if k.endswith(".w_quantizer.scale"):
            pre = k[:-len("w_quantizer.scale")]
            packed, des, s, z = _pack_weight(take(pre + "weight"), *wq(pre + "w_quantizer."))
            out[pre + "weight"], out[pre + "w_des"], out[pre + "w_scale"], out[pre + "w_zero"] = packed, des, s, z
        elif k.endswith(".q_proj_quantizer.scale"):
            pre = k[:-len("q_proj_quantizer.scale")]
            if pre + "in_proj_weight" in sd:
                chunks = take(pre + "in_proj_weight").chunk(3)
            else:
                chunks = [take(pre + n + "_proj_weight") for n in ("q", "k", "v")]
            for n, w in zip(("q", "k", "v"), chunks):
                packed, des, s, z = _pack_weight(w, *wq(pre + n + "_proj_quantizer."))
                out[pre + n + "_proj_weight"], out[pre + n + "_proj_des"] = packed, des
                out[pre + n + "_proj_scale"], out[pre + n + "_proj_zero"] = s, z
            packed, des, s, z = _pack_weight(take(pre + "out_proj.weight"), *wq(pre + "out_proj_quantizer."))
            out[pre + "out_proj.weight"], out[pre + "out_proj_des"], out[pre + "out_proj_scale"], out[pre + "out_proj_zero"] = \
                packed, des, s, z
    for k, v in sd.items():
        if k in used:
            continue
        if re.search(r"(a_quantizer|[qkv]_quantizer)\.(scale|zero|qmin|qmax)$", k) or \
                re.search(r"(\.bias|ln_[12]\.weight|ln\.weight|class_token|pos_embedding)$", k) or k.endswith("in_proj_bias"):
            out[k] = v.detach().cpu() if torch.is_tensor(v) else v
            used.add(k)
    left = sorted(set(sd) - used)
    if left:
        raise ValueError("pack_vit_state_dict: keys of no known ViT layer: %s" % left[:8])
    return out


# ---------------------------------------------------------------------------------------------
# Synthetic packed ViTs (tests and tools/bench_vit_forward.py share this construction)
# ---------------------------------------------------------------------------------------------
CONFIGS = {
    "vit_b_16": dict(image_size=224, patch=16, width=768, heads=12, mlp=3072, depth=12, num_classes=1000),
    "vit_tiny_test": dict(image_size=32, patch=8, width=64, heads=4, mlp=256, depth=2, num_classes=10),
}


def _lin_entries(rng, O, K, w_bits, bias, signed_act=True, a_bits=8):
    lim = (1 << (w_bits - 1)) - 1
    q = rng.randint(-lim, lim + 1, size=(O, K))
    std_q = np.sqrt(((2 * lim + 1) ** 2 - 1) / 12.0)
    ws = np.sqrt(1.0 / K) / std_q * rng.uniform(0.8, 1.2, size=(O, 1))
    qmin, qmax = (-(1 << (a_bits - 1)), (1 << (a_bits - 1)) - 1) if signed_act else (0, (1 << a_bits) - 1)
    e = {"weight": torch.from_numpy(pack_codes(q, w_bits, True)),
         "w_des": torch.tensor([w_bits, 1, O, K], dtype=torch.int32),
         "w_scale": torch.from_numpy(ws.astype(np.float32)),
         "w_zero": torch.zeros((O, 1), dtype=torch.float32),
         "a_quantizer.scale": torch.tensor([1.0], dtype=torch.float32),
         "a_quantizer.zero": torch.tensor([0.0], dtype=torch.float32),
         "a_quantizer.qmin": torch.tensor(float(qmin)), "a_quantizer.qmax": torch.tensor(float(qmax))}
    if bias:
        e["bias"] = torch.from_numpy(rng.normal(0, 0.02, size=O).astype(np.float32))
    return e


def synthetic_state_dict(arch="vit_b_16", w_bits=8, a_bits=8, seed=0, **over):
    """A packed ViT state_dict in the key layout pack() leaves (host tensors, activation scales not calibrated: 1.0).
    Random b-bit weights scaled to unit gain, LayerNorm affine parameters near (1, 0); every activation quantiser signed
    per tensor except fc2's (after the GELU): unsigned and asymmetric once calibrated.  See calibrated_state_dict."""
    cfg = dict(CONFIGS[arch])
    cfg.update(over)
    rng = np.random.RandomState(seed)
    E, p, C, M = cfg["width"], cfg["patch"], 3, cfg["mlp"]
    L = (cfg["image_size"] // p) ** 2 + 1
    sd = {}
    conv = _lin_entries(rng, E, C * p * p, w_bits, True, True, a_bits)
    conv["w_des"] = torch.tensor([w_bits, 1, E, C, p, p], dtype=torch.int32)
    conv["w_scale"] = conv["w_scale"].reshape(E, 1, 1, 1)
    conv["w_zero"] = conv["w_zero"].reshape(E, 1, 1, 1)
    synthetic.put(sd, "conv_proj", conv)
    sd["class_token"] = torch.from_numpy(rng.normal(0, 0.02, size=(1, 1, E)).astype(np.float32))
    sd["encoder.pos_embedding"] = torch.from_numpy(rng.normal(0, 0.02, size=(1, L, E)).astype(np.float32))
    for i in range(cfg["depth"]):
        pre = "encoder.layers.encoder_layer_%d." % i
        for ln in ("ln_1", "ln_2"):
            sd[pre + ln + ".weight"] = torch.from_numpy(rng.uniform(0.8, 1.2, size=E).astype(np.float32))
            sd[pre + ln + ".bias"] = torch.from_numpy(rng.normal(0, 0.05, size=E).astype(np.float32))
        att = pre + "self_attention."
        for n in ("q", "k", "v"):
            e = _lin_entries(rng, E, E, w_bits, False, True, a_bits)
            sd[att + n + "_proj_weight"], sd[att + n + "_proj_des"] = e["weight"], e["w_des"]
            sd[att + n + "_proj_scale"], sd[att + n + "_proj_zero"] = e["w_scale"], e["w_zero"]
            for k in ("scale", "zero", "qmin", "qmax"):
                sd[att + n + "_quantizer." + k] = e["a_quantizer." + k]
        sd[att + "in_proj_bias"] = torch.from_numpy(rng.normal(0, 0.02, size=3 * E).astype(np.float32))
        o = _lin_entries(rng, E, E, w_bits, True)
        o["w_scale"] = o["w_scale"] * 0.5            # residual branches at half gain: activations stay O(1) through the depth
        sd[att + "out_proj.weight"], sd[att + "out_proj_des"] = o["weight"], o["w_des"]
        sd[att + "out_proj_scale"], sd[att + "out_proj_zero"] = o["w_scale"], o["w_zero"]
        sd[att + "out_proj.bias"] = o["bias"]
        synthetic.put(sd, pre + "mlp.0", _lin_entries(rng, M, E, w_bits, True, True, a_bits))
        f2 = _lin_entries(rng, E, M, w_bits, True, False, a_bits)
        f2["w_scale"] = f2["w_scale"] * 0.5
        synthetic.put(sd, pre + "mlp.3", f2)
    sd["encoder.ln.weight"] = torch.ones(E, dtype=torch.float32)
    sd["encoder.ln.bias"] = torch.zeros(E, dtype=torch.float32)
    synthetic.put(sd, "heads.head", _lin_entries(rng, cfg["num_classes"], E, w_bits, True, True, a_bits))
    return sd


def calibrated_state_dict(arch="vit_b_16", device="cuda", calib_images=None, calib_batch=2, **kw):
    """synthetic_state_dict on `device` with every activation quantiser calibrated from one `layers` pass."""
    cfg = dict(CONFIGS[arch])
    cfg.update({k: v for k, v in kw.items() if k in cfg})
    images = synthetic.calibration_images(calib_images, calib_batch, cfg["image_size"], kw.get("seed", 0))
    return synthetic.calibrated(synthetic_state_dict(arch, **kw), device, lambda sd: PackedViT.from_state_dict(sd, cfg["heads"]),
                                images, PackedViT.state_dict_quantizers)
