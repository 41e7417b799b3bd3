"""Opt-in wiring of packed Quant modules to the operator path.

The reference's packed forward still dequantises and calls F.conv2d / F.linear; the operator call is commented out
(modelzoo/modules/quantconv2d.py:198-210, quantlinear.py:150-161) and the runners' packing loop with it
(runner/ptq.py:106-114).  These two classes are what those call sites become on this engine.  They take the STATE of a
packed module -- tensors only, exactly the state_dict entries pack() leaves behind (quantconv2d.py:187-192:
weight = packed uint8 stream, w_des, w_scale, w_zero, bias, a_quantizer.{scale, zero, qmin, qmax}) -- so no reference
Python is needed where they run, and they keep the weights PACKED (no tunpack on load, the TODO of quantconv2d.py:230-233).

Sign conventions, reconciled here and nowhere else:
  * the modules dequantise as (q + zero) * scale (quantizer.py:218);
  * quantconv2d / quantconv2d_float_input / quantlinear_float_input take (q - zero) * scale -> zeros are negated;
  * quantlinear (packed x packed) takes (q + zero) (quantlinear.cu:115,120)             -> zeros pass unchanged.

Two routes per layer, as the operator's dtype dispatch offers them (quantconv2dop.py:88-95):
  route="packed"  activations are quantised AND packed on the device in one pass (engine.quantize_pack: the
                  Quantizer's round(x / scale - zero).clamp(qmin, qmax) + tpack) and meet the packed weights on the
                  int8 MFMA kernels;
  route="float"   the form the reference's TODO names first ("only support float input and packed weight"): the
                  fake-quantised fp32 activations (q + zero) * scale with the packed weights.
"""
import functools

import torch

from . import capi, engine
from .operator import quantconv2d_forward, quantlinear_forward

OUT_OF_RANGE = "The input tensor is out of range."    # tpack.cu:14, as engine.tpack raises it


def _first(v):
    return int(v[0]) if isinstance(v, (tuple, list)) else int(v)


def quantizer_bits(qmin, qmax):
    """(n_bits, signed) of a quantiser whose codes span [qmin, qmax]."""
    qmin, qmax = float(qmin), float(qmax)
    return max(1, int(round(qmax - qmin)).bit_length()), qmin < 0


def _host_des(des):
    """A (packed, des) pair's description as host integers: one device -> host read when it is a tensor."""
    return [int(v) for v in (des.tolist() if torch.is_tensor(des) else des)]


class _PackedBase:
    LINEAR = False      # True: the layer's own op is the packed x packed quantlinear, which takes (q + zero)

    def __init__(self, weight, w_des, w_scale, w_zero, bias, a_scale, a_zero, a_qmin, a_qmax, a_bits, a_signed, name=None):
        assert weight.dtype == torch.uint8 and weight.dim() == 1, "weight must be the packed 1-D uint8 stream pack() stores"
        self.weight, self.w_des, self.bias, self.name = weight, w_des, bias, name
        # parsed once, here, where the state_dict tensors normally still live on the host
        wd = [int(v) for v in w_des.tolist()]
        self.w_bits, self.w_signed, self.w_shape = wd[0], bool(wd[1]), wd[2:]
        self.w_scale, self.w_zero = w_scale.contiguous(), w_zero.contiguous()            # module convention (q + zero)
        self._neg_w_zero = (-self.w_zero).contiguous()       # kernel convention, built once (tensors stay alive: cache keys)
        self.a_qmin, self.a_qmax = float(a_qmin), float(a_qmax)
        self.a_bits, self.a_signed = int(a_bits), bool(a_signed)
        self._set_quantizer(a_scale, a_zero)

    @classmethod
    def _state(cls, sd, prefix):
        g = lambda k: sd[prefix + k]
        qmin, qmax = float(g("a_quantizer.qmin")), float(g("a_quantizer.qmax"))
        a_bits, a_signed = quantizer_bits(qmin, qmax)
        return dict(weight=g("weight"), w_des=g("w_des"), w_scale=g("w_scale"), w_zero=g("w_zero"),
                    bias=sd.get(prefix + "bias"), a_scale=g("a_quantizer.scale"), a_zero=g("a_quantizer.zero"),
                    a_qmin=qmin, a_qmax=qmax, a_bits=a_bits, a_signed=a_signed, name=prefix.rstrip("."))

    # ---- the activation quantiser: assigning a_scale or a_zero updates everything derived from them ----
    a_scale = property(lambda self: self._a_scale, lambda self, v: self._set_quantizer(v, self._a_zero))
    a_zero = property(lambda self: self._a_zero, lambda self, v: self._set_quantizer(self._a_scale, v))

    def _set_quantizer(self, scale, zero):
        self._a_scale = scale.reshape(-1).contiguous().float()
        self._a_zero = zero.reshape(-1).contiguous().float()
        self._neg_a_zero = (-self._a_zero).contiguous()
        s, z = tuple(self._a_scale.tolist()), tuple(self._a_zero.tolist())
        self.q_key = (s, z, self.a_qmin, self.a_qmax, self.a_bits, self.a_signed)      # two layers share codes when equal
        # round(max(y, 0) / s - 0).clamp(0, qmax) == round(y / s).clamp(0, qmax): the producer's ReLU folds into the clamp
        self.folds_relu = (not self.a_signed) and self.a_qmin == 0.0 and all(v == 0.0 for v in z) and all(v > 0.0 for v in s)

    def to(self, device):
        for k, v in list(vars(self).items()):
            if torch.is_tensor(v):
                setattr(self, k, v.to(device))
        return self

    # ---- operands of the C ABI.  The sign convention is decided here and nowhere else: the packed x packed quantlinear
    # takes the module's (q + zero); the convs and the float-input operators take (q - zero) -> the negated zeros ----
    def wq(self, linear=None):
        """The packed weights as a capi.qparam for this layer's own op, or for the packed x packed quantlinear
        (linear=True: a conv run as the GEMM it is)."""
        zero = self.w_zero if (self.LINEAR if linear is None else linear) else self._neg_w_zero
        return capi.qparam(self.weight, self.w_bits, self.w_signed, self.w_scale.reshape(-1), zero.reshape(-1))

    def xq(self, codes, n_bits=None, signed=None, linear=None):
        """A code stream of this layer's activation quantiser (or of n_bits / signed codes at its scale) as a capi.qparam."""
        zero = self._a_zero if (self.LINEAR if linear is None else linear) else self._neg_a_zero
        return capi.qparam(codes, self.a_bits if n_bits is None else n_bits, self.a_signed if signed is None else signed,
                           self._a_scale, zero)

    def requant(self):
        """This layer's activation quantiser as a capi.requant, for the epilogue of the layer that feeds it."""
        return capi.requant(self._a_scale, self._a_zero, self.a_qmin, self.a_qmax, self.a_bits, self.a_signed)

    def quantize_codes(self, x, status):
        """quantize() through the C ABI with no host synchronisation: the range flag accumulates in `status`.  Returns
        (packed, des) with des on the host; x is (N, C, ...) with a per-channel quantiser's channels in dimension 1."""
        inner = 1
        for v in x.shape[2:]:
            inner *= v
        codes = capi.quantize_pack(x, self._a_scale, self._a_zero, self.a_qmin, self.a_qmax, self.a_bits, self.a_signed,
                                   inner=inner, status=status)[0]
        return codes, (self.a_bits, int(self.a_signed), *x.shape)

    def quantize(self, x, channel_dim=1):
        """Quantizer.simulate in packed mode (quantizer.py:215,226) fused with tpack: (packed, des)."""
        return engine.quantize_pack(x.contiguous(), self.a_scale, self.a_zero, self.a_qmin, self.a_qmax, self.a_bits,
                                    self.a_signed, channel_dim)

    def fake_quant(self, x, channel_dim=1):
        """(q + zero) * scale in fp32: what the reference's packed forward feeds F.conv2d (quantconv2d.py:207-208)."""
        shape = [1] * x.dim()
        if self.a_scale.numel() > 1:
            shape[channel_dim] = -1
        s, z = self.a_scale.view(shape), self.a_zero.view(shape)
        q = (x / s - z).round().clamp(self.a_qmin, self.a_qmax)
        return ((q + z) * s).contiguous()


class _PackedConvBase(_PackedBase):
    """The geometry the three conv classes share; IC, OC, KH, KW, stride and padding are their constructors'."""

    def out_hw(self, H, W):
        return ((H + 2 * self.padding - self.KH) // self.stride + 1, (W + 2 * self.padding - self.KW) // self.stride + 1)

    def shape(self, N, H, W):
        return capi.conv_shape(N, self.IC, H, W, self.OC, self.KH, self.KW, self.stride, self.padding)


class PackedConv2d(_PackedConvBase):
    """A packed QuantConv2d's forward on the engine: quantconv2d_forward(x, (weight, w_des, w_scale, w_zero), bias,
    stride, padding, dilation, groups) -- the commented call of quantconv2d.py:204-206 -- with the activation operand
    produced on the device."""

    def __init__(self, *, stride=1, padding=0, **state):
        super().__init__(**state)
        self.stride, self.padding = _first(stride), _first(padding)
        self.OC, self.IC, self.KH, self.KW = self.w_shape
        self._prep = {}

    @classmethod
    def from_state_dict(cls, state_dict, prefix="", stride=1, padding=0):
        return cls(stride=stride, padding=padding, **cls._state(state_dict, prefix))

    def to(self, device):
        self._prep = {}
        return super().to(device)

    def operands(self, codes, N, H, W, n_bits=None, signed=None):
        """(qe_conv_shape, activation operand, weight operand, prepared weight tables) of this conv on `codes` of an
        N x IC x H x W input.  The tables are prepared once per table layout (batch size does not enter)."""
        sh, xq, wq = self.shape(N, H, W), self.xq(codes, n_bits, signed), self.wq()
        key = (xq.n_bits, capi.conv_prepared_layout(sh, xq.n_bits, self.w_bits))
        if key not in self._prep:
            self._prep[key] = capi.conv_prepare(wq, self.bias, sh, xq.n_bits)
        return sh, xq, wq, self._prep[key]

    # ---- the two steps of a model's fused route: codes of this layer's own quantiser in, no host read ----
    def fp32_from_codes(self, codes, N, H, W):
        """The fp32 output on `codes` of an N x IC x H x W input."""
        sh, xq, wq, prep = self.operands(codes, N, H, W)
        return capi.quantconv2d_prepared(xq, wq, self.bias, sh, prep)

    def relu_codes(self, codes, N, H, W, consumer, status):
        """relu(output) as consumer's codes: from this conv's own epilogue where the ReLU folds into consumer's clamp, else
        fp32 + relu + quantize_pack.  The range flag accumulates in `status`."""
        if not consumer.folds_relu:
            return consumer.quantize_codes(torch.relu(self.fp32_from_codes(codes, N, H, W)), status)[0]
        sh, xq, wq, prep = self.operands(codes, N, H, W)
        return capi.quantconv2d_requant_prepared(xq, wq, self.bias, sh, prep, consumer.requant(), status=status)[0]

    def __call__(self, x, route="packed"):
        w = (self.weight, self.w_des, self.w_scale, self._neg_w_zero)
        if route == "packed":
            xq, x_des = self.quantize(x)
            return quantconv2d_forward((xq, x_des, self.a_scale, self._neg_a_zero), w, self.bias,
                                       (self.stride, self.stride), (self.padding, self.padding), (1, 1), 1)
        if route == "float":
            return quantconv2d_forward(self.fake_quant(x), w, self.bias, self.stride, self.padding, 1, 1)
        raise ValueError("route must be 'packed' or 'float'")

    # ---- packed in, packed out: the conv-epilogue form of f-2 ----
    def call_packed(self, xq, x_des, consumer=None, status=None):
        """Activations as (packed stream, des) -- what quantize(), quantize_codes() or an earlier call_packed() returned.
        consumer=None: the fp32 output.  consumer = the Packed* layer that reads this layer's output directly: returns the
        (packed, des) pair of ITS activation quantiser, written by this layer's conv kernel itself
        (qe_quantconv2d_requant_prepared): no fp32 tensor between the two layers.  Bit-identical to
        consumer.quantize(self.call_packed(xq, x_des)).  (A ReLU in between folds into the clamp when the consumer's codes
        are unsigned with zero point 0: round(max(y, 0) / s).clamp(0, qmax) == round(y / s).clamp(0, qmax).)
        status: a device int32 the range flag accumulates in; nothing is read back or copied, des comes back as host
        integers.  None: raise when the codes are out of range."""
        n_bits, sign, N, IC, H, W = _host_des(x_des)
        if IC != self.IC:
            raise ValueError("codes of %d channels for a conv of %d" % (IC, self.IC))
        sh, x, w, prepared = self.operands(xq, N, H, W, n_bits, sign)
        if consumer is None:
            return capi.quantconv2d_prepared(x, w, self.bias, sh, prepared)
        out, flag = capi.quantconv2d_requant_prepared(x, w, self.bias, sh, prepared, consumer.requant(), status=status)
        if status is None and int(flag.item()) != 0:
            raise RuntimeError(OUT_OF_RANGE)
        des = (consumer.a_bits, int(consumer.a_signed), N, self.OC, *self.out_hw(H, W))
        return out, (des if status is not None else torch.tensor(des, dtype=torch.int32, device=xq.device))


class _PackedSpanConv(_PackedConvBase):
    """The calls the depthwise and the grouped class share.  KIND names the layer in messages; _conv is its entry point."""
    KIND = None

    def _conv(self, x, w, sh, **kw):
        raise NotImplementedError

    def __call__(self, x, route="packed"):
        if route == "float":
            raise ValueError("route='float': there is no float-input %s kernel; use route='packed'" % self.KIND)
        if route != "packed":
            raise ValueError("route must be 'packed'")
        xq, x_des = self.quantize(x)
        return self.call_packed(xq, x_des)

    def call_packed(self, xq, x_des, consumer=None, relu=False, status=None):
        """Activations as (packed stream, des), as PackedConv2d.call_packed.  consumer=None: the fp32 output (after the ReLU
        when relu).  consumer = the Packed* layer that reads [relu of] this layer's output: the (packed, des) pair of ITS
        activation quantiser from this layer's own epilogue, bit-identical to consumer.quantize([relu](fp32 output)).
        Sub-8-bit consumers go through an fp32 tensor inside the call (two planes can share a byte of their stream)."""
        n_bits, sign, N, C, H, W = _host_des(x_des)
        if C != self.IC:
            raise ValueError("codes of %d channels for a %s conv of %d" % (C, self.KIND, self.IC))
        sh, x, w = self.shape(N, H, W), self.xq(xq, n_bits, sign), self.wq()
        if consumer is None:
            return self._conv(x, w, sh, relu=relu)[0]
        _, codes, flag = self._conv(x, w, sh, relu=relu, rq=consumer.requant(), out="new" if consumer.a_bits < 8 else None,
                                    status=status)
        if status is None and int(flag.item()) != 0:
            raise RuntimeError(OUT_OF_RANGE)
        des = (consumer.a_bits, int(consumer.a_signed), N, self.OC, *self.out_hw(H, W))
        return codes, (des if status is not None else torch.tensor(des, dtype=torch.int32, device=xq.device))

    def relu_codes(self, codes, N, H, W, consumer, status):
        """As PackedConv2d.relu_codes: the ReLU is applied in this layer's own epilogue, whatever consumer's quantiser."""
        return self.call_packed(codes, (self.a_bits, int(self.a_signed), N, self.IC, H, W), consumer, relu=True, status=status)[0]


class PackedDepthwiseConv2d(_PackedSpanConv):
    """A packed depthwise QuantConv2d (groups == in_channels == out_channels; pack() leaves w_des [b, s, C, 1, KH, KW]) on
    qe_quantconv2d_depthwise: codes in, fp32 and / or the consumer's codes out.  The sign convention is the convs':
    (q - zero), so the zeros are negated.  There is no float-input depthwise kernel and nothing runs in its place."""
    KIND = "depthwise"

    def __init__(self, *, stride=1, padding=0, **state):
        super().__init__(**state)
        self.stride, self.padding = _first(stride), _first(padding)
        self.C, per_group, self.KH, self.KW = self.w_shape
        if per_group != 1:
            raise ValueError("%s: w_des %s is not a depthwise layer's (its second shape entry, the input channels of a group, "
                             "must be 1); use PackedConv2d" % (self.name or "layer", [self.w_bits, int(self.w_signed)] + self.w_shape))
        self.IC = self.OC = self.C

    @classmethod
    def from_state_dict(cls, state_dict, prefix="", stride=1, padding=0):
        return cls(stride=stride, padding=padding, **cls._state(state_dict, prefix))

    def _conv(self, x, w, sh, **kw):
        return capi.quantconv2d_depthwise(x, w, self.bias, sh, **kw)


class PackedGroupedConv2d(_PackedSpanConv):
    """A packed grouped QuantConv2d (1 < groups < channels; pack() leaves w_des [b, s, OC, IC / groups, KH, KW]) on
    qe_quantconv2d_grouped: codes in, fp32 and / or the consumer's codes out.  w_des does not name the groups, so the layer's
    input channels are given.  The sign convention is the convs': (q - zero), so the zeros are negated.  There is no
    float-input grouped kernel and nothing runs in its place."""
    KIND = "grouped"

    def __init__(self, *, stride=1, padding=0, in_channels, **state):
        super().__init__(**state)
        self.stride, self.padding = _first(stride), _first(padding)
        self.OC, self.ICg, self.KH, self.KW = self.w_shape
        self.IC = int(in_channels)
        who = self.name or "layer"
        if self.ICg < 1 or self.IC % self.ICg != 0:
            raise ValueError("%s: %d input channels are no multiple of the %d a group has in w_des" % (who, self.IC, self.ICg))
        self.groups = self.IC // self.ICg
        if self.groups == 1:
            raise ValueError("%s: groups == 1 is a dense layer; use PackedConv2d" % who)
        if self.OC % self.groups != 0:
            raise ValueError("%s: %d output channels are no multiple of the %d groups" % (who, self.OC, self.groups))
        if self.groups == self.IC and self.OC == self.IC:
            raise ValueError("%s: groups == in_channels == out_channels is a depthwise layer; use PackedDepthwiseConv2d" % who)

    @classmethod
    def from_state_dict(cls, state_dict, prefix="", stride=1, padding=0, in_channels=None):
        if in_channels is None:
            raise ValueError("PackedGroupedConv2d.from_state_dict: in_channels is required (w_des does not name the groups)")
        return cls(stride=stride, padding=padding, in_channels=in_channels, **cls._state(state_dict, prefix))

    def _conv(self, x, w, sh, **kw):
        return capi.quantconv2d_grouped(x, w, self.bias, sh, self.groups, **kw)


class PackedLinear(_PackedBase):
    """A packed QuantLinear's forward on the engine (quantlinear.py:150-161).  The packed x packed kernel of the
    reference indexes the activation scale by batch ROW (quantlinear.cu:96), so a per-tensor scale is what the modules'
    'layer' granularity provides; inputs with leading dimensions are flattened to (rows, in_features)."""
    LINEAR = True

    def __init__(self, **state):
        super().__init__(**state)
        self.O, self.K = self.w_shape[0], self.w_shape[-1]

    @classmethod
    def from_state_dict(cls, state_dict, prefix=""):
        return cls(**cls._state(state_dict, prefix))

    def __call__(self, x, route="packed"):
        lead = x.shape[:-1]
        x2 = x.reshape(-1, x.shape[-1])
        ws, wz = self.w_scale.reshape(-1), self.w_zero.reshape(-1)
        if route == "packed":
            assert self.a_scale.numel() == 1, "quantlinear takes a per-tensor or per-row activation scale"
            xq, x_des = self.quantize(x2, channel_dim=x2.dim() - 1)
            y = quantlinear_forward((xq, x_des, self.a_scale, self.a_zero), (self.weight, self.w_des, ws, wz), self.bias)
        elif route == "float":
            y = quantlinear_forward(self.fake_quant(x2, channel_dim=x2.dim() - 1),
                                    (self.weight, self.w_des, ws, self._neg_w_zero.reshape(-1)), self.bias)
        else:
            raise ValueError("route must be 'packed' or 'float'")
        return y.reshape(*lead, y.shape[-1])

    # ---- packed in, packed out: the linear-epilogue forms ----
    def call_packed(self, xq, x_des, consumer=None, act=None, residual=None, status=None):
        """Activations as (packed stream, des [n_bits, sign, rows, in_features]) -- what quantize(), quantize_codes() or an
        earlier call_packed() returned.  consumer=None: the fp32 (rows, out_features) output, plus `residual` when given
        (qe_quantlinear_residual: the add in the kernel's epilogue; bit-identical to self.call_packed(xq, x_des) + residual).
        consumer = the Packed* layer that reads this layer's output: returns the (packed, des) pair of ITS activation quantiser
        of act(y) (act None or "gelu"), written by this layer's kernel itself where it can (qe_quantlinear_requant):
        bit-identical to consumer.quantize(act(self.call_packed(xq, x_des))) with act applied in fp32 as F.gelu does.
        status: a device int32 the range flag accumulates in; nothing is read back or copied, des comes back as host
        integers.  None: raise when the codes are out of range."""
        n_bits, sign, *lead, K = _host_des(x_des)
        B, O = 1, self.O
        for v in lead:
            B *= v
        if self.a_scale.numel() != 1:
            raise ValueError("quantlinear takes a per-tensor or per-row activation scale")
        x, w = self.xq(xq, n_bits, sign), self.wq()
        if consumer is None:
            if act is not None:
                raise ValueError("act applies to the consumer's codes; the fp32 output is y itself")
            if residual is None:
                return capi.quantlinear(x, w, self.bias, B, K, O)
            return capi.quantlinear_residual(x, w, self.bias, B, K, O, residual.contiguous().reshape(B, O))
        if residual is not None:
            raise ValueError("residual and consumer are exclusive")
        codes, flag = capi.quantlinear_requant(x, w, self.bias, B, K, O, consumer.requant(), act=act, status=status)
        if status is None and int(flag.item()) != 0:
            raise RuntimeError(OUT_OF_RANGE)
        des = (consumer.a_bits, int(consumer.a_signed), B, O)
        return codes, (des if status is not None else torch.tensor(des, dtype=torch.int32, device=xq.device))


class PackedMultiheadAttention:
    """A packed QuantMultiheadAttention's forward on the engine (modelzoo/modules/quantmultiheadattention.py:262-...).
    pack() leaves the q / k / v projection weights and out_proj.weight as packed streams with {q,k,v,out}_proj_{scale,
    zero,des} beside them and one activation quantiser per input (:165-223); the reference's packed forward dequantises
    all four and calls F.multi_head_attention_forward.  Here the three input projections run as packed linears (either
    route of PackedLinear, each with its own activation quantiser and its slice of in_proj_bias), the attention core
    softmax(Q K^T / sqrt(d) + masks) V stays fp32 as in the reference (torch, or the engine core), and out_proj -- whose input has no quantiser in the
    reference -- takes the fp32 x packed-weight operator (quantlinear_float_input).  Inputs are (L, N, E) / (S, N, kdim)
    (batch_first=False, the module's default); returns (attn_output, averaged attention weights or None)."""

    def __init__(self, q, k, v, out_weight, out_des, out_scale, out_zero, out_bias, num_heads):
        self.q, self.k, self.v = q, k, v
        self.out_weight, self.out_des, self.out_bias = out_weight, out_des, out_bias
        self.out_scale = out_scale.reshape(-1).contiguous()
        self._neg_out_zero = (-out_zero).reshape(-1).contiguous()          # kernel convention of the float-input operator
        self.num_heads = int(num_heads)

    @functools.cached_property
    def _out_bits_sign(self):
        """out_des's n_bits and sign as host integers: read once, by from_state_dict or else on first use."""
        return tuple(int(v) for v in self.out_des.tolist()[:2])

    def out_wq(self):
        """out_proj's packed weights as a capi.qparam for the float-input quantlinear: (q - zero)."""
        return capi.qparam(self.out_weight, *self._out_bits_sign, self.out_scale, self._neg_out_zero)

    @classmethod
    def from_state_dict(cls, sd, prefix="", num_heads=1):
        embed = int(sd[prefix + "q_proj_des"][2])
        bias = sd.get(prefix + "in_proj_bias")

        def proj(name, i):
            qmin, qmax = float(sd[prefix + name + "_quantizer.qmin"]), float(sd[prefix + name + "_quantizer.qmax"])
            a_bits, a_signed = quantizer_bits(qmin, qmax)
            return PackedLinear(weight=sd[prefix + name + "_proj_weight"], w_des=sd[prefix + name + "_proj_des"],
                                w_scale=sd[prefix + name + "_proj_scale"], w_zero=sd[prefix + name + "_proj_zero"],
                                bias=None if bias is None else bias[i * embed:(i + 1) * embed].contiguous(),
                                a_scale=sd[prefix + name + "_quantizer.scale"], a_zero=sd[prefix + name + "_quantizer.zero"],
                                a_qmin=qmin, a_qmax=qmax, a_bits=a_bits, a_signed=a_signed, name=prefix + name)
        mha = cls(proj("q", 0), proj("k", 1), proj("v", 2), sd[prefix + "out_proj.weight"], sd[prefix + "out_proj_des"],
                  sd[prefix + "out_proj_scale"], sd[prefix + "out_proj_zero"], sd.get(prefix + "out_proj.bias"), num_heads)
        mha._out_bits_sign       # parsed here, where the state_dict tensors normally still live on the host
        return mha

    def to(self, device):
        for p in (self.q, self.k, self.v):
            p.to(device)
        for name, val in list(vars(self).items()):
            if torch.is_tensor(val):
                setattr(self, name, val.to(device))
        return self

    @staticmethod
    def _additive_masks(attn_mask, key_padding_mask, N, H, L, S):
        """nn.MultiheadAttention's mask arguments, validated, as additive fp32: attn_mask (L, S) or (N*H, L, S),
        key_padding_mask (N, S); bool True = masked -> -inf, float as given."""
        if key_padding_mask is not None:
            if key_padding_mask.dtype != torch.bool and not torch.is_floating_point(key_padding_mask):
                raise AssertionError("only bool and floating types of key_padding_mask are supported")
            if tuple(key_padding_mask.shape) != (N, S):
                raise ValueError("key_padding_mask must be (N, S) = %s; got %s" % ((N, S), tuple(key_padding_mask.shape)))
        if attn_mask is not None:
            if attn_mask.dtype != torch.bool and not torch.is_floating_point(attn_mask):
                raise ValueError("only bool and floating types of attn_mask are supported")
            if tuple(attn_mask.shape) not in ((L, S), (N * H, L, S)):
                raise ValueError("attn_mask must be (L, S) = %s or (N*H, L, S) = %s; got %s"
                                 % ((L, S), (N * H, L, S), tuple(attn_mask.shape)))

        def additive(m):
            if m is None:
                return None
            if m.dtype == torch.bool:
                return torch.zeros(m.shape, dtype=torch.float32, device=m.device).masked_fill_(m, float("-inf"))
            return m.to(torch.float32).contiguous()
        return additive(attn_mask), additive(key_padding_mask)

    def __call__(self, query, key, value, route="packed", need_weights=True, attention="torch", attn_mask=None,
                 key_padding_mask=None, is_causal=False):
        """attention="torch": the core as torch bmm / softmax / bmm (the reference's own arithmetic).  "engine": the fp32
        qe_attention kernel reads the three projections in their (L N, E) / (S N, E) layout and writes the context in
        place for out_proj -- no score matrix, so need_weights must be False.  "engine_bf16": the same through
        qe_attention_bf16 (both products on the bf16 matrix cores; head sizes d % 16 == 0, d <= 128 only, no fallback).
        attn_mask ((L, S) or (N*H, L, S)) and key_padding_mask ((N, S)) follow nn.MultiheadAttention: bool (True = not
        allowed / ignored key) or float (added to the scores).  is_causal=True without attn_mask is the top-left aligned
        tril mask.  The engine core takes attn_mask with its broadcast strides and key_padding_mask as a key bias row:
        no merged (N, H, L, S) tensor.  A row with no visible key is NaN in both cores."""
        if attention not in ("torch", "engine", "engine_bf16"):
            raise ValueError("attention must be 'torch', 'engine' or 'engine_bf16'")
        L, N, E = query.shape
        S = key.shape[0]
        H, d = self.num_heads, E // self.num_heads
        masked = attn_mask is not None or key_padding_mask is not None or is_causal
        if masked:
            attn_mask, key_padding_mask = self._additive_masks(attn_mask, key_padding_mask, N, H, L, S)
        if attention != "torch":
            if need_weights:
                raise ValueError("attention='%s' materialises no attention weights: pass need_weights=False" % attention)
            precision = "bf16" if attention == "engine_bf16" else "fp32"
            if precision == "bf16" and capi.attention_bf16_path(L, S, H, d) < 0:
                raise ValueError("attention='engine_bf16' takes head sizes d %% 16 == 0, d <= 128; got d = %d" % d)
            Q, K, V = (p(x, route).reshape(-1, E).contiguous() for p, x in ((self.q, query), (self.k, key), (self.v, value)))
            if masked:
                ctx = capi.attention(Q, K, V, N, L, H, S=S, layout="seq", mask=attn_mask, key_bias=key_padding_mask,
                                     causal=bool(is_causal) and attn_mask is None, precision=precision)
            else:
                ctx = capi.attention(Q, K, V, N, L, H, S=S, layout="seq", precision=precision)
            out = quantlinear_forward(ctx, (self.out_weight, self.out_des, self.out_scale, self._neg_out_zero), self.out_bias)
            return out.reshape(L, N, E), None
        Q = self.q(query, route).reshape(L, N * H, d).transpose(0, 1)      # (N H, L, d), as F.multi_head_attention_forward splits heads
        K = self.k(key, route).reshape(S, N * H, d).transpose(0, 1)
        V = self.v(value, route).reshape(S, N * H, d).transpose(0, 1)
        if masked:
            scores = torch.bmm(Q * (float(d) ** -0.5), K.transpose(1, 2))
            if attn_mask is None and is_causal:
                attn_mask = torch.zeros(L, S, dtype=torch.float32, device=scores.device).masked_fill_(
                    torch.ones(L, S, dtype=torch.bool, device=scores.device).tril().logical_not(), float("-inf"))
            if attn_mask is not None:
                scores = scores + attn_mask
            if key_padding_mask is not None:
                scores = (scores.view(N, H, L, S) + key_padding_mask.view(N, 1, 1, S)).view(N * H, L, S)
            attn = torch.softmax(scores, dim=-1)
        else:
            attn = torch.softmax(torch.bmm(Q * (float(d) ** -0.5), K.transpose(1, 2)), dim=-1)
        ctx = torch.bmm(attn, V).transpose(0, 1).reshape(L * N, E).contiguous()
        out = quantlinear_forward(ctx, (self.out_weight, self.out_des, self.out_scale, self._neg_out_zero), self.out_bias)
        return out.reshape(L, N, E), (attn.reshape(N, H, L, S).mean(dim=1) if need_weights else None)


class _PackedQuantLayer:
    """A packed layer that owns nothing but its activation quantiser (QuantReLU, the quantised pools): pack() leaves
    a_quantizer.{scale, zero, qmin, qmax} in the state_dict and no weight.  The quantiser reaches the engine in the module's
    convention (capi.requant) for the fp32 forwards and as the (q - zero') operand of a code stream for call_packed."""

    def __init__(self, a_scale, a_zero, a_qmin, a_qmax, name=None):
        self.name = name
        self.a_qmin, self.a_qmax = float(a_qmin), float(a_qmax)
        self.a_bits, self.a_signed = quantizer_bits(a_qmin, a_qmax)
        self._a_scale = a_scale.reshape(-1).contiguous().float()
        self._a_zero = a_zero.reshape(-1).contiguous().float()
        self._neg_a_zero = (-self._a_zero).contiguous()

    a_scale = property(lambda self: self._a_scale)
    a_zero = property(lambda self: self._a_zero)

    @classmethod
    def _state(cls, sd, prefix):
        g = lambda k: sd[prefix + "a_quantizer." + k]
        return dict(a_scale=g("scale"), a_zero=g("zero"), a_qmin=float(g("qmin")), a_qmax=float(g("qmax")), name=prefix.rstrip("."))

    def to(self, device):
        for k, v in list(vars(self).items()):
            if torch.is_tensor(v):
                setattr(self, k, v.to(device))
        return self

    def requant(self):
        """This layer's quantiser as a capi.requant: the operand of its own fp32 forward, or of a producer's epilogue."""
        return capi.requant(self._a_scale, self._a_zero, self.a_qmin, self.a_qmax, self.a_bits, self.a_signed)

    def _check(self, x):
        if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32):
            raise ValueError("%s takes an fp32 CUDA tensor" % type(self).__name__)
        if self._a_scale.numel() not in (1, x.shape[1]):
            raise ValueError("%s: %d scales for %d channels" % (self.name or "layer", self._a_scale.numel(), x.shape[1]))
        return x.contiguous()


class PackedReLU(_PackedQuantLayer):
    """A packed QuantReLU's forward (quantrelu.py:81-86) in one kernel: relu((q + zero) * scale), q the layer's codes of x."""

    def __init__(self, *, inplace=False, **state):
        super().__init__(**state)
        self.inplace = bool(inplace)

    @classmethod
    def from_state_dict(cls, state_dict, prefix="", inplace=False):
        return cls(inplace=inplace, **cls._state(state_dict, prefix))

    def __call__(self, x):
        xc = self._check(x)
        return capi.quant_relu(xc, self.requant(), out=xc if self.inplace and xc is x else None)


class PackedMaxPool2d(_PackedQuantLayer):
    """A packed QuantMaxPool2d's forward (quant_pooling.py:90-97) in one kernel.  Square kernel / stride / padding, dilation 1,
    floor mode, no indices: a layer with anything else is refused here (QeError, unsupported) and nothing runs in its place."""

    def __init__(self, *, kernel_size, stride=None, padding=0, dilation=1, return_indices=False, ceil_mode=False, **state):
        super().__init__(**state)
        for v in (kernel_size, stride, padding, dilation):
            if isinstance(v, (tuple, list)) and len(set(v)) != 1:
                capi.check(capi.QE_ERR_UNSUPPORTED)
        self.kernel = _first(kernel_size)
        self.stride = self.kernel if stride is None else _first(stride)
        self.padding = _first(padding)
        if _first(dilation) != 1 or return_indices or ceil_mode:
            capi.check(capi.QE_ERR_UNSUPPORTED)

    @classmethod
    def from_state_dict(cls, state_dict, prefix="", kernel_size=None, stride=None, padding=0, **kw):
        if kernel_size is None:
            raise ValueError("PackedMaxPool2d.from_state_dict: kernel_size is required (a state_dict holds no geometry)")
        return cls(kernel_size=kernel_size, stride=stride, padding=padding, **kw, **cls._state(state_dict, prefix))

    def __call__(self, x):
        return capi.quant_maxpool2d(self._check(x), self.requant(), self.kernel, self.stride, self.padding)


class _PackedAvgPoolBase(_PackedQuantLayer):
    """call_packed of the two average pools: codes of this layer's quantiser in, through qe_avgpool2d_codes."""

    def _window(self, H, W):
        raise NotImplementedError          # (kernel, stride, output_size) of the codes-domain call

    def call_packed(self, xq, x_des, consumer=None, relu=False, status=None):
        """Activations as (packed stream, des) of THIS layer's quantiser -- what a producer's call_packed(consumer=this layer)
        returned.  consumer=None: the fp32 window means (of max(q - zero', 0) per tap when relu: the producer's codes are
        pre-ReLU).  consumer = the Packed* layer that reads them: the (packed, des) pair of ITS quantiser from this call's own
        epilogue, bit-identical to consumer.quantize(fp32 output).  status as PackedDepthwiseConv2d.call_packed."""
        n_bits, sign, N, C, H, W = _host_des(x_des)
        if self._a_scale.numel() not in (1, C):
            raise ValueError("%s: %d scales for codes of %d channels" % (self.name or "layer", self._a_scale.numel(), C))
        kernel, stride, osize = self._window(H, W)
        x = capi.qparam(xq, n_bits, sign, self._a_scale, self._neg_a_zero)
        if consumer is None:
            return capi.avgpool2d_codes(x, N, C, H, W, kernel, stride, osize, relu=relu)[0]
        _, codes, flag = capi.avgpool2d_codes(x, N, C, H, W, kernel, stride, osize, relu=relu, rq=consumer.requant(), out=None,
                                              status=status)
        if status is None and int(flag.item()) != 0:
            raise RuntimeError(OUT_OF_RANGE)
        des = (consumer.a_bits, int(consumer.a_signed), N, C, *capi.avgpool2d_out_hw(H, W, kernel, stride, osize))
        return codes, (des if status is not None else torch.tensor(des, dtype=torch.int32, device=xq.device))


class PackedAdaptiveAvgPool2d(_PackedAvgPoolBase):
    """A packed QuantAdaptiveAvgPool2d's forward (quant_pooling.py:159-165) in one kernel: the mean of (q + zero) * scale over
    torch's adaptive windows, added up in the fixed order include/quant_engine.h states (not torch's bit pattern)."""

    def __init__(self, *, output_size, **state):
        super().__init__(**state)
        self.output_size = (output_size, output_size) if isinstance(output_size, int) else tuple(output_size)

    @classmethod
    def from_state_dict(cls, state_dict, prefix="", output_size=None):
        if output_size is None:
            raise ValueError("PackedAdaptiveAvgPool2d.from_state_dict: output_size is required (a state_dict holds no geometry)")
        return cls(output_size=output_size, **cls._state(state_dict, prefix))

    def _size(self, H, W):
        return (H if self.output_size[0] is None else int(self.output_size[0]), W if self.output_size[1] is None else int(self.output_size[1]))

    def _window(self, H, W):
        return 0, 1, self._size(H, W)

    def __call__(self, x):
        xc = self._check(x)
        return capi.quant_adaptive_avgpool2d(xc, self.requant(), self._size(*xc.shape[2:]))


class PackedAvgPool2d(_PackedAvgPoolBase):
    """nn.AvgPool2d(kernel_size, stride) (no padding, floor mode) behind a quantiser: what stands between two quantised layers
    of CLIP's ModifiedResNet and at the end of wrn_40_2.  call_packed runs any kernel / stride on codes.  The fp32 forward is the
    adaptive module kernel, whose windows are these exactly when stride == kernel divides H and W; other geometries have no fp32
    kernel and raise ValueError (nothing runs in its place)."""

    def __init__(self, *, kernel_size, stride=None, **state):
        super().__init__(**state)
        self.kernel = _first(kernel_size)
        self.stride = self.kernel if stride is None else _first(stride)

    @classmethod
    def from_state_dict(cls, state_dict, prefix="", kernel_size=None, stride=None):
        if kernel_size is None:
            raise ValueError("PackedAvgPool2d.from_state_dict: kernel_size is required (a state_dict holds no geometry)")
        return cls(kernel_size=kernel_size, stride=stride, **cls._state(state_dict, prefix))

    def _window(self, H, W):
        return self.kernel, self.stride, None

    def __call__(self, x):
        xc = self._check(x)
        H, W = xc.shape[2:]
        if self.stride != self.kernel or H % self.kernel or W % self.kernel:
            raise ValueError("PackedAvgPool2d: the fp32 forward takes stride == kernel_size dividing H and W; got kernel %d, stride %d "
                             "on %d x %d (call_packed takes any)" % (self.kernel, self.stride, H, W))
        return capi.quant_adaptive_avgpool2d(xc, self.requant(), (H // self.kernel, W // self.kernel))


POOL_KINDS = {"relu": (PackedReLU, ("inplace",)), "maxpool": (PackedMaxPool2d, ("kernel_size", "stride", "padding")),
              "adaptive_avgpool": (PackedAdaptiveAvgPool2d, ("output_size",))}


def from_state_dict(state_dict, conv_geometry=None, num_heads=None, pool_geometry=None):
    """Every packed layer of a model's state_dict -> {module prefix (no trailing dot): PackedConv2d | PackedLinear |
    PackedMultiheadAttention}: what the packing loop of runner/ptq.py:106-114 / runner/qat.py:84-92 leaves behind, ready to
    run on the engine with no reference Python in the process.  A packed conv / linear is recognised by its `w_des` entry
    (6 fields = conv: n_bits, sign, OC, IC, KH, KW; 4 = linear), an attention block by `q_proj_des`.
    conv_geometry: {prefix: (stride, padding)} -- geometry is not part of the state_dict; default stride 1, padding
    (KH - 1) // 2 ("same" for odd kernels).  num_heads: {prefix: heads} (or one int for every attention block).
    pool_geometry: {prefix: ("relu"[, inplace]) | ("maxpool", kernel_size[, stride[, padding]]) | ("adaptive_avgpool",
    output_size)} -- a packed QuantReLU / QuantMaxPool2d / QuantAdaptiveAvgPool2d leaves only its a_quantizer entries behind,
    which do not say what the layer is: the map names each one -> PackedReLU | PackedMaxPool2d | PackedAdaptiveAvgPool2d."""
    conv_geometry = conv_geometry or {}
    layers = {}
    for name, (kind, *args) in (pool_geometry or {}).items():
        if kind not in POOL_KINDS:
            raise ValueError("%s: pool_geometry kind %r is none of %s" % (name, kind, sorted(POOL_KINDS)))
        cls, names = POOL_KINDS[kind]
        if len(args) > len(names):
            raise ValueError("%s: %r takes at most %s" % (name, kind, names))
        layers[name] = cls.from_state_dict(state_dict, name + "." if name else "", **dict(zip(names, args)))
    for key in state_dict:
        if key.endswith("w_des"):
            prefix = key[:-len("w_des")]
            name = prefix[:-1] if prefix.endswith(".") else prefix
            des = state_dict[key]
            if des.numel() == 6:
                kh = int(des[4])
                stride, padding = conv_geometry.get(name, (1, (kh - 1) // 2))
                layers[name] = PackedConv2d.from_state_dict(state_dict, prefix, stride=stride, padding=padding)
            elif des.numel() == 4:
                layers[name] = PackedLinear.from_state_dict(state_dict, prefix)
            else:
                raise ValueError("%s: a description of %d fields is neither a conv (6) nor a linear (4)" % (key, des.numel()))
        elif key.endswith("q_proj_des"):
            prefix = key[:-len("q_proj_des")]
            name = prefix[:-1] if prefix.endswith(".") else prefix
            heads = num_heads.get(name) if isinstance(num_heads, dict) else num_heads
            if heads is None:
                raise ValueError("%s: num_heads is not part of a state_dict; pass num_heads" % name)
            layers[name] = PackedMultiheadAttention.from_state_dict(state_dict, prefix, heads)
    return layers
