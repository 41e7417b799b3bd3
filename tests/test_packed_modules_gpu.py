"""GPU: the module wiring shim (quantize_amd/packed.py) on the captured runs of the
reference's own modules (tests/golden/g4_module.npz, g6_linear_module.npz: QuantConv2d / QuantLinear calibrated, packed,
reloaded and run through their packed forward).  From the raw fp32 input and the packed state alone -- no reference code
here -- both operator routes must reproduce the reference module's output, and the on-device quantisation must reproduce
the module's integer activations bit for bit."""
import numpy as np
import pytest
import torch

from quantize_amd.packed import PackedConv2d, PackedLinear

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _state(g, key):
    """The state_dict entries pack() leaves behind, as the reference names them."""
    qmin, qmax = [float(v) for v in g.get(key, "a_qmin_qmax")]
    return {"weight": _t(g.get(key, "weight_packed")), "w_des": _t(g.get(key, "w_des")), "w_scale": _t(g.get(key, "w_scale")),
            "w_zero": _t(g.get(key, "w_zero_py")), "bias": _t(g.get(key, "bias")),
            "a_quantizer.scale": _t(g.get(key, "a_scale")), "a_quantizer.zero": _t(g.get(key, "a_zero_py")),
            "a_quantizer.qmin": torch.tensor(qmin), "a_quantizer.qmax": torch.tensor(qmax)}


def test_packed_conv2d_on_reference_captures(g4):
    import quantize_amd.engine as engine
    for key in g4.index:
        stride, pad = [int(v) for v in g4.get(key, "stride_pad")]
        m = PackedConv2d.from_state_dict(_state(g4, key), stride=(stride, stride), padding=(pad, pad))
        a_bits, a_sign = [int(v) for v in g4.get(key, "a_bits_sign")]
        assert m.a_bits == a_bits and (m.a_signed or not a_sign)
        x = _t(g4.get(key, "x"))
        ref = g4.get(key, "y_packed")
        tol = 2e-5 * max(1.0, float(np.abs(ref).max()))
        # the device-side Quantizer + packer reproduces the module's integer activations exactly
        xq, x_des = m.quantize(x)
        q = engine.tunpack(xq, x_des).cpu().numpy().astype(np.float32)
        assert np.array_equal(q, g4.get(key, "qx")), key
        for route in ("packed", "float"):
            y = m(x, route=route)
            assert y.dtype == torch.float32 and tuple(y.shape) == ref.shape
            assert np.abs(y.cpu().numpy() - ref).max() <= tol, (key, route)
    with pytest.raises(ValueError):
        m(x, route="other")


def test_packed_linear_on_reference_captures(g6):
    import quantize_amd.engine as engine
    for key in g6.index:
        m = PackedLinear.from_state_dict(_state(g6, key))
        x = _t(g6.get(key, "x"))
        ref = g6.get(key, "y_packed")
        tol = 2e-5 * max(1.0, float(np.abs(ref).max()))
        xq, x_des = m.quantize(x, channel_dim=1)
        assert np.array_equal(engine.tunpack(xq, x_des).cpu().numpy().astype(np.float32), g6.get(key, "qx")), key
        for route in ("packed", "float"):
            y = m(x, route=route)
            assert np.abs(y.cpu().numpy() - ref).max() <= tol, (key, route)
        # leading dimensions (tokens) are flattened and restored
        y3 = m(x.reshape(3, 4, -1), route="packed")
        assert tuple(y3.shape) == (3, 4, ref.shape[1]) and np.abs(y3.reshape(12, -1).cpu().numpy() - ref).max() <= tol


def _synthetic_state(rng, IC, OC, K, a_signed):
    """A packed QuantConv2d's state_dict entries (quantconv2d.py:187-192) with random codes and per-channel weight scales."""
    import quantize_amd.engine as engine
    qw = torch.from_numpy(rng.randint(-128, 128, size=(OC, IC, K, K)).astype(np.int8)).to(DEV)
    wp, wd = engine.tpack(qw, 8, True)
    qmin, qmax = (-128.0, 127.0) if a_signed else (0.0, 255.0)
    return {"weight": wp, "w_des": wd, "w_scale": _t(rng.uniform(1e-3, 3e-3, size=(OC, 1, 1, 1)).astype(np.float32)),
            "w_zero": _t(np.zeros((OC, 1, 1, 1), np.float32)), "bias": _t(rng.normal(0, 0.1, size=OC).astype(np.float32)),
            "a_quantizer.scale": _t(np.array([0.02 if a_signed else 0.011], np.float32)),
            "a_quantizer.zero": _t(np.array([0.0], np.float32)),
            "a_quantizer.qmin": torch.tensor(qmin), "a_quantizer.qmax": torch.tensor(qmax)}


def test_packed_layers_chain_without_fp32_in_between():
    """Three packed convs chained: each layer's conv kernel writes the NEXT layer's activation codes (fused
    re-quantisation) -- same final output, bit for bit, as quantising every fp32 intermediate with the consumer's
    quantizer (quantize_pack), which test_packed_conv2d_on_reference_captures pins to the reference module."""
    rng = np.random.RandomState(11)
    a = PackedConv2d.from_state_dict(_synthetic_state(rng, 64, 128, 1, True), stride=1, padding=0)
    b = PackedConv2d.from_state_dict(_synthetic_state(rng, 128, 128, 3, False), stride=1, padding=1)    # unsigned: ReLU folded
    c = PackedConv2d.from_state_dict(_synthetic_state(rng, 128, 256, 1, True), stride=2, padding=0)
    # the consumers' scales must suit what arrives: calibrate them from one fp32 pass
    x = torch.randn(4, 64, 28, 28, device=DEV)
    xq, xd = a.quantize(x)
    ya = a.call_packed(xq, xd)
    b.a_scale = (ya.clamp(min=0).max() / 255.0).reshape(1)
    yb = b.call_packed(*b.quantize(ya))
    c.a_scale = (yb.abs().max() / 127.0).reshape(1)
    ref = c.call_packed(*c.quantize(yb))
    # fused chain
    qb, db = a.call_packed(xq, xd, consumer=b)
    qb_ref, db_ref = b.quantize(ya)
    assert torch.equal(qb, qb_ref) and torch.equal(db.cpu(), db_ref.cpu())
    qc, dc = b.call_packed(qb, db, consumer=c)
    out = c.call_packed(qc, dc)
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    assert tuple(out.shape) == (4, 256, 14, 14)
    # the same chain with a caller's status tensor: the same codes, nothing read back, no host synchronisation
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    xq2, xd2 = a.quantize_codes(x, flag)
    torch.cuda.set_sync_debug_mode("error")
    try:
        qb2, db2 = a.call_packed(xq2, xd2, consumer=b, status=flag)
        qc2, dc2 = b.call_packed(qb2, db2, consumer=c, status=flag)
        out2 = c.call_packed(qc2, dc2, status=flag)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(qb2, qb) and list(db2) == db.tolist() and torch.equal(out2, out) and int(flag.item()) == 0


def test_resnet_bottleneck_chained_through_call_packed():
    """A whole ResNet bottleneck (1x1 -> 3x3 -> 1x1, ReLU after the first two, + identity, ReLU) built from a state_dict
    by packed.from_state_dict and run two ways: (a) layer by layer through the operator route -- every fp32 intermediate
    is ReLU'd, then quantised and packed by the next layer (what the reference's dataflow does with the engine plugged
    in); (b) chained through call_packed -- each conv kernel writes the codes of the NEXT layer's activation quantiser,
    the ReLUs folded into the clamp of the unsigned consumers (no fp32 tensor between the convs).  Same block output, bit
    for bit."""
    from quantize_amd.packed import from_state_dict
    rng = np.random.RandomState(29)
    sd = {}
    for name, (ic, oc, k, signed) in {"layer2.1.conv1": (256, 64, 1, True), "layer2.1.conv2": (64, 64, 3, False),
                                      "layer2.1.conv3": (64, 256, 1, False)}.items():
        for kk, vv in _synthetic_state(rng, ic, oc, k, signed).items():
            sd[name + "." + kk] = vv
    layers = from_state_dict(sd, conv_geometry={"layer2.1.conv1": (1, 0), "layer2.1.conv2": (1, 1), "layer2.1.conv3": (1, 0)})
    c1, c2, c3 = (layers["layer2.1.conv" + str(i)] for i in (1, 2, 3))
    x = torch.randn(8, 256, 28, 28, device=DEV)
    # calibrate the two unsigned (post-ReLU) quantisers from one fp32 pass, as a PTQ run would
    y1 = torch.relu(c1(x))
    c2.a_scale = (y1.max() / 255.0).reshape(1)
    y2 = torch.relu(c2(y1))
    c3.a_scale = (y2.max() / 255.0).reshape(1)
    # (a) layer by layer
    ref = torch.relu(c3(torch.relu(c2(torch.relu(c1(x))))) + x)
    # (b) chained: quantise once, codes from epilogue to epilogue
    xq, xd = c1.quantize(x)
    q2, d2 = c1.call_packed(xq, xd, consumer=c2)
    q3, d3 = c2.call_packed(q2, d2, consumer=c3)
    out = torch.relu(c3.call_packed(q3, d3) + x)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (8, 256, 28, 28)
    assert torch.equal(out, ref)


def test_packed_multihead_attention_on_reference_captures(g7):
    """PackedMultiheadAttention on the captured runs of the reference's QuantMultiheadAttention (calibrate -> pack() ->
    state_dict -> reload -> packed forward; separate projection weights, the only form the reference's pack() supports):
    from the raw fp32 query / key / value and the packed state alone, both routes reproduce the module's output and its
    averaged attention weights (2e-5 abs on O(1) values: three integer-exact projections, an fp32 softmax, one more
    projection)."""
    from quantize_amd.packed import from_state_dict
    for key in g7.index:
        pre = key + "_sd_"
        sd = {f[len(pre):]: _t(g7._z[f]) for f in g7._z.files if f.startswith(pre)}
        E, H, KD = [int(v) for v in g7.get(key, "heads")]
        mha = from_state_dict({"attn." + k: v for k, v in sd.items()}, num_heads=H)["attn"]
        q, k, v = _t(g7.get(key, "query")), _t(g7.get(key, "key")), _t(g7.get(key, "value"))
        ref, ref_attn = g7.get(key, "y_packed"), g7.get(key, "attn")
        for route in ("packed", "float"):
            y, attn = mha(q, k, v, route=route)
            assert tuple(y.shape) == ref.shape and tuple(attn.shape) == ref_attn.shape
            assert np.abs(y.cpu().numpy() - ref).max() <= 2e-5, (key, route, float(np.abs(y.cpu().numpy() - ref).max()))
            assert np.abs(attn.cpu().numpy() - ref_attn).max() <= 2e-5, (key, route)
