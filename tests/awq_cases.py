"""What the tests of the group-quantised (AWQ layout) int8 entry points share: the generator of packed code streams, the random
operands of a grouped linear, and the decoding of a case dict's streams and (row, group) parameters for the float64 references
(tests/linear_grouped_codes_ref.py, tests/awq_conv_ref.py).  A plain helper module."""
import numpy as np

from quantize_amd.synthetic import pack_codes

from linear_grouped_ref import decode


def codes(rng, shape, bits, sym, mean):
    """(stream, signed, centre): a symmetric operand has signed codes (centre 0), an asymmetric one unsigned codes (centre
    2^(bits-1)); `mean` shifts the centred codes (a non-zero mean: the cancellation regime of the zero-point terms)."""
    half = 1 << (bits - 1)
    q = np.clip(np.rint(rng.randn(*shape) * half / 3 + mean), -half, half - 1).astype(np.int64) + (0 if sym else half)
    return pack_codes(q, bits, sym), sym, 0 if sym else half


def linear_case(seed, w_bits, G, K, B, O, wsym, xsym, per_row, x_bits=8):
    """Random operands of qe_quantlinear_grouped.  Symmetric: zeros at the stream's centre; asymmetric: the centre plus a
    fraction in (-0.5, 0.5)."""
    rng = np.random.RandomState(seed)
    NG, n_x = K // G, B if per_row else 1
    c = dict(w_bits=w_bits, x_bits=x_bits, G=G, K=K, B=B, O=O, wsym=wsym, xsym=xsym)
    c["x_stream"], c["x_signed"], cx = codes(rng, (B, K), x_bits, xsym, (1 << x_bits) / 8)
    c["w_stream"], c["w_signed"], cw = codes(rng, (O, K), w_bits, wsym, 0)
    c["sx"] = (rng.uniform(0.5, 1.5, size=n_x) * 2.0 ** (5 - x_bits)).astype(np.float32)
    c["zx"] = (cx + (0 if xsym else 1) * rng.uniform(-0.5, 0.5, size=n_x)).astype(np.float32)
    c["sw"] = (rng.uniform(0.5, 1.5, size=O * NG) * 2.0 ** (4 - w_bits) / np.sqrt(K)).astype(np.float32)
    c["zw"] = (cw + (0 if wsym else 1) * rng.uniform(-0.5, 0.5, size=O * NG)).astype(np.float32)
    c["bias"] = rng.randn(O).astype(np.float32)
    return c


def decoded(c, x_shape, w_shape, groups):
    """Of a case dict, in float64: the decoded codes qx (x_shape) and qw (w_shape; its first axis is the output row), and the
    weight parameters sw / zw as (rows, groups)."""
    qx = decode(c["x_stream"], int(np.prod(x_shape)), c["x_bits"], c["x_signed"]).reshape(x_shape).astype(np.float64)
    qw = decode(c["w_stream"], int(np.prod(w_shape)), c["w_bits"], c["w_signed"]).reshape(w_shape).astype(np.float64)
    sw, zw = (np.asarray(c[k], np.float64).reshape(w_shape[0], groups) for k in ("sw", "zw"))
    return qx, qw, sw, zw
