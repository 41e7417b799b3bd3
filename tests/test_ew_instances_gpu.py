"""GPU: every instance of the pack / unpack / quantise kernels of qe_tpack.hip at its edges against tests/ew_ref.py (numpy,
independent of the engine and of the C oracle), bit for bit.

The contract each case is held to:
  * the codes are the fp32 operation sequence of ew_ref.quantise -- division, subtraction, round-half-even, clamp -- on
    inputs dense in `.5` ties of x / scale - zero (tests/test_ew_instances_cpu.py measures that those inputs tell the sequence
    from a reciprocal multiply and from float64 arithmetic), packed LSB first with zero padding in the last byte;
  * every output lies inside a buffer prefilled with 0xA5 (ew_instances.Guarded): the bytes round it are unchanged and every
    byte of it was written;
  * one out-of-range element anywhere -- element 0, the ragged tail, a tile's last element, lane 63, an unaligned run -- raises
    the flag and changes no other element's code; clean input leaves the flag 0.
The cases and the instance each reaches are the tables of tests/ew_instances.py."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ew_instances as ei
import ew_ref
from quantize_amd import capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAIR_IDS = ["b%d_%s" % (b, "s" if s else "u") for b, s in ei.PAIRS]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _status():
    return torch.zeros(1, dtype=torch.int32, device=DEV)


# ---- tpack / tunpack -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tpack_ref(bits, sign, n, lo, hi):
    """n integers over [lo, hi] with both ends present, and their reference stream (shared by the element types)."""
    rng = np.random.RandomState(1000 * bits + 100 * int(sign) + n % 97)
    q = rng.randint(lo, hi + 1, size=n)
    q[-1], q[0] = hi, lo
    q.setflags(write=False)
    packed = ew_ref.pack(ew_ref.stored(q, bits, sign), bits)
    packed.setflags(write=False)
    return q, packed


def _tpack_input(q, dtype, lo, hi):
    """The integers in the element type; float types carry a fraction toward zero's far side (the packer truncates) wherever
    the value stays inside the range test."""
    if dtype.startswith("float"):
        frac = np.where((q >= 0) & (q < hi), 0.25, np.where((q < 0) & (q > lo), -0.25, 0.0))
        return (q + frac).astype(dtype)
    return q.astype(dtype)


@pytest.mark.parametrize("dtype", ei.DTYPES)
def test_tpack_every_width_size_and_alignment(dtype):
    st = _status()
    for bits, sign in ei.PAIRS:
        lo, hi = ei.tpack_values(dtype, bits, sign)
        variants = ei.F32_CROSS if (dtype == "float32" and bits in ei.F32_CROSS_BITS) else ei.TPACK_VARIANTS
        for n in ei.NS:
            q, want = _tpack_ref(bits, sign, n, lo, hi)
            xv = _tpack_input(q, dtype, lo, hi)
            for in_off, out_off in variants:
                in_off = ei.in_offset(dtype) if in_off is None else in_off
                x = ei.device_input(xv, dtype, in_off)
                g = ei.Guarded(want.size, out_off)
                assert capi.packed_nbytes(n, bits) == want.size
                capi.tpack(x, bits, sign, out=g.out, status=st)
                what = "tpack %s b%d sign %d n %d, x + %d elements, out + %d bytes" % (dtype, bits, sign, n, in_off, out_off)
                got = g.result(what)
                assert np.array_equal(got, want), what
    assert int(st.item()) == 0


@pytest.mark.parametrize("bits,sign", ei.PAIRS, ids=PAIR_IDS)
def test_tunpack_every_size_and_alignment(bits, sign):
    """Against ew_ref.unpack of a reference stream: no round trip through the packer under test."""
    lo, hi = ew_ref.qrange(bits, sign)
    variants = ei.F32_CROSS if bits in ei.F32_CROSS_BITS else ((0, 0), (3, 0), (0, ei.OUT_OFFSET))
    for n in ei.NS:
        q, packed = _tpack_ref(bits, sign, n, lo, hi)
        want = ew_ref.unpack(packed, n, bits, sign)
        assert np.array_equal(want.astype(np.int64), q)
        for in_off, out_off in variants:
            src = ei.device_input(packed, "uint8", in_off)
            g = ei.Guarded(n, out_off)
            capi.tunpack(src, n, bits, sign, out=g.view(torch.int8 if sign else torch.uint8))
            what = "tunpack b%d sign %d n %d, in + %d bytes, out + %d bytes" % (bits, sign, n, in_off, out_off)
            got = g.result(what)
            assert np.array_equal(got, want.view(np.uint8)), what


# ---- qe_quantize_pack ------------------------------------------------------------------------------------------------
def _quant_case(bits, sign, scale, zero, inner, n, seed):
    qmin, qmax = ew_ref.qrange(bits, sign)
    x = ew_ref.tie_dense(np.random.RandomState(seed), n, scale, zero, qmin, qmax, inner)
    want = ew_ref.pack(ew_ref.stored(ew_ref.quantise(x, scale, zero, qmin, qmax, inner), bits, sign), bits)
    return x, want


def _run_quantize_pack(x, scale, zero, bits, sign, inner, want, st, x_off=0, out_off=0, what=""):
    qmin, qmax = ew_ref.qrange(bits, sign)
    g = ei.Guarded(want.size, out_off)
    capi.quantize_pack(ei.device_input(x, "float32", x_off), _t(scale), _t(zero), qmin, qmax, bits, sign, inner=inner,
                       out=g.out, status=st)
    what = "quantize_pack b%d sign %d n %d inner %d x %d channels, x + %d floats, out + %d bytes %s" % (
        bits, sign, x.size, inner, scale.size, x_off, out_off, what)
    got = g.result(what)
    if not np.array_equal(got, want):
        a, b = ew_ref.unpack_codes(got, x.size, bits), ew_ref.unpack_codes(want, x.size, bits)
        bad = np.flatnonzero(a != b)
        raise AssertionError("%s: %d of %d codes differ, first at element %d (x %r: got %d, want %d)" % (
            what, bad.size, x.size, bad[0], x[bad[0]], a[bad[0]], b[bad[0]]))


@pytest.mark.parametrize("bits,sign", ei.PAIRS, ids=PAIR_IDS)
def test_quantize_pack_per_tensor(bits, sign):
    st = _status()
    for i in range(len(ei.PER_TENSOR)):
        scale, zero = ei.tensor_params(i)
        for n in ei.NS:
            x, want = _quant_case(bits, sign, scale, zero, 1, n, 31 * i + n)
            _run_quantize_pack(x, scale, zero, bits, sign, 1, want, st)
    scale, zero = ei.tensor_params(bits)
    x, want = _quant_case(bits, sign, scale, zero, 1, ei.NS[-1], 5)
    for x_off, out_off in ei.QPACK_OFFSETS:
        _run_quantize_pack(x, scale, zero, bits, sign, 1, want, st, x_off, out_off)
    assert int(st.item()) == 0


@pytest.mark.parametrize("bits,sign", ei.PAIRS, ids=PAIR_IDS)
def test_quantize_pack_per_channel(bits, sign):
    """Tiles that start mid-plane, channels that wrap inside a tile, and both the inner % 4 == 0 vector path and the scalar one."""
    st = _status()
    for inner, n_ch in ei.QPACK_PC_CASES:
        scale, zero = ei.channel_params(n_ch)
        n = ei.pc_n(inner, n_ch)
        x, want = _quant_case(bits, sign, scale, zero, inner, n, inner + n_ch)
        _run_quantize_pack(x, scale, zero, bits, sign, inner, want, st)
        if (inner, n_ch) in ((196, 3), (5, 64), (8193, 2)):
            for x_off, out_off in ei.QPACK_OFFSETS:
                _run_quantize_pack(x, scale, zero, bits, sign, inner, want, st, x_off, out_off)
    assert int(st.item()) == 0


@pytest.mark.parametrize("bits,sign", ei.PAIRS, ids=PAIR_IDS)
def test_quantize_pack_infinities_and_a_subnormal_scale(bits, sign):
    qmin, qmax = ew_ref.qrange(bits, sign)
    st = _status()
    # +-inf clamp to the ends of the range; the flag stays 0
    n = ei.TILE + 13
    scale, zero = ei.tensor_params(1)
    x = ew_ref.tie_dense(np.random.RandomState(bits), n, scale, zero, qmin, qmax)
    x[[0, 5, n - 1]], x[[1, ei.TILE - 1, n - 2]] = np.inf, -np.inf
    q = ew_ref.quantise(x, scale, zero, qmin, qmax)
    assert q[0] == qmax and q[1] == qmin and q[n - 1] == qmax and q[n - 2] == qmin
    _run_quantize_pack(x, scale, zero, bits, sign, 1, ew_ref.pack(ew_ref.stored(q, bits, sign), bits), st, what="(+-inf)")
    # a subnormal scale: 0 / scale is 0 (not NaN, not flushed into a division by zero), so the code is -zero
    zero_v = 1.0 if sign else -1.0          # -zero = -1 (signed) or 1 (unsigned): inside the range of every width
    for n_ch, inner in ((1, 1), (3, 5)):
        scale = np.full(n_ch, 1e-40, np.float32)
        assert 0 < scale[0] < np.finfo(np.float32).tiny
        zero = np.full(n_ch, zero_v, np.float32)
        x = np.zeros(n, np.float32)
        q = ew_ref.quantise(x, scale, zero, qmin, qmax, inner)
        assert (q == -zero_v).all()
        _run_quantize_pack(x, scale, zero, bits, sign, inner, ew_ref.pack(ew_ref.stored(q, bits, sign), bits), st,
                           what="(subnormal scale)")
    assert int(st.item()) == 0


# ---- qe_quantize_pack_act ----------------------------------------------------------------------------------------------
def _bits_of(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _run_act(x, scale, zero, bits, sign, inner, act, y_mode, st, x_off=0, y_off=0, c_off=0):
    """One call.  Returns (codes bytes, y as float32 numpy or None); the guard bands of the codes and of y (which is x's own
    buffer when in place) are checked."""
    qmin, qmax = ew_ref.qrange(bits, sign)
    n = x.size
    gc = ei.Guarded(capi.packed_nbytes(n, bits), c_off)
    what = "quantize_pack_act %s y %s b%d sign %d n %d inner %d x %d ch, x + %d, y + %d floats, codes + %d bytes" % (
        act, y_mode, bits, sign, n, inner, scale.size, x_off, y_off, c_off)
    gy = None
    if y_mode == "inplace":
        gy = ei.Guarded(4 * n, 4 * x_off)
        xd = gy.view(torch.float32)
        xd.copy_(_t(x))
        yd = xd
    else:
        xd = ei.device_input(x, "float32", x_off)
        if y_mode == "new":
            gy = ei.Guarded(4 * n, 4 * y_off)
        yd = gy.view(torch.float32) if gy is not None else None
    capi.quantize_pack_act(xd, _t(scale), _t(zero), qmin, qmax, bits, sign, act=act, inner=inner, out=gc.out, y=yd, status=st)
    codes = gc.result(what + " (codes)")
    y = gy.result(what + " (y)").view(np.float32) if gy is not None else None
    return codes, y, what


def _codes_of(y, scale, zero, bits, sign, inner):
    qmin, qmax = ew_ref.qrange(bits, sign)
    return ew_ref.pack(ew_ref.stored(ew_ref.quantise(y, scale, zero, qmin, qmax, inner), bits, sign), bits)


def _check_gelu(x, y):
    """The rule of test_gelu_accuracy: no further from float64 than torch's own fp32 GELU plus 1 ulp."""
    ref = ew_ref.gelu64(x)
    tg = F.gelu(_t(x)).cpu().numpy()
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    e_k, e_t = np.abs(y.astype(np.float64) - ref), np.abs(tg.astype(np.float64) - ref)
    assert (e_k <= e_t + ulp).all(), float(((e_k - e_t) / ulp).max())


@pytest.mark.parametrize("bits,sign", ei.PAIRS, ids=PAIR_IDS)
def test_quantize_pack_act_modes_and_ragged_ends(bits, sign):
    """act x y at every remainder of the group of 8.  The codes are those of the fp32 y the kernel itself made (so the GELU's
    accuracy does not enter); y for act=None is a bit copy of x; the GELU is held to test_gelu_accuracy's rule."""
    qmin, qmax = ew_ref.qrange(bits, sign)
    st = _status()
    for i, n in enumerate(ei.ACT_NS):
        scale, zero = ei.tensor_params(i)
        x = ew_ref.tie_dense(np.random.RandomState(n), n, scale, zero, qmin, qmax)
        want_none = _codes_of(x, scale, zero, bits, sign, 1)
        y_gelu = want_gelu = None
        for act, y_mode in (("gelu", "new"), ("gelu", None), ("gelu", "inplace"), (None, "new"), (None, "inplace")):
            codes, y, what = _run_act(x, scale, zero, bits, sign, 1, act, y_mode, st)
            if act is None:
                assert np.array_equal(_bits_of(y), _bits_of(x)), what
                assert np.array_equal(codes, want_none), what
                continue
            if y_gelu is None:
                y_gelu, want_gelu = y, _codes_of(y, scale, zero, bits, sign, 1)
                _check_gelu(x, y)
            elif y is not None:
                assert np.array_equal(_bits_of(y), _bits_of(y_gelu)), what
            assert np.array_equal(codes, want_gelu), what
    assert int(st.item()) == 0


@pytest.mark.parametrize("bits,sign", ei.PAIRS, ids=PAIR_IDS)
def test_quantize_pack_act_alignments(bits, sign):
    """x and y each 0..3 floats past a 16-byte boundary (only 0, 0 takes the 16-byte loads and stores), the codes 0, 4, 8 and
    1 bytes past one (at 8 bits, 0 and 8 take the 8-byte store, 4 and 1 the byte loop)."""
    qmin, qmax = ew_ref.qrange(bits, sign)
    st = _status()
    n = ei.ACT_OFFSET_N
    scale, zero = ei.tensor_params(bits + 1)
    x = ew_ref.tie_dense(np.random.RandomState(bits), n, scale, zero, qmin, qmax)
    for act in (None, "gelu"):
        y0 = want = None
        for x_off in ei.ACT_FLOAT_OFFSETS:
            for c_off in ei.ACT_CODE_OFFSETS:
                runs = [("new", y_off) for y_off in ei.ACT_FLOAT_OFFSETS] + [("inplace", x_off)]
                for y_mode, y_off in runs:
                    codes, y, what = _run_act(x, scale, zero, bits, sign, 1, act, y_mode, st, x_off, y_off, c_off)
                    if y0 is None:
                        y0, want = y, _codes_of(y, scale, zero, bits, sign, 1)
                        if act is None:
                            assert np.array_equal(_bits_of(y), _bits_of(x)), what
                    assert np.array_equal(_bits_of(y), _bits_of(y0)), what
                    assert np.array_equal(codes, want), what
    assert int(st.item()) == 0


@pytest.mark.parametrize("bits,sign", ei.PAIRS, ids=PAIR_IDS)
def test_quantize_pack_act_per_channel(bits, sign):
    qmin, qmax = ew_ref.qrange(bits, sign)
    st = _status()
    for j, (inner, n_ch) in enumerate(ei.QPACK_PC_CASES):
        scale, zero = ei.channel_params(n_ch)
        n = ei.pc_n(inner, n_ch)
        x = ew_ref.tie_dense(np.random.RandomState(inner + n_ch), n, scale, zero, qmin, qmax, inner)
        act, y_mode = ei.ACT_MODES[j % len(ei.ACT_MODES)]
        codes, y, what = _run_act(x, scale, zero, bits, sign, inner, act, "new" if y_mode is None else y_mode, st,
                                  x_off=j % 2, y_off=j % 2, c_off=(0, 1)[j % 3 == 0])
        if act is None:
            assert np.array_equal(_bits_of(y), _bits_of(x)), what
        assert np.array_equal(codes, _codes_of(y, scale, zero, bits, sign, inner)), what
        if y_mode is None:      # codes only: the same codes without the fp32 output
            codes2, _, what = _run_act(x, scale, zero, bits, sign, inner, act, None, st)
            assert np.array_equal(codes2, codes), what
    assert int(st.item()) == 0


def test_quantize_pack_act_without_act_or_y_is_quantize_pack():
    scale, zero = ei.channel_params(3)
    x = ew_ref.tie_dense(np.random.RandomState(1), 3 * ei.TILE + 5, scale, zero, -8, 7, 49)
    xd = _t(x)
    a, y, st_a = capi.quantize_pack_act(xd, _t(scale), _t(zero), -8, 7, 4, True, act=None, inner=49, y=None)
    b, st_b = capi.quantize_pack(xd, _t(scale), _t(zero), -8, 7, 4, True, inner=49)
    assert y is None and torch.equal(a, b) and int(st_a.item()) == 0 and int(st_b.item()) == 0
    assert np.array_equal(a.cpu().numpy(), _codes_of(x, scale, zero, 4, True, 49))


def test_quantize_pack_act_refuses_a_partial_overlap():
    n = 4096
    base = torch.zeros(3 * n, device=DEV)
    one, nil = torch.ones(1, device=DEV), torch.zeros(1, device=DEV)
    x = base[n:2 * n]
    for act in (None, "gelu"):
        for lo in (n + 4, n - 4, n + 1, 1, 2 * n - 1):
            with pytest.raises(capi.QeError, match="invalid argument"):
                capi.quantize_pack_act(x, one, nil, -128, 127, 8, True, act=act, y=base[lo:lo + n])
        for lo in (0, n, 2 * n):                       # disjoint on either side, or in place
            _, _, st = capi.quantize_pack_act(x, one, nil, -128, 127, 8, True, act=act, y=base[lo:lo + n])
            assert int(st.item()) == 0
    assert float(base.abs().max()) == 0.0


# ---- the range flag ----------------------------------------------------------------------------------------------------
def _elementwise_equal_but(got, want, n, bits, skip, what):
    a, b = ew_ref.unpack_codes(got, n, bits), ew_ref.unpack_codes(want, n, bits)
    keep = np.ones(n, bool)
    keep[skip] = False
    assert np.array_equal(a[keep], b[keep]), what


@pytest.mark.parametrize("dtype", ei.DTYPES)
def test_tpack_flag_from_any_position(dtype):
    n = ei.FLAG_N
    for bits, sign in ((3, False), (4, True)):
        lo, hi = ei.tpack_values(dtype, bits, sign)
        q, want = _tpack_ref(bits, sign, n, lo, hi)
        for in_off in (0, ei.in_offset(dtype)):
            runs = [("clean input", None)] + sorted(ei.flag_positions(n, ei.tpack_epl(dtype)).items())
            for name, pos in runs:
                v = q.copy()
                if pos is not None:
                    v[pos] = hi + 1
                st = _status()
                g = ei.Guarded(want.size, 0)
                capi.tpack(ei.device_input(v.astype(dtype), dtype, in_off), bits, sign, out=g.out, status=st)
                what = "tpack %s b%d sign %d, x + %d elements, %s" % (dtype, bits, sign, in_off, name)
                got = g.result(what)
                assert int(st.item()) == (0 if pos is None else 1), what
                _elementwise_equal_but(got, want, n, bits, [] if pos is None else [pos], what)


@pytest.mark.parametrize("bits,sign", [(8, True), (3, False)], ids=["b8_s", "b3_u"])
@pytest.mark.parametrize("kernel", ["quantize_pack", "act_none", "act_gelu"])
def test_quantiser_flag_from_any_position(kernel, bits, sign):
    """A NaN anywhere raises the flag; every other element's code is the reference's."""
    qmin, qmax = ew_ref.qrange(bits, sign)
    n = ei.FLAG_N
    for scale, zero, inner in ((*ei.tensor_params(0), 1), (*ei.channel_params(3), 5), (*ei.channel_params(2), 196)):
        x0 = ew_ref.tie_dense(np.random.RandomState(n), n, scale, zero, qmin, qmax, inner)
        for x_off in (0, 1):
            runs = [("clean input", None)] + sorted(ei.flag_positions(n, 4 if kernel == "quantize_pack" else 8).items())
            for name, pos in runs:
                x = x0.copy()
                if pos is not None:
                    x[pos] = np.nan
                st = _status()
                what = "%s b%d sign %d inner %d x %d ch, x + %d floats, %s" % (kernel, bits, sign, inner, scale.size, x_off, name)
                if kernel == "quantize_pack":
                    g = ei.Guarded(capi.packed_nbytes(n, bits), 0)
                    capi.quantize_pack(ei.device_input(x, "float32", x_off), _t(scale), _t(zero), qmin, qmax, bits, sign,
                                       inner=inner, out=g.out, status=st)
                    got, y = g.result(what), x
                else:
                    got, y, _ = _run_act(x, scale, zero, bits, sign, inner, None if kernel == "act_none" else "gelu", "new", st,
                                         x_off=x_off, y_off=x_off)
                    if pos is not None:
                        assert np.isnan(y[pos]), what
                assert int(st.item()) == (0 if pos is None else 1), what
                _elementwise_equal_but(got, _codes_of(y, scale, zero, bits, sign, inner), n, bits, [] if pos is None else [pos], what)
