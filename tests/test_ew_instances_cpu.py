"""CPU: the elementwise instance table (tests/ew_instances.py) reaches all 93 kernels of the family, the numpy reference
(tests/ew_ref.py) packs what the C oracle and the reference packer's golden streams pack, and the inputs the GPU tests
quantise can tell the contract -- fp32 division, subtraction, round-half-even -- from a reciprocal multiply and from
float64 arithmetic.  The last is measured on the reference alone, so a GPU test cannot pass for want of a hard input."""
import numpy as np
import pytest

import ew_instances as ei
import ew_ref
import oracle


def test_cases_cover_every_instance():
    every = ei.every_instance()
    assert len(every) == 93
    assert len([i for i in every if i[0] == "tpack_kernel"]) == 80
    assert len([i for i in every if i[0] == "tunpack_kernel"]) == 8
    missing = every - ei.covered()
    assert not missing, "no case reaches %s" % sorted(missing, key=str)
    assert ei.covered() <= every
    print("elementwise instances reached: %d of %d" % (len(ei.covered()), len(every)))


def test_cases_reach_the_edges():
    assert {1, 7, ei.TILE - 1, ei.TILE, ei.TILE + 1} <= set(ei.NS) and max(ei.NS) > 3 * ei.TILE and max(ei.NS) % 8 != 0
    for t in ei.DTYPES:
        vec = min(16, 4 * ei.ITEMSIZE[t])
        assert (ei.in_offset(t) * ei.ITEMSIZE[t]) % vec != 0, t
    assert ei.OUT_OFFSET % 16 != 0
    # per channel: both the inner % 4 == 0 vector path and the scalar one, planes shorter and longer than a tile, and
    # channels that wrap inside the case
    assert any(i % 4 == 0 for i in ei.INNERS) and any(i % 4 != 0 for i in ei.INNERS)
    assert min(ei.INNERS) == 1 and max(ei.INNERS) > ei.TILE and any(ei.TILE % i != 0 for i in ei.INNERS)
    for inner in ei.INNERS:
        assert any(ei.pc_n(inner, c) > inner * c for c in ei.CHANNELS), inner
    # quantize_pack_act: every remainder of the group of 8, and fewer than / one more than a group
    assert {n % 8 for n in ei.ACT_NS} == set(range(8)) and {1, 7, 9} <= set(ei.ACT_NS)
    assert ei.GRIDCAP_N > ei.TP_MAX_BLOCKS * ei.TILE and (ei.GRIDCAP_N + 7) // 8 > 8192 * 256
    N, C, H, W, p = ei.GRIDCAP_PATCHIFY
    assert N * C * H * W == 16859136 and (N * C * H * W + 7) // 8 > ei.PATCHIFY_MAX_GROUPS
    # patchify: a ragged last group, p % 8 == 0 and not, an unaligned x under p % 8 == 0
    assert any((n * c * h * w) % 8 != 0 for n, c, h, w, *_ in ei.PATCHIFY_CASES)
    assert any(p % 8 == 0 and off == 0 for *_, p, off, _ in ei.PATCHIFY_CASES)
    assert any(p % 8 == 0 and off != 0 for *_, p, off, _ in ei.PATCHIFY_CASES)
    assert any(p % 8 != 0 for *_, p, off, _ in ei.PATCHIFY_CASES)
    # maxpool: the plane sizes at which a thread's 16 outputs cross planes, and the ragged ends
    planes, rag = set(), set()
    for N, C, H, W, k, s, p, _ in ei.MAXPOOL_CASES:
        oh, ow = ei.maxpool_out_hw(H, W, k, s, p)
        planes.add(oh * ow)
        rag.add((N * C * oh * ow) % 16)
        if oh * ow < 16:
            assert N * C >= 40
    assert {1, 4, 9, 15, 17} <= planes and {1, 15} <= rag
    assert any(k > H and p > 0 for _, _, H, _, k, _, p, _ in ei.MAXPOOL_CASES)
    assert any(s > k for *_, k, s, _, _ in ei.MAXPOOL_CASES)
    assert any(N * C * np.prod(ei.maxpool_out_hw(H, W, k, s, p)) > 16 * 256 for N, C, H, W, k, s, p, _ in ei.MAXPOOL_CASES)
    assert 64 * ei.AVGPOOL_P[-1] * 4 == 60 * 1024 and ei.AVGPOOL_P_REFUSED == ei.AVGPOOL_P[-1] + 1


@pytest.mark.parametrize("bits,sign", ei.PAIRS)
def test_reference_packer_equals_the_oracle(bits, sign):
    rng = np.random.RandomState(bits * 2 + sign)
    lo, hi = ew_ref.qrange(bits, sign)
    for n in (1, 7, 9, 8193):
        q = rng.randint(lo, hi + 1, size=n)
        q[0], q[-1] = hi, lo
        want, _ = oracle.tpack(q.astype(np.float32), bits, sign)
        got = ew_ref.pack(ew_ref.stored(q.astype(np.float32), bits, sign), bits)
        assert got.dtype == np.uint8 and np.array_equal(got, want), n
        back = ew_ref.unpack(got, n, bits, sign)
        assert back.dtype == (np.int8 if sign else np.uint8) and np.array_equal(back.astype(np.int64), q), n
        assert not ew_ref.range_bad(q, bits, sign).any()


def test_reference_packer_equals_the_golden_streams(g1):
    pairs = set()
    for key in g1.index:
        des = g1.get(key, "des")
        bits, sign = int(des[0]), bool(des[1])
        x = g1.get(key, "x").reshape(-1)
        assert np.array_equal(ew_ref.pack(ew_ref.stored(x, bits, sign), bits), g1.get(key, "packed")), key
        assert np.array_equal(ew_ref.unpack(g1.get(key, "packed"), x.size, bits, sign), g1.get(key, "unpacked").reshape(-1)), key
        pairs.add((bits, sign))
    assert pairs == set(ei.PAIRS)


def test_range_test_is_on_the_value_as_float():
    for bits, sign in ei.PAIRS:
        lo, hi = ew_ref.qrange(bits, sign)
        v = np.array([lo, hi, lo - 1, hi + 1, hi + 0.5, lo - 0.5, np.nan, np.inf, -np.inf, 0.0])
        assert ew_ref.range_bad(v, bits, sign).tolist() == [False, False, True, True, True, True, True, True, True, False]


def test_quantise_is_the_fp32_sequence():
    x = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 1e9, -1e9, np.inf, -np.inf, np.nan, 0.0], np.float32)
    q = ew_ref.quantise(x, [1.0], [0.0], -128, 127)
    assert q.dtype == np.float32
    assert q[:9].tolist() == [0.0, 2.0, 2.0, -0.0, -2.0, 127.0, -128.0, 127.0, -128.0] and np.isnan(q[9]) and q[10] == 0.0
    # a subnormal scale: 0 / scale = 0, minus zero
    assert ew_ref.quantise(np.zeros(4, np.float32), [1e-40], [3.0], -128, 127).tolist() == [-3.0] * 4
    # per channel: the channel of element i is (i // inner) % n_ch
    x = np.full(12, 3.0, np.float32)
    q = ew_ref.quantise(x, [1.0, 0.5, 0.25], [0.0, 0.0, 1.0], -128, 127, inner=2)
    assert q.tolist() == [3, 3, 6, 6, 11, 11, 3, 3, 6, 6, 11, 11]


def _variants(x, scale, zero, qmin, qmax, inner):
    ref = ew_ref.quantise(x, scale, zero, qmin, qmax, inner)
    rec = ew_ref.quantise_reciprocal(x, scale, zero, qmin, qmax, inner)
    f64 = ew_ref.quantise_f64(x, scale, zero, qmin, qmax, inner)
    return float((ref != rec).mean()), float((ref != f64).mean())


@pytest.mark.parametrize("sign", [True, False])
def test_tie_dense_inputs_separate_the_wrong_variants(sign):
    """Every scale set the GPU tests use, at 8 bits: at least a quarter of the elements within 4 ulp of a tie, and at least
    1 % of the codes change under either wrong variant."""
    qmin, qmax = ew_ref.qrange(8, sign)
    for i, (name, scale, zero, inner) in enumerate(ei.scale_sets()):
        x = ew_ref.tie_dense(np.random.RandomState(i), 1 << 16, scale, zero, qmin, qmax, inner)
        near = float((ew_ref.tie_distance_ulp(x, scale, zero, inner) <= 4.0).mean())
        d_rec, d_f64 = _variants(x, scale, zero, qmin, qmax, inner)
        print("%-18s signed %d: %.1f %% near a tie; reciprocal changes %.1f %%, float64 %.1f %% of the codes" % (
            name, sign, 100 * near, 100 * d_rec, 100 * d_f64))
        assert near >= 0.25, name
        assert d_rec >= 0.01 and d_f64 >= 0.01, name


def test_a_scale_set_that_does_not_separate_is_not_used():
    for sz in ei.REJECTED:
        assert sz not in ei.PER_TENSOR
        scale, zero = np.array([sz[0]], np.float32), np.array([sz[1]], np.float32)
        x = ew_ref.tie_dense(np.random.RandomState(0), 1 << 16, scale, zero, -128, 127)
        d_rec, d_f64 = _variants(x, scale, zero, -128, 127, 1)
        assert d_rec < 0.01 <= d_f64, (sz, d_rec, d_f64)


def test_random_normals_do_not_separate():
    """Why the generator exists: unit normals, as the first quantiser tests drew them, change under neither variant often
    enough to notice."""
    scale, zero = ei.tensor_params(0)
    x = (np.random.RandomState(0).normal(0, 40, size=1 << 16)).astype(np.float32)
    d_rec, d_f64 = _variants(x, scale, zero, -128, 127, 1)
    assert d_rec < 0.001 and d_f64 < 0.001


def test_small_references():
    # maxpool over stored codes: padding taps take no part, signed codes order as their values do
    c = np.array([[[[0, 200], [100, 50]]]], np.uint8)
    assert ew_ref.maxpool_codes(c, False, 3, 2, 1).tolist() == [[[[200]]]]
    assert ew_ref.maxpool_codes(c, True, 3, 1, 1).tolist() == [[[[200, 200], [200, 200]]]]
    assert ew_ref.maxpool_codes(c, True, 1, 1, 0).tolist() == c.tolist()
    x = np.arange(2 * 3 * 4 * 6, dtype=np.float32).reshape(2, 3, 4, 6)
    m = ew_ref.patch_matrix(x, 2)
    assert m.shape == (12, 12)
    # row (image 1, patch row 1, patch column 2), column (c 2, kh 1, kw 0)
    assert m[6 + 3 + 2, 2 * 4 + 2 + 0] == x[1, 2, 2 + 1, 4 + 0]
    assert ew_ref.avgpool64(x)[1, 2] == x[1, 2].astype(np.float64).mean()
    assert abs(ew_ref.gelu64(np.array([1.0]))[0] - 0.8413447460685429) < 1e-15
