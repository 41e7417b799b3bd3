"""GPU: the elementwise kernels past their grid caps.  n = 2049 * 8192 + 5 elements is more than the 2048 tiles a tpack /
tunpack grid holds and more than the 8192 * 256 groups of 8 a quantize_pack_act grid holds, so every block goes round its
grid-stride loop and the last one ends in a ragged tile; quantize_patchify at 112 images of 3 x 224 x 224 is past its own
cap.  The whole stream is compared with the C oracle's packer (fast enough at this size) and three windows -- the first two
tiles, the tiles either side of tile 2048, the last tile with the ragged one -- with tests/ew_ref.py; the quantiser in front
is ew_ref.quantise on all-tie inputs in every case.  Outputs sit between guard bands (ew_instances.Guarded)."""
import numpy as np
import pytest
import torch

import ew_instances as ei
import ew_ref
import oracle
from quantize_amd import capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = ei.GRIDCAP_N


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _check_stream(got, q, bits, sign, what):
    """got: the kernel's stream; q: the reference's integer-valued floats."""
    n = q.size
    assert got.size == (n * bits + 7) // 8
    for start, count in ei.gridcap_windows(n):
        want = ew_ref.pack(ew_ref.stored(q[start:start + count], bits, sign), bits)
        b0 = start * bits // 8
        assert np.array_equal(got[b0:b0 + want.size], want), "%s: window at element %d" % (what, start)
    whole, _ = oracle.tpack(q, bits, sign)
    if not np.array_equal(got, whole):
        bad = np.flatnonzero(got != whole)
        raise AssertionError("%s: %d bytes differ, first at byte %d (tile %d)" % (what, bad.size, bad[0], bad[0] * 8 // bits // ei.TILE))


def _all_ties(seed, n, scale, zero, bits, sign, inner=1):
    qmin, qmax = ew_ref.qrange(bits, sign)
    x = ew_ref.tie_dense(np.random.RandomState(seed), n, scale, zero, qmin, qmax, inner, fraction=1.0)
    return x, ew_ref.quantise(x, scale, zero, qmin, qmax, inner)


def test_tpack_past_the_grid_cap():
    v = np.random.RandomState(1).randint(0, 8, size=N).astype(np.uint8)
    g = ei.Guarded(capi.packed_nbytes(N, 3))
    _, st = capi.tpack(_t(v), 3, False, out=g.out)
    got = g.result("tpack uint8 b3")
    assert int(st.item()) == 0
    _check_stream(got, v.astype(np.float32), 3, False, "tpack uint8 b3")


def test_tunpack_past_the_grid_cap():
    bits, sign = 5, True
    q = np.random.RandomState(2).randint(-16, 16, size=N).astype(np.float32)
    packed, _ = oracle.tpack(q, bits, sign)
    g = ei.Guarded(N)
    capi.tunpack(_t(packed), N, bits, sign, out=g.view(torch.int8))
    got = g.result("tunpack b5").view(np.int8)
    for start, count in ei.gridcap_windows(N):
        b0 = start * bits // 8
        want = ew_ref.unpack(packed[b0:b0 + (count * bits + 7) // 8], count, bits, sign)
        assert np.array_equal(got[start:start + count], want), start
    assert np.array_equal(got, q.astype(np.int8))


def test_quantize_pack_per_tensor_past_the_grid_cap():
    bits, sign = 8, True
    scale, zero = ei.tensor_params(0)
    x, q = _all_ties(3, N, scale, zero, bits, sign)
    g = ei.Guarded(capi.packed_nbytes(N, bits))
    _, st = capi.quantize_pack(_t(x), _t(scale), _t(zero), -128, 127, bits, sign, out=g.out)
    got = g.result("quantize_pack per tensor")
    assert int(st.item()) == 0
    _check_stream(got, q, bits, sign, "quantize_pack per tensor")


def test_quantize_pack_per_channel_past_the_grid_cap():
    bits, sign, inner = 6, False, 12544
    scale, zero = ei.channel_params(64)
    x, q = _all_ties(4, N, scale, zero, bits, sign, inner)
    g = ei.Guarded(capi.packed_nbytes(N, bits))
    _, st = capi.quantize_pack(_t(x), _t(scale), _t(zero), 0, 63, bits, sign, inner=inner, out=g.out)
    got = g.result("quantize_pack per channel")
    assert int(st.item()) == 0
    _check_stream(got, q, bits, sign, "quantize_pack per channel, inner 12544 x 64")


def test_quantize_pack_act_past_the_grid_cap():
    bits, sign = 4, True
    scale, zero = ei.tensor_params(1)
    x, q = _all_ties(5, N, scale, zero, bits, sign)
    gc, gy = ei.Guarded(capi.packed_nbytes(N, bits)), ei.Guarded(4 * N)
    _, _, st = capi.quantize_pack_act(_t(x), _t(scale), _t(zero), -8, 7, bits, sign, act=None, out=gc.out, y=gy.view(torch.float32))
    got, y = gc.result("quantize_pack_act codes"), gy.result("quantize_pack_act y").view(np.float32)
    assert int(st.item()) == 0
    assert np.array_equal(y.view(np.uint32), x.view(np.uint32))
    _check_stream(got, q, bits, sign, "quantize_pack_act (None, y new)")


def test_quantize_patchify_past_the_grid_cap():
    Nimg, C, H, W, p = ei.GRIDCAP_PATCHIFY
    bits, sign = 8, True
    scale, zero = ei.tensor_params(2)
    n = Nimg * C * H * W
    x, _ = _all_ties(6, n, scale, zero, bits, sign)
    x = x.reshape(Nimg, C, H, W)
    q = ew_ref.quantise(ew_ref.patch_matrix(x, p), scale, zero, -128, 127)
    g = ei.Guarded(capi.packed_nbytes(n, bits))
    _, st = capi.quantize_patchify(_t(x), p, _t(scale), _t(zero), -128, 127, bits, sign, out=g.out)
    got = g.result("quantize_patchify")
    assert int(st.item()) == 0
    _check_stream(got, q, bits, sign, "quantize_patchify 112 x 3 x 224 x 224")
