"""GPU: every row of tests/grp_instances.py through qe_quantconv2d_grouped, checked three ways against tests/grp_ref.py
(numpy float64, independent of the engine).

  Pass A    exact grid (power-of-two scales, integer zeros, bias on the grid, |I| < 2^24): out, pre-filled with NaN, equals
            float64 bit for bit -- one code decoded one LSB wrong, or one off-group product let in, fails.
  Pass B    ordinary operands: conftest.conv_tolerance, |out - exact64| <= max(1e-5, max |chain - exact64|), the chain being
            fp32 F.conv2d(groups=g) on the dequantised tensors on the CPU (the reference's packed forward).
  Epilogues with and without ReLU; codes for signed / unsigned, per-tensor / per-channel consumers, alone and next to out:
            bit-equal to qe_quantize_pack of the same call's fp32 out and (pass A) to grp_ref's quantiser and packer; out at +1
            float and codes at +1 byte give the same bytes while the plan reports the narrower store forms; sub-8-bit
            consumers take two passes inside the call and are refused without out.
  Flag      a NaN bias on the LAST channel (an element of the last slab) raises status and changes no other channel's codes;
            clean input leaves it 0."""
import numpy as np
import pytest
import torch

import grp_instances as gi
import grp_ref
from conftest import conv_tolerance
from quantize_amd import capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL = range(len(gi.rows()))
IDS = [gi.row_id(k) for k in ALL]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _dev(k, regime, bias="own"):
    row = gi.rows()[k]
    o = gi.operands(k, regime)
    xq = capi.qparam(_t(o["x"]), row[5][0], row[5][1], _t(o["sx"]), _t(o["zx"]))
    wq = capi.qparam(_t(o["w"]), row[6][0], row[6][1], _t(o["sw"]), _t(o["zw"]))
    b = o["bias"] if isinstance(bias, str) else bias
    return xq, wq, (None if b is None else _t(b)), gi.shape_of(row), row[8]


def _rq(k, which, regime):
    s, z, lo, hi, bits, sign = gi.consumer(k, which, regime)
    return capi.requant(_t(s), _t(z), lo, hi, bits, sign), (s, z, lo, hi, bits, sign)


def _nan_out(k):
    row = gi.rows()[k]
    (N, IC, H, W), (KH, KW) = row[1], row[2]
    OH, OW = grp_ref.out_hw(H, W, KH, KW, row[3], row[4])
    return torch.full((N, row[9], OH, OW), float("nan"), dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("k", ALL, ids=IDS)
def test_pass_a_exact_grid(k):
    xq, wq, bias, sh, g = _dev(k, "exact")
    for relu in (False, True):
        out, _, st = capi.quantconv2d_grouped(xq, wq, bias, sh, g, relu=relu, out=_nan_out(k))
        got = out.cpu().numpy().astype(np.float64)
        ref = gi.reference(k, "exact", relu)
        bad = np.argwhere(got != ref)
        assert bad.size == 0, "%s relu=%d: %d of %d differ, first at %s: %r vs %r" % (
            gi.row_id(k), relu, len(bad), ref.size, tuple(bad[0]), got[tuple(bad[0])], ref[tuple(bad[0])])
        assert int(st.item()) == 0


@pytest.mark.parametrize("k", ALL, ids=IDS)
def test_pass_b_conv_parity_rule(k):
    xq, wq, bias, sh, g = _dev(k, "parity")
    out, _, _ = capi.quantconv2d_grouped(xq, wq, bias, sh, g, out=_nan_out(k))
    err, allowed = conv_tolerance(out.cpu().numpy(), gi.reference(k, "parity"), gi.chain(k))
    print("%s: max err %.3e allowed %.3e" % (gi.row_id(k), np.nanmax(err), allowed))
    assert not np.isnan(err).any() and err.max() <= allowed, "%s: %.3e > %.3e" % (gi.row_id(k), err.max(), allowed)


def _pack_of(out, cons, OHW):
    s, z, lo, hi, bits, sign = cons
    return capi.quantize_pack(out.contiguous(), _t(s), _t(z), lo, hi, bits, sign, inner=OHW)


@pytest.mark.parametrize("k", ALL, ids=IDS)
def test_epilogues(k):
    row = gi.rows()[k]
    for regime in ("exact", "parity"):
        xq, wq, bias, sh, g = _dev(k, regime)
        OH, OW = capi.out_hw(sh)
        n = sh.N * sh.OC * OH * OW
        for relu in (False, True):
            plain_out, _, _ = capi.quantconv2d_grouped(xq, wq, bias, sh, g, relu=relu, out=_nan_out(k))
            for which in ("u8", "s8c"):
                rq, cons = _rq(k, which, regime)
                # out and codes together: the same fp32 bytes as the out-only call, codes = qe_quantize_pack(out)
                both_codes = torch.full((n,), 0xA5, dtype=torch.uint8, device=DEV)
                out, codes, st = capi.quantconv2d_grouped(xq, wq, bias, sh, g, relu=relu, rq=rq, out=_nan_out(k), codes=both_codes)
                assert torch.equal(out.view(torch.int32), plain_out.view(torch.int32)), (gi.row_id(k), regime, relu, which)
                want, wst = _pack_of(out, cons, OH * OW)
                assert torch.equal(codes, want), (gi.row_id(k), regime, relu, which)
                assert int(st.item()) == int(wst.item()) == 0
                # codes alone
                _, only, st = capi.quantconv2d_grouped(xq, wq, bias, sh, g, relu=relu, rq=rq, out=None,
                                                       codes=torch.full((n,), 0x5A, dtype=torch.uint8, device=DEV))
                assert torch.equal(only, want) and int(st.item()) == 0, (gi.row_id(k), regime, relu, which)
                if regime == "exact":
                    q = grp_ref.quantize(gi.reference(k, "exact", relu), cons[0], cons[1], cons[2], cons[3])
                    assert np.array_equal(only.cpu().numpy(), grp_ref.pack(q, cons[4], cons[5])), (gi.row_id(k), relu, which)
                # out at +1 float, codes at +1 byte: narrower store forms in the plan, the same bytes
                obuf = torch.full((n + 1,), float("nan"), dtype=torch.float32, device=DEV)
                cbuf = torch.full((n + 1,), 0xA5, dtype=torch.uint8, device=DEV)
                o1, c1 = obuf[1:].view(out.shape), cbuf[1:]
                assert o1.data_ptr() % 16 == 4 and c1.data_ptr() % 4 == 1
                p0 = capi.grouped_plan_info(sh, g, xq, wq, rq, out.data_ptr(), codes.data_ptr())
                p1 = capi.grouped_plan_info(sh, g, xq, wq, rq, o1.data_ptr(), c1.data_ptr())
                assert (p0.out16, p0.codes16, p1.out16, p1.codes16) == (1, 1, 0, 0)
                assert p0.kernel == p1.kernel == gi.expected_kernel(row, 2)
                capi.quantconv2d_grouped(xq, wq, bias, sh, g, relu=relu, rq=rq, out=o1, codes=c1)
                assert torch.equal(o1.view(torch.int32), out.view(torch.int32)) and torch.equal(c1, codes)
                assert int(cbuf[0]) == 0xA5 and bool(torch.isnan(obuf[0]))
        # sub-8-bit consumers: two passes inside the call with out, refused without
        for which in ("u4", "s3c"):
            rq, cons = _rq(k, which, regime)
            assert capi.grouped_plan_info(sh, g, xq, wq, rq, 256, 256).two_pass == 1
            out, codes, st = capi.quantconv2d_grouped(xq, wq, bias, sh, g, relu=True, rq=rq, out=_nan_out(k))
            want, _ = _pack_of(out, cons, OH * OW)
            assert codes.numel() == (n * cons[4] + 7) // 8 and torch.equal(codes, want) and int(st.item()) == 0
            assert torch.equal(out.view(torch.int32), plain_out.view(torch.int32))
            with pytest.raises(capi.QeError):
                capi.quantconv2d_grouped(xq, wq, bias, sh, g, relu=True, rq=rq, out=None)


_WITH_BIAS = [k for k in ALL if not gi.rows()[k][7] & {"nobias"}]
# a sample of the table, and every fast row of three slabs (the flag then comes from the last slab's workgroups)
FLAG_ROWS = sorted(set(_WITH_BIAS[::9]) | {k for k in _WITH_BIAS if gi.rows()[k][0] == "fast" and
                                           gi.rows()[k][9] >= 3 * gi.plan(gi.rows()[k]).slab})


@pytest.mark.parametrize("k", FLAG_ROWS, ids=[IDS[k] for k in FLAG_ROWS])
def test_flag(k):
    """The NaN sits on the last output channel: with more than one slab, an element of the last slab."""
    o = gi.operands(k, "exact")
    OC = gi.rows()[k][9]
    rq, _ = _rq(k, "u8", "exact")
    xq, wq, bias, sh, g = _dev(k, "exact")
    _, clean, st = capi.quantconv2d_grouped(xq, wq, bias, sh, g, relu=True, rq=rq, out=None)
    assert int(st.item()) == 0
    nan_bias = o["bias"].copy()
    nan_bias[OC - 1] = np.nan
    xq, wq, bias, sh, g = _dev(k, "exact", bias=nan_bias)
    _, codes, st = capi.quantconv2d_grouped(xq, wq, bias, sh, g, relu=True, rq=rq, out=None)
    assert int(st.item()) & 1
    keep = torch.ones(clean.numel(), dtype=torch.bool, device=DEV).view(sh.N, OC, -1)
    keep[:, OC - 1] = False
    assert torch.equal(codes[keep.view(-1)], clean[keep.view(-1)])
