"""CPU: every refused request of qe_affine_relu_quantize_pack and the code it returns, in the order include/quant_engine.h states
(rows with two faults pin the order).

The addresses are numbers, not memory.  That is safe only because no row reaches a launch: each is refused by a host check, which
the first test asserts of the table itself (no expected code is QE_OK or QE_ERR_HIP).  On a machine with a GPU a row that a broken
check wrongly accepted would launch on a bogus pointer, so the module skips there, as tests/test_api_refusals_cpu.py does."""
import ctypes

import pytest
import torch

from quantize_amd import capi

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="fake addresses: a wrongly accepted row would launch on them")

OK, NBITS, ARG, HIP = 0, 1, 4, 5
N, C, P = 2, 3, 64
BYTES = N * C * P * 4
# disjoint fake buffers, 1 MiB apart
X, ID, AL, SH, SUM, ACT, C0, C1, ST, S0, Z0, S1, Z1 = (0x100000 * (i + 1) for i in range(13))


def rq(scale=S0, zero=Z0, n_param=1, bits=8, sign=0):
    return capi.QeRequant(scale, zero, n_param, 0.0, 255.0, bits, sign)


def call(x=X, identity=ID, n=N, c=C, p=P, alpha=AL, shift=SH, rqs=(rq(),), codes=(C0, C1), sum_out=SUM, act_out=ACT, status=ST, n_out=None,
         rq_null=False, codes_null=False):
    rqs = list(rqs)
    arr = (capi.QeRequant * max(1, len(rqs)))(*rqs)
    cp = (ctypes.c_void_p * 2)(*codes)
    n_out = len(rqs) if n_out is None else n_out
    return capi.lib().qe_affine_relu_quantize_pack(x, identity, n, c, p, alpha, shift, n_out, None if rq_null else arr,
                                                   None if codes_null else cp, sum_out, act_out, status, None)


ROWS = [
    # n_out and the rq array, before anything else
    ("n_out -1", dict(n_out=-1), ARG),
    ("n_out 3 (and bad n_bits)", dict(n_out=3, rqs=(rq(bits=9), rq())), ARG),
    ("rq NULL with n_out 1", dict(n_out=1, rq_null=True), ARG),
    # each quantiser: NULL scale / zero, then n_bits, then n_param < 1
    ("rq scale NULL (and bad n_bits)", dict(rqs=(rq(scale=None, bits=9),)), ARG),
    ("rq zero NULL", dict(rqs=(rq(zero=None),)), ARG),
    ("n_bits 0", dict(rqs=(rq(bits=0),)), NBITS),
    ("n_bits 9 (and N 0)", dict(rqs=(rq(bits=9),), n=0), NBITS),
    ("second rq n_bits 9", dict(rqs=(rq(), rq(S1, Z1, bits=9))), NBITS),
    ("n_param 0", dict(rqs=(rq(n_param=0),)), ARG),
    # sizes
    ("N 0", dict(n=0), ARG), ("N -1", dict(n=-1), ARG), ("C 0", dict(c=0), ARG), ("P 0", dict(p=0), ARG), ("P -5", dict(p=-5), ARG),
    # n_param neither 1 nor C
    ("n_param 2 of C 3", dict(rqs=(rq(n_param=2),)), ARG),
    ("second n_param 4 of C 3", dict(rqs=(rq(), rq(S1, Z1, n_param=4))), ARG),
    # NULL operands
    ("x NULL", dict(x=None), ARG), ("alpha NULL", dict(alpha=None), ARG), ("shift NULL", dict(shift=None), ARG),
    ("codes NULL", dict(codes_null=True), ARG), ("codes[0] NULL", dict(codes=(None, C1)), ARG),
    ("codes[1] NULL", dict(rqs=(rq(), rq(S1, Z1)), codes=(C0, None)), ARG),
    # no output requested
    ("no output", dict(rqs=(), sum_out=None, act_out=None), ARG),
    # alignment of the fp32 pointers and of status
    ("x + 2", dict(x=X + 2), ARG), ("identity + 1", dict(identity=ID + 1), ARG), ("sum_out + 2", dict(sum_out=SUM + 2), ARG),
    ("act_out + 3", dict(act_out=ACT + 3), ARG), ("status + 2", dict(status=ST + 2), ARG), ("alpha + 1", dict(alpha=AL + 1), ARG),
    # overlaps: an output with an operand
    ("act_out == x", dict(act_out=X), ARG), ("act_out == identity", dict(act_out=ID), ARG),
    ("act_out inside x", dict(act_out=X + BYTES - 4), ARG),
    ("codes == x", dict(codes=(X, C1)), ARG), ("codes inside identity", dict(codes=(ID + BYTES - 1, C1)), ARG),
    ("codes over alpha", dict(codes=(AL - 8, C1)), ARG), ("act_out over shift", dict(act_out=SH - BYTES + 4), ARG),
    ("sum_out over the rq scale", dict(sum_out=S0 - 4), ARG), ("status == rq zero", dict(status=Z0), ARG),
    ("status inside x", dict(status=X + 8), ARG), ("codes over the second rq's zero", dict(rqs=(rq(), rq(S1, Z1)), codes=(C0, Z1 - 4)), ARG),
    # overlaps: an output with another output
    ("sum_out == act_out", dict(sum_out=ACT), ARG), ("codes[0] == codes[1]", dict(rqs=(rq(), rq(S1, Z1)), codes=(C0, C0)), ARG),
    ("codes inside act_out", dict(codes=(ACT + 16, C1)), ARG), ("status inside sum_out", dict(status=SUM + 4), ARG),
    ("status inside the codes", dict(status=C0 + 4), ARG),
    # sum_out partly over x or identity: only the same address is in place
    ("sum_out = x + 4", dict(sum_out=X + 4), ARG), ("sum_out = x - 4", dict(sum_out=X - 4), ARG),
    ("sum_out = identity + 16", dict(sum_out=ID + 16), ARG), ("sum_out = identity - 16", dict(sum_out=ID - 16), ARG),
]


def test_no_row_can_reach_a_launch():
    names = [r[0] for r in ROWS]
    assert len(names) == len(set(names))
    for name, kw, code in ROWS:
        assert code not in (OK, HIP), name


@pytest.mark.parametrize("name,kw,code", ROWS, ids=[r[0] for r in ROWS])
def test_refusal_code(name, kw, code):
    assert call(**kw) == code, name
    # the path query names no instance for a request whose counts or formats are refused
    if set(kw) <= {"n", "c", "p", "rqs", "n_out", "rq_null"} and not (kw.get("sum_out", 1) is None):
        rqs = list(kw.get("rqs", (rq(),)))
        arr = (capi.QeRequant * max(1, len(rqs)))(*rqs)
        got = capi.lib().qe_affine_relu_quantize_pack_path(kw.get("n", N), kw.get("c", C), kw.get("p", P), kw.get("n_out", len(rqs)),
                                                           None if kw.get("rq_null") else arr, SUM, ACT)
        assert got == -1, name
