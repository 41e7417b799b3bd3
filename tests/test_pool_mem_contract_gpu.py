"""GPU: the memory contract of the quantised ReLU / pooling entry points inside poisoned arenas (tests/arena.py): each module
form, and qe_avgpool2d_codes on one row per instance (and the sub-8-bit plain form) in each epilogue.

Every buffer a call sees -- x, its scale and zero, the consumer's scale and zero, out, codes, status -- lies between guard bands,
once in an arena of 0x00 and once in one of 0xFF:
  * no guard byte and no input byte changes;
  * out and codes equal the plain call's byte for byte under both fills, so every output byte was written (the payloads are
    pre-filled too) and none depends on what surrounds the buffers -- the pair kernel's 16-byte pieces and the plane kernel's
    aligned pieces reach up to and past the ends of a row or plane and must not let a neighbour's byte into a sum.
The code streams are also placed off a 256-byte boundary: x at +1 and +7, out at +4, codes at +3 (fp32 x at +4)."""
import numpy as np
import pytest
import torch

import arena
import pool_instances as pi
from quantize_amd import capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _placer(A):
    if A is None:
        return lambda a, off=0, name=None, inplace=False: _t(a)
    return lambda a, off=0, name=None, inplace=False: A.place(_t(a), off=off, name=name, inplace=inplace)


def _first(pred):
    return next(k for k, r in enumerate(pi.ROWS) if pred(r))


# one row per instance where its pieces reach over an edge: ragged pair chunks, planes that are no multiple of 16 bytes on more
# planes than a workgroup takes, a plain strided window, and the plain kernel packing 4-bit codes
CODES_ROWS = (_first(lambda r: r[0] == "pair" and r[1] == (2, 5, 10, 66)), _first(lambda r: r[0] == "pair" and r[1] == (1, 3, 9, 11)),
              _first(lambda r: r[0] == "plane" and r[1] == (3, 70, 7, 7)), _first(lambda r: r[0] == "plane" and r[1] == (1, 2, 1, 241)),
              _first(lambda r: r[0] == "plain" and r[2] == 3), _first(lambda r: r[7] == "u4" and r[2] == 2),
              _first(lambda r: r[7] == "u4" and r[4] == (5, 7)))
CODES_CASES = [(k, ep, relu) for k in CODES_ROWS for ep in pi.EPILOGUES for relu in (False, True)]


def _run_codes(k, ep, relu, A=None, offs=(0, 0, 0)):
    inst, (N, C, H, W), kernel, stride, osize, xs = pi.ROWS[k][:6]
    o = pi.operands(k, "parity")
    place = _placer(A)
    xq = capi.qparam(place(o["x"].reshape(-1), offs[0], "x"), 8, xs, place(o["sx"], name="sx"), place(o["zx"], name="zx"))
    OH, OW = pi.out_hw(pi.ROWS[k])
    n = N * C * OH * OW
    rq = None
    if ep != "out":
        s, z, lo, hi, bits, sign = pi.consumer(k, "parity")
        rq = capi.requant(place(s, name="rq scale"), place(z, name="rq zero"), lo, hi, bits, sign)
    if A is None:
        out = torch.empty((N, C, OH, OW), dtype=torch.float32, device=DEV) if ep != "codes" else None
        codes = torch.empty(capi.packed_nbytes(n, rq.n_bits), dtype=torch.uint8, device=DEV) if rq is not None else None
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
    else:
        out = A.blank((N, C, OH, OW), torch.float32, off=offs[1], name="out") if ep != "codes" else None
        codes = A.blank(capi.packed_nbytes(n, rq.n_bits), off=offs[2], name="codes") if rq is not None else None
        status = A.status()
    capi.avgpool2d_codes(xq, N, C, H, W, kernel, stride, osize, relu=relu, rq=rq, out=out, codes=codes, status=status)
    return out, codes, status


@pytest.mark.parametrize("k,ep,relu", CODES_CASES, ids=["%s-%s-%s" % (pi.row_id(k), ep, "relu" if r else "lin") for k, ep, r in CODES_CASES])
def test_avgpool2d_codes_contract(k, ep, relu):
    plain = _run_codes(k, ep, relu)
    for offs in ((0, 0, 0), (1, 4, 3), (7, 4, 3)):
        for fill in arena.FILLS:
            A = arena.Arena(DEV, fill)
            got = _run_codes(k, ep, relu, A, offs)
            what = "%s %s relu %d fill 0x%02x offs %s" % (pi.row_id(k), ep, relu, fill, offs)
            A.check(what)
            for name, a, b in zip(("out", "codes", "status"), got, plain):
                assert (a is None) == (b is None)
                if a is not None:
                    assert arena.same_bytes(a, b), "%s: %s differs from the plain call" % (what, name)
    assert int(plain[2].item()) == 0


MODULE_CASES = [(form, shape, which) for form in ("relu", "relu_inplace", "maxpool321", "maxpool2", "avg11", "avg57")
                for shape, which in (((2, 3, 7, 7), (8, 0, True)), ((1, 2, 5, 33), (4, 0, False)), ((3, 17, 8, 8), (8, 1, False)))]


def _run_module(form, shape, which, A=None, offs=(0, 0)):
    scale, zero, lo, hi = pi.module_quantiser(shape, which)
    place = _placer(A)
    x = place(pi.module_input(shape, seed=7, nonfinite=True), offs[0], "x", inplace=form == "relu_inplace")
    rq = capi.requant(place(scale, name="scale"), place(zero, name="zero"), lo, hi, 8, 0)
    N, C, H, W = shape
    if form == "relu_inplace":
        return capi.quant_relu(x, rq, out=x)
    oshape = {"relu": shape, "maxpool321": (N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1), "maxpool2": (N, C, H // 2, W // 2),
              "avg11": (N, C, 1, 1), "avg57": (N, C, 5, 7)}[form]
    out = torch.empty(oshape, dtype=torch.float32, device=DEV) if A is None else A.blank(oshape, torch.float32, off=offs[1], name="out")
    if form == "relu":
        return capi.quant_relu(x, rq, out=out)
    if form.startswith("maxpool"):
        return capi.quant_maxpool2d(x, rq, *((3, 2, 1) if form == "maxpool321" else (2, 2, 0)), out=out)
    return capi.quant_adaptive_avgpool2d(x, rq, (1, 1) if form == "avg11" else (5, 7), out=out)


@pytest.mark.parametrize("form,shape,which", MODULE_CASES,
                         ids=["%s-%s-%d%s%s" % (f, "x".join(map(str, s)), w[0], "su"[1 - w[1]], "c" if w[2] else "") for f, s, w in MODULE_CASES])
def test_module_form_contract(form, shape, which):
    plain = _run_module(form, shape, which)
    for offs in ((0, 0), (4, 4), (12, 8)):
        for fill in arena.FILLS:
            A = arena.Arena(DEV, fill)
            got = _run_module(form, shape, which, A, offs)
            what = "%s %s fill 0x%02x offs %s" % (form, shape, fill, offs)
            A.check(what)
            assert arena.same_bytes(got, plain), "%s: out differs from the plain call" % what
