"""GPU: the memory contract of qe_quantconv2d_grouped inside poisoned arenas (tests/arena.py), one problem per kernel instance.

Every buffer the call sees -- x, w, both scales and zeros, bias, the consumer's scale and zero, out, codes, status -- lies
between guard bands, once in an arena of 0x00 and once in one of 0xFF:
  * no guard byte and no input byte changes;
  * out and codes equal the plain call's byte for byte under both fills, so every output byte was written (the payloads are
    pre-filled too) and none depends on what surrounds the buffers -- the fast kernels' 16-byte chunks reach past both ends
    of a channel's span, into the guards of x, and must neither fault nor let a neighbour's byte into a sum.
x, out and codes are also placed off a 256-byte boundary (x at +1 and +7, out at +4, codes at +3)."""
import numpy as np
import pytest
import torch

import arena
import grp_instances as gi
from quantize_amd import capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = ("out", "codes", "both")


def _first(pred):
    return next(k for k, r in enumerate(gi.rows()) if pred(r))


# (row, epilogue): each of the 24 fast instances (Cg x stride x epilogue) on a partial-last-slab problem of two images, the
# band problem of each stride at Cg = 4, the plain kernel in each epilogue, and the two-pass form
def _cases():
    out = []
    for cg in gi.FAST_CG:
        for s in (1, 2):
            k = _first(lambda r: r[0] == "fast" and r[3] == s and r[1][1] // r[8] == cg and r[1][0] == 2 and r[1][2:] == (9, 11))
            out += [(k, ep) for ep in EPS]
    for s in (1, 2):
        bands = _first(lambda r: r[0] == "fast" and r[3] == s and r[1][3] == 20 and gi.plan(r).tiles >= 2)
        out += [(bands, ep) for ep in EPS]
    plain = _first(lambda r: r[0] == "plain" and r[2] == (5, 5))
    low = _first(lambda r: r[0] == "plain" and r[5][0] == 4)
    for k in (plain, low):
        out += [(k, ep) for ep in EPS]
    out.append((_first(lambda r: r[0] == "fast" and r[1][2:] == (6, 9)), "sub8"))
    out.append((plain, "sub8"))
    return out


CASES = _cases()


def _run(k, ep, A=None, offs=(0, 0, 0)):
    row = gi.rows()[k]
    o = gi.operands(k, "parity")
    s, z, lo, hi, bits, sign = gi.consumer(k, "u4" if ep == "sub8" else "s8c", "parity")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    place = (lambda a, off=0, name=None: t(a)) if A is None else (lambda a, off=0, name=None: A.place(t(a), off=off, name=name))
    xq = capi.qparam(place(o["x"], offs[0], "x"), row[5][0], row[5][1], place(o["sx"], name="sx"), place(o["zx"], name="zx"))
    wq = capi.qparam(place(o["w"], name="w"), row[6][0], row[6][1], place(o["sw"], name="sw"), place(o["zw"], name="zw"))
    bias = None if o["bias"] is None else place(o["bias"], name="bias")
    sh = gi.shape_of(row)
    OH, OW = capi.out_hw(sh)
    n = sh.N * sh.OC * OH * OW
    rq = capi.requant(place(s, name="rq scale"), place(z, name="rq zero"), lo, hi, bits, sign) if ep != "out" else None
    if A is None:
        out = torch.empty((sh.N, sh.OC, OH, OW), dtype=torch.float32, device=DEV) if ep != "codes" else None
        codes = torch.empty(capi.packed_nbytes(n, bits), dtype=torch.uint8, device=DEV) if rq is not None else None
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
    else:
        out = A.blank((sh.N, sh.OC, OH, OW), torch.float32, off=offs[1], name="out") if ep != "codes" else None
        codes = A.blank(capi.packed_nbytes(n, bits), off=offs[2], name="codes") if rq is not None else None
        status = A.status()
    capi.quantconv2d_grouped(xq, wq, bias, sh, row[8], relu=True, rq=rq, out=out, codes=codes, status=status)
    return out, codes, status


def test_cases_name_every_instance():
    seen = {gi.expected_kernel(gi.rows()[k], EPS.index(ep)) for k, ep in CASES if ep in EPS}
    assert seen == set(range(25))


@pytest.mark.parametrize("k,ep", CASES, ids=["%s-%s" % (gi.row_id(k), ep) for k, ep in CASES])
def test_contract(k, ep):
    plain = _run(k, ep)
    for offs in ((0, 0, 0), (1, 4, 3), (7, 4, 3)):
        if gi.rows()[k][5][0] != 8 and offs[0]:
            continue
        for fill in arena.FILLS:
            A = arena.Arena(DEV, fill)
            got = _run(k, ep, A, offs)
            A.check("%s %s fill 0x%02x offs %s" % (gi.row_id(k), ep, fill, offs))
            for name, a, b in zip(("out", "codes", "status"), got, plain):
                assert (a is None) == (b is None)
                if a is not None:
                    assert arena.same_bytes(a, b), "%s %s fill 0x%02x offs %s: %s differs from the plain call" % (
                        gi.row_id(k), ep, fill, offs, name)
    assert int(plain[2].item()) == 0
