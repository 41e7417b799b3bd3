"""GPU: the memory contract of qe_affine_relu_quantize_pack inside poisoned arenas (tests/arena.py), on the pattern of
tests/test_pool_mem_contract_gpu.py: one row per instance where its pieces reach an edge, in every output form.

Every buffer the call sees -- x, identity, alpha, shift, each consumer's scale and zero, sum_out, act_out, each code stream,
status -- lies between guard bands, once in an arena of 0x00 and once in one of 0xFF (NaN as fp32, code 255):
  * no guard byte and no input byte changes, except the in-place target (sum_out == identity or sum_out == x);
  * the outputs equal the plain call's byte for byte under both fills, so every output byte was written (the payloads are
    pre-filled too) and none depends on what surrounds the buffers;
  * the path query names the same instance whatever the addresses.
The fp32 buffers are also placed 4 and 12 bytes off a 256-byte boundary and the code streams 1 and 3 bytes off."""
import numpy as np
import pytest
import torch

import arena
import preact_instances as pi
from quantize_amd import capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.array(a, copy=True)).to(DEV)          # the shared operands are read-only


def _first(pred):
    return next(k for k, r in enumerate(pi.ROWS) if pred(r))


# fast on the smallest plane (one thread per plane) and on 256-element planes; plain on a one-element plane, on planes that are no
# multiple of 8 (a ragged last group) and packing 4-bit and 1-bit codes
ROWS = (_first(lambda r: r[0] == "fast" and r[1] == (2, 3, 16)), _first(lambda r: r[0] == "fast" and r[1] == (2, 3, 256)),
        _first(lambda r: r[1] == (2, 3, 1)), _first(lambda r: r[1] == (2, 5, 17)), _first(lambda r: r[2] == ("s4c", "u1")),
        _first(lambda r: r[2] == ("s1", "u4")))
# each in-place target, both fp32 outputs together, each alone, and codes only; with and without identity
FORMS = ((True, "identity", True), (True, "x", False), (True, "new", True), (False, None, True), (False, "x", False), (True, None, False))
assert set(FORMS) <= set(pi.FORMS)
CASES = [(k, form, n_out) for k in ROWS for form in FORMS for n_out in (0, 2) if n_out or form[1] or form[2]]


def _run(k, form, n_out, A=None, offs=(0, 0)):
    ident, smode, act = form
    inst, (N, C, P), _ = pi.ROWS[k]
    o, cons = pi.operands(k), pi.consumers(k)[:n_out]
    fo, co = offs
    if A is None:
        place = lambda a, off=0, name=None, inplace=False: _t(a)
        blank = lambda shape, dtype, off, name: torch.empty(shape, dtype=dtype, device=DEV)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
    else:
        place = lambda a, off=0, name=None, inplace=False: A.place(_t(a), off=off, name=name, inplace=inplace)
        blank = lambda shape, dtype, off, name: A.blank(shape, dtype, off=off, name=name)
        status = A.status()
    x = place(o["x"].reshape(N, C, 1, P), fo, "x", inplace=smode == "x")
    identity = place(o["identity"].reshape(N, C, 1, P), fo, "identity", inplace=smode == "identity") if ident else None
    rqs = [capi.requant(place(s, name="rq%d scale" % i), place(z, name="rq%d zero" % i), lo, hi, bits, sign)
           for i, (s, z, lo, hi, bits, sign) in enumerate(cons)]
    sum_out = {None: None, "identity": identity, "x": x}.get(smode, False)
    if sum_out is False:
        sum_out = blank((N, C, 1, P), torch.float32, fo, "sum_out")
    act_out = blank((N, C, 1, P), torch.float32, fo, "act_out") if act else None
    codes = [blank((capi.packed_nbytes(N * C * P, r.n_bits),), torch.uint8, co, "codes %d" % i) for i, r in enumerate(rqs)]
    got, s, a, status = capi.affine_relu_quantize_pack(x, place(o["alpha"], name="alpha"), place(o["shift"], name="shift"),
                                                       identity=identity, rqs=rqs, sum_out=sum_out, act_out=act_out, codes=codes,
                                                       status=status)
    path = capi.affine_relu_quantize_pack_path(N, C, P, rqs, sum_out=0 if s is None else s.data_ptr(), act_out=0 if a is None else a.data_ptr())
    return [s, a, status] + list(got), path


@pytest.mark.parametrize("k,form,n_out", CASES, ids=["%s-%s-n%d" % (pi.row_id(k), pi.form_id(f), n) for k, f, n in CASES])
def test_affine_relu_quantize_pack_contract(k, form, n_out):
    plain, path = _run(k, form, n_out)
    assert capi.PREACT_KERNELS[path] == pi.expected_instance(k, n_out)
    for offs in ((0, 0), (4, 1), (12, 3)):
        for fill in arena.FILLS:
            A = arena.Arena(DEV, fill)
            got, p = _run(k, form, n_out, A, offs)
            what = "%s %s n_out %d fill 0x%02x offs %s" % (pi.row_id(k), pi.form_id(form), n_out, fill, offs)
            A.check(what)
            assert p == path, what
            for i, (a, b) in enumerate(zip(got, plain)):
                assert (a is None) == (b is None)
                if a is not None:
                    assert arena.same_bytes(a, b), "%s: output %d differs from the plain call" % (what, i)
    assert int(plain[2].item()) == 0
