"""CPU: the host side of qe_quantconv2d_awq_fused: the exports, the path of a table of requests and its independence of alignment,
the code of every refused request.  The addresses are numbers, not memory: every request is a host-only query or is refused."""
import ctypes
import os
import re

import pytest

from quantize_amd import capi

from test_conv_awq_cpu import ARG, NBITS, _request

OUT, CODES, IDENT, STATUS = 1 << 20, 1 << 21, 1 << 22, 1 << 23
PLAIN = [dict(k=3, padding=1), dict(stride=2), dict(w_bits=3), dict(G=48, IC=96)]


def RQ(bits=8, n=1, scale=1 << 16):
    return capi.QeRequant(scale, (1 << 16) + 4096, n, 0.0, 255.0, bits, 0)


def _path(kw, rq=None, out=OUT, codes=CODES, identity=None, status=None):
    xq, wq, G, sh = _request(**kw)
    return capi.conv_awq_fused_path(xq, wq, G, sh, identity=identity, relu=True, out=out, rq=rq, codes=codes if rq is not None else None,
                                    status=status)


def test_symbols_and_header():
    for name in ("qe_quantconv2d_awq_fused", "qe_quantconv2d_awq_fused_path"):
        assert name in capi.PROTOTYPES and name in capi.SYMBOLS and hasattr(capi.lib(), name)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "quant_engine.h")).read()
    assert not re.findall(r"qe_\w*awq\w*(?:workspace_bytes|prepared_bytes)", header)      # no workspace, no prepared tables


@pytest.mark.parametrize("kw,rq,out,path", [(dict(), None, OUT, 1), (dict(), RQ(), OUT, 1), (dict(), RQ(n=8), None, 1)] +
                         [(kw, RQ(n=8), OUT, 0) for kw in PLAIN] + [(dict(), RQ(4), OUT, 0), (dict(), RQ(4), None, -1), (PLAIN[0], RQ(4), None, -1)])
def test_path_is_answered_on_the_host(kw, rq, out, path):
    assert _path(kw, rq, out) == path
    if out is not None:         # one element / one byte off, and in place: the same answer
        assert _path(kw, rq, OUT + 4, CODES + 1, IDENT + 4) == _path(kw, rq, OUT, CODES, IDENT) == _path(kw, rq, OUT, CODES, OUT) == path


# two faults at once where the order matters: (request, call keywords, code)
REFUSED = {"conv check first": (dict(w_bits=0), dict(out=None), NBITS), "no output": (dict(), dict(out=None), ARG),
           "codes without rq": (dict(), dict(codes=CODES), ARG), "rq without codes": (dict(), dict(rq=RQ()), ARG),
           "rq.scale before n_bits": (dict(), dict(rq=RQ(9, scale=0), codes=CODES), ARG),
           "rq.n_bits before n_param": (dict(), dict(rq=RQ(9, n=3), codes=CODES), NBITS), "rq.n_param": (dict(), dict(rq=RQ(n=3), codes=CODES), ARG),
           "out over x": (dict(), dict(out=8192), ARG), "codes over out": (dict(), dict(rq=RQ(), codes=OUT + 16), ARG),
           "identity over out": (dict(), dict(identity=OUT + 4), ARG), "identity over codes": (dict(), dict(rq=RQ(), codes=IDENT + 4, identity=IDENT), ARG),
           "status over codes": (dict(), dict(rq=RQ(), codes=CODES, status=CODES), ARG),
           "overlap before sub-8-bit": (dict(), dict(rq=RQ(4), codes=8192, out=None), ARG),
           "sub-8-bit without out": (dict(), dict(rq=RQ(4), codes=CODES, out=None), capi.QE_ERR_UNSUPPORTED)}


@pytest.mark.parametrize("what", list(REFUSED))
def test_refused_requests(what):
    kw, call, code = REFUSED[what]
    xq, wq, G, sh = _request(**kw)
    c = dict(dict(identity=None, out=OUT, rq=None, codes=None, status=None), **call)
    rq = None if c["rq"] is None else ctypes.byref(c["rq"])
    head = (ctypes.byref(xq), ctypes.byref(wq), G, 0, 0)
    L = capi.lib()
    assert L.qe_quantconv2d_awq_fused(*head, None, ctypes.byref(sh), c["identity"], 1, c["out"], rq, c["codes"], c["status"], None) == code
    assert L.qe_quantconv2d_awq_fused_path(*head, ctypes.byref(sh), c["identity"], 1, c["out"], rq, c["codes"], c["status"]) == -1
