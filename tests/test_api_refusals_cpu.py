"""CPU: the code every refused C-ABI request returns, pinned row by row (tests/api_refusal_table.py).

The order of the host checks decides which code a caller sees when a request has more than one fault, so the rows carry two
faults at once and the codes are the ones the library returned BEFORE the checks were gathered into csrc/qe_request.hpp.

The table's addresses are numbers, not memory.  That is safe only because no row reaches a launch: every row is refused by
a host check or names no element, and the first test asserts that of the table itself.  On a machine with a GPU a row that
a broken check wrongly accepted would launch a kernel on a bogus pointer, so the whole module skips there: it is a test of
host code and loses nothing by running where there is no device.
"""
import ctypes

import pytest
import torch

from quantize_amd import capi

from api_refusal_table import CALLS, OK, QUERIES

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="fake addresses: a wrongly accepted row would launch on them")

QE_ERR_HIP = 5


def _call(symbol, args):
    return getattr(capi.lib(), symbol)(*(ctypes.byref(a) if isinstance(a, ctypes.Structure) else a for a in args))


def test_no_row_can_reach_a_launch():
    """The condition on the table: a call row is refused, or answers QE_OK for an output of 0 elements; a query row answers
    0 or -1 (a bad request) or a code.  No expected code is QE_ERR_HIP, which only a HIP call can produce."""
    ids = [r[0] for r in CALLS] + [r[0] for r in QUERIES]
    assert len(ids) == len(set(ids))
    for name, symbol, _, code, elements in CALLS:
        assert symbol in capi.PROTOTYPES, name
        assert code != QE_ERR_HIP, name
        assert code != OK or elements == 0, name
    for name, symbol, _, answer in QUERIES:
        assert symbol in capi.PROTOTYPES, name
        assert symbol.endswith(("_path", "_bytes", "_layout", "_plan_info", "_has_instance")), name
        assert answer in (0, -1) or (symbol.endswith("_plan_info") and answer != QE_ERR_HIP), name


@pytest.mark.parametrize("name,symbol,args,code", [r[:4] for r in CALLS] + QUERIES, ids=lambda v: v if isinstance(v, str) and "." in v else "")
def test_refusal_code(name, symbol, args, code):
    assert _call(symbol, args) == code, name
