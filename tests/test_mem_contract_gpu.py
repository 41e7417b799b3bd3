"""GPU: the memory contract of every entry point of the C ABI (the table of tests/mem_cases.py) inside poisoned arenas.

Each entry runs three times -- on ordinary tensors, and with every buffer (inputs, scale / zero arrays, bias, masks,
outputs, workspaces and prepared tables of exactly the queried size, status words) inside a 0x00 and a 0xFF arena
(tests/arena.py):
  (a) no guard byte and no input byte changes;
  (b) the arena outputs equal the plain ones byte for byte under both pre-fills, so every output byte was written and
      none depends on what surrounds the buffers;
  (c) the plan / form / path query, asked with each call's own pointers, names the same kernel -- on aligned buffers the
      instance the table records;
and the plain outputs meet float64 on every element under the family's existing rule.  Entries whose path query looks at
a pointer run once more with that buffer at the smallest offset its element type allows.  An entry the library refuses
(LayerNorm at E = 66) must raise in all three calls and leave every byte of every buffer alone."""
import pytest

import mem_cases as mc

pytestmark = pytest.mark.gpu
CASES = mc.all_cases()
OFFSET = [c for c in CASES if c.offsets]


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_contract(case):
    plain = mc.run_contract(case)
    if plain is not None:
        case.check_ref(plain)


@pytest.mark.parametrize("case", OFFSET, ids=[c.id for c in OFFSET])
def test_contract_off_alignment(case):
    """The pointer the path query looks at -- re-quantised codes, the first LayerNorm codes (1 byte), bf16 `out`, bf16-input
    `x` (2 bytes) -- off a 256-byte boundary: the query with this pointer and the call agree (the call succeeds on the
    workspace that query sized), and the result still meets float64."""
    plain = mc.run_contract(case, offs=case.offsets)
    if plain is not None:
        case.check_ref(plain)
