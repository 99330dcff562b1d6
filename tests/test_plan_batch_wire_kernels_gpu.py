"""k_batch_wire_size and k_batch_wire_write alone ON THE DEVICE: exactly the cases, the definition and the check of
tests/test_plan_batch_wire_kernels_emulated.py (tests/batch_wire_cases.py), through the same entry compiled by hipcc for gfx950
(tests/kernels/batch_wire_cases.hip -> libblance_batch_wire_cases.so, made by __graft_entry__.build_batch_wire_cases).  Only
that library is loaded here.  The file's name puts it behind tests/test_hip_parity.py in the suite's one process on purpose: a
further code-object library loaded in front of that file's RCCL tests is what DESIGN.md 4.14 saw ncclCommInitRank trip over."""
import ctypes

import pytest

import batch_wire_cases as K

pytestmark = pytest.mark.gpu
WORLDS = K.worlds()


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    return ctypes.CDLL(entry.build_batch_wire_cases())


@pytest.mark.parametrize("which", [3, 1, 2])
@pytest.mark.parametrize("name", sorted(WORLDS))
def test_kernels_against_the_definition(lib, name, which):
    K.check(lib, WORLDS[name], which)
