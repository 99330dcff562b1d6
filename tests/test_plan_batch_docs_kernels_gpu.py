"""k_batch_decode alone ON THE DEVICE: exactly the cases, the definition and the check of
tests/test_plan_batch_docs_kernels_emulated.py (tests/batch_decode_cases.py), through the same entry compiled by hipcc for gfx950
(tests/kernels/batch_decode_cases.hip -> libblance_batch_decode_cases.so, made by __graft_entry__.build_batch_decode_cases).
Only that library is loaded here.  The file's name puts it behind tests/test_hip_parity.py in the suite's one process on
purpose, as tests/test_plan_batch_wire_kernels_gpu.py's does."""
import ctypes

import pytest

import batch_decode_cases as K

pytestmark = pytest.mark.gpu
WORLDS = K.worlds()


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    return ctypes.CDLL(entry.build_batch_decode_cases())


@pytest.mark.parametrize("name", sorted(WORLDS))
def test_kernel_against_the_definition(lib, name):
    K.check(lib, WORLDS[name])
