"""Stage 1 of the device decoder alone ON THE DEVICE: exactly the documents, the definition and the check of
tests/test_wire_decode_kernels_emulated.py (tests/wire_decode_cases.py), through the same entry compiled by hipcc for gfx950
(tests/kernels/wire_decode_cases.hip -> libblance_wire_decode_cases.so, made by __graft_entry__.build_wire_decode_cases).  Only
that library is loaded here."""
import pytest

import wire_decode_cases as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sc():
    import __graft_entry__ as entry
    return W.SplitCases(entry.build_wire_decode_cases())


def test_split_is_the_definition(sc):
    assert W.run_split_cases(sc) > 60


def test_entry_refuses_bad_tiles(sc):
    W.check_split_refusals(sc)
