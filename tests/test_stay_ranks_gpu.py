"""k_stay_by_top's rank function alone ON THE DEVICE: exactly the cases, the reference and the check of
tests/test_stay_ranks_emulated.py (tests/stay_rank_tables.py), through the same entry compiled by hipcc for gfx950
(tests/kernels/stay_rank_cases.hip -> libblance_stay_rank_cases.so, made by __graft_entry__.build_stay_rank_cases) -- on a
real wave64, where a ballot is one v_cmp.  Only that library is loaded here."""
import pytest

import stay_rank_tables as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rc():
    import __graft_entry__ as entry
    return T.RankCases(entry.build_stay_rank_cases())


@pytest.mark.parametrize("size", T.SIZES)
@pytest.mark.parametrize("km", T.KMS)
def test_round_ranks(rc, km, size):
    T.check(rc, km, size)


def test_entry_refuses_leaves_outside_the_region(rc):
    T.check_refusals(rc)
