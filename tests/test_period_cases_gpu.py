"""k_period_find alone ON THE DEVICE: exactly the tables, the reference and the check of tests/test_period_cases_emulated.py
(tests/period_case_tables.py), through the same entry compiled by hipcc for gfx950 (tests/kernels/period_cases.hip ->
libblance_period_cases.so, made by __graft_entry__.build_period_cases).  Only that library is loaded here."""
import pytest

import period_case_tables as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pc():
    import __graft_entry__ as entry
    return T.PeriodCases(entry.build_period_cases())


@pytest.mark.parametrize("name", list(T.TABLES))
def test_known_mode_is_the_search(pc, name):
    T.check(pc, name)


def test_entry_refuses_tables_out_of_bounds(pc):
    T.check_refusals(pc)
