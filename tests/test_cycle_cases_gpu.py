"""k_cycle_group and k_cycle_top alone ON THE DEVICE: exactly the worlds, the reference and the checks of
tests/test_cycle_cases_emulated.py (tests/cycle_case_tables.py), through the same entry compiled by hipcc for gfx950
(tests/kernels/cycle_cases.hip -> libblance_cycle_cases.so, made by __graft_entry__.build_cycle_cases).  Only that library is
loaded here."""
import pytest

import cycle_case_tables as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cc():
    import __graft_entry__ as entry
    return T.CycleCases(entry.build_cycle_cases())


@pytest.mark.parametrize("name", list(T.WORLDS))
def test_tables_give_the_sorts(cc, name):
    T.check(cc, name)


def test_events_and_orphans(cc):
    T.check_events_and_orphans(cc)


def test_closed_gate_writes_nothing(cc):
    T.check_closed_gate(cc)


def test_refute_knob_raises_not_local_only(cc):
    T.check_refute(cc)


def test_step_off_the_round_robin(cc):
    T.check_premise(cc)


def test_entry_refuses_tables_out_of_bounds(cc):
    T.check_refusals(cc)
