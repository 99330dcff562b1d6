"""The sweep's record, category, bit-map, list-edit and tail kernels one at a time, under the SIMT emulator: k_gather (every
record width up to the 64 words validation admits), k_category, k_ntn_bits, k_invert, k_chain_classify + k_chain_ev_fill + k_chain_orphans, k_gather_chain, and the sweep's end both ways --
k_scatter, k_converge, k_count_prev, k_live_refresh against k_invert + k_sweep_tail -- on hand-made problems, against plain
references (tests/sweep_case_tables.py has the tables, the references and the checks; tests/test_sweep_cases_gpu.py runs the
same on the device)."""
import pytest

import kernel_case_tables as T
import sweep_case_tables as S
from test_kernel_cases_emulated import build_emu_cases


@pytest.fixture(scope="module")
def kc():
    return S.ChainCases(build_emu_cases())


def test_category_table(kc):
    S.check_category_table(kc)


@pytest.mark.parametrize("P", S.GEOM_P)
def test_category_geometry(kc, P):
    S.check_category_geometry(kc, P)


@pytest.mark.parametrize("P", S.GEOM_P)
def test_gather_geometry(kc, P):
    S.check_gather_geometry(kc, P)


@pytest.mark.parametrize("P", S.GATHER_WIDE_P)
@pytest.mark.parametrize("M,L", S.GATHER_WIDE)
def test_gather_widest_records(kc, M, L, P):
    S.check_gather_wide(kc, M, L, P)


def test_gather_header(kc):
    S.check_gather_header(kc)


@pytest.mark.parametrize("P", T.ROW_COUNT_P)
def test_gather_row_count(kc, P):
    S.check_gather_row_count(kc, P)


@pytest.mark.parametrize("N", S.BITS_N)
def test_ntn_bits(kc, N):
    S.check_ntn_bits(kc, N)


@pytest.mark.parametrize("n", S.GEOM_P)
def test_invert(kc, n):
    S.check_invert(kc, n)


@pytest.mark.parametrize("name", sorted(S.CHAIN_STEPS))
def test_chain_step(kc, name):
    S.check_chain_step(kc, name)


@pytest.mark.parametrize("P", S.GEOM_P)
def test_chain_geometry(kc, P):
    S.check_chain_geometry(kc, P)


def test_chain_event_counts(kc):
    S.check_chain_events_counts(kc)


def test_gather_chain_flat(kc):
    S.check_chain_flat(kc)


def test_chain_closed_gate(kc):
    S.check_chain_gate(kc)


def test_chain_entries_refuse_what_a_kernel_would_index_with(kc):
    S.check_chain_refusals(kc)


def test_list_edits(kc):
    S.check_list_edits(kc)


def test_converge_all_equal(kc):
    S.check_converge_all_equal(kc)


@pytest.mark.parametrize("name", sorted(S.DIFF_CASES))
def test_converge_one_difference(kc, name):
    S.check_converge_case(kc, name)


@pytest.mark.parametrize("P,p", S.CONVERGE_SEAMS)
def test_converge_wave_seams(kc, P, p):
    S.check_converge_seam(kc, P, p)


def test_converge_word_set_on_entry(kc):
    S.check_converge_word_set_on_entry(kc)


@pytest.mark.parametrize("P", S.GEOM_P)
def test_sweep_end_geometry(kc, P):
    S.check_sweep_end_geometry(kc, P)


def test_sweep_end_closed_gate(kc):
    S.check_sweep_end_gate(kc)


def test_sweep_entries_refuse_what_a_kernel_would_index_with(kc):
    S.check_sweep_refusals(kc)
