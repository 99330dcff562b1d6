"""The bulk primitives one kernel at a time ON THE DEVICE: exactly the tables, references and checks of
tests/test_kernel_cases_emulated.py (tests/kernel_case_tables.py), through the same entries compiled by hipcc for gfx950
(tests/kernels/kernel_cases.hip -> libblance_kernel_cases.so, made by __graft_entry__.build_kernel_cases) -- on real wave64
hardware, where ballots, __shfl_up and LDS atomics are the real thing.  Only that library is loaded here."""
import pytest

import kernel_case_tables as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kc():
    import __graft_entry__ as entry
    return T.KernelCases(entry.build_kernel_cases())


@pytest.mark.parametrize("n", T.SCAN_SIZES)
def test_scan_excl(kc, n):
    T.check_scan(kc, n)


@pytest.mark.parametrize("n", T.PART_SIZES)
def test_group_by_key(kc, n):
    T.check_group_by_key(kc, n)


def test_group_by_key_refuses_a_key_out_of_range(kc):
    T.check_group_by_key_refuses(kc)


@pytest.mark.parametrize("n", T.PART_SIZES)
def test_partition_category(kc, n):
    T.check_partition_category(kc, n)


@pytest.mark.parametrize("n", T.SORT_SIZES)
def test_radix_sort_pairs(kc, n):
    T.check_radix(kc, n)


def test_radix_sort_orders_doubles(kc):
    T.check_radix_doubles_order(kc)


def test_radix_sort_tiled_histogram_scan(kc):
    T.check_radix_big(kc)


@pytest.mark.parametrize("n", T.VARBITS_SIZES)
def test_sort_varbits(kc, n):
    T.check_varbits(kc, n)


@pytest.mark.parametrize("n_waves", T.SCAN_MIN_WAVES)
def test_flat_scan_min(kc, n_waves):
    T.check_flat_scan_min(kc, n_waves)


@pytest.mark.parametrize("P", T.ROW_COUNT_P)
def test_flat_row_count(kc, P):
    T.check_flat_row_count(kc, P)


@pytest.mark.parametrize("N", T.FRESH_N)
def test_fresh_selection(kc, N):
    T.check_fresh(kc, N)


def test_fresh_selection_refuses_what_validation_excludes(kc):
    T.check_fresh_refuses(kc)


@pytest.mark.parametrize("N,mask,RS", T.CYCLE_SHAPES)
def test_fresh_cycle_is_the_general_path(kc, N, mask, RS):
    T.check_fresh_cycle(kc, N, mask, RS)


@pytest.mark.parametrize("R", T.EXCL_R)
def test_fresh_exclusion_automaton(kc, R):
    T.check_excl(kc, R)


@pytest.mark.parametrize("N", T.PREPARE_N)
def test_flat_prepare(kc, N):
    T.check_flat_prepare(kc, N)


@pytest.mark.parametrize("group", T.STAY_GROUPS)
def test_flat_scan_stay_table(kc, group):
    T.check_flat_scan_table(kc, "stay", group)


@pytest.mark.parametrize("group", T.FRESH_GROUPS)
def test_flat_scan_fresh_table(kc, group):
    T.check_flat_scan_table(kc, "fresh", group)


@pytest.mark.parametrize("P", T.FLAT_SCAN_P)
def test_flat_scan_geometry(kc, P):
    T.check_flat_scan_geometry(kc, P)


@pytest.mark.parametrize("group", T.STAY_GROUPS)
def test_flat_stay_live(kc, group):
    T.check_flat_stay_live(kc, group)


def test_flat_stay_live_stickiness_sources(kc):
    T.check_flat_stay_live_stickiness(kc)


@pytest.mark.parametrize("P", T.COMMIT_P)
def test_flat_commit_stay(kc, P):
    T.check_flat_commit_stay(kc, P)


def test_flat_entries_refuse_what_a_kernel_would_index_with(kc):
    T.check_flat_refusals(kc)
