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
