"""The bulk primitives one kernel at a time, under the SIMT emulator: the exclusive scan, the stable counting sort (int32
keys and the category form), the stable 64-bit radix sort, k_flat_scan_min / k_flat_row_count, the fresh-run selection and
the exclusion automaton -- at the sizes on both sides of every tile, chunk, round, slice and workgroup seam --, and the flat
pass's certain-stay decision: k_flat_prepare, k_flat_scan (both predicates, every table step alone in its wave),
k_flat_prepare_count_live + k_flat_stay_live over the same tables as live lists, k_flat_commit_stay; against plain
references (tests/kernel_case_tables.py has the tables, the references and the checks; tests/test_kernel_cases_gpu.py
runs the same on the device).

n = 0 is not a case of the scan: no call site passes it.  The driver scans P + 1 or PM + 1 words (events, downloads, moves),
256 histogram words per sort tile of a run of at least one element, and B * cdiv(n, 1024) bucket counts of a grouping or a
category partition that only runs with P > 0.

The exclusion table on the references alone (test_excl_table_exercises_both_outcomes): of 135 cases with exclusions, 123
run to the end and 12 end early at a bad step.  The stay and fresh tables (test_flat_tables_have_both_outcomes): every
group has steps that pass its predicate and steps that fail it."""
import os
import subprocess

import pytest

import kernel_case_tables as T
from test_simt_emulated import HERE, _deps

SRC = os.path.join(HERE, "simt", "emu_kernel_cases.cpp")
INC = os.path.join(HERE, "kernels", "kernel_cases.inc")
INC_SWEEP = os.path.join(HERE, "kernels", "sweep_cases.inc")
SO = os.path.join(HERE, "simt", "_build", "libblance_emu_kernel_cases.so")


def build_emu_cases():
    """The emulator library with the entries (tests/test_fewer_launches_kernels_emulated.py loads the same file).  Workers
    of one run take turns at a lock: one compiles, under a name of its own that is moved into place whole, the others find
    it made."""
    import fcntl
    deps = _deps() + [SRC, INC, INC_SWEEP]
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    with open(SO + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
            tmp = "%s.%d.tmp" % (SO, os.getpid())
            subprocess.check_call(["g++", "-x", "c++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off",
                                   "-Wno-unknown-pragmas", "-o", tmp, SRC])
            os.replace(tmp, SO)
    return SO


@pytest.fixture(scope="module")
def kc():
    return T.KernelCases(build_emu_cases())


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


def test_excl_table_exercises_both_outcomes():
    """On the references alone, so that the bad-step logic cannot hide a failure: at least a third of the cases with
    exclusions run to the end, at least five end early (123 and 12 of 135)."""
    to_end, early = T.excl_reference_counts()
    assert 3 * to_end >= to_end + early
    assert early >= 5
    assert (to_end, early) == (123, 12)


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


@pytest.mark.parametrize("kind,group", [("stay", g) for g in T.STAY_GROUPS] + [("fresh", g) for g in T.FRESH_GROUPS])
def test_flat_tables_have_both_outcomes(kind, group):
    """On the references alone: in every group of the stay and the fresh table some listed step passes the predicate and
    some step fails it, and every listed step is the only one of its wave that can fail (T.table_outcomes)."""
    yes, no = T.table_outcomes(kind, group)
    assert yes >= 1 and no >= 1
