"""k_period_find alone ON THE DEVICE: exactly the tables, the reference and the check of tests/test_period_cases_emulated.py
(tests/period_case_tables.py), through the same entry compiled by hipcc for gfx950 (tests/kernels/period_cases.hip ->
libblance_period_cases.so, made by __graft_entry__.build_period_cases).  Only that library is loaded here.  Below them the
other four kernels of the form alone and the form as a whole against one sequential walk (tests/period_kernel_cases.py)."""
import pytest

import period_case_tables as T
import period_kernel_cases as K

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


# ---- the other four kernels alone, and the form as a whole: the tables, references and checks of tests/period_kernel_cases.py ----


@pytest.fixture(scope="module")
def pk():
    import __graft_entry__ as entry
    return K.PeriodKernels(entry.build_period_cases())


@pytest.mark.parametrize("name", list(K.VERIFY_CASES))
def test_verify_alone(pk, name):
    K.check_verify(pk, name)


@pytest.mark.parametrize("cut", K.SEGMENT_CUTS)
def test_segments_alone(pk, cut):
    K.check_segments(pk, len(K.SEGMENT_REGIONS), cut, 64)
    K.check_segments(pk, 65, cut, 64)
    K.check_segments(pk, 65, cut, 256)


@pytest.mark.parametrize("threads", [128, 64, 256])
@pytest.mark.parametrize("name", list(K.JUDGE_TABLES))
def test_judge_alone(pk, name, threads):
    K.check_judge(pk, name, threads)


@pytest.mark.parametrize("threads", [128, 64])
@pytest.mark.parametrize("name", ["rests", "refusals", "picks_to_skip", "wide"])
def test_judge_refuses_behind_an_escape(pk, name, threads):
    assert not any(K.check_judge(pk, name, threads, escaped=1))
    assert not any(K.check_judge(pk, name, threads, escaped=-5))


@pytest.mark.parametrize("OW", [2, 3, 4, 5])
@pytest.mark.parametrize("name", list(K.REPLICATE_TABLES))
def test_replicate_alone(pk, name, OW):
    K.check_replicate(pk, name, OW)
    if name == "three_regions":
        K.check_replicate(pk, name, OW, threads=64)


def test_entries_refuse_tables_out_of_bounds(pk):
    K.check_entry_refusals(pk)


@pytest.mark.parametrize("name", K.PIPELINE_FIND_TABLES)
def test_form_on_the_find_tables(pk, name):
    w, init = K.world_of_find_table(name, k=2)
    K.check_pipeline(pk, w, init)


@pytest.mark.parametrize("threads", [128, 64])
@pytest.mark.parametrize("name", list(K.PIPELINE_WORLDS))
def test_form_against_one_walk(pk, name, threads):
    w, init, cut = K.pipeline_world(name)
    K.check_pipeline(pk, w, init, cut, judge_threads=threads)


@pytest.mark.parametrize("seed", K.RANDOM_SEEDS)
def test_form_on_random_worlds(pk, seed):
    w, init = K.random_world(seed)
    K.check_pipeline(pk, w, init)
