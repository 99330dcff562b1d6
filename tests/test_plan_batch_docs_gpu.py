"""blance_plan_batch_docs on the MI355X: k_batch_decode + k_plan_batch and the kernels behind it against the host decoder and
problem.wire_adopted_problem planned by blance_plan_batch_wire, the C oracle and the single route (upload, adopt_wire,
plan_resident); refusals against Planner.decode_wire, `why` codes against the definition and adopt_wire.  The cases are
those of test_plan_batch_docs_emulated.py."""
import pytest

from blance_amd import hip
from test_plan_batch_docs_emulated import (run_api, run_both_classes, run_context_holds_nothing, run_fallback, run_golden, run_mixed,
                                           run_mutants, run_partition_counts, run_random, run_refusals, run_round_trip, run_seams,
                                           run_whole_call_refusals, run_whys)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def batch_planner():
    pl = hip.Planner(device_id=0)
    yield pl
    pl.close()


@pytest.mark.parametrize("keep", [False, True])
def test_golden_documents(batch_planner, golden_cases, keep):
    run_golden(batch_planner, golden_cases, keep)


def test_random_documents(batch_planner):
    run_random(batch_planner)


def test_both_size_classes(batch_planner):
    run_both_classes(batch_planner)


def test_documents_that_are_not_the_plan(batch_planner):
    run_mutants(batch_planner)


@pytest.mark.parametrize("tile", [64, None])
def test_every_refusal_reason(monkeypatch, tile):
    """BLANCE_WIRE_IN_TILE is read when a context is made: a planner of its own."""
    run_refusals(lambda: hip.Planner(device_id=0), monkeypatch, tile)


@pytest.mark.parametrize("tile,stage", [(64, None), (None, None), (64, 64), (64, 256)])
def test_seams(monkeypatch, tile, stage):
    run_seams(lambda: hip.Planner(device_id=0), monkeypatch, tile, stage)


def test_partition_counts(batch_planner):
    run_partition_counts(batch_planner)


def test_why_codes(batch_planner):
    run_whys(batch_planner)


def test_mixed_batch(batch_planner):
    run_mixed(batch_planner)


def test_round_trip(batch_planner):
    run_round_trip(batch_planner)


def test_fallback_problems(batch_planner):
    run_fallback(batch_planner)


def test_context_holds_nothing(batch_planner):
    run_context_holds_nothing(batch_planner)


def test_whole_call_refusals(batch_planner):
    run_whole_call_refusals(batch_planner)


def test_plan_next_map_ex_batch_docs(batch_planner):
    run_api(batch_planner)
