"""blance_plan_batch_wire on the MI355X: k_plan_batch + k_batch_wire_size + k_batch_wire_write against the host encoder, json
and the single path (blance_plan, blance_plan_wire_names, blance_plan_wire_get); the plans against blance_plan_batch and the
C oracle.  The cases are those of test_plan_batch_wire_emulated.py."""
import pytest

from blance_amd import hip, synth
from test_plan_batch_stats_emulated import both_classes, edge_problems, random_problems
from test_plan_batch_wire_emulated import (STAGES, run_context_holds_nothing, run_docs, run_empty_map, run_escapes, run_fallback,
                                           run_golden, run_residues, run_seams, run_small_stage, run_some_ask,
                                           run_untouched_tails, run_with_moves_and_stats)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def batch_planner():
    pl = hip.Planner(device_id=0)
    yield pl
    pl.close()


def test_golden_cases_one_batch(batch_planner, golden_cases):
    run_golden(batch_planner, golden_cases)


def test_random_and_edge_cases(batch_planner):
    fps = random_problems()
    _, _, _, info, _ = run_docs(batch_planner, fps, "random")
    assert info["n_batched"] == len(fps) and info["n_fallback"] == 0
    edges = edge_problems()
    _, _, _, info, _ = run_docs(batch_planner, edges, "edge", single=len(edges))
    assert info["n_batched"] + info["n_fallback"] == len(edges)


def test_both_size_classes(batch_planner):
    fps = both_classes()
    _, _, _, info, winfo = run_docs(batch_planner, fps, "classes")
    assert info["n_batched"] == 16 and winfo["kernel_launches"] == 2 and info["kernel_launches"] == 4
    assert sum(fp.n_nodes_ext > 64 for fp in fps) >= 2 and sum(fp.n_nodes_ext <= 64 for fp in fps) >= 2


def test_partition_counts_at_the_seams(batch_planner):
    run_seams(batch_planner)


def test_escapes(batch_planner):
    run_escapes(batch_planner)


@pytest.mark.parametrize("stage", STAGES)
def test_small_stage(monkeypatch, batch_planner, stage):
    run_small_stage(lambda: hip.Planner(device_id=0), monkeypatch, batch_planner, stage)


def test_every_length_residue(batch_planner):
    run_residues(batch_planner)


def test_untouched_tails(batch_planner):
    run_untouched_tails(batch_planner)


def test_some_ask_some_do_not(batch_planner):
    run_some_ask(batch_planner)


def test_with_moves_and_statistics_in_the_same_call(batch_planner):
    run_with_moves_and_stats(batch_planner)


def test_batch_with_fallback_problems(batch_planner):
    run_fallback(batch_planner, 200, 300, synth.cbgt_batch(6, seed=7, P_range=(20, 300), N_range=(30, 200)))


def test_empty_map(batch_planner):
    run_empty_map(batch_planner)


def test_context_holds_no_problem_and_no_names_afterwards(batch_planner):
    run_context_holds_nothing(batch_planner)


def test_cbgt_64_default_shape(batch_planner):
    fps = synth.cbgt_batch(64, seed=2)
    _, docs, _, info, _ = run_docs(batch_planner, fps, "cbgt 64", single=4, oracle=8)
    assert info["n_batched"] == 64 and info["n_fallback"] == 0 and info["kernel_launches"] <= 4
    assert all(len(d) > 2 for d in docs)
