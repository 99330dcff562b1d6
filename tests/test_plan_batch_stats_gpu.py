"""blance_plan_batch_stats on the MI355X: k_plan_batch + k_batch_stats against oracle.stats_ref and the single path
(blance_plan, then blance_plan_stats_get); the plans against blance_plan_batch and the C oracle."""
import numpy as np
import pytest

from blance_amd import hip, synth
from oracle import stats_ref
from test_plan_batch_stats_emulated import (both_classes, check_stats, edge_problems, fallback_problems, golden_problems,
                                            not_vacuous, random_problems, run_stats, same_plan, same_stats, sumsq_problem)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def batch_planner():
    pl = hip.Planner(device_id=0)
    yield pl
    pl.close()


def test_golden_cases_one_batch(batch_planner, golden_cases):
    fps = golden_problems(batch_planner, golden_cases)
    assert len(fps) >= 60
    _, stats, info, _ = run_stats(batch_planner, fps, "golden")
    assert info["n_batched"] == len(fps) and info["n_fallback"] == 0
    not_vacuous(fps, stats)


def test_random_and_edge_cases(batch_planner):
    fps = random_problems()
    _, stats, info, _ = run_stats(batch_planner, fps, "random")
    assert info["n_batched"] == len(fps) and info["n_fallback"] == 0
    not_vacuous(fps, stats)
    edges = edge_problems()
    _, stats, info, _ = run_stats(batch_planner, edges, "edge")
    assert info["n_batched"] + info["n_fallback"] == len(edges)


def test_both_size_classes(batch_planner):
    fps = both_classes()
    _, stats, info, winfo = run_stats(batch_planner, fps, "classes")
    assert info["n_batched"] == 16 and winfo["kernel_launches"] == 2 and info["kernel_launches"] == 3
    assert sum(fp.n_nodes_ext > 64 for fp in fps) >= 2 and sum(fp.n_nodes_ext <= 64 for fp in fps) >= 2
    not_vacuous(fps, stats, unmet=False)


def test_sums_are_64_bit(batch_planner):
    _, stats, info, _ = run_stats(batch_planner, [sumsq_problem()], "sumsq")
    assert info["n_batched"] == 1 and stats[0]["load_sumsq"][0] > 2**32


def test_with_moves_in_the_same_call(batch_planner):
    fps = synth.cbgt_batch(12, seed=43, P_range=(20, 300), N_range=(5, 200))
    favor = [bool(i % 2) for i in range(len(fps))]
    got, moves, stats, info = batch_planner.plan_batch_stats(fps, True, favor)
    _, mmoves, _ = batch_planner.plan_batch_moves(fps, favor)
    _, _, sstats, _ = batch_planner.plan_batch_stats(fps)
    want, winfo = batch_planner.plan_batch(fps)
    for i, (g, w) in enumerate(zip(got, want)):
        same_plan(g, w, ("with moves", i))
        assert all(np.array_equal(a, b) for a, b in zip(moves[i], mmoves[i])), i
        same_stats(stats[i], sstats[i], ("stats only", i))
    assert info["kernel_launches"] == winfo["kernel_launches"] + 2 <= 4
    check_stats(batch_planner, fps, got, stats, "with moves", single=False)


def test_batch_with_fallback_problems(batch_planner):
    fps = fallback_problems(200, 300, synth.cbgt_batch(6, seed=7, P_range=(20, 300), N_range=(30, 200)))
    _, _, info, _ = run_stats(batch_planner, fps, "fallback")
    assert info["n_fallback"] >= 2 and info["n_batched"] == 6


def test_cbgt_64_default_shape(batch_planner):
    from oracle import loader
    fps = synth.cbgt_batch(64, seed=2)
    got, moves, stats, info = batch_planner.plan_batch_stats(fps)
    assert info["n_batched"] == 64 and info["n_fallback"] == 0 and info["kernel_launches"] <= 3
    for i, (fp, r, s) in enumerate(zip(fps, got, stats)):
        same_stats(s, stats_ref.plan_stats(fp, r), ("stats_ref", i))
    for i in range(8):
        same_plan(got[i], loader.plan(fps[i]), ("oracle", i))
    check_stats(batch_planner, fps[:4], got[:4], stats[:4], "cbgt 64")
