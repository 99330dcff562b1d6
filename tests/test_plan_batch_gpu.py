"""blance_plan_batch on the MI355X: k_plan_batch against the C oracle."""
import pytest

from blance_amd import abi, hip, synth
from helpers import build_from_case
from randgen import random_case, random_flat_wide_case, random_regular_case

pytestmark = pytest.mark.gpu


def _oracle(fp):
    from oracle import loader
    return loader.plan(fp)


def _same(got, want, tag):
    assert got.iterations == want.iterations, tag
    assert got.converged == want.converged, tag
    assert got.warnings() == want.warnings(), tag
    assert got.digest() == want.digest(), tag


@pytest.fixture(scope="module")
def batch_planner():
    pl = hip.Planner(device_id=0)
    yield pl
    pl.close()


def test_golden_cases_one_batch(batch_planner, golden_cases):
    fps = [fp for fp in (build_from_case(c) for c in golden_cases) if batch_planner.validate(fp) == abi.OK]
    got, info = batch_planner.plan_batch(fps)
    assert info["n_batched"] == len(fps) and info["kernel_launches"] <= 2
    for i, (fp, r) in enumerate(zip(fps, got)):
        _same(r, _oracle(fp), ("golden", i))
        _same(r, batch_planner.plan(fp), ("golden vs blance_plan", i))


def test_random_batches(batch_planner):
    from blance_amd import problem
    fps = []
    for s in range(60):
        for gen in (random_case, random_regular_case, random_flat_wide_case):
            try:
                fps.append(build_from_case(gen(s)))
            except problem.Unsupported:
                pass
    fps = [fp for fp in fps if batch_planner.validate(fp) == abi.OK]
    got, info = batch_planner.plan_batch(fps)
    assert info["n_batched"] + info["n_fallback"] == len(fps)
    for i, (fp, r) in enumerate(zip(fps, got)):
        _same(r, _oracle(fp), ("random", i))


def test_cbgt_shaped_512(batch_planner):
    """512 index-sized problems (64-2,048 partitions, 8-256 nodes, primary + 1-2 replicas; half with a server-group
    rule, half rebalances) in one call: every digest the oracle's, a constant number of launches."""
    fps = synth.cbgt_batch(512, seed=1)
    got, info = batch_planner.plan_batch(fps)
    assert info["n_batched"] == 512 and info["n_fallback"] == 0
    assert info["kernel_launches"] <= 2
    for i, (fp, r) in enumerate(zip(fps, got)):
        _same(r, _oracle(fp), ("cbgt", i))
