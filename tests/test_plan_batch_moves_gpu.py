"""blance_plan_batch_moves on the MI355X: k_plan_batch + k_batch_moves against the C oracle's plan and
oracle.moves_ref's moves."""
import pytest

from blance_amd import abi, hip, problem, synth
from helpers import build_from_case
from test_plan_batch_moves_emulated import _check_moves, _mixed, _other_of

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


def _run(pl, fps, favor, others=None):
    others = others if others is not None else [None] * len(fps)
    got, moves, info = pl.plan_batch_moves(fps, favor, others)
    favors = favor if isinstance(favor, list) else [favor] * len(fps)
    for i, (fp, r, mv, o, f) in enumerate(zip(fps, got, moves, others, favors)):
        _same(r, _oracle(fp), ("plan", i))
        _check_moves(fp, r, mv, o, f, ("moves", i))
    return got, moves, info


@pytest.mark.parametrize("favor", [False, True])
def test_golden_cases_one_batch(batch_planner, golden_cases, favor):
    cases = [c for c in golden_cases if batch_planner.validate(build_from_case(c)) == abi.OK]
    fps = [build_from_case(c) for c in cases]
    others = [_other_of(fp, c["prevMap"] or {}) for fp, c in zip(fps, cases)]
    _, _, info = _run(batch_planner, fps, favor, others)
    assert info["n_batched"] == len(fps) and info["kernel_launches"] <= 3


@pytest.mark.parametrize("seed", [0, 100])
def test_random_batches(batch_planner, seed):
    pairs = [(fp, prev) for fp, prev in _mixed(seed) if batch_planner.validate(fp) == abi.OK]
    fps = [fp for fp, _ in pairs]
    favor = [bool((i + seed) % 2) for i in range(len(fps))]
    got, _, info = _run(batch_planner, fps, favor, [_other_of(fp, prev) for fp, prev in pairs])
    assert info["n_batched"] + info["n_fallback"] == len(fps)
    assert any(r.iterations >= 2 for r in got)


def test_cbgt_512_with_moves(batch_planner):
    fps = synth.cbgt_batch(512, seed=2)
    want, winfo = batch_planner.plan_batch(fps)
    got, _, info = _run(batch_planner, fps, [i % 2 == 0 for i in range(len(fps))])
    assert info["n_batched"] == 512 and info["n_fallback"] == 0
    assert info["kernel_launches"] == winfo["kernel_launches"] + 1 <= 3
    for i, (g, w) in enumerate(zip(got, want)):
        _same(g, w, ("vs plan_batch", i))


def test_batch_with_fallback_problems(batch_planner):
    inside = synth.cbgt_batch(6, seed=7, P_range=(20, 300), N_range=(30, 200))
    wide = problem.build_problem(**synth.cbgt_case(8, P_range=(200, 200), N_range=(300, 300), rebalance=True))
    assert wide.n_nodes_ext > 256
    nodes = ["n%02d" % i for i in range(12)]
    model = {"primary": {"priority": 0, "constraints": 1}, "replica": {"priority": 1, "constraints": 2}}
    prev = {"a": {"name": "a", "nodesByState": {"primary": nodes[:1], "replica": nodes[1:10]}},
            "b": {"name": "b", "nodesByState": {"primary": nodes[2:3], "old": nodes[5:7]}}}
    assign = {"a": {"name": "a", "nodesByState": {"primary": nodes[:1], "replica": nodes[1:10]}},
              "b": {"name": "b", "nodesByState": {"primary": nodes[2:3]}}}
    list9 = problem.build_problem(prev, assign, nodes, ["n05"], [], model)
    fps = inside[:3] + [wide] + inside[3:] + [list9]
    others = [None] * 7 + [_other_of(list9, prev)]
    for favor in (False, True):
        _, _, info = _run(batch_planner, fps, favor, others)
        assert info["n_fallback"] >= 2 and info["n_batched"] == 6
