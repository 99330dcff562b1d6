"""blance_plan_moves_get on the MI355X: k_plan_moves against oracle.moves_ref's moves on the C oracle's plan, and against
blance_calc_moves on host-built CSRs (the route the call replaces)."""
import numpy as np
import pytest

from blance_amd import abi, hip, problem, synth
from helpers import build_from_case
from oracle.moves_ref import calc_partition_moves
from test_plan_batch_moves_emulated import _begin, _check_moves, _decoded, _ends, _mixed, _other_of
from test_plan_moves_emulated import (_rebalance, check_counters, plan_and_check, same_moves, scan_split_problem,
                                      via_calc_moves)

pytestmark = pytest.mark.gpu


def _oracle(fp):
    from oracle import loader
    return loader.plan(fp)


@pytest.fixture(scope="module")
def planner():
    pl = hip.Planner(device_id=0)
    yield pl
    pl.close()


@pytest.mark.parametrize("favor", [False, True])
def test_golden_cases(planner, golden_cases, favor):
    n, kinds = 0, set()
    for c in golden_cases:
        fp = build_from_case(c)
        if planner.validate(fp) != abi.OK:
            continue
        got = plan_and_check(planner, fp, c["prevMap"] or {}, favor, (c["source"], favor))
        if got is not None:
            n += 1
            kinds |= set(got[1][3].tolist())
    assert n >= 60 and kinds == {0, 1, 2, 3}


@pytest.mark.parametrize("seed", [0, 100])
def test_random_cases(planner, seed):
    pairs = [(fp, prev) for fp, prev in _mixed(seed) if planner.validate(fp) == abi.OK]
    sweeps = []
    for i, (fp, prev) in enumerate(pairs):
        res, _, _, _ = plan_and_check(planner, fp, prev, bool((i + seed) % 2), ("mixed", seed, i))
        sweeps.append(res.iterations if fp.n_prev > 0 else 0)
    assert max(sweeps) >= 2                          # the begin map is prevMap as uploaded, not as written back


@pytest.mark.parametrize("hierarchy", [True, False])
def test_mid_size_rebalance(planner, hierarchy):
    P, N = 4096, 128
    fp1 = synth.config5_initial(P, N, hierarchy=hierarchy)
    fp = synth.config5_rebalance(fp1, planner.plan(fp1), P, N, hierarchy=hierarchy)
    res = planner.plan(fp)
    assert res.digest() == _oracle(fp).digest()
    ends = _ends(res)
    for favor in (False, True):
        mv, info = planner.plan_moves(favor)
        same_moves(mv, via_calc_moves(planner, fp, res, None, favor), ("mid size", hierarchy, favor))
        check_counters(mv, info)
        assert info["n_by_kind"]["add"] > 0 and info["n_by_kind"]["del"] > 0
        for p in range(256):
            assert _decoded(mv, p) == calc_partition_moves([0, 1], _begin(fp, None, p), ends[p], favor), (hierarchy, favor, p)


@pytest.mark.parametrize("P", [1, 255, 257])
def test_shapes(planner, P):
    fp = _rebalance(planner, P, 10)
    for favor in (False, True):
        _, mv, info, _ = plan_and_check(planner, fp, {}, favor, ("shape", P, favor))
        assert len(mv[0]) == P + 1 and info["n_moves"] > 0


def test_scan_split(planner):
    """P + 1 > 4 * kScanTile: the scan of the counts takes its three-launch form."""
    fp = scan_split_problem()
    res = planner.plan(fp)
    assert res.digest() == _oracle(fp).digest()
    ends = _ends(res)
    for favor in (False, True):
        mv, info = planner.plan_moves(favor)
        same_moves(mv, via_calc_moves(planner, fp, res, None, favor), "scan split")
        check_counters(mv, info)
        assert info["n_moves"] == 3 * fp.n_parts
        for p in range(0, fp.n_parts, fp.n_parts // 512):
            assert _decoded(mv, p) == calc_partition_moves([0, 1], _begin(fp, None, p), ends[p], favor), p


def test_host_memory(planner):
    """The output arrays in page-locked memory (written by DMA where they lie) and in ordinary numpy arrays."""
    fp = _rebalance(planner, 3000, 64)
    res = planner.plan(fp)
    pageable, info_a = planner.plan_moves(False)
    arena = hip.HostArena()
    pinned, info_b = planner.plan_moves(False, arena=arena)
    assert arena.n_blocks == 4
    same_moves(pageable, pinned, "pinned")
    assert {k: info_a[k] for k in ("n_moves", "n_by_kind", "n_parts_moved")} == \
        {k: info_b[k] for k in ("n_moves", "n_by_kind", "n_parts_moved")}
    _check_moves(fp, res, pinned, None, False, "pinned")
    check_counters(pinned, info_b)


def test_count_only_and_capacity(planner):
    fp = _rebalance(planner, 3000, 64)
    planner.plan(fp)
    want, info = planner.plan_moves(True)
    none, counted = planner.plan_moves(True, count_only=True)
    assert none is None
    assert {k: counted[k] for k in ("n_moves", "n_by_kind", "n_parts_moved")} == \
        {k: info[k] for k in ("n_moves", "n_by_kind", "n_parts_moved")}
    n = info["n_moves"]
    assert n > 0
    exact, _ = planner.plan_moves(True, capacity=n)
    same_moves(want, exact, "exact capacity")
    with pytest.raises(hip.BlanceError) as e:
        planner.plan_moves(True, capacity=n - 1)
    assert e.value.status == abi.ERR_CAPACITY and e.value.info["n_moves"] == n
    again, _ = planner.plan_moves(True)
    same_moves(want, again, "after the capacity error")


def test_context_undisturbed(planner):
    fp = _rebalance(planner, 3000, 64)
    planner.upload(fp)
    planner.plan_resident()
    before = planner.download()
    stats0 = planner.plan_stats(fp.n_states)
    mv1, _ = planner.plan_moves(False)
    assert planner.download().digest() == before.digest() == _oracle(fp).digest()
    stats1 = planner.plan_stats(fp.n_states)
    assert all(np.array_equal(stats0[k], stats1[k]) for k in stats0)
    planner.plan_resident()                          # the begin map is still the upload
    mv2, _ = planner.plan_moves(False)
    same_moves(mv1, mv2, "second plan")
    assert planner.download().digest() == before.digest()
    _check_moves(fp, before, mv2, None, False, "resident")


def test_fallback_agreement(planner):
    """A problem outside the batched envelope gets its batch moves from the host detour; plan + plan_moves agree."""
    wide = problem.build_problem(**synth.cbgt_case(8, P_range=(200, 200), N_range=(300, 300), rebalance=True))
    assert wide.n_nodes_ext > 256
    for favor in (False, True):
        got, moves, info = planner.plan_batch_moves([wide], favor)
        assert info["n_fallback"] == 1
        res = planner.plan(wide)
        assert res.digest() == got[0].digest()
        mv, minfo = planner.plan_moves(favor)
        same_moves(moves[0], mv, ("fallback", favor))
        check_counters(mv, minfo)
        assert minfo["n_moves"] > 0
