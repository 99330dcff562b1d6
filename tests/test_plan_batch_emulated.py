"""blance_plan_batch without a GPU: k_plan_batch and its host driver compiled against the SIMT emulator
(tests/simt), every result against the C oracle and against blance_plan on the same problem."""
import copy

import pytest

from blance_amd import abi, hip, planner, problem, synth
from helpers import build_from_case
from randgen import random_case, random_flat_wide_case, random_regular_case
from test_simt_emulated import build_emu


@pytest.fixture(scope="module")
def emu_planner():
    pl = hip.Planner(lib_path=build_emu())
    yield pl
    pl.close()


def _oracle(fp):
    from oracle import loader
    return loader.plan(fp)


def _same(got, want, tag):
    assert got.iterations == want.iterations, tag
    assert got.converged == want.converged, tag
    assert got.warnings() == want.warnings(), tag
    assert got.digest() == want.digest(), tag


def _valid(pl, fps):
    return [fp for fp in fps if pl.validate(fp) == abi.OK]


def test_golden_cases_one_batch(emu_planner, golden_cases):
    fps = _valid(emu_planner, [build_from_case(c) for c in golden_cases])
    assert len(fps) >= 60
    got, info = emu_planner.plan_batch(fps)
    assert info["n_batched"] == len(fps) and info["n_fallback"] == 0
    assert info["kernel_launches"] <= 2
    for i, (fp, r) in enumerate(zip(fps, got)):
        _same(r, _oracle(fp), ("golden", i))
        _same(r, emu_planner.plan(fp), ("golden vs blance_plan", i))
    assert info["steps_total"] == sum(r.struct.steps_total for r in got)


def _built(case):
    try:
        return [build_from_case(case)]
    except problem.Unsupported:                  # inputs the reference would panic on
        return []


def _mixed(seed):
    fps = []
    for s in range(seed, seed + 12):
        fps += _built(random_case(s)) + _built(random_regular_case(s)) + _built(random_flat_wide_case(s))
    for hier in (False, True):
        c = synth.rebalance_case(P=300, N=40, seed=seed, hierarchy=hier)
        fresh = {p: {"name": p, "nodesByState": {}} for p in c["partitions"]}
        fps.append(problem.build_problem({}, fresh, c["oldNodes"], [], c["oldNodes"], c["model"],
                                         partition_weights=c["partitionWeights"], state_stickiness=c["stateStickiness"],
                                         node_weights=c["nodeWeights"], node_hierarchy=c["nodeHierarchy"],
                                         hierarchy_rules=c["hierarchyRules"]))
    fps += synth.cbgt_batch(6, seed=seed, P_range=(16, 200), N_range=(4, 100))
    return fps


@pytest.mark.parametrize("seed", [0, 100])
def test_random_mixed_batches(emu_planner, seed):
    fps = _valid(emu_planner, _mixed(seed))
    got, info = emu_planner.plan_batch(fps)
    assert info["n_batched"] + info["n_fallback"] == len(fps)
    for i, (fp, r) in enumerate(zip(fps, got)):
        _same(r, _oracle(fp), ("mixed", seed, i))


def test_envelope_edges(emu_planner):
    """In-envelope problems beside ones just outside: 257 node names, a list longer than 8 -- all exact."""
    inside = synth.cbgt_batch(3, seed=7, P_range=(20, 60), N_range=(200, 256))
    wide = problem.build_problem(**synth.cbgt_case(8, P_range=(30, 30), N_range=(257, 257), rebalance=False))
    assert wide.n_nodes_ext == 257
    c = random_flat_wide_case(3, k=4)
    fp_long = build_from_case(c)
    # a state list of 9 entries in partitionsToAssign: beyond the batched list length
    nodes = ["n%02d" % i for i in range(12)]
    model = {"primary": {"priority": 0, "constraints": 1}, "replica": {"priority": 1, "constraints": 2}}
    long_prev = {"a": {"name": "a", "nodesByState": {"primary": nodes[:1], "replica": nodes[1:10]}},
                 "b": {"name": "b", "nodesByState": {"primary": nodes[2:3]}}}
    fp_list9 = problem.build_problem(long_prev, copy.deepcopy(long_prev), nodes, [], [], model)
    fps = inside + [wide, fp_long, fp_list9]
    got, info = emu_planner.plan_batch(fps)
    assert info["n_fallback"] == 2 and info["n_batched"] == len(fps) - 2
    for i, (fp, r) in enumerate(zip(fps, got)):
        _same(r, _oracle(fp), ("edge", i))
    assert got[3].struct.kernel_launches > 0 and got[0].struct.kernel_launches == 0


def test_contract_empty_single_and_twice(emu_planner):
    got, info = emu_planner.plan_batch([])
    assert got == [] and info["n_batched"] == 0 and info["kernel_launches"] == 0
    fp = synth.cbgt_batch(1, seed=3, P_range=(50, 80), N_range=(10, 30))[0]
    (r,), info = emu_planner.plan_batch([fp])
    assert info["n_batched"] == 1
    _same(r, _oracle(fp), "one")
    (a, b), _ = emu_planner.plan_batch([fp, fp])
    _same(a, b, "twice")
    _same(a, r, "twice vs once")


def test_contract_invalid_problem_refused(emu_planner):
    good = synth.cbgt_batch(2, seed=5, P_range=(20, 40), N_range=(5, 20))
    bad = synth.cbgt_batch(1, seed=6, P_range=(20, 40), N_range=(5, 20))[0]
    bad.arrays["part_order"][0] = bad.arrays["part_order"][1]          # not a permutation
    bad._struct = None
    fps = [good[0], bad, good[1]]
    results = [abi.FlatResult(fp) for fp in fps]
    for r in results:
        r.out_off[:] = -7
    import ctypes as C
    lib = emu_planner.lib
    pbs = (C.POINTER(abi.Problem) * 3)(*[C.pointer(fp.as_struct()) for fp in fps])
    rss = (C.POINTER(abi.Result) * 3)(*[C.pointer(r.struct) for r in results])
    st = lib.blance_plan_batch(emu_planner._h, 3, pbs, rss, None)
    assert st == abi.ERR_BAD_ARG
    assert b"problem 1" in lib.blance_last_error()
    assert all((r.out_off == -7).all() and r.iterations == 0 for r in results)


def test_contract_capacity(emu_planner):
    fps = synth.cbgt_batch(3, seed=9, P_range=(20, 40), N_range=(5, 20))
    with pytest.raises(hip.BlanceError) as e:
        import ctypes as C
        results = [abi.FlatResult(fp) for fp in fps]
        results[2].struct.out_capacity = fps[2].result_capacity() - 1
        pbs = (C.POINTER(abi.Problem) * 3)(*[C.pointer(fp.as_struct()) for fp in fps])
        rss = (C.POINTER(abi.Result) * 3)(*[C.pointer(r.struct) for r in results])
        emu_planner._check(emu_planner.lib.blance_plan_batch(emu_planner._h, 3, pbs, rss, None))
    assert e.value.status == abi.ERR_CAPACITY and "problem 2" in str(e.value)


def test_contract_no_resident_problem_after_batch(emu_planner):
    fp = synth.cbgt_batch(1, seed=11, P_range=(20, 40), N_range=(5, 20))[0]
    emu_planner.plan(fp)
    emu_planner.plan_resident()                                       # a problem is resident after blance_plan ...
    emu_planner.plan_batch([fp])
    with pytest.raises(hip.BlanceError) as e:                          # ... and none after a batch
        emu_planner.plan_resident()
    assert e.value.status == abi.ERR_BAD_ARG
    with pytest.raises(hip.BlanceError) as e:
        emu_planner.download(into=abi.FlatResult(fp))
    assert e.value.status == abi.ERR_BAD_ARG


def _api_calls(seed):
    calls = []
    for i in range(4):
        kw = synth.cbgt_case(seed + i, P_range=(10, 60), N_range=(4, 40))
        calls.append((kw["prev_map"], kw["partitions_to_assign"], kw["nodes_all"], kw["nodes_to_remove"],
                      kw["nodes_to_add"], kw["model"],
                      planner.PlanNextMapOptions(NodeWeights=kw["node_weights"], NodeHierarchy=kw["node_hierarchy"],
                                                 HierarchyRules=_rules(kw["hierarchy_rules"])), "cbgt"))
    return calls


def _rules(r):
    if r is None:
        return None
    return {s: [planner.HierarchyRule(x["includeLevel"], x["excludeLevel"]) for x in lst] for s, lst in r.items()}


def test_plan_next_map_ex_batch_matches_loop(emu_planner):
    calls_a, calls_b = _api_calls(40), _api_calls(40)
    want = [planner.PlanNextMapEx(*c, planner=emu_planner) for c in calls_a]
    got = planner.PlanNextMapExBatch(calls_b, planner=emu_planner)
    assert got == want
    for ca, cb in zip(calls_a, calls_b):                               # the write-back into each call's own input maps
        assert ca[0] == cb[0] and ca[1] == cb[1]


def test_plan_next_map_ex_batch_zero_iterations(emu_planner, monkeypatch):
    monkeypatch.setattr(planner, "MaxIterationsPerPlan", 0)
    assert planner.PlanNextMapExBatch(_api_calls(50)[:2], planner=emu_planner) == [(None, None), (None, None)]
    with pytest.raises(problem.Unsupported):
        c = list(_api_calls(50)[0])
        c[7] = lambda *a: 0
        planner.PlanNextMapExBatch([c], planner=emu_planner)
