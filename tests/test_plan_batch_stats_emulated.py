"""blance_plan_batch_stats without a GPU: k_batch_stats and its host driver compiled against the SIMT emulator
(tests/simt).  Every statistics block is checked against oracle.stats_ref on the plan it came with and against the single
path (blance_plan, then blance_plan_stats_get), never against the batch's own output: n_nodes_next and all seven arrays as
int64, exactly equal.  The plans themselves are checked against blance_plan_batch."""
import copy
import ctypes as C

import numpy as np
import pytest

from blance_amd import abi, hip, planner, problem, synth
from helpers import build_from_case, edge_cases
from oracle import stats_ref
from randgen import random_case
from test_simt_emulated import build_emu

KEYS = ("load_min", "load_max", "load_sum", "load_sumsq", "nodes_used", "unmet_slots", "rule_violations")


@pytest.fixture(scope="module")
def emu_planner():
    pl = hip.Planner(lib_path=build_emu())
    yield pl
    pl.close()


def same_plan(got, want, tag):
    assert got.iterations == want.iterations, tag
    assert got.converged == want.converged, tag
    assert got.warnings() == want.warnings(), tag
    assert got.digest() == want.digest(), tag


def same_stats(got, want, tag):
    assert set(got) == set(KEYS) | {"n_nodes_next"}, tag
    assert got["n_nodes_next"] == want["n_nodes_next"], (tag, "n_nodes_next")
    for k in KEYS:
        assert np.array_equal(np.asarray(got[k], dtype=np.int64), np.asarray(want[k], dtype=np.int64)), \
            (tag, k, np.asarray(got[k]).tolist(), np.asarray(want[k]).tolist())


def check_stats(pl, fps, results, stats, tag, single=True):
    """Every statistics block against stats_ref on its plan and (single) against the single path."""
    for i, (fp, r, s) in enumerate(zip(fps, results, stats)):
        if s is None:
            continue
        same_stats(s, stats_ref.plan_stats(fp, r), (tag, "stats_ref", i))
        if single:
            same_plan(pl.plan(fp), r, (tag, "single plan", i))
            same_stats(s, pl.plan_stats(fp.n_states), (tag, "single path", i))


def run_stats(pl, fps, tag, single=True, plans=None):
    """plan_batch_stats with statistics for every problem and no moves: the statistics, the plans and the info fields
    against plan_batch (`plans`: a (results, info) of plan_batch on the same problems computed before)."""
    got, moves, stats, info = pl.plan_batch_stats(fps)
    want, winfo = plans if plans is not None else pl.plan_batch(fps)
    assert moves == [None] * len(fps), tag
    assert all(s is not None for s in stats), tag
    for i, (g, w) in enumerate(zip(got, want)):
        same_plan(g, w, (tag, "plan", i))
    assert info["steps_total"] == winfo["steps_total"], tag
    assert (info["n_batched"], info["n_fallback"]) == (winfo["n_batched"], winfo["n_fallback"]), tag
    if info["n_fallback"] == 0 and info["n_batched"] > 0:
        assert info["kernel_launches"] == winfo["kernel_launches"] + 1, tag
    check_stats(pl, fps, got, stats, tag, single)
    return got, stats, info, winfo


def not_vacuous(fps, stats, at_least=3, unmet=True):
    """`unmet=False` for the cbgt shape: its plans fill every constraint slot, so only violations and removals count."""
    assert sum(int(s["rule_violations"].sum() > 0) for s in stats) >= at_least
    if unmet:
        assert sum(int(s["unmet_slots"].sum() > 0) for s in stats) >= at_least
    assert sum(int(0 < s["n_nodes_next"] < fp.n_nodes) for fp, s in zip(fps, stats)) >= at_least


def golden_problems(pl, golden_cases):
    fps = [build_from_case(c) for c in golden_cases]
    return [fp for fp in fps if pl.validate(fp) == abi.OK]


def random_problems():
    fps = []
    for seed in range(300, 380):
        try:
            fps.append(build_from_case(random_case(seed)))
        except problem.Unsupported:
            continue
    return fps


def edge_problems():
    return [problem.build_problem(*a, **k) for a, k in edge_cases()]


def both_classes():
    return synth.cbgt_batch(16, seed=2, P_range=(20, 200), N_range=(8, 120))


def sumsq_problem():
    """200 fresh partitions of weight 1000 on two nodes, one state with constraint 1: a node's load is about 100,000 and
    its square does not fit 32 bits."""
    names = ["%03d" % i for i in range(200)]
    fresh = {p: {"name": p, "nodesByState": {}} for p in names}
    return problem.build_problem({}, fresh, ["a", "b"], [], ["a", "b"], {"primary": {"priority": 0, "constraints": 1}},
                                 partition_weights={p: 1000 for p in names})


def fallback_problems(P_wide, wide_nodes, inside):
    """`inside` plus the two shapes outside the batched envelope: more than 256 node names, and a list of 9."""
    wide = problem.build_problem(**synth.cbgt_case(8, P_range=(P_wide, P_wide), N_range=(wide_nodes, wide_nodes), rebalance=True))
    assert wide.n_nodes_ext > 256
    nodes = ["n%02d" % i for i in range(12)]
    model = {"primary": {"priority": 0, "constraints": 1}, "replica": {"priority": 1, "constraints": 2}}
    prev = {"a": {"name": "a", "nodesByState": {"primary": nodes[:1], "replica": nodes[1:10]}},
            "b": {"name": "b", "nodesByState": {"primary": nodes[2:3], "old": nodes[5:7]}}}
    assign = {"a": copy.deepcopy(prev["a"]), "b": {"name": "b", "nodesByState": {"primary": nodes[2:3]}}}
    list9 = problem.build_problem(prev, assign, nodes, ["n05"], [], model)
    half = len(inside) // 2
    return inside[:half] + [wide] + inside[half:] + [list9]


def test_golden_cases_one_batch(emu_planner, golden_cases):
    fps = golden_problems(emu_planner, golden_cases)
    assert len(fps) >= 60
    _, stats, info, _ = run_stats(emu_planner, fps, "golden")
    assert info["n_batched"] == len(fps) and info["n_fallback"] == 0
    not_vacuous(fps, stats)


def test_random_cases_one_batch(emu_planner):
    fps = random_problems()
    assert len(fps) >= 60
    _, stats, info, _ = run_stats(emu_planner, fps, "random")
    assert info["n_batched"] == len(fps) and info["n_fallback"] == 0
    not_vacuous(fps, stats)


def test_edge_cases_one_batch(emu_planner):
    fps = edge_problems()
    _, stats, info, _ = run_stats(emu_planner, fps, "edge")
    assert info["n_batched"] + info["n_fallback"] == len(fps)
    assert any(s["n_nodes_next"] == 0 for s in stats)


def test_both_size_classes(emu_planner):
    all16 = both_classes()
    small = sorted((fp for fp in all16 if fp.n_nodes_ext <= 64), key=lambda fp: fp.n_parts)[:3]
    large = sorted((fp for fp in all16 if fp.n_nodes_ext > 64), key=lambda fp: fp.n_parts)[:2]
    assert len(small) >= 2 and len(large) >= 2
    fps = [small[0], large[0]] + small[1:] + large[1:]
    _, stats, info, winfo = run_stats(emu_planner, fps, "classes")
    assert info["n_batched"] == len(fps) and winfo["kernel_launches"] == 2 and info["kernel_launches"] == 3
    assert any(s["rule_violations"].sum() > 0 for s in stats)


def test_sums_are_64_bit(emu_planner):
    fp = sumsq_problem()
    _, stats, info, _ = run_stats(emu_planner, [fp], "sumsq")
    assert info["n_batched"] == 1
    assert stats[0]["load_sumsq"][0] > 2**32
    assert stats[0]["load_sum"][0] == 200 * 1000


def test_some_ask_some_do_not(emu_planner):
    fps = synth.cbgt_batch(7, seed=41, P_range=(20, 60), N_range=(5, 40))
    ask = [i % 3 != 0 for i in range(len(fps))]
    got, moves, stats, info = emu_planner.plan_batch_stats(fps, ask)
    want, winfo = emu_planner.plan_batch(fps)
    for i, (g, w) in enumerate(zip(got, want)):
        same_plan(g, w, ("some", i))
    assert [s is not None for s in stats] == ask and moves == [None] * len(fps)
    assert info["kernel_launches"] == winfo["kernel_launches"] + 1
    check_stats(emu_planner, fps, got, stats, "some")
    # nobody asks: no statistics launch
    got, _, stats, info = emu_planner.plan_batch_stats(fps, False)
    assert stats == [None] * len(fps) and info["kernel_launches"] == winfo["kernel_launches"]
    for i, (g, w) in enumerate(zip(got, want)):
        same_plan(g, w, ("none", i))


def test_with_moves_in_the_same_call(emu_planner):
    fps = synth.cbgt_batch(5, seed=43, P_range=(20, 60), N_range=(5, 80))
    favor = [bool(i % 2) for i in range(len(fps))]
    got, moves, stats, info = emu_planner.plan_batch_stats(fps, True, favor)
    mres, mmoves, minfo = emu_planner.plan_batch_moves(fps, favor)
    sres, _, sstats, _ = emu_planner.plan_batch_stats(fps)
    want, winfo = emu_planner.plan_batch(fps)
    for i, (g, w) in enumerate(zip(got, want)):
        same_plan(g, w, ("with moves", i))
        assert all(np.array_equal(a, b) for a, b in zip(moves[i], mmoves[i])), i
        same_stats(stats[i], sstats[i], ("stats only", i))
    assert sum(int(m[0][-1]) for m in moves) > 0
    assert info["kernel_launches"] == winfo["kernel_launches"] + 2 <= 4
    assert minfo["kernel_launches"] == winfo["kernel_launches"] + 1
    check_stats(emu_planner, fps, got, stats, "with moves", single=False)


def test_envelope_fallback(emu_planner):
    fps = fallback_problems(30, 257, synth.cbgt_batch(2, seed=7, P_range=(20, 60), N_range=(30, 60)))
    got, stats, info, _ = run_stats(emu_planner, fps, "fallback")
    assert info["n_fallback"] >= 2 and info["n_batched"] == 2
    assert got[1].struct.kernel_launches > 0 and got[0].struct.kernel_launches == 0
    # with moves for the fallback problems too
    got2, moves, stats2, _ = emu_planner.plan_batch_stats(fps[:3], True, False)
    for i in range(3):
        same_plan(got2[i], got[i], ("fallback moves", i))
        same_stats(stats2[i], stats_ref.plan_stats(fps[i], got2[i]), ("fallback moves", i))
        assert moves[i] is not None


def test_max_iterations_zero(emu_planner):
    fps = synth.cbgt_batch(2, seed=45, P_range=(20, 40), N_range=(5, 20))
    fps[1].scalars["max_iterations"] = 0
    fps[1]._struct = None
    got, stats, info, _ = run_stats(emu_planner, fps, "zero")
    assert got[1].iterations == 0 and stats[1]["n_nodes_next"] == 0
    assert all(not np.asarray(stats[1][k]).any() and len(stats[1][k]) == fps[1].n_states for k in KEYS)
    assert stats[0]["n_nodes_next"] > 0


# ---- the C contract ------------------------------------------------------------------------------------------------

def _stats_req(M, short=0, null=None, fill=-7):
    st = abi.PlanStats()
    arr = {k: np.full(max(M, 1), fill, np.int32 if k == "nodes_used" else np.int64) for k in KEYS}
    st.n_states = M - short
    for k, a in arr.items():
        if k != null:
            setattr(st, k, a.ctypes.data_as(C.POINTER(C.c_int32 if k == "nodes_used" else C.c_int64)))
    st.n_nodes_next = fill
    st._keep = arr
    return st, arr


def _raw(pl, fps, reqs):
    results = [abi.FlatResult(fp) for fp in fps]
    for r in results:
        r.out_off[:] = -7
    n = len(fps)
    pbs = (C.POINTER(abi.Problem) * n)(*[C.pointer(fp.as_struct()) for fp in fps])
    rss = (C.POINTER(abi.Result) * n)(*[C.pointer(r.struct) for r in results])
    sts = (C.POINTER(abi.PlanStats) * n)(*[C.pointer(s) for s, _ in reqs])
    info = abi.BatchInfo()
    st = pl.lib.blance_plan_batch_stats(pl._h, n, pbs, rss, None, sts, C.byref(info))
    return st, results


@pytest.mark.parametrize("bad", ["short"] + [k for k in KEYS if k != "rule_violations"])
def test_contract_refusals(emu_planner, bad):
    fps = synth.cbgt_batch(4, seed=47, P_range=(20, 40), N_range=(5, 20))
    reqs = [_stats_req(fp.n_states, short=int(bad == "short" and i == 2), null=bad if (bad != "short" and i == 2) else None)
            for i, fp in enumerate(fps)]
    st, results = _raw(emu_planner, fps, reqs)
    assert st == abi.ERR_BAD_ARG
    with pytest.raises(hip.BlanceError) as e:
        emu_planner._check(st)
    assert e.value.status == abi.ERR_BAD_ARG and "problem 2" in str(e.value)
    assert all((r.out_off == -7).all() and r.iterations == 0 for r in results)
    assert all((a == -7).all() for _, arr in reqs for a in arr.values()) and all(s.n_nodes_next == -7 for s, _ in reqs)
    # the same planner answers a valid call
    run_stats(emu_planner, fps[:2], ("after refusal", bad), single=False)


def test_contract_rule_violations_may_be_null(emu_planner):
    fps = synth.cbgt_batch(4, seed=47, P_range=(20, 40), N_range=(5, 20))
    reqs = [_stats_req(fp.n_states, null="rule_violations" if i == 2 else None) for i, fp in enumerate(fps)]
    st, results = _raw(emu_planner, fps, reqs)
    assert st == abi.OK
    for i, (fp, r, (s, arr)) in enumerate(zip(fps, results, reqs)):
        want = stats_ref.plan_stats(fp, r)
        assert s.n_nodes_next == want["n_nodes_next"]
        for k in KEYS:
            if i == 2 and k == "rule_violations":
                assert (arr[k] == -7).all()
            else:
                assert np.array_equal(arr[k][:fp.n_states].astype(np.int64), np.asarray(want[k], dtype=np.int64)), (i, k)


def test_context_holds_no_problem_afterwards(emu_planner):
    fps = synth.cbgt_batch(2, seed=49, P_range=(20, 40), N_range=(5, 20))
    emu_planner.plan(fps[0])
    emu_planner.plan_stats(fps[0].n_states)                  # (a plan is held here)
    emu_planner.plan_batch_stats(fps)
    with pytest.raises(hip.BlanceError) as e:
        emu_planner.plan_stats(2)
    assert e.value.status == abi.ERR_BAD_ARG
    emu_planner.plan_batch_stats(fallback_problems(30, 257, [])[:1])    # a single-path problem leaves none either
    with pytest.raises(hip.BlanceError):
        emu_planner.plan_stats(2)


# ---- the Python API ------------------------------------------------------------------------------------------------

def _call_of(c):
    objects = lambda d: None if d is None else {k: planner.Partition(v.get("name", ""), copy.deepcopy(v.get("nodesByState")))   # noqa: E731
                                                for k, v in d.items()}
    prev = objects(c["prevMap"])
    assign = prev if c.get("aliased") else objects(c["partitionsToAssign"])
    model = {s: planner.PartitionModelState(v["priority"], v["constraints"]) for s, v in c["model"].items()}
    rules = c.get("hierarchyRules")
    if rules is not None:
        rules = {s: [planner.HierarchyRule(r["includeLevel"], r["excludeLevel"]) for r in rl] for s, rl in rules.items()}
    opts = planner.PlanNextMapOptions(c.get("modelStateConstraints"), c.get("partitionWeights"), c.get("stateStickiness"),
                                      c.get("nodeWeights"), c.get("nodeHierarchy"), rules)
    return (prev, assign, list(c["nodesAll"]), c["nodesToRemove"], c["nodesToAdd"], model, opts, c.get("booster"))


def test_plan_next_map_ex_batch_stats(emu_planner, golden_cases):
    ok = [c for c in golden_cases if emu_planner.validate(build_from_case(c)) == abi.OK]
    picked = [[c for c in ok if c.get("hierarchyRules") is not None and c["nodesToRemove"]][-1],
              next(c for c in ok if c["prevMap"] and c.get("partitionWeights")),
              next(c for c in ok if c.get("nodeWeights") and c.get("hierarchyRules") is not None)]
    calls_a, calls_b = [_call_of(c) for c in picked], [_call_of(c) for c in picked]
    fps = [planner._build_call(*_call_of(c)) for c in picked]
    refs = [stats_ref.plan_stats(fp, emu_planner.plan(fp)) for fp in fps]
    want = [planner.PlanNextMapEx(*c, planner=emu_planner) for c in calls_a]
    got = planner.PlanNextMapExBatchStats(calls_b, planner=emu_planner)
    assert len(got) == 3
    for i, ((nm, w, st, n_next), (wnm, ww), fp, ref) in enumerate(zip(got, want, fps, refs)):
        assert (nm, w) == (wnm, ww), i
        assert n_next == ref["n_nodes_next"], i
        assert list(st) == list(fp.state_names), i
        for m, name in enumerate(fp.state_names):
            assert st[name] == {k: int(ref[k][m]) for k in KEYS}, (i, name)
    for ca, cb in zip(calls_a, calls_b):          # the write-back into each call's own input maps
        assert ca[0] == cb[0] and ca[1] == cb[1]


def test_library_exports_the_symbol():
    import __graft_entry__ as g
    g.build_hip()
    lib = hip.load_library()
    assert hasattr(lib, "blance_plan_batch_stats") and lib.blance_abi_version() == 6
