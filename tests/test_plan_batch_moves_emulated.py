"""blance_plan_batch_moves without a GPU: k_batch_moves and its host driver compiled against the SIMT emulator
(tests/simt).  Every moves list is checked against oracle.moves_ref on the decoded begin map (prevMap as passed in, keys
outside the model included) and end map (the plan's result); batched problems also against blance_calc_moves
(planner.CalcPartitionMovesBatch)."""
import copy
import ctypes as C

import numpy as np
import pytest

from blance_amd import abi, hip, planner, problem, synth
from helpers import build_from_case
from oracle.moves_ref import calc_partition_moves
from randgen import random_case, random_flat_wide_case, random_regular_case
from test_simt_emulated import build_emu


@pytest.fixture(scope="module")
def emu_planner():
    pl = hip.Planner(lib_path=build_emu())
    yield pl
    pl.close()


def _same(got, want, tag):
    assert got.iterations == want.iterations, tag
    assert got.converged == want.converged, tag
    assert got.warnings() == want.warnings(), tag
    assert got.digest() == want.digest(), tag


def _other_of(fp, prev_map):
    """prevMap's nodes under keys outside the model as (offsets [P + 1], ids), from the map itself."""
    ids = {x: i for i, x in enumerate(fp.node_names)}
    off, nodes = [0], []
    for name in fp.part_names:
        prev = prev_map.get(name)
        nbs = (prev or {}).get("nodesByState") if isinstance(prev, dict) else getattr(prev, "NodesByState", None)
        for s, lst in sorted((nbs or {}).items()):
            if s not in fp.state_names:
                nodes += [ids[x] for x in (lst or [])]
        off.append(len(nodes))
    return (np.asarray(off, np.int32), np.asarray(nodes, np.int32)) if nodes else None


def _begin(fp, other, p):
    """{state id: [node ids]} of partition p's prevMap entry as the flat problem carries it; key M: keys outside the model."""
    M, off, nodes = fp.n_states, fp.prev_off, fp.prev_nodes
    beg = {m: nodes[off[p * M + m]:off[p * M + m + 1]].tolist() for m in range(M)}
    if other is not None:
        beg[M] = other[1][other[0][p]:other[0][p + 1]].tolist()
    return beg


def _ends(res):
    return [{m: ids.tolist() for m, (_, ids) in enumerate(lists)} for lists in res.lists()]


def _decoded(mv, p):
    op_off, op_node, op_state, op_kind = mv
    return [(int(op_node[j]), "" if op_state[j] < 0 else int(op_state[j]), abi.OP_NAMES[op_kind[j]])
            for j in range(op_off[p], op_off[p + 1])]


def _check_moves(fp, res, mv, other, favor, tag):
    M = fp.n_states
    assert mv[0][0] == 0 and len(mv[0]) == fp.n_parts + 1, tag
    ends = _ends(res)
    for p in range(fp.n_parts):
        want = calc_partition_moves(list(range(M)), _begin(fp, other, p), ends[p], favor)
        assert _decoded(mv, p) == want, (tag, p)


def _check_vs_calc_moves(pl, fp, res, mv, other, favor, tag):
    """The same moves from blance_calc_moves (one call over every partition) on names built from the ids."""
    M = fp.n_states
    states = ["s%02d" % m for m in range(M)]

    def named(d):
        return {("zz_other" if m == M else states[m]): ["n%d" % x for x in lst] for m, lst in d.items()}
    names = ["p%05d" % p for p in range(fp.n_parts)]
    beg = {names[p]: named(_begin(fp, other, p)) for p in range(fp.n_parts)}
    ends = _ends(res)
    end = {names[p]: named(ends[p]) for p in range(fp.n_parts)}
    got = planner.CalcPartitionMovesBatch(states, beg, end, favor, planner=pl)
    for p in range(fp.n_parts):
        want = [("n%d" % x, "" if s == "" else states[s], op) for x, s, op in _decoded(mv, p)]
        assert [(o.Node, o.State, o.Op) for o in got[names[p]]] == want, (tag, p)


def _run(pl, fps, favor, others=None, batched_check=True, tag=""):
    others = others if others is not None else [None] * len(fps)
    got, moves, info = pl.plan_batch_moves(fps, favor, others)
    want, winfo = pl.plan_batch(fps)
    favors = favor if isinstance(favor, list) else [favor] * len(fps)
    for i, (fp, r, w, mv, o, f) in enumerate(zip(fps, got, want, moves, others, favors)):
        _same(r, w, (tag, "plan", i))
        if f is None:
            assert mv is None
            continue
        _check_moves(fp, r, mv, o, f, (tag, i))
        if batched_check:
            _check_vs_calc_moves(pl, fp, r, mv, o, f, (tag, i))
    return got, moves, info, winfo


@pytest.mark.parametrize("favor", [False, True])
def test_golden_cases_one_batch(emu_planner, golden_cases, favor):
    cases = [c for c in golden_cases if emu_planner.validate(build_from_case(c)) == abi.OK]
    fps = [build_from_case(c) for c in cases]
    others = [_other_of(fp, c["prevMap"] or {}) for fp, c in zip(fps, cases)]
    assert len(fps) >= 60
    got, moves, info, winfo = _run(emu_planner, fps, favor, others, tag=("golden", favor))
    assert info["n_batched"] == len(fps) and info["n_fallback"] == 0
    assert info["kernel_launches"] <= 3 and info["kernel_launches"] == winfo["kernel_launches"] + 1
    assert info["steps_total"] == winfo["steps_total"]
    assert sum(int(m[0][-1]) for m in moves) > 0


def _built(case):
    try:
        return [(build_from_case(case), case["prevMap"] or {})]
    except problem.Unsupported:
        return []


def _with_other_keys(seed):
    """A rebalance whose prevMap carries nodes under state keys that are not in the model."""
    kw = synth.cbgt_case(seed, P_range=(30, 80), N_range=(8, 40), rebalance=True)
    prev = copy.deepcopy(kw["prev_map"])
    nodes = kw["nodes_all"]
    for i, name in enumerate(sorted(prev)):
        if i % 3 == 0:
            prev[name]["nodesByState"]["dead"] = [nodes[(i * 7) % len(nodes)], nodes[(i * 7 + 1) % len(nodes)]]
        if i % 5 == 0:
            prev[name]["nodesByState"]["zombie"] = [nodes[i % len(nodes)]]
    kw["prev_map"] = prev
    return problem.build_problem(**kw), prev


def _mixed(seed):
    out = []
    for s in range(seed, seed + 6):
        out += _built(random_case(s)) + _built(random_regular_case(s)) + _built(random_flat_wide_case(s))
    c = synth.rebalance_case(P=200, N=30, seed=seed, hierarchy=False)
    fresh = {p: {"name": p, "nodesByState": {}} for p in c["partitions"]}
    out.append((problem.build_problem({}, fresh, c["oldNodes"], [], c["oldNodes"], c["model"],
                                      partition_weights=c["partitionWeights"], state_stickiness=c["stateStickiness"],
                                      node_weights=c["nodeWeights"]), {}))
    for i in range(4):
        kw = synth.cbgt_case(seed * 10 + i, P_range=(16, 150), N_range=(4, 80), rebalance=True)
        out.append((problem.build_problem(**kw), kw["prev_map"]))
    out.append(_with_other_keys(seed + 1))
    return out


@pytest.mark.parametrize("seed", [0, 100])
def test_random_mixed_batches(emu_planner, seed):
    pairs = [(fp, prev) for fp, prev in _mixed(seed) if emu_planner.validate(fp) == abi.OK]
    fps = [fp for fp, _ in pairs]
    others = [_other_of(fp, prev) for fp, prev in pairs]
    favor = [bool((i + seed) % 2) for i in range(len(fps))]
    got, moves, info, _ = _run(emu_planner, fps, favor, others, tag=("mixed", seed))
    assert info["n_batched"] + info["n_fallback"] == len(fps)
    # what the batch must contain to mean anything
    assert any(r.iterations >= 2 for r, fp in zip(got, fps) if fp.n_prev > 0)         # write-back between sweeps
    assert any(fp.node_removed.any() and fp.node_added.any() and fp.n_prev > 0 for fp in fps)   # a rebalance
    assert any(fp.n_prev > 0 and not fp.part_in_prev.all() for fp in fps)             # partitions not in prevMap
    assert any(o is not None for o in others)                                         # keys outside the model
    kinds = {abi.OP_NAMES[k] for m in moves for k in m[3].tolist()}
    assert kinds == {"add", "del", "promote", "demote"}


def test_envelope_fallback(emu_planner):
    """Problems outside the batched envelope (257 node names, a list of 9) get the single path's moves."""
    inside = synth.cbgt_batch(2, seed=7, P_range=(20, 60), N_range=(30, 60))
    kw = synth.cbgt_case(8, P_range=(30, 30), N_range=(257, 257), rebalance=True)
    wide = problem.build_problem(**kw)
    assert wide.n_nodes_ext == 257
    nodes = ["n%02d" % i for i in range(12)]
    model = {"primary": {"priority": 0, "constraints": 1}, "replica": {"priority": 1, "constraints": 2}}
    long_prev = {"a": {"name": "a", "nodesByState": {"primary": nodes[:1], "replica": nodes[1:10]}},
                 "b": {"name": "b", "nodesByState": {"primary": nodes[2:3], "old": nodes[5:7]}}}
    assign = {"a": copy.deepcopy(long_prev["a"]), "b": {"name": "b", "nodesByState": {"primary": nodes[2:3]}}}
    fp_list9 = problem.build_problem(long_prev, assign, nodes, ["n05"], [], model)
    fps = inside + [wide, fp_list9]
    others = [None, None, None, _other_of(fp_list9, long_prev)]
    assert others[3] is not None
    for favor in (False, True):
        got, moves, info, _ = _run(emu_planner, fps, favor, others, tag=("envelope", favor))
        assert info["n_fallback"] >= 2 and info["n_batched"] == 2
        assert got[2].struct.kernel_launches > 0 and got[0].struct.kernel_launches == 0


def test_packing_edges(emu_planner):
    """Node id 255, 16 states, deletions (state "" -> -1) through the one-word packing of a move."""
    nodes = ["n%03d" % i for i in range(256)]
    model = {"s%02d" % m: {"priority": m, "constraints": 1} for m in range(16)}
    prev, assign = {}, {}
    for p in range(24):
        nbs = {"s%02d" % m: [nodes[(p * 16 + m * 5 + 255) % 256]] for m in range(16) if (p + m) % 3}
        if p % 4 == 0:
            nbs["s15"] = ["n255"]
            nbs.pop("s14", None)
        prev["%d" % p] = {"name": "%d" % p, "nodesByState": nbs}
        assign["%d" % p] = copy.deepcopy(prev["%d" % p])
    fp = problem.build_problem(prev, assign, nodes, ["n255", "n010"], [], model)
    assert fp.n_nodes_ext == 256 and fp.n_states == 16
    for favor in (False, True):
        got, moves, info, _ = _run(emu_planner, [fp], favor, tag=("edges", favor))
        assert info["n_batched"] == 1
        op_off, node, state, kind = moves[0]
        assert (node == 255).any() and (state == 15).any() and (state == -1).any()
        assert ((state == -1) == (kind == abi.OP_DEL)).all()


# ---- the C contract ------------------------------------------------------------------------------------------------

def _raw(pl, fps, mvs_list, n=None):
    """blance_plan_batch_moves through ctypes: mvs_list None (NULL) or a list of abi.BatchMoves / None."""
    results = [abi.FlatResult(fp) for fp in fps]
    n = len(fps) if n is None else n
    pbs = (C.POINTER(abi.Problem) * max(len(fps), 1))(*[C.pointer(fp.as_struct()) for fp in fps])
    rss = (C.POINTER(abi.Result) * max(len(fps), 1))(*[C.pointer(r.struct) for r in results])
    mvp = None
    if mvs_list is not None:
        mvp = (C.POINTER(abi.BatchMoves) * max(len(fps), 1))(*[C.pointer(m) if m is not None else
                                                                C.POINTER(abi.BatchMoves)() for m in mvs_list])
    info = abi.BatchInfo()
    st = pl.lib.blance_plan_batch_moves(pl._h, n, pbs, rss, mvp, C.byref(info))
    return st, results, info


def _moves_req(pl, fp, favor=False, other=None, short=0, fill=0):
    mv = abi.BatchMoves()
    mv.favor_min_nodes = int(favor)
    keep = []
    if other is not None:
        keep = [np.ascontiguousarray(a, dtype=np.int32) for a in other]
        mv.beg_other_off, mv.beg_other_nodes = [a.ctypes.data_as(C.POINTER(C.c_int32)) for a in keep]
    cap = int(pl.lib.blance_batch_moves_capacity(C.byref(fp.as_struct()), C.byref(mv)))
    arr = [np.full(fp.n_parts + 1, fill, np.int32)] + [np.full(max(cap, 1), fill, np.int32) for _ in range(3)]
    mv.out.op_off, mv.out.op_node, mv.out.op_state, mv.out.op_kind = [a.ctypes.data_as(C.POINTER(C.c_int32)) for a in arr]
    mv.out.capacity = cap - short
    mv._keep = (keep, arr)
    return mv, arr


def test_contract_mvs_null_is_plan_batch(emu_planner):
    fps = synth.cbgt_batch(3, seed=21, P_range=(20, 50), N_range=(5, 30))
    st, got, info = _raw(emu_planner, fps, None)
    assert st == abi.OK
    want, winfo = emu_planner.plan_batch(fps)
    for i, (g, w) in enumerate(zip(got, want)):
        _same(g, w, ("mvs NULL", i))
    assert info.kernel_launches == winfo["kernel_launches"] and info.n_batched == 3
    # single entries NULL: no moves for those, and no moves launch when none asks
    st, got, info = _raw(emu_planner, fps, [None, None, None])
    assert st == abi.OK and info.kernel_launches == winfo["kernel_launches"]
    got, moves, info = emu_planner.plan_batch_moves(fps, [None, True, None])
    assert moves[0] is None and moves[2] is None and moves[1] is not None
    assert info["kernel_launches"] == winfo["kernel_launches"] + 1
    _check_moves(fps[1], got[1], moves[1], None, True, "single entry")


def test_contract_capacity_one_short(emu_planner):
    fps = synth.cbgt_batch(3, seed=23, P_range=(20, 50), N_range=(5, 30))
    reqs = [_moves_req(emu_planner, fp, short=(1 if i == 2 else 0), fill=-7) for i, fp in enumerate(fps)]
    results = [abi.FlatResult(fp) for fp in fps]
    for r in results:
        r.out_off[:] = -7
    pbs = (C.POINTER(abi.Problem) * 3)(*[C.pointer(fp.as_struct()) for fp in fps])
    rss = (C.POINTER(abi.Result) * 3)(*[C.pointer(r.struct) for r in results])
    mvp = (C.POINTER(abi.BatchMoves) * 3)(*[C.pointer(m) for m, _ in reqs])
    st = emu_planner.lib.blance_plan_batch_moves(emu_planner._h, 3, pbs, rss, mvp, None)
    assert st == abi.ERR_CAPACITY
    assert b"problem 2" in emu_planner.lib.blance_last_error()
    assert all((r.out_off == -7).all() and r.iterations == 0 for r in results)
    assert all((a == -7).all() for _, arr in reqs for a in arr)
    # the exact capacity is enough
    reqs[2] = _moves_req(emu_planner, fps[2])
    mvp = (C.POINTER(abi.BatchMoves) * 3)(*[C.pointer(m) for m, _ in reqs])
    assert emu_planner.lib.blance_plan_batch_moves(emu_planner._h, 3, pbs, rss, mvp, None) == abi.OK


def test_contract_bad_requests(emu_planner):
    fps = synth.cbgt_batch(2, seed=25, P_range=(20, 40), N_range=(5, 20))
    P, NX = fps[1].n_parts, fps[1].n_nodes_ext
    off = np.zeros(P + 1, np.int32)
    off[1:] = 1
    for bad_id in (NX, -1):
        other = (off, np.asarray([bad_id], np.int32))
        st, results, _ = _raw(emu_planner, fps, [_moves_req(emu_planner, fps[0])[0],
                                                 _moves_req(emu_planner, fps[1], other=other)[0]])
        assert st == abi.ERR_BAD_ARG and b"problem 1" in emu_planner.lib.blance_last_error()
        assert all(r.iterations == 0 for r in results)
    not_monotone = np.zeros(P + 1, np.int32)
    not_monotone[1] = 1
    st, _, _ = _raw(emu_planner, fps[1:], [_moves_req(emu_planner, fps[1], other=(not_monotone, np.zeros(1, np.int32)))[0]])
    assert st == abi.ERR_BAD_ARG
    zero = synth.cbgt_batch(1, seed=26, P_range=(20, 40), N_range=(5, 20))[0]
    zero.scalars["max_iterations"] = 0
    zero._struct = None
    st, _, _ = _raw(emu_planner, [fps[0], zero], [None, _moves_req(emu_planner, zero)[0]])
    assert st == abi.ERR_BAD_ARG and b"problem 1" in emu_planner.lib.blance_last_error()
    st, _, _ = _raw(emu_planner, [fps[0], zero], [None, None])           # no moves asked: a plan without a map is fine
    assert st == abi.OK


def test_contract_empty_and_communicator(emu_planner):
    st, _, info = _raw(emu_planner, [], [])
    assert st == abi.OK and info.n_batched == 0 and info.kernel_launches == 0
    got, moves, info = emu_planner.plan_batch_moves([], False)
    assert got == [] and moves == [] and info["kernel_launches"] == 0
    pl = hip.Planner(lib_path=build_emu())
    try:
        pl.comm_set_callback(0, 2, lambda p, n: None)
        fp = synth.cbgt_batch(1, seed=27, P_range=(20, 40), N_range=(5, 20))[0]
        with pytest.raises(hip.BlanceError) as e:
            pl.plan_batch_moves([fp], False)
        assert e.value.status == abi.ERR_UNSUPPORTED
    finally:
        pl.close()


# ---- the Python API ------------------------------------------------------------------------------------------------

def _rules(r):
    if r is None:
        return None
    return {s: [planner.HierarchyRule(x["includeLevel"], x["excludeLevel"]) for x in lst] for s, lst in r.items()}


def _api_calls(seed):
    calls = []
    for i in range(5):
        kw = synth.cbgt_case(seed + i, P_range=(10, 60), N_range=(4, 40), rebalance=i % 2 == 0)
        prev, assign = kw["prev_map"], kw["partitions_to_assign"]
        if i == 4:                                   # keys outside the model in prevMap (not in partitionsToAssign)
            prev = copy.deepcopy(prev)
            for j, name in enumerate(sorted(prev)):
                if j % 2 == 0:
                    prev[name]["nodesByState"]["retired"] = [kw["nodes_all"][j % len(kw["nodes_all"])]]
        calls.append((prev, assign, kw["nodes_all"], kw["nodes_to_remove"], kw["nodes_to_add"], kw["model"],
                      planner.PlanNextMapOptions(NodeWeights=kw["node_weights"], NodeHierarchy=kw["node_hierarchy"],
                                                 HierarchyRules=_rules(kw["hierarchy_rules"])), "cbgt"))
    return calls


def _nbs(p):
    return p.NodesByState if hasattr(p, "NodesByState") else p.get("nodesByState")


@pytest.mark.parametrize("favor", [False, True, "per-call"])
def test_plan_next_map_ex_batch_moves_matches_loop(emu_planner, favor):
    calls_a, calls_b = _api_calls(60), _api_calls(60)
    favors = [bool(i % 2) for i in range(len(calls_a))] if favor == "per-call" else [favor] * len(calls_a)
    states = [problem.sort_state_names(c[5]) for c in calls_a]
    begs = [copy.deepcopy(c[0]) for c in calls_a]
    want = [planner.PlanNextMapEx(*c, planner=emu_planner) for c in calls_a]
    got = planner.PlanNextMapExBatchMoves(calls_b, favorMinNodes=favors if favor == "per-call" else favor,
                                          planner=emu_planner)
    assert any(any(s not in st for p in b.values() for s in (_nbs(p) or {})) for b, st in zip(begs, states))
    for i, ((nm, w, mv), (wnm, ww)) in enumerate(zip(got, want)):
        assert (nm, w) == (wnm, ww), i
        assert list(mv) == list(calls_b[i][1])     # every partition of partitionsToAssign, in its order
        for name, ops in mv.items():
            beg = _nbs(begs[i][name]) if name in begs[i] else {}
            want_ops = calc_partition_moves(states[i], beg, nm[name].NodesByState, favors[i])
            assert [(o.Node, o.State, o.Op) for o in ops] == want_ops, (i, name)
    for ca, cb in zip(calls_a, calls_b):          # the write-back into each call's own input maps
        assert ca[0] == cb[0] and ca[1] == cb[1]


def test_plan_next_map_ex_batch_moves_zero_iterations(emu_planner, monkeypatch):
    monkeypatch.setattr(planner, "MaxIterationsPerPlan", 0)
    assert planner.PlanNextMapExBatchMoves(_api_calls(70)[:2], planner=emu_planner) == [(None, None, None)] * 2


def test_struct_layout_and_symbols(tmp_path):
    """abi.BatchMoves matches include/blance_batch.h; the gfx950 library exports both new symbols, and the capacity is
    prev entries + other entries + blance_result_capacity (a host-only call)."""
    import os
    import subprocess
    import __graft_entry__ as g
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "blance_batch.h")
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\n'
                    'int main(){printf("%%zu %%zu %%zu\\n", sizeof(blance_batch_moves), offsetof(blance_batch_moves, '
                    'beg_other_off), offsetof(blance_batch_moves, out));return 0;}\n' % header)
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-o", str(exe), str(prog)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(abi.BatchMoves), abi.BatchMoves.beg_other_off.offset, abi.BatchMoves.out.offset]
    g.build_hip()
    lib = hip.load_library()
    assert hasattr(lib, "blance_plan_batch_moves") and hasattr(lib, "blance_batch_moves_capacity")
    fp = synth.cbgt_batch(1, seed=31, P_range=(20, 40), N_range=(5, 20))[0]
    mv = abi.BatchMoves()
    base = int(fp.prev_off[-1]) + fp.result_capacity()
    assert lib.blance_batch_moves_capacity(C.byref(fp.as_struct()), C.byref(mv)) == base
    off = np.arange(fp.n_parts + 1, dtype=np.int32)
    mv.beg_other_off = off.ctypes.data_as(C.POINTER(C.c_int32))
    assert lib.blance_batch_moves_capacity(C.byref(fp.as_struct()), C.byref(mv)) == base + fp.n_parts
