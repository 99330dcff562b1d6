"""blance_plan_moves_get without a GPU: k_plan_moves and its host driver compiled against the SIMT emulator (tests/simt).
Every moves list is checked against oracle.moves_ref on the decoded begin map (prevMap as uploaded, keys outside the model
included) and end map (the plan's result), the plans against the C oracle, and the same moves are asked of
blance_calc_moves on host-built CSRs (the route the call replaces)."""
import ctypes as C

import numpy as np
import pytest

from blance_amd import abi, hip, problem, synth
from helpers import build_from_case
from oracle.moves_ref import calc_partition_moves
from test_plan_batch_moves_emulated import _begin, _check_moves, _check_vs_calc_moves, _decoded, _ends, _mixed, _other_of
from test_simt_emulated import build_emu

SENTINEL = -7


def _oracle(fp):
    from oracle import loader
    return loader.plan(fp)


@pytest.fixture(scope="module")
def emu_planner():
    pl = hip.Planner(lib_path=build_emu())
    yield pl
    pl.close()


def check_counters(mv, info):
    """The three counters are what the arrays imply."""
    op_off, node, state, kind = mv
    assert info["n_moves"] == int(op_off[-1]) == len(node) == len(state) == len(kind)
    by_kind = np.bincount(kind, minlength=4) if len(kind) else np.zeros(4, int)
    assert [info["n_by_kind"][k] for k in abi.OP_NAMES] == by_kind.tolist()
    assert info["n_parts_moved"] == int((np.diff(op_off) > 0).sum())
    assert ((state == -1) == (kind == abi.OP_DEL)).all()


def same_moves(a, b, tag=""):
    for x, y in zip(a, b):
        assert np.array_equal(x, y), tag


def via_calc_moves(pl, fp, res, other, favor):
    """The host route: both maps as (M + 1)-state CSRs through blance_calc_moves."""
    out = pl.calc_moves(fp.n_states, favor, *hip.moves_problem_of(fp, res, other))
    n = int(out[0][-1])
    return out[0], out[1][:n], out[2][:n], out[3][:n]


def plan_and_check(pl, fp, prev_map, favor, tag, vs_oracle=True):
    other = _other_of(fp, prev_map) if prev_map else None
    res = pl.plan(fp)
    if vs_oracle:
        assert res.digest() == _oracle(fp).digest(), tag
    if res.iterations == 0:
        return None
    mv, info = pl.plan_moves(favor, other)
    _check_moves(fp, res, mv, other, favor, tag)
    same_moves(mv, via_calc_moves(pl, fp, res, other, favor), tag)
    check_counters(mv, info)
    return res, mv, info, other


@pytest.mark.parametrize("favor", [False, True])
def test_golden_cases(emu_planner, golden_cases, favor):
    n, kinds, others = 0, set(), 0
    for c in golden_cases:
        fp = build_from_case(c)
        if emu_planner.validate(fp) != abi.OK:
            continue
        got = plan_and_check(emu_planner, fp, c["prevMap"] or {}, favor, (c["source"], favor))
        if got is None:
            continue
        res, mv, info, other = got
        if n % 8 == 0:
            _check_vs_calc_moves(emu_planner, fp, res, mv, other, favor, c["source"])      # (through names, as the batch's tests)
        n += 1
        others += other is not None
        kinds |= set(mv[3].tolist())
    assert n >= 60 and kinds == {0, 1, 2, 3}


@pytest.mark.parametrize("seed", [0, 100])
def test_random_cases(emu_planner, seed):
    """Plans of two and more sweeps among them: the begin map is prevMap as uploaded, not as written back (plan.go:49-52)."""
    pairs = [(fp, prev) for fp, prev in _mixed(seed) if emu_planner.validate(fp) == abi.OK]
    sweeps, others, kinds = [], 0, set()
    for i, (fp, prev) in enumerate(pairs):
        res, mv, info, other = plan_and_check(emu_planner, fp, prev, bool((i + seed) % 2), ("mixed", seed, i))
        sweeps.append(res.iterations if fp.n_prev > 0 else 0)
        others += other is not None
        kinds |= set(mv[3].tolist())
    assert max(sweeps) >= 2 and others >= 1
    assert kinds == {0, 1, 2, 3}
    assert any(fp.n_prev > 0 and not fp.part_in_prev.all() for fp, _ in pairs)             # partitions not in prevMap


def _rebalance(pl, P, N, every=5):
    """A plan over N nodes and the flat problem that rebalances it after every `every`-th node left."""
    fp1 = synth.config_flat(2, P=P, N=N)
    return synth.config3_rebalance_flat(fp1, pl.plan(fp1), every=every, which=1)


class _RoundRobin:
    """A map of P partitions, primary on node p % N and replica on the next node, in the shape of a downloaded result."""

    def __init__(self, P, N):
        self.out_off = np.arange(2 * P + 1, dtype=np.int32)
        self.out_nodes = ((np.arange(2 * P) + 1) // 2 % N).astype(np.int32)
        self.out_kind = np.full(2 * P, abi.LIST_SET, np.uint8)


def test_resident_twice_and_context_undisturbed(emu_planner):
    pl = emu_planner
    fp = _rebalance(pl, 300, 20)
    pl.upload(fp)
    pl.plan_resident()
    before = pl.download()
    stats0 = pl.plan_stats(fp.n_states)
    mv1, info1 = pl.plan_moves(False)
    assert info1["n_moves"] > 0
    _check_moves(fp, before, mv1, None, False, "first plan")
    after = pl.download()
    assert after.digest() == before.digest() == _oracle(fp).digest()
    stats1 = pl.plan_stats(fp.n_states)
    assert all(np.array_equal(stats0[k], stats1[k]) for k in stats0)
    r2 = pl.plan_resident()                           # the upload is still the begin map: k_live_init starts from it again
    assert r2.iterations == before.iterations
    mv2, info2 = pl.plan_moves(False)
    same_moves(mv1, mv2, "second plan")
    assert info1["n_moves"] == info2["n_moves"] and info1["n_by_kind"] == info2["n_by_kind"]
    assert pl.download().digest() == before.digest()
    mv3, _ = pl.plan_moves(True)
    _check_moves(fp, before, mv3, None, True, "favor after two plans")


def test_fresh_plan_is_all_adds(emu_planner):
    fp = synth.config_flat(3, P=300, N=64)
    res = emu_planner.plan(fp)
    mv, info = emu_planner.plan_moves(False)
    _check_moves(fp, res, mv, None, False, "fresh")
    check_counters(mv, info)
    assert info["n_parts_moved"] == fp.n_parts and info["n_by_kind"]["add"] == info["n_moves"] == 3 * fp.n_parts


def test_nothing_changed(emu_planner):
    fp1 = synth.config_flat(3, P=300, N=64)
    fp2 = synth.replan_problem(fp1, emu_planner.plan(fp1))
    res = emu_planner.plan(fp2)
    assert res.converged and res.iterations == 1
    for favor in (False, True):
        mv, info = emu_planner.plan_moves(favor)
        assert info["n_moves"] == 0 and info["n_parts_moved"] == 0 and not any(info["n_by_kind"].values())
        assert (mv[0] == 0).all() and len(mv[0]) == fp2.n_parts + 1 and len(mv[1]) == 0


def test_list_kinds(emu_planner):
    """Absent keys and nil lists on either side count as empty lists."""
    nodes = ["n%d" % i for i in range(6)]
    model = {"primary": {"priority": 0, "constraints": 1}, "replica": {"priority": 1, "constraints": 1},
             "spare": {"priority": 2, "constraints": 0}}
    prev = {"a": {"name": "a", "nodesByState": {"primary": None, "replica": ["n1"]}},           # nil list, absent key
            "b": {"name": "b", "nodesByState": {"primary": ["n2"], "replica": [], "spare": ["n3"]}},
            "c": {"name": "c", "nodesByState": {"spare": ["n0", "n4"]}},
            "d": {"name": "d", "nodesByState": None}}
    assign = {"a": {"name": "a", "nodesByState": {"primary": None, "replica": ["n1"]}},
              "b": {"name": "b", "nodesByState": {"primary": ["n2"], "replica": None}},        # spare absent in the result
              "c": {"name": "c", "nodesByState": {"spare": ["n0", "n4"]}},
              "d": {"name": "d", "nodesByState": {}},
              "e": {"name": "e", "nodesByState": {"replica": ["n5"]}}}                         # not in prevMap
    fp = problem.build_problem(prev, assign, nodes, [], [], model)
    assert emu_planner.validate(fp) == abi.OK
    assert {abi.LIST_ABSENT, abi.LIST_NIL, abi.LIST_SET} <= set(fp.prev_kind.tolist())
    seen = set()
    for favor in (False, True):
        res, mv, info, _ = plan_and_check(emu_planner, fp, prev, favor, ("kinds", favor))
        seen |= set(res.out_kind.tolist())
        assert info["n_by_kind"]["del"] > 0 and info["n_by_kind"]["add"] > 0
    assert abi.LIST_ABSENT in seen


def test_beg_other_blocks_a_clean_add(emu_planner):
    """A node that prevMap holds only under a key outside the model: it is in flattenNodesByState(beg), so its arrival
    is no clean add (moves.go:77-82), and state id M never shows in the result."""
    model = {"primary": {"priority": 0, "constraints": 1}}
    prev = {"a": {"name": "a", "nodesByState": {"primary": [], "old": ["n1"]}},
            "b": {"name": "b", "nodesByState": {"primary": []}}}
    assign = {"a": {"name": "a", "nodesByState": {"primary": []}}, "b": {"name": "b", "nodesByState": {"primary": []}}}
    fp = problem.build_problem(prev, assign, ["n1"], [], [], model)
    other = _other_of(fp, prev)
    assert other is not None
    res = emu_planner.plan(fp)
    assert [ids.tolist() for lists in res.lists() for _, ids in lists] == [[fp.node_names.index("n1")]] * 2
    for favor in (False, True):
        with_other, info = emu_planner.plan_moves(favor, other)
        assert _decoded(with_other, 0) == [] and _decoded(with_other, 1) == [(0, 0, "add")]
        assert info["n_moves"] == 1 and info["n_parts_moved"] == 1
        assert (with_other[2] < fp.n_states).all()
        _check_moves(fp, res, with_other, other, favor, "other")
        without, _ = emu_planner.plan_moves(favor)
        assert _decoded(without, 0) == [(0, 0, "add")]


@pytest.mark.parametrize("P", [0, 1, 255, 256, 257])
def test_shapes(emu_planner, P):
    model = {"primary": {"priority": 0, "constraints": 1}}
    fp = _rebalance(emu_planner, P, 10) if P else problem.build_problem({}, {}, ["n0", "n1"], [], [], model)
    assert fp.n_parts == P
    for favor in (False, True):
        res, mv, info, _ = plan_and_check(emu_planner, fp, {}, favor, ("shape", P, favor))
        assert len(mv[0]) == P + 1
        assert (info["n_moves"] > 0) == (P > 0)


def scan_split_problem(P=32768, N=16):
    """P partitions on few nodes whose plan is cheap -- partitionsToAssign is a balanced round robin that stays -- and whose
    prevMap differs from it in every partition: the old primary is the new replica (a demote), the new primary is new (an
    add) and the old replica goes (a del).  Every node carries the same load in both maps, so the plan is all stays."""
    fp = synth.replan_problem(synth.config_flat(2, P=P, N=N), _RoundRobin(P, N))
    prev = fp.prev_nodes.copy().reshape(P, 2)
    prev[:, 0] = (np.arange(P) + 1) % N
    prev[:, 1] = (np.arange(P) + 5) % N
    fp.set("prev_nodes", prev.reshape(-1))
    return fp


def test_scan_split(emu_planner):
    """P + 1 > 4 * kScanTile = 32,768: launch_scan_excl goes from one launch to three."""
    pl = emu_planner
    fp = scan_split_problem()
    res = pl.plan(fp)
    assert res.digest() == _oracle(fp).digest()
    ends = _ends(res)
    for favor in (False, True):
        mv, info = pl.plan_moves(favor)
        same_moves(mv, via_calc_moves(pl, fp, res, None, favor), "scan split")
        check_counters(mv, info)
        assert info["n_moves"] == 3 * fp.n_parts and info["n_by_kind"]["demote"] == fp.n_parts
        for p in range(0, fp.n_parts, fp.n_parts // 512):
            assert _decoded(mv, p) == calc_partition_moves([0, 1], _begin(fp, None, p), ends[p], favor), p


# ---- the C contract ------------------------------------------------------------------------------------------------

def _request(pl, fp, favor=False, other=None, capacity=None, arrays=True, op_off=True):
    """An abi.PlanMoves with sentinel-filled numpy arrays behind it."""
    mv = abi.PlanMoves()
    mv.favor_min_nodes = int(favor)
    keep = []
    if other is not None:
        keep = [None if a is None else np.ascontiguousarray(a, dtype=np.int32) for a in other]
        if keep[0] is not None:
            mv.beg_other_off = keep[0].ctypes.data_as(C.POINTER(C.c_int32))
        if keep[1] is not None:
            mv.beg_other_nodes = keep[1].ctypes.data_as(C.POINTER(C.c_int32))
    whole = all(a is not None for a in keep)                    # (half a beg_other: the capacity call would read it)
    full = int(pl.lib.blance_plan_moves_capacity(C.byref(fp.as_struct()), C.byref(mv))) if whole else 1024
    cap = full if capacity is None else capacity
    arr = [np.full(fp.n_parts + 1, SENTINEL, np.int32)] + [np.full(max(full, 1), SENTINEL, np.int32) for _ in range(3)]
    if op_off:
        mv.out.op_off = arr[0].ctypes.data_as(C.POINTER(C.c_int32))
    if arrays:
        mv.out.op_node, mv.out.op_state, mv.out.op_kind = [a.ctypes.data_as(C.POINTER(C.c_int32)) for a in arr[1:]]
        mv.out.capacity = cap
    mv.n_moves = mv.n_parts_moved = SENTINEL
    for k in range(4):
        mv.n_by_kind[k] = SENTINEL
    mv._keep = (keep, arr)
    return mv, arr


def _untouched(mv, arr, counters=True):
    ok = all((a == SENTINEL).all() for a in arr)
    if counters:
        ok = ok and mv.n_moves == SENTINEL and mv.n_parts_moved == SENTINEL and list(mv.n_by_kind) == [SENTINEL] * 4
    return ok


def _get(pl, mv):
    return pl.lib.blance_plan_moves_get(pl._h, C.byref(mv))


def test_count_only(emu_planner):
    pl = emu_planner
    fp = _rebalance(pl, 300, 20)
    pl.plan(fp)
    full, info = pl.plan_moves(True)
    none, counted = pl.plan_moves(True, count_only=True)
    assert none is None and info["n_moves"] > 0
    assert {k: counted[k] for k in ("n_moves", "n_by_kind", "n_parts_moved")} == \
        {k: info[k] for k in ("n_moves", "n_by_kind", "n_parts_moved")}
    # no array at all; then op_off alone, which is filled when it is given
    mv, arr = _request(pl, fp, True, arrays=False, op_off=False)
    assert _get(pl, mv) == abi.OK and mv.n_moves == info["n_moves"] and _untouched(mv, arr, counters=False)
    mv, arr = _request(pl, fp, True, arrays=False)
    assert _get(pl, mv) == abi.OK and mv.n_parts_moved == info["n_parts_moved"]
    assert np.array_equal(arr[0], full[0]) and all((a == SENTINEL).all() for a in arr[1:])


def test_capacity(emu_planner):
    pl = emu_planner
    fp = _rebalance(pl, 300, 20)
    other = (np.arange(fp.n_parts + 1, dtype=np.int32), np.zeros(fp.n_parts, np.int32))
    bm = abi.BatchMoves()
    pm = abi.PlanMoves()
    for o in (None, other):
        if o is not None:
            bm.beg_other_off = pm.beg_other_off = o[0].ctypes.data_as(C.POINTER(C.c_int32))
            bm.beg_other_nodes = pm.beg_other_nodes = o[1].ctypes.data_as(C.POINTER(C.c_int32))
        a = pl.lib.blance_plan_moves_capacity(C.byref(fp.as_struct()), C.byref(pm))
        assert a == pl.lib.blance_batch_moves_capacity(C.byref(fp.as_struct()), C.byref(bm))
        assert a == int(fp.prev_off[-1]) + fp.result_capacity() + (fp.n_parts if o is not None else 0)
    pl.plan(fp)
    want, info = pl.plan_moves(False)
    n = info["n_moves"]
    assert 0 < n < int(fp.prev_off[-1]) + fp.result_capacity()
    mv, arr = _request(pl, fp, capacity=n)                       # exactly the moves made: enough
    assert _get(pl, mv) == abi.OK and mv.n_moves == n
    same_moves(want, (arr[0], arr[1][:n], arr[2][:n], arr[3][:n]), "exact capacity")
    assert all((a[n:] == SENTINEL).all() for a in arr[1:])
    exact, _ = pl.plan_moves(False, capacity=n)
    same_moves(want, exact)
    mv, arr = _request(pl, fp, capacity=n - 1)                   # one short: the count comes back, no array is touched
    assert _get(pl, mv) == abi.ERR_CAPACITY and pl.lib.blance_last_error()
    assert mv.n_moves == n and mv.n_parts_moved == info["n_parts_moved"] and _untouched(mv, arr, counters=False)
    with pytest.raises(hip.BlanceError) as e:
        pl.plan_moves(False, capacity=n - 1)
    assert e.value.status == abi.ERR_CAPACITY and e.value.info["n_moves"] == n
    after, _ = pl.plan_moves(False)                              # and the context is as before
    same_moves(want, after)


def _refused(pl, mv, arr):
    st = _get(pl, mv)
    return st == abi.ERR_BAD_ARG and len(pl.lib.blance_last_error()) > 0 and _untouched(mv, arr)


def test_refusals(emu_planner):
    fp = _rebalance(emu_planner, 64, 10)
    P, NX = fp.n_parts, fp.n_nodes_ext
    pl = hip.Planner(lib_path=build_emu())
    try:
        assert pl.lib.blance_plan_moves_get(None, C.byref(abi.PlanMoves())) == abi.ERR_BAD_ARG and pl.lib.blance_last_error()
        assert pl.lib.blance_plan_moves_get(pl._h, None) == abi.ERR_BAD_ARG and pl.lib.blance_last_error()
        assert _refused(pl, *_request(pl, fp))                                       # a new context: nothing planned
        pl.upload(fp)
        assert _refused(pl, *_request(pl, fp))                                       # uploaded, not planned
        pl.plan_resident()
        assert _get(pl, _request(pl, fp)[0]) == abi.OK
        pl.plan_batch([fp])
        assert _refused(pl, *_request(pl, fp))                                       # after a batch the context holds no problem
        zero = _rebalance(emu_planner, 64, 10)
        zero.scalars["max_iterations"] = 0
        zero._struct = None
        assert pl.plan(zero).iterations == 0
        assert _refused(pl, *_request(pl, zero))                                     # PlanNextMapEx returned no map
        pl.plan(fp)
        assert _refused(pl, *_request(pl, fp, op_off=False))                         # move arrays without op_off
        mv, arr = _request(pl, fp)
        mv.out.op_state = None
        assert _refused(pl, mv, arr)                                                 # one of the three arrays missing
        off = np.zeros(P + 1, np.int32)
        off[1:] = 1
        ids = np.zeros(1, np.int32)
        assert _refused(pl, *_request(pl, fp, other=(off, None)))
        assert _refused(pl, *_request(pl, fp, other=(None, ids)))
        for bad_id in (NX, -1):
            assert _refused(pl, *_request(pl, fp, other=(off, np.asarray([bad_id], np.int32))))
        from_one = off.copy()
        from_one[0] = 1
        assert _refused(pl, *_request(pl, fp, other=(from_one, np.zeros(2, np.int32))))
        not_monotone = np.zeros(P + 1, np.int32)
        not_monotone[1] = 1
        assert _refused(pl, *_request(pl, fp, other=(not_monotone, ids)))
        assert _get(pl, _request(pl, fp, other=(off, ids))[0]) == abi.OK             # and the context still answers
    finally:
        pl.close()


def test_struct_layout_and_symbols(tmp_path):
    """abi.PlanMoves matches include/blance_hip.h, and the gfx950 library exports both new symbols."""
    import os
    import subprocess
    import __graft_entry__ as g
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "blance_hip.h")
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\n'
                    'int main(){printf("%%zu %%zu %%zu %%zu %%zu\\n", sizeof(blance_plan_moves), offsetof(blance_plan_moves, out), '
                    'offsetof(blance_plan_moves, n_moves), offsetof(blance_plan_moves, n_by_kind), '
                    'offsetof(blance_plan_moves, n_parts_moved));return 0;}\n' % header)
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-o", str(exe), str(prog)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(abi.PlanMoves), abi.PlanMoves.out.offset, abi.PlanMoves.n_moves.offset,
                   abi.PlanMoves.n_by_kind.offset, abi.PlanMoves.n_parts_moved.offset]
    g.build_hip()
    lib = hip.load_library()
    assert hasattr(lib, "blance_plan_moves_get") and hasattr(lib, "blance_plan_moves_capacity")
    assert lib.blance_abi_version() == 6
