"""blance_plan_adopt: the cases tests/test_adopt_emulated.py runs on the SIMT emulator and tests/test_adopt_gpu.py on the
device, and the checks both make.  The definition every adopted plan is compared with is problem.adopted_problem planned by
the C oracle; the kernels alone (k_adopt_len, k_adopt_write through tests/kernels/adopt_cases.inc) are compared with
kernel_reference below."""
import ctypes as C

import numpy as np
import pytest

from blance_amd import abi, hip, problem, synth, wire
from helpers import build_from_case

POISON32, POISON8 = -0x5A5A5A5B, 0xA5


def _oracle(fp):
    from oracle import loader
    return loader.plan(fp)


def same(got, want, tag):
    assert got.iterations == want.iterations, tag
    assert got.converged == want.converged, tag
    assert got.warnings() == want.warnings(), tag
    assert got.digest() == want.digest(), tag


class Change:
    """The node change of one adoption: byte arrays [n_nodes_ext] or None, and the two flags of blance_adopt."""

    def __init__(self, removed=None, added=None, add_nil=None, keep=False):
        self.removed, self.added, self.keep = removed, added, keep
        self.add_nil = (added is None) if add_nil is None else add_nil

    def kw(self):
        return dict(node_removed=self.removed, node_added=self.added, nodes_to_add_nil=self.add_nil, keep_prev_only=self.keep)


def flags(fp, ids):
    a = np.zeros(fp.n_nodes_ext, dtype=np.uint8)
    a[np.asarray(list(ids), dtype=np.int64)] = 1
    return a


def named(fp):
    fp.part_names = fp.part_names or [str(p) for p in range(fp.n_parts)]
    fp.node_names = fp.node_names or ["n%04d" % i for i in range(fp.n_nodes_ext)]
    fp.state_names = fp.state_names or ["primary", "replica", "spare", "dead"][:fp.n_states]
    return fp


class Round:
    def __init__(self, fp, res, moves):
        self.fp, self.res, self.moves = fp, res, moves          # the adopted problem, its plan, plan_moves' counters


def around_checks(pl, wdict, fp, res, tag, stats=True):
    """What stands around an adopted plan: its document, its moves, its statistics, and a dictionary made before."""
    from oracle import stats_ref
    from test_plan_moves_emulated import same_moves, via_calc_moves
    P, M = fp.n_parts, fp.n_states
    doc, info = pl.plan_wire()
    assert doc == wire.ResultEncoder(fp.part_names, fp.node_names, fp.state_names).encode(res), tag
    for favor in (False, True):
        mv, minfo = pl.plan_moves(favor)
        same_moves(mv, via_calc_moves(pl, fp, res, None, favor), (tag, favor))
        assert minfo["n_moves"] == len(mv[1])
    if stats:
        got, want = pl.plan_stats(M), stats_ref.plan_stats(fp, res)
        assert got["n_nodes_next"] == want["n_nodes_next"], tag
        for key in ("load_min", "load_max", "load_sum", "load_sumsq", "nodes_used", "unmet_slots", "rule_violations"):
            assert np.array_equal(np.asarray(got[key], dtype=np.int64), np.asarray(want[key], dtype=np.int64)), (tag, key)
    dec = pl.decode_wire(wdict, doc)
    assert dec["refusal"] == 0, tag
    total = int(res.out_off[P * M])
    assert np.array_equal(dec["off"], res.out_off[:P * M + 1]) and np.array_equal(dec["kind"], res.out_kind[:P * M]), tag
    assert dec["n_node_refs"] == total and np.array_equal(dec["nodes"], res.out_nodes[:total]), tag


def run_chain(pl, pl2, fp0, changes, tag, around=False, stats=True):
    """Upload and plan fp0 on `pl`, then adopt round by round, each from the one before.  Per round the three assertions of the
    definition: the adopted plan is the oracle's plan of problem.adopted_problem, it is what a second planner (`pl2`) makes of
    that problem uploaded fresh, and a second plan_resident gives it again.  Returns the rounds, or None when fp0's plan made
    no sweep (nothing to adopt)."""
    wdict = None
    pl.upload(fp0)
    if around:
        named(fp0)
        pl.set_wire_names(fp0)
        wdict = pl.wire_dict(fp0)
    pl.plan_resident()
    res = pl.download()
    same(res, _oracle(fp0), (tag, "round 0"))
    if res.iterations == 0:
        return None
    cur, rounds = fp0, []
    try:
        for i, ch in enumerate(changes):
            t = (tag, "round", i + 1)
            pl.adopt(**ch.kw())
            with pytest.raises(hip.BlanceError) as e:
                pl.download()
            assert e.value.status == abi.ERR_BAD_ARG, t
            nxt = problem.adopted_problem(cur, res, ch.removed, ch.added, ch.add_nil, ch.keep)
            want = _oracle(nxt)
            st = pl.plan_resident()
            got = pl.download()
            assert st.iterations == want.iterations, t
            same(got, want, t)
            same(pl2.plan(nxt), want, (t, "fresh upload"))
            pl.plan_resident()
            same(pl.download(), want, (t, "planned twice"))
            _, info = pl.plan_moves(False, count_only=True)
            rounds.append(Round(nxt, got, info))
            if around:
                nxt.part_names, nxt.node_names, nxt.state_names = fp0.part_names, fp0.node_names, fp0.state_names
                around_checks(pl, wdict, nxt, got, t, stats)
            cur, res = nxt, got
    finally:
        if wdict is not None:
            wdict.close()
    return rounds


def honest(rounds, tag, sweeps=True):
    """The conditions that keep a family honest: enough adopted plans of two and more sweeps, and moves with adds and dels."""
    assert rounds, tag
    if sweeps:
        assert 3 * sum(r.res.iterations >= 2 for r in rounds) >= len(rounds), (tag, [r.res.iterations for r in rounds])
    assert any(r.moves["n_by_kind"]["add"] > 0 and r.moves["n_by_kind"]["del"] > 0 for r in rounds), tag


# ---- the families ---------------------------------------------------------------------------------------------------------

def golden_change(fp, i, keep):
    """Every other golden case loses the last node of its nodesNext (when it has two); every third names it in nodesToAdd
    instead -- a node the map holds already."""
    alive = [n for n in range(fp.n_nodes) if not fp.node_removed[n]]
    if len(alive) >= 2 and i % 2 == 1:
        return Change(removed=flags(fp, alive[-1:]), keep=keep)
    if alive and i % 3 == 0:
        return Change(added=flags(fp, alive[-1:]), keep=keep)
    return Change(keep=keep)


def run_golden(pl, pl2, golden_cases, keep):
    """The reference's golden cases that validate and plan with a sweep.  None of them has surviving and dropped load entries
    at once (checked below: the day one does, loads_case can go), so with keep_prev_only they exercise the flag only where
    all their load entries stay or all go; run_loads has the mixed case."""
    rounds, kinds, lens_at_L, lens_zero = [], set(), 0, 0
    for i, c in enumerate(golden_cases):
        fp = build_from_case(c)
        if pl.validate(fp) != abi.OK:
            continue
        got = run_chain(pl, pl2, fp, [golden_change(fp, i, keep)], ("golden", c["source"], keep), around=i % 4 == 0)
        if got is None:
            continue
        rounds += got
        r = got[0]
        P, M = fp.n_parts, fp.n_states
        if P * M:
            prevk = r.fp.prev_kind[:P * M]
            kinds |= set(prevk.tolist())
            lens = np.diff(r.fp.prev_off[:P * M + 1])
            L = max([1, int(lens.max())] + [int(k) for k in fp.state_constraints] +
                    [int(np.diff(fp.assign_off).max()), int(np.diff(fp.prev_off).max())])
            lens_at_L += int((lens == L).any())
            lens_zero += int(((lens == 0) & (prevk != abi.LIST_ABSENT)).any())
        first = fp.load_first_sweep_only[:fp.n_loads]
        assert not (fp.n_loads and (first == 0).any() and (first != 0).any()), c["source"]
        if keep:
            assert r.fp.n_loads == int((first == 0).sum()), c["source"]
    assert len(rounds) >= 60
    # absent and set lists, and lists of every length from nothing to the row, were adopted (a plan's map has no nil list:
    # every key a sweep keeps is a non-nil slice, plan.go:418 -- the kernels alone get nil lists too, run_kernel_cases)
    assert kinds >= {abi.LIST_ABSENT, abi.LIST_SET} and lens_at_L > 0 and lens_zero > 0, (kinds, lens_at_L, lens_zero)
    return rounds


def loads_case():
    """prevMap holds a partition that is not assigned (its loads survive an adoption with keep_prev_only) beside partitions
    whose prevMap entry has a state outside the model (those loads go: the adopted map replaces the entry)."""
    nodes = ["n%d" % i for i in range(6)]
    model = {"primary": {"priority": 0, "constraints": 1}, "replica": {"priority": 1, "constraints": 1}}
    prev = {"only%d" % i: {"name": "only%d" % i, "nodesByState": {"primary": [nodes[i % 2]], "replica": [nodes[2]]}} for i in range(7)}
    assign = {}
    for i in range(20):
        name = "p%02d" % i
        assign[name] = {"name": name, "nodesByState": {"primary": [nodes[i % 3]], "replica": [nodes[(i + 1) % 3]]}}
        prev[name] = {"name": name, "nodesByState": {"primary": [nodes[i % 3]], "replica": [nodes[(i + 1) % 3]],
                                                      "ghost": [nodes[4], nodes[5]]}}
    return problem.build_problem(prev, assign, nodes, [], None, model)


def run_loads(pl, pl2):
    fp = loads_case()
    first = fp.load_first_sweep_only[:fp.n_loads]
    assert (first == 0).sum() == 14 and (first != 0).sum() == 40
    out = []
    for keep in (True, False):
        rounds = run_chain(pl, pl2, fp, [Change(removed=flags(fp, [0]), keep=keep), Change(added=flags(fp, [0]), keep=keep),
                                         Change(removed=flags(fp, [1]), keep=not keep)], ("loads", keep), around=True)
        assert rounds[0].fp.n_loads == (14 if keep else 0) and rounds[0].fp.n_prev == (27 if keep else 20)
        out += rounds
    # the surviving loads weigh on the plan: keeping them gives another map
    assert out[0].res.digest() != out[3].res.digest()
    return out


def mixed_problems(seed):
    from test_plan_batch_emulated import _mixed
    return _mixed(seed)


def run_mixed(pl, pl2, seed):
    rounds = []
    for i, fp in enumerate(mixed_problems(seed)):
        if pl.validate(fp) != abi.OK:
            continue
        alive = [n for n in range(fp.n_nodes) if not fp.node_removed[n]]
        gone = flags(fp, alive[1::3]) if len(alive) >= 3 else None
        got = run_chain(pl, pl2, fp, [Change(removed=gone, keep=bool(i % 2)), Change(added=gone, keep=bool(i % 2))],
                        ("mixed", seed, i), around=i % 6 == 0, stats=fp.n_parts <= 400)
        rounds += got or []
    return rounds


def config5_changes(fp, P, N, hierarchy):
    """rebalance_case's removal and addition on config5_initial's problem.  That problem knows the old nodes only, so the
    addition can name none of its nodes: nodesToAdd is there and empty.  config5_all_nodes below has the real addition."""
    c = synth.rebalance_case(P=P, N=N, hierarchy=hierarchy)
    ids = {n: i for i, n in enumerate(fp.node_names)}
    return [Change(removed=flags(fp, [ids[n] for n in c["nodesToRemove"]]),
                   added=flags(fp, [ids[n] for n in c["nodesToAdd"] if n in ids]), add_nil=False)]


def config5_all_nodes(P, N, hierarchy):
    """config5_initial over ALL nodes of rebalance_case, and three rounds: its nodesToAdd leave (the cluster is the old
    nodes), they come back as nodesToAdd while its nodesToRemove leave (the rebalance of config 5), others leave."""
    c = synth.rebalance_case(P=P, N=N, hierarchy=hierarchy)
    fresh = {p: {"name": p, "nodesByState": {}} for p in c["partitions"]}
    fp = problem.build_problem({}, fresh, c["nodesAll"], [], c["nodesAll"], c["model"], **synth._config5_opts(c))
    ids = {n: i for i, n in enumerate(fp.node_names)}
    add, rm = [ids[n] for n in c["nodesToAdd"]], [ids[n] for n in c["nodesToRemove"]]
    others = [i for i in range(N) if i % 9 == 4 and i not in rm][:6]
    return fp, [Change(removed=flags(fp, add)), Change(removed=flags(fp, rm), added=flags(fp, add)), Change(removed=flags(fp, others))]


def config3_chain(P=4096, N=256):
    """config3_rebalance_flat's change -- every tenth node leaves --, then they come back as nodesToAdd, then others leave."""
    fp = synth.config_flat(3, P=P, N=N)
    tenth = flags(fp, [n for n in range(N) if n % 10 == 3])
    return fp, [Change(removed=tenth), Change(added=tenth), Change(removed=flags(fp, [n for n in range(N) if n % 10 == 7]))]


def rack_chain(P=2100):
    """Racks of four nodes are the regions of the replica's rule (includeLevel 1): a whole rack leaves, so a region has no node
    of nodesNext left; the next round brings it back in nodesToAdd; then half of another rack leaves."""
    N = 48
    nodes = ["n%02d" % i for i in range(N)]
    hier = synth.hierarchy_names(N, rack=4, racks_per_zone=3, zones_per_dc=2, width=2)
    model = {"primary": {"priority": 0, "constraints": 1}, "replica": {"priority": 1, "constraints": 2}}
    fresh = {str(i): {"name": str(i), "nodesByState": {}} for i in range(P)}
    fp = problem.build_problem({}, fresh, nodes, [], nodes, model, node_hierarchy=hier,
                               hierarchy_rules={"replica": [{"includeLevel": 1, "excludeLevel": 0}]})
    rack = flags(fp, range(8, 12))
    return fp, [Change(removed=rack), Change(added=rack), Change(removed=flags(fp, [20, 21]))]


def seam_problem(P, M):
    if M == 2:
        return synth.config_flat(2, P=P, N=16)
    model = {"a": {"priority": 0, "constraints": 1}, "b": {"priority": 1, "constraints": 2}, "c": {"priority": 2, "constraints": 1}}
    fresh = {str(i): {"name": str(i), "nodesByState": {}} for i in range(P)}
    nodes = ["n%d" % i for i in range(7)]
    return problem.build_problem({}, fresh, nodes, [], nodes, model)


def warnings_case():
    """Two nodes for a replica constraint of five: every plan of it ends with warnings."""
    model = {"primary": {"priority": 0, "constraints": 1}, "replica": {"priority": 1, "constraints": 5}}
    fresh = {str(i): {"name": str(i), "nodesByState": {}} for i in range(5)}
    return problem.build_problem({}, fresh, ["a", "b", "c"], [], [], model)


# ---- refusals -------------------------------------------------------------------------------------------------------------

def _adopt_raw(pl, fp, removed="zeros", added="zeros", reserved=None):
    ad = abi.Adopt()
    keep = [np.zeros(max(fp.n_nodes_ext, 1), dtype=np.uint8) for _ in range(2)]
    if removed is not None:
        ad.node_removed = keep[0].ctypes.data_as(C.POINTER(C.c_uint8))
    if added is not None:
        ad.node_added = keep[1].ctypes.data_as(C.POINTER(C.c_uint8))
    ad.nodes_to_add_nil = 1
    for i, v in enumerate(reserved or []):
        ad.reserved[i] = v
    return pl.lib.blance_plan_adopt(pl._h, C.byref(ad))


def run_refusals(make_planner):
    pl = make_planner()
    try:
        fp = synth.config_flat(3, P=300, N=32)
        assert _adopt_raw(pl, fp) == abi.ERR_BAD_ARG                                   # a context that holds nothing
        pl.upload(fp)
        assert _adopt_raw(pl, fp) == abi.ERR_BAD_ARG                                   # uploaded, nothing planned
        assert b"nothing planned" in pl.lib.blance_last_error()
        pl.plan_resident()
        r0 = pl.download()
        want0 = _oracle(fp).digest()
        assert r0.digest() == want0

        def intact(tag):
            assert pl.download().digest() == want0, tag

        assert _adopt_raw(pl, fp, removed=None) == abi.ERR_BAD_ARG
        intact("null node_removed")
        assert _adopt_raw(pl, fp, added=None) == abi.ERR_BAD_ARG
        intact("null node_added")
        assert pl.lib.blance_plan_adopt(pl._h, None) == abi.ERR_BAD_ARG
        intact("null request")
        for slot in range(4):
            assert _adopt_raw(pl, fp, reserved=[0] * slot + [1]) == abi.ERR_BAD_ARG
            intact(("reserved", slot))
        pl.comm_set_callback(0, 1, lambda ptr, n: None)
        assert _adopt_raw(pl, fp) == abi.ERR_UNSUPPORTED
        intact("communicator of one rank")
        pl.comm_clear()
        pl.comm_set_callback(0, 2, lambda ptr, n: None, lambda ptr, n: None)
        assert _adopt_raw(pl, fp) == abi.ERR_UNSUPPORTED
        pl.comm_clear()
        intact("communicator of two ranks")
        # a plan that made no sweep holds no map
        fp_none = synth.config_flat(3, P=300, N=32, max_iterations=0)
        pl.upload(fp_none)
        pl.plan_resident()
        assert pl.download().iterations == 0
        assert _adopt_raw(pl, fp_none) == abi.ERR_BAD_ARG
        assert pl.download().iterations == 0
        # a batch leaves no problem on the context
        pl.plan(fp)
        pl.plan_batch([synth.config_flat(2, P=40, N=8)])
        assert _adopt_raw(pl, fp) == abi.ERR_BAD_ARG
        # after a successful adoption nothing is planned; an ordinary upload of another problem plans as ever
        pl.upload(fp)
        pl.plan_resident()
        pl.adopt()
        for call in (pl.download, lambda: pl.plan_stats(fp.n_states), lambda: pl.plan_moves(False, count_only=True)):
            with pytest.raises(hip.BlanceError) as e:
                call()
            assert e.value.status == abi.ERR_BAD_ARG
        with pytest.raises(ValueError):
            pl.adopt(node_removed=np.zeros(fp.n_nodes_ext + 1, dtype=np.uint8))
        other = synth.config_flat(2, P=500, N=24)
        assert pl.plan(other).digest() == _oracle(other).digest()
        pl.upload(fp)
        pl.plan_resident()
        assert pl.download().digest() == want0
    finally:
        pl.close()


# ---- the kernels alone ----------------------------------------------------------------------------------------------------

class AdoptKernels:
    """blance_case_adopt of tests/kernels/adopt_cases.inc."""

    def __init__(self, lib_path):
        self.lib = C.CDLL(lib_path)
        self.lib.blance_case_adopt.restype = C.c_int
        self.lib.blance_case_adopt.argtypes = [C.c_int] * 4 + [C.c_void_p] * 6 + [C.c_int] + [C.c_void_p] * 2 + [C.c_int] + \
            [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 2 + [C.c_int] + [C.c_void_p] * 2 + [C.c_int] + [C.c_void_p] * 2 + [C.c_int]

    def run(self, case, grid_len=0, slack=3):
        P, M, L = case["P"], case["M"], case["L"]
        PM = P * M
        total = int(kernel_reference(case)["off"][-1])
        o = {"len": np.full(PM + 1 + slack, POISON32, np.int32), "scanned": np.full(PM + 1 + slack, POISON32, np.int32),
             "res": np.zeros(16, np.int32),
             "a_off": np.full(PM + 1 + slack, POISON32, np.int32), "p_off": np.full(PM + 1 + slack, POISON32, np.int32),
             "a_nodes": np.full(total + slack, POISON32, np.int32), "p_nodes": np.full(total + slack, POISON32, np.int32),
             "a_kind": np.full(PM + slack, POISON8, np.uint8), "p_kind": np.full(PM + slack, POISON8, np.uint8),
             "in_prev": np.full(P + slack, POISON8, np.uint8), "never": np.full(P + slack, POISON8, np.uint8)}
        o["res"][[0, 2, 3, 14, 15]] = POISON32                  # the words of the summary block k_adopt_len does not own
        ins = [np.ascontiguousarray(case[k]) for k in ("k", "prv", "prv_len", "prv_kind", "part_weight", "part_has_weight")]
        ptr = lambda a: a.ctypes.data                            # noqa: E731
        st = self.lib.blance_case_adopt(P, M, L, case["weights_nil"], *[ptr(a) for a in ins], grid_len,
                                        ptr(o["len"]), ptr(o["scanned"]), PM + 1 + slack, ptr(o["res"]),
                                        ptr(o["a_off"]), ptr(o["p_off"]), PM + 1 + slack, ptr(o["a_nodes"]), ptr(o["p_nodes"]),
                                        total + slack, ptr(o["a_kind"]), ptr(o["p_kind"]), PM + slack, ptr(o["in_prev"]),
                                        ptr(o["never"]), P + slack)
        return st, o


def kernel_case(seed, P, M, L, weights=False, garbage=True):
    """A planned map by hand: kinds absent / nil / set, lengths 0 .. L, an absent list's length word anything at all, the
    rows' unused words poison."""
    rng = np.random.RandomState(seed)
    PM = P * M
    kind = rng.randint(0, 3, PM).astype(np.uint8)
    ln = rng.randint(0, L + 1, PM).astype(np.int32)
    ln[kind == abi.LIST_NIL] = 0
    ln[rng.randint(0, PM, max(PM // 7, 1))] = L
    ln[kind == abi.LIST_NIL] = 0
    prv = rng.randint(0, 8192, (PM, L)).astype(np.int32)
    lens = np.where(kind == abi.LIST_ABSENT, 0, ln)
    prv[np.arange(L)[None, :] >= lens[:, None]] = POISON32
    if garbage:
        ln[kind == abi.LIST_ABSENT] = rng.randint(-3, 70000, int((kind == abi.LIST_ABSENT).sum()))
    has = (rng.randint(0, 2, P) if weights else np.zeros(P)).astype(np.uint8)
    return {"P": P, "M": M, "L": L, "weights_nil": int(not weights), "k": rng.randint(-1, 5, M).astype(np.int32),
            "prv": prv.reshape(-1), "prv_len": ln, "prv_kind": kind,
            "part_weight": rng.randint(-50, 1000, P).astype(np.int32), "part_has_weight": has}


def kernel_reference(case):
    P, M, L = case["P"], case["M"], case["L"]
    PM = P * M
    kind = case["prv_kind"]
    lens = np.where(kind == abi.LIST_ABSENT, 0, np.clip(case["prv_len"], 0, L)).astype(np.int64)
    off = np.zeros(PM + 1, np.int64)
    off[1:] = np.cumsum(lens)
    rows = case["prv"].reshape(PM, L)
    nodes = rows[np.arange(L)[None, :] < lens[:, None]]
    k = case["k"].astype(np.int64)
    w = np.ones(P, np.int64)
    if not case["weights_nil"]:
        w = np.where(case["part_has_weight"] != 0, np.abs(case["part_weight"].astype(np.int64)), 1)
    kinds = 0
    for m in range(M):
        col = kind[m::M]
        kinds |= (1 << m) if (col == abi.LIST_ABSENT).any() else 0
        kinds |= (1 << (16 + m)) if (col != abi.LIST_ABSENT).any() else 0
    return {"len": lens, "off": off, "nodes": nodes, "kind": kind, "longest": int(lens.max()), "kinds": kinds,
            "cap": int(np.maximum(lens.reshape(P, M), k[None, :]).sum()), "aprev": int((lens.reshape(P, M).sum(axis=1) * w).sum()),
            "total": int(off[-1])}


KERNEL_SHAPES = [(1, 1, 1), (1, 2, 3), (85, 3, 2), (128, 2, 4), (257, 1, 59), (300, 3, 7), (3, 16, 3), (1000, 2, 1),
                 (127, 2, 9), (129, 2, 5), (64, 4, 8), (32768, 2, 2)]


def run_kernel_cases(ak):
    """Both kernels on maps by hand against kernel_reference; every word they do not own comes back as poison."""
    n = 0
    for i, (P, M, L) in enumerate(KERNEL_SHAPES):
        case = kernel_case(i, P, M, L, weights=bool(i % 2))
        want = kernel_reference(case)
        PM = P * M
        for grid_len in ([0, 1, 3] if PM < 4000 else [0]):
            st, o = ak.run(case, grid_len)
            tag = (P, M, L, grid_len)
            assert st == want["total"], tag
            assert np.array_equal(o["len"][:PM], want["len"]) and o["len"][PM] == 0 and (o["len"][PM + 1:] == POISON32).all(), tag
            assert np.array_equal(o["scanned"][:PM + 1], want["off"]) and (o["scanned"][PM + 1:] == POISON32).all(), tag
            res = o["res"]
            r64 = res[4:14].view(np.int64)
            assert res[1] == want["longest"] and int(res[10]) & 0xFFFFFFFF == want["kinds"], tag
            assert (r64[0], r64[2], r64[4]) == (want["cap"], want["aprev"], want["total"]), tag
            assert (res[[0, 2, 3, 14, 15]] == POISON32).all() and r64[1] == 0 and res[11] == 0, tag
            for pre in ("a_", "p_"):
                assert np.array_equal(o[pre + "off"][:PM + 1], want["off"]) and (o[pre + "off"][PM + 1:] == POISON32).all(), tag
                assert np.array_equal(o[pre + "nodes"][:want["total"]], want["nodes"]), tag
                assert (o[pre + "nodes"][want["total"]:] == POISON32).all(), tag
                assert np.array_equal(o[pre + "kind"][:PM], want["kind"]) and (o[pre + "kind"][PM:] == POISON8).all(), tag
            assert (o["in_prev"][:P] == 1).all() and (o["in_prev"][P:] == POISON8).all(), tag
            assert (o["never"][:P] == 0).all() and (o["never"][P:] == POISON8).all(), tag
            n += 1
    # the entry refuses what the kernels' buffers could not hold
    case = kernel_case(0, 4, 2, 3)
    st, _ = ak.run(dict(case, L=60, prv=np.zeros(4 * 2 * 60, np.int32)))
    assert st == -100
    return n


def write_program_input(path):
    """The shapes of the kernel cases for the stand-alone sanitizer program (tests/simt/adopt_asan_main.cpp): one line
    `P M L weights seed-free arrays`, every array as decimal words."""
    with open(path, "w") as f:
        for i, (P, M, L) in enumerate(KERNEL_SHAPES):
            if P * M > 4000:
                continue
            case = kernel_case(i, P, M, L, weights=bool(i % 2))
            want = kernel_reference(case)
            f.write("C %d %d %d %d %d\n" % (P, M, L, case["weights_nil"], want["total"]))
            for key in ("k", "prv", "prv_len", "prv_kind", "part_weight", "part_has_weight"):
                f.write(key + " " + " ".join(str(int(v)) for v in case[key]) + "\n")
            f.write("want " + " ".join(str(int(v)) for v in [want["longest"], want["kinds"], want["cap"], want["aprev"]]) + "\n")
            f.write("off " + " ".join(str(int(v)) for v in want["off"]) + "\n")
            f.write("nodes " + " ".join(str(int(v)) for v in want["nodes"]) + "\n")
