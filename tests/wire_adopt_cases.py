"""blance_wire_adopt: the cases tests/test_wire_adopt_emulated.py runs on the SIMT emulator and tests/test_wire_adopt_gpu.py on
the device, and the checks both make.  The definition every plan behind an adopted document is compared with is
problem.wire_adopted_problem -- over the lists the HOST decoder makes of the document -- planned by the C oracle; the
kernels alone (k_wire_adopt_sum, k_wire_adopt_write through tests/kernels/wire_adopt_cases.inc) are compared with
kernel_reference below."""
import ctypes as C
import json

import numpy as np
import pytest

import adopt_cases as A
from blance_amd import abi, hip, planner, problem, synth, wire
from helpers import build_from_case

POISON32, POISON8 = -0x5A5A5A5B, 0xA5
INT_MAX = 2 ** 31 - 1
WHY = abi.WIRE_ADOPT


def _oracle(fp):
    from oracle import loader
    return loader.plan(fp)


same = A.same


def host_lists(wdict, doc):
    """The document through the host decoder, in the dictionary's ids (independent of the device's decoder)."""
    wm = wire.decode(bytes(doc))
    try:
        return planner.lists_of_wire_map(wm, wdict)
    finally:
        wm.close()


def row_stride(fp):
    """c->L of an upload of fp: the longest list or constraint."""
    PM = fp.n_parts * fp.n_states
    lens = [int(np.diff(fp.assign_off[:PM + 1]).max()), int(np.diff(fp.prev_off[:PM + 1]).max())] if PM else []
    return max([1] + [int(k) for k in fp.state_constraints[:fp.n_states]] + lens)


def dumps(m):
    return json.dumps(m, separators=(",", ":")).encode()


class Held:
    """A planner with the problem it holds as arrays (`fp`), the row stride its upload fixed and a dictionary of its names."""

    def __init__(self, pl, fp):
        self.pl, self.fp = pl, A.named(fp)
        pl.upload(fp)
        pl.set_wire_names(fp)
        self.wdict = pl.wire_dict(fp)
        self.L = row_stride(fp)

    def close(self):
        self.wdict.close()

    def expect(self, doc, ch, assign_too):
        return problem.wire_adopted_problem(self.fp, host_lists(self.wdict, doc), ch.removed, ch.added, ch.add_nil, assign_too,
                                            ch.keep, row_stride=self.L)

    def adopt_wire(self, doc, ch, assign_too, tag):
        """adopt_wire on the device route -- never the host's --, and the definition of what the planner holds then."""
        nxt = self.expect(doc, ch, assign_too)
        info = self.pl.adopt_wire(self.wdict, doc, assign_too=assign_too, **ch.kw())
        assert info["adopted"] and info["refusal"] == 0 and info["why"] == 0, (tag, info)
        lists = host_lists(self.wdict, doc)
        assert info["n_node_refs"] == lists["n_node_refs"] and info["n_parts_seen"] == lists["n_parts_seen"], (tag, info)
        assert info["result_capacity"] == nxt.result_capacity(), (tag, info)
        assert info["refusal_at"] == -1 and info["why_at"] == -1, (tag, info)
        for call in (self.pl.download, lambda: self.pl.plan_stats(self.fp.n_states), lambda: self.pl.plan_moves(False, count_only=True),
                     lambda: self.pl.plan_wire(size_only=True)):
            with pytest.raises(hip.BlanceError) as e:
                call()
            assert e.value.status == abi.ERR_BAD_ARG, tag
        nxt.part_names, nxt.node_names, nxt.state_names = self.fp.part_names, self.fp.node_names, self.fp.state_names
        self.fp = nxt
        return nxt

    def plan_and_check(self, pl2, tag, around=True, stats=True):
        """plan_resident of the held problem against the oracle, a fresh upload on pl2 and a second plan; the readers."""
        want = _oracle(self.fp)
        st = self.pl.plan_resident()
        got = self.pl.download()
        assert st.iterations == want.iterations, tag
        same(got, want, tag)
        same(pl2.plan(self.fp), want, (tag, "fresh upload"))
        self.pl.plan_resident()
        same(self.pl.download(), want, (tag, "planned twice"))
        if around and got.iterations > 0:
            self.readers(got, tag, stats)
        return got

    def readers(self, res, tag, stats=True):
        from oracle import stats_ref
        from test_plan_moves_emulated import same_moves, via_calc_moves
        fp, pl = self.fp, self.pl
        doc, _ = pl.plan_wire()
        assert doc == wire.ResultEncoder(fp.part_names, fp.node_names, fp.state_names).encode(res), tag
        for favor in (False, True):
            mv, minfo = pl.plan_moves(favor)
            same_moves(mv, via_calc_moves(pl, fp, res, None, favor), (tag, favor))
            assert minfo["n_moves"] == len(mv[1])
        if stats:
            got, want = pl.plan_stats(fp.n_states), stats_ref.plan_stats(fp, res)
            assert got["n_nodes_next"] == want["n_nodes_next"], tag
            for key in ("load_min", "load_max", "load_sum", "load_sumsq", "nodes_used", "unmet_slots", "rule_violations"):
                assert np.array_equal(np.asarray(got[key], dtype=np.int64), np.asarray(want[key], dtype=np.int64)), (tag, key)
        return doc


# ---- family 1: equal to blance_plan_adopt ---------------------------------------------------------------------------------

def equal_to_adopt(pls, fp, ch, tag, around=False):
    """Planner a plans fp and adopts its plan; planner b holds fp and adopts a's document.  Both plans, a fresh upload of
    wire_adopted_problem on c and the oracle are equal.  Returns the adopted plan, or None when fp's plan made no sweep (it
    has no map, and blance_plan_wire_get no document)."""
    a, b, c = pls
    A.named(fp)
    a.upload(fp)
    a.set_wire_names(fp)
    a.plan_resident()
    res = a.download()
    if res.iterations == 0:
        return None
    doc, _ = a.plan_wire()
    hb = Held(b, fp)
    try:
        nxt = hb.adopt_wire(doc, ch, True, tag)
        via_plan = problem.adopted_problem(fp, res, ch.removed, ch.added, ch.add_nil, ch.keep)
        for name in sorted(via_plan.arrays):
            assert np.array_equal(np.asarray(via_plan.arrays[name]), np.asarray(nxt.arrays[name])), (tag, name)
        assert via_plan.scalars == nxt.scalars, tag
        a.adopt(**ch.kw())
        want = _oracle(nxt)
        sa, sb = a.plan_resident(), b.plan_resident()
        ga, gb = a.download(), b.download()
        assert sa.iterations == sb.iterations == want.iterations, tag
        same(ga, want, (tag, "blance_plan_adopt"))
        same(gb, want, (tag, "blance_wire_adopt"))
        same(c.plan(nxt), want, (tag, "fresh upload"))
        if around:
            hb.readers(gb, tag)
        return gb
    finally:
        hb.close()


def run_equal_golden(pls, golden_cases, keep):
    n, sweeps2, no_map = 0, 0, 0
    for i, case in enumerate(golden_cases):
        fp = build_from_case(case)
        if pls[0].validate(fp) != abi.OK:
            continue
        got = equal_to_adopt(pls, fp, A.golden_change(fp, i, keep), ("golden", case["source"], keep), around=i % 5 == 0)
        if got is None:
            no_map += 1
            continue
        n += 1
        sweeps2 += got.iterations >= 2
    assert n >= 60, (n, no_map)
    return n, sweeps2


def run_equal_random(pls, seed):
    n = 0
    for i, fp in enumerate(A.mixed_problems(seed)):
        if pls[0].validate(fp) != abi.OK:
            continue
        alive = [x for x in range(fp.n_nodes) if not fp.node_removed[x]]
        gone = A.flags(fp, alive[1::3]) if len(alive) >= 3 else None
        ch = A.Change(removed=gone, keep=bool(i % 2)) if i % 3 else A.Change(added=gone, keep=bool(i % 2))
        if equal_to_adopt(pls, fp, ch, ("random", seed, i), around=i % 7 == 0) is not None:
            n += 1
    return n


# ---- family 2: documents that are not the plan ----------------------------------------------------------------------------

MODEL = {"primary": {"priority": 0, "constraints": 1}, "replica": {"priority": 1, "constraints": 2}}
NODES = ["n%d" % i for i in range(8)]


def mutant_base(P=41, prev=True):
    """41 partitions over 8 nodes and one more node name outside nodesAll ("zz", known from the node weights), a model of
    1 + 2 copies; one prevMap list of three nodes makes the rows three wide.  prev=False: the same call with prevMap = {}."""
    assign, pm = {}, {}
    for i in range(P):
        name = "p%02d" % i
        nbs = {"primary": [NODES[i % 5]], "replica": [NODES[(i + 1) % 5], NODES[(i + 3) % 5]]}
        if i % 9 == 4:
            nbs = {"primary": [NODES[i % 5]]}
        assign[name] = {"name": name, "nodesByState": nbs}
        pm[name] = {"name": name, "nodesByState": {"primary": [NODES[(i + 2) % 8]], "replica": [NODES[(i + 4) % 8]]}}
    pm["p00"]["nodesByState"]["replica"] = [NODES[4], NODES[5], NODES[6]]
    return problem.build_problem(pm if prev else {}, assign, NODES, [], None, MODEL, node_weights={"zz": 3, "n1": 2})


def mutants(planned, rng):
    """(name, document, legal with assign_too, node removal allowed) from the planned map (a dict as json.loads gives it)."""
    def copy():
        return json.loads(json.dumps(planned))
    names = list(planned)
    out = []
    m = copy()
    for nm in names[3::7]:
        del m[nm]
    out.append(("dropped", m, False, False))
    m = copy()
    m[names[0]]["nodesByState"] = None
    del m[names[5]]["nodesByState"]
    m[names[-1]]["nodesByState"] = None
    out.append(("nil-map", m, True, True))
    m = copy()
    m[names[1]]["nodesByState"]["primary"] = None
    m[names[2]]["nodesByState"]["replica"] = []
    m[names[6]]["nodesByState"].pop("replica", None)
    m[names[-1]]["nodesByState"] = {}
    out.append(("lists-nil-empty-absent", m, True, True))
    m = copy()
    for nm in names:
        for lst in m[nm]["nodesByState"].values():
            if lst:
                rng.shuffle(lst)
    m = {nm: m[nm] for nm in sorted(names, key=lambda x: rng.random())}
    out.append(("shuffled", m, True, True))
    m = copy()
    m[names[4]]["nodesByState"]["replica"] = ["zz", "n0"]
    m[names[9]]["nodesByState"]["primary"] = ["zz"]
    out.append(("beyond-nodes-all", m, True, True))
    m = copy()
    m[names[0]]["nodesByState"]["replica"] = ["n1", "n1"]
    m[names[20]]["nodesByState"]["replica"] = ["n2", "n3", "n2"]
    m[names[-1]]["nodesByState"]["primary"] = ["n7", "n7"]
    out.append(("duplicates", m, False, True))
    out.append(("empty-document", {}, False, False))
    return out


def run_mutants(pl, pl2):
    """Every mutant with assign_too 0 and 1 where it is legal: the plan that follows against the oracle's plan of
    wire_adopted_problem and a fresh upload, the three readers, then a second adopt_wire (the new plan's own document, with a
    node change) and a plain adopt -- each planned and compared again."""
    rng = np.random.RandomState(7)
    base = mutant_base()
    pl.upload(A.named(base))
    pl.set_wire_names(base)
    pl.plan_resident()
    planned = json.loads(pl.plan_wire()[0])
    n, never, absent_parts = 0, 0, 0
    for name, m, with_assign, may_remove in mutants(planned, rng):
        for assign_too in ([False, True] if with_assign else [False]):
            for keep in (False, True):
                tag = ("mutant", name, assign_too, keep)
                h = Held(pl, mutant_base())
                try:
                    ch = A.Change(removed=A.flags(h.fp, [2]) if may_remove else None, added=None if may_remove else A.flags(h.fp, [7]),
                                  keep=keep)
                    nxt = h.adopt_wire(dumps(m), ch, assign_too, tag)
                    never += int(nxt.part_prev_never_equal.sum())
                    absent_parts += int((nxt.part_in_prev == 0).sum())
                    got = h.plan_and_check(pl2, tag)
                    if name == "empty-document" and not keep:
                        nothing = mutant_base(prev=False)
                        nothing.set("node_added", ch.added)
                        nothing.scalars["nodes_to_add_nil"] = 0
                        same(got, _oracle(nothing), (tag, "a plan from nothing"))
                    # the map the cluster has now is the new plan, but for one partition whose moves did not complete
                    m2 = json.loads(pl.plan_wire()[0])
                    first = sorted(m2)[0]
                    m2[first]["nodesByState"] = {"primary": ["n6"], "replica": []}
                    ch2 = A.Change(removed=A.flags(h.fp, [3]), keep=keep)
                    h.adopt_wire(dumps(m2), ch2, True, (tag, "second"))
                    res2 = h.plan_and_check(pl2, (tag, "second"), stats=False)
                    pl.adopt(node_added=A.flags(h.fp, [3]), nodes_to_add_nil=False, keep_prev_only=keep)
                    h.fp = problem.adopted_problem(h.fp, res2, None, A.flags(h.fp, [3]), False, keep)
                    h.fp.part_names, h.fp.node_names, h.fp.state_names = base.part_names, base.node_names, base.state_names
                    h.plan_and_check(pl2, (tag, "plain adopt"), stats=False)
                    n += 1
                finally:
                    h.close()
    assert never > 0 and absent_parts > 0
    return n


# ---- family 3: seams ------------------------------------------------------------------------------------------------------

def run_seam(pls, P, M):
    fp = A.seam_problem(P, M)
    ch = A.Change(removed=A.flags(fp, [1]))
    got = equal_to_adopt(pls, fp, ch, ("seam", P, M), around=True)
    assert got is not None


def run_scan_split(pls):
    """P * M + 1 = 65,537 list offsets: the decoder's launch_scan_excl goes from one launch to three."""
    from test_plan_moves_emulated import scan_split_problem
    fp = scan_split_problem()
    assert fp.n_parts * fp.n_states + 1 == 65537
    assert equal_to_adopt(pls, fp, A.Change(removed=A.flags(fp, [3])), "scan split") is not None


def seam_base(P=300):
    """Rows of exactly three words (the replica constraint), every list shorter."""
    model = {"primary": {"priority": 0, "constraints": 1}, "replica": {"priority": 1, "constraints": 3}}
    assign = {"p%03d" % i: {"name": "p%03d" % i, "nodesByState": {"primary": [NODES[i % 8]], "replica": [NODES[(i + 1) % 8]]}}
              for i in range(P)}
    return problem.build_problem({}, assign, NODES, [], None, model)


def run_row_stride(pl, pl2):
    """A list of exactly L entries is accepted, one of L + 1 refused -- at the first, a middle and the last list, alone and
    together: why_at is the smallest offender."""
    h = Held(pl, seam_base())
    try:
        assert h.L == 3
        P, M = h.fp.n_parts, h.fp.n_states
        names = h.fp.part_names
        full = {nm: {"name": nm, "nodesByState": {"primary": ["n0"], "replica": ["n1", "n2"]}} for nm in names}
        at = [(0, 0), (P // 2, 1), (P - 1, 1)]

        def with_lists(spots, lst):
            m = json.loads(json.dumps(full))
            for p, s in spots:
                m[names[p]]["nodesByState"][h.fp.state_names[s]] = list(lst)
            return m

        exact = with_lists(at, ["n3", "n4", "n5"])
        h.adopt_wire(dumps(exact), A.Change(), True, "L entries")
        h.plan_and_check(pl2, "L entries", stats=False)
        for spots in ([at[0]], [at[1]], [at[2]], at[1:], at):
            for assign_too in (True, False):
                over = with_lists(spots, ["n3", "n4", "n5", "n6"])
                info = pl.adopt_wire(h.wdict, dumps(over), assign_too=assign_too)
                want_at = min(p * M + s for p, s in spots)
                assert (info["adopted"], info["refusal"], info["why"], info["why_at"]) == (False, 0, WHY["list_too_long"], want_at), (spots, info)
                with pytest.raises(problem.Unsupported) as e:
                    h.expect(dumps(over), A.Change(), assign_too)
                assert (e.value.why, e.value.why_at) == (WHY["list_too_long"], want_at)
        for spots in ([at[0]], [at[1]], [at[2]], at[1:], at):
            dup = with_lists(spots, ["n3", "n4", "n3"])
            info = pl.adopt_wire(h.wdict, dumps(dup), assign_too=True)
            want_at = min(p * M + s for p, s in spots)
            assert (info["adopted"], info["why"], info["why_at"]) == (False, WHY["duplicate_node"], want_at), (spots, info)
            with pytest.raises(problem.Unsupported) as e:
                h.expect(dumps(dup), A.Change(), True)
            assert (e.value.why, e.value.why_at) == (WHY["duplicate_node"], want_at)
            missing = json.loads(json.dumps(full))
            for p, _ in spots:
                del missing[names[p]]
            info = pl.adopt_wire(h.wdict, dumps(missing), assign_too=True)
            want_p = min(p for p, _ in spots)
            assert (info["adopted"], info["why"], info["why_at"]) == (False, WHY["partition_missing"], want_p), (spots, info)
            info = pl.adopt_wire(h.wdict, dumps(missing), assign_too=False, node_removed=A.flags(h.fp, [1]))
            assert (info["adopted"], info["why"], info["why_at"]) == (False, WHY["removed_without_prev"], want_p), (spots, info)
        # over-long wins over a duplicate in an earlier list: the order of the codes
        both = with_lists([(P - 1, 0)], ["n1", "n2", "n3", "n4"])
        both[names[0]]["nodesByState"]["replica"] = ["n5", "n5"]
        info = pl.adopt_wire(h.wdict, dumps(both), assign_too=True)
        assert (info["why"], info["why_at"]) == (WHY["list_too_long"], (P - 1) * M), info
        # after all these refusals the planner still holds the problem of the last success, and its plan
        same(pl.download(), _oracle(h.fp), "refusals left the plan")
    finally:
        h.close()


# ---- family 4: every refusal leaves the context as found ------------------------------------------------------------------

def _raw(pl, wdict, doc, fp, **over):
    wa = abi.WireAdopt()
    keep = [np.zeros(max(fp.n_nodes_ext, 1), dtype=np.uint8) for _ in range(2)]
    buf = C.create_string_buffer(bytes(doc), len(doc) + 1)
    wa.dict, wa.json, wa.len = wdict._h if wdict is not None else None, C.cast(buf, C.c_void_p).value, len(doc)
    wa.node_removed = keep[0].ctypes.data_as(C.POINTER(C.c_uint8))
    wa.node_added = keep[1].ctypes.data_as(C.POINTER(C.c_uint8))
    wa.nodes_to_add_nil, wa.assign_too = 1, 1
    for key, v in over.items():
        if key == "reserved":
            for i, x in enumerate(v):
                wa.reserved[i] = x
        else:
            setattr(wa, key, v)
    return pl.lib.blance_wire_adopt(pl._h, C.byref(wa)), wa


def overflow_base():
    """Partition weights just inside the int32 load bound for lists of one node, beyond it for lists of three."""
    model = {"primary": {"priority": 0, "constraints": 1}, "replica": {"priority": 1, "constraints": 3}}
    names = ["p%d" % i for i in range(4)]
    assign = {nm: {"name": nm, "nodesByState": {"primary": [NODES[0]], "replica": [NODES[1]]}} for nm in names}
    return problem.build_problem({}, assign, NODES, [], None, model, partition_weights={nm: 50000000 for nm in names})


def run_refusals(make_planner):
    pl = make_planner()
    other = make_planner()
    try:
        fp = A.named(synth.config_flat(3, P=300, N=32))
        wd_early = pl.wire_dict(fp)
        good = None
        st, wa = _raw(pl, wd_early, b"{}", fp)
        assert st == abi.ERR_BAD_ARG and b"no problem" in pl.lib.blance_last_error()          # a context that holds nothing
        pl.upload(fp)
        pl.set_wire_names(fp)
        pl.plan_resident()
        r0 = pl.download()
        want0 = _oracle(fp).digest()
        assert r0.digest() == want0
        good, _ = pl.plan_wire()
        moves0 = pl.plan_moves(False)[0]
        stats0 = pl.plan_stats(fp.n_states)
        P, M = fp.n_parts, fp.n_states

        def intact(tag):
            from test_plan_moves_emulated import same_moves
            again = pl.download()
            for name in ("out_off", "out_nodes", "out_kind", "warn_part", "warn_state"):
                assert getattr(again, name).tobytes() == getattr(r0, name).tobytes(), (tag, name)
            assert again.digest() == want0, tag
            assert pl.plan_wire()[0] == good, tag
            same_moves(pl.plan_moves(False)[0], moves0, tag)
            assert np.array_equal(pl.plan_stats(fp.n_states)["load_sum"], stats0["load_sum"]), tag

        planned = json.loads(good)
        names = fp.part_names
        # the five reasons
        over = json.loads(good)
        over[names[7]]["nodesByState"]["replica"] = ["n0001", "n0002", "n0003", "n0004", "n0005"]
        pl_dict = wd_early
        info = pl.adopt_wire(pl_dict, dumps(over))
        assert (info["adopted"], info["refusal"], info["why"], info["why_at"]) == (False, 0, WHY["list_too_long"], 7 * M + fp.state_names.index("replica")), info
        intact("list too long")
        miss = json.loads(good)
        del miss[names[11]]
        info = pl.adopt_wire(pl_dict, dumps(miss))
        assert (info["why"], info["why_at"]) == (WHY["partition_missing"], 11), info
        intact("partition missing")
        info = pl.adopt_wire(pl_dict, dumps(miss), assign_too=False, node_removed=A.flags(fp, [0]))
        assert (info["why"], info["why_at"]) == (WHY["removed_without_prev"], 11), info
        intact("removed without prev")
        dup = json.loads(good)
        lst = dup[names[200]]["nodesByState"]["primary"]
        dup[names[200]]["nodesByState"]["primary"] = [lst[0], lst[0]] if row_stride(fp) >= 2 else lst
        info = pl.adopt_wire(pl_dict, dumps(dup))
        assert (info["why"], info["why_at"]) == (WHY["duplicate_node"], 200 * M + fp.state_names.index("primary")), info
        intact("duplicate")
        # one refusal of the document itself: exactly the decoder's
        bad = good[:-1] + b',"nobody":{"name":"nobody","nodesByState":{}}}'
        dec = pl.decode_wire(pl_dict, bad)
        info = pl.adopt_wire(pl_dict, bad)
        assert dec["refusal"] == abi.WIRE_REFUSED["unknown_partition"]
        assert (info["adopted"], info["refusal"], info["refusal_at"], info["why"]) == (False, dec["refusal"], dec["refusal_at"], 0), info
        intact("document refusal")
        # BAD_ARG, each one
        assert pl.lib.blance_wire_adopt(pl._h, None) == abi.ERR_BAD_ARG
        for over_kw in (dict(dict=None), dict(json=None), dict(node_removed=None), dict(node_added=None)):
            st, wa = _raw(pl, pl_dict, good, fp, **over_kw)
            assert st == abi.ERR_BAD_ARG and wa.why == 0 and wa.refusal == 0, over_kw
            intact(("null", tuple(over_kw)))
        for slot in range(4):
            st, _ = _raw(pl, pl_dict, good, fp, reserved=[0] * slot + [1])
            assert st == abi.ERR_BAD_ARG
            intact(("reserved", slot))
        foreign = other.wire_dict(fp)
        st, _ = _raw(pl, foreign, good, fp)
        assert st == abi.ERR_BAD_ARG and b"not one of this context" in pl.lib.blance_last_error()
        intact("foreign dictionary")
        foreign.close()
        small = A.named(synth.config_flat(3, P=299, N=32))
        wd_small = pl.wire_dict(small)
        st, _ = _raw(pl, wd_small, b"{}", fp)
        assert st == abi.ERR_BAD_ARG and b"sizes" in pl.lib.blance_last_error()
        intact("dictionary sizes")
        wd_small.close()
        # a communicator
        pl.comm_set_callback(0, 1, lambda ptr, n: None)
        st, wa = _raw(pl, pl_dict, good, fp)
        assert st == abi.ERR_UNSUPPORTED and wa.why == 0 and wa.refusal == 0
        pl.comm_clear()
        intact("communicator of one rank")
        pl.comm_set_callback(0, 2, lambda ptr, n: None, lambda ptr, n: None)
        st, _ = _raw(pl, pl_dict, good, fp)
        assert st == abi.ERR_UNSUPPORTED
        pl.comm_clear()
        intact("communicator of two ranks")
        # ... and plan_resident gives the same plan again
        pl.plan_resident()
        intact("planned again")
        with pytest.raises(ValueError):
            pl.adopt_wire(pl_dict, good, node_removed=np.zeros(fp.n_nodes_ext + 1, dtype=np.uint8))
        assert planned
        wd_early.close()
        # the load bound, on a problem of its own
        fo = A.named(overflow_base())
        pl.upload(fo)
        wd = pl.wire_dict(fo)
        pl.plan_resident()
        before = pl.download().digest()
        heavy = {nm: {"name": nm, "nodesByState": {"primary": ["n0"], "replica": ["n1", "n2", "n3"]}} for nm in fo.part_names}
        info = pl.adopt_wire(wd, dumps(heavy))
        assert (info["adopted"], info["refusal"], info["why"], info["why_at"]) == (False, 0, WHY["load_overflow"], -1), info
        with pytest.raises(problem.Unsupported) as e:
            problem.wire_adopted_problem(fo, host_lists(wd, dumps(heavy)), row_stride=3)
        assert e.value.why == WHY["load_overflow"]
        assert pl.download().digest() == before
        light = {nm: {"name": nm, "nodesByState": {"primary": ["n0"], "replica": ["n1"]}} for nm in fo.part_names}
        assert pl.adopt_wire(wd, dumps(light))["adopted"]
        wd.close()
    finally:
        pl.close()
        other.close()


# ---- family 6: adopt_partition_map ----------------------------------------------------------------------------------------

def run_switch(pl, pl2):
    """The device route and the forced host route leave the same problem (its plans are equal, and equal to the oracle's); a
    document the device refuses and a list beyond the rows go the host route by themselves; the other reasons raise."""
    base = A.named(mutant_base())
    pl.upload(base)
    pl.set_wire_names(base)
    pl.plan_resident()
    planned = json.loads(pl.plan_wire()[0])
    rng = np.random.RandomState(3)
    ch = A.Change(added=A.flags(base, [6]))
    n = 0
    for name, m, with_assign, _ in mutants(planned, rng):
        for assign_too in ([False, True] if with_assign else [False]):
            doc = dumps(m)
            plans = {}
            for route in ("device", "host"):
                fp = A.named(mutant_base())
                pl.upload(fp)
                wd = pl.wire_dict(fp)
                info = planner.adopt_partition_map(pl, wd, doc, fp, assign_too=assign_too, force_host=route == "host", **ch.kw())
                assert info["route"] == route and info["adopted"], (name, route, info)
                pl.plan_resident()
                plans[route] = pl.download()
                want = problem.wire_adopted_problem(fp, host_lists(wd, doc), ch.removed, ch.added, ch.add_nil, assign_too, ch.keep,
                                                    row_stride=row_stride(fp))
                same(plans[route], _oracle(want), (name, assign_too, route))
                wd.close()
            assert plans["device"].digest() == plans["host"].digest(), (name, assign_too)
            n += 1
    fp = A.named(mutant_base())
    pl.upload(fp)
    wd = pl.wire_dict(fp)
    # the device refuses a repeated key (Go: the last one wins): the host route by itself
    names = list(planned)
    rep = dumps(planned)[:-1] + b"," + dumps({names[0]: {"name": names[0], "nodesByState": {"primary": ["n7"]}}})[1:]
    info = planner.adopt_partition_map(pl, wd, rep, fp, **ch.kw())
    assert info["route"] == "host" and info["refusal"] == abi.WIRE_REFUSED["repeated_partition"], info
    pl.plan_resident()
    same(pl.download(), _oracle(info["problem"]), "repeated key")
    assert info["problem"].prev_nodes[info["problem"].prev_off[0]] == fp.node_names.index("n7")
    # a list of four nodes where the rows hold three
    pl.upload(fp)
    long_doc = json.loads(json.dumps(planned))
    long_doc[names[3]]["nodesByState"]["replica"] = ["n0", "n1", "n2", "n3"]
    info = planner.adopt_partition_map(pl, wd, dumps(long_doc), fp, **ch.kw())
    assert info["route"] == "host" and info["why"] == WHY["list_too_long"], info
    pl.plan_resident()
    same(pl.download(), _oracle(info["problem"]), "long list")
    # the other reasons raise on both routes
    pl.upload(fp)
    miss = json.loads(json.dumps(planned))
    del miss[names[2]]
    for force in (False, True):
        with pytest.raises(problem.Unsupported) as e:
            planner.adopt_partition_map(pl, wd, dumps(miss), fp, force_host=force)
        assert (e.value.why, e.value.why_at) == (WHY["partition_missing"], 2)
    wd.close()
    return n


# ---- family 5: the kernels alone ------------------------------------------------------------------------------------------

class WireAdoptKernels:
    """blance_case_wire_adopt of tests/kernels/wire_adopt_cases.inc."""

    def __init__(self, lib_path):
        self.lib = C.CDLL(lib_path)
        self.lib.blance_case_wire_adopt.restype = C.c_int
        self.lib.blance_case_wire_adopt.argtypes = [C.c_int] * 5 + [C.c_void_p] * 9 + [C.c_int] * 2 + [C.c_void_p] * 3 + [C.c_int] + \
            [C.c_void_p] * 2 + [C.c_int] + [C.c_void_p] * 2 + [C.c_int] + [C.c_void_p] * 2 + [C.c_int]

    def run(self, case, grid_sum=0, grid_write=0, slack=3):
        P, M = case["P"], case["M"]
        PM = P * M
        total = int(case["off"][-1])
        o = {"res": np.full(16, POISON32, np.int32),
             "a_off": np.full(PM + 1 + slack, POISON32, np.int32), "p_off": np.full(PM + 1 + slack, POISON32, np.int32),
             "a_nodes": np.full(total + slack, POISON32, np.int32), "p_nodes": np.full(total + slack, POISON32, np.int32),
             "a_kind": np.full(PM + slack, POISON8, np.uint8), "p_kind": np.full(PM + slack, POISON8, np.uint8),
             "in_prev": np.full(P + slack, POISON8, np.uint8), "never": np.full(P + slack, POISON8, np.uint8)}
        o["res"][[1, 2, 4, 5, 8, 9, 10, 12, 13]] = 0                    # the driver's preset: sums zero, first offenders INT_MAX
        o["res"][[0, 3, 11]] = INT_MAX
        nodes = case["nodes"] if total else np.zeros(1, np.int32)
        ins = [np.ascontiguousarray(a) for a in (case["k"], case["part_kind"], case["off"], case["kind"], nodes, case["cur_a_off"],
                                                 case["cur_a_kind"], case["part_weight"], case["part_has_weight"])]
        ptr = lambda a: a.ctypes.data                            # noqa: E731
        st = self.lib.blance_case_wire_adopt(P, M, case["L"], case["weights_nil"], case["assign_too"], *[ptr(a) for a in ins],
                                             grid_sum, grid_write, ptr(o["res"]), ptr(o["a_off"]), ptr(o["p_off"]), PM + 1 + slack,
                                             ptr(o["a_nodes"]), ptr(o["p_nodes"]), total + slack, ptr(o["a_kind"]), ptr(o["p_kind"]),
                                             PM + slack, ptr(o["in_prev"]), ptr(o["never"]), P + slack)
        return st, o


def kernel_case(seed, P, M, L, assign_too, weights=False):
    """A decoded document by hand: partitions absent / nil / set, lists absent / nil / set of 0 .. L + 2 entries, duplicates
    here and there; beside it the lists to assign a context might hold."""
    rng = np.random.RandomState(seed)
    PM = P * M
    part_kind = rng.choice([0, 1, 2, 2, 2, 2], P).astype(np.uint8)
    if seed % 3 == 0:
        part_kind[:] = 2
    kind = rng.randint(0, 3, PM).astype(np.uint8)
    kind[np.repeat(part_kind != 2, M)] = 0
    ln = rng.randint(0, L + 1, PM)
    if seed % 2:
        ln[rng.randint(0, PM, max(PM // 50, 1))] = L + rng.randint(1, 3)
    ln[rng.randint(0, PM, max(PM // 9, 1))] = L
    ln[kind != 2] = 0
    off = np.zeros(PM + 1, np.int32)
    off[1:] = np.cumsum(ln)
    nodes = np.zeros(int(off[-1]), np.int32)
    for i in range(PM):                                     # distinct ids inside a list, but for a few
        n = int(ln[i])
        if n:
            ids = rng.choice(4096, n, replace=False)
            if n >= 2 and rng.randint(0, 23) == 0:
                ids[rng.randint(1, n)] = ids[0]
            nodes[off[i]:off[i + 1]] = ids
    cur_len = rng.randint(0, L + 1, PM)
    cur_off = np.zeros(PM + 1, np.int32)
    cur_off[1:] = np.cumsum(cur_len)
    has = (rng.randint(0, 2, P) if weights else np.zeros(P)).astype(np.uint8)
    return {"P": P, "M": M, "L": L, "weights_nil": int(not weights), "assign_too": int(assign_too),
            "k": rng.randint(-1, 5, M).astype(np.int32), "part_kind": part_kind, "off": off, "kind": kind, "nodes": nodes,
            "cur_a_off": cur_off, "cur_a_kind": rng.randint(0, 3, PM).astype(np.uint8),
            "part_weight": rng.randint(-50, 1000, P).astype(np.int32), "part_has_weight": has}


def kernel_reference(case):
    P, M, L = case["P"], case["M"], case["L"]
    PM = P * M
    off = case["off"].astype(np.int64)
    lens = np.diff(off)
    a_lens = lens if case["assign_too"] else np.diff(case["cur_a_off"].astype(np.int64))
    a_kind = case["kind"] if case["assign_too"] else case["cur_a_kind"]
    k = case["k"].astype(np.int64)
    w = np.ones(P, np.int64)
    if not case["weights_nil"]:
        w = np.where(case["part_has_weight"] != 0, np.abs(case["part_weight"].astype(np.int64)), 1)
    kinds = 0
    for m in range(M):
        col = a_kind[m::M]
        kinds |= (1 << m) if (col == abi.LIST_ABSENT).any() else 0
        kinds |= (1 << (16 + m)) if (col != abi.LIST_ABSENT).any() else 0
    over = np.flatnonzero(lens > L)
    dups = []
    if case["assign_too"]:
        dups = [i for i in np.flatnonzero((lens >= 2) & (lens <= L))
                if len(set(case["nodes"][off[i]:off[i + 1]].tolist())) != lens[i]]
    absent = np.flatnonzero(case["part_kind"] == abi.LIST_ABSENT)
    per_part = lens.reshape(P, M).sum(axis=1)
    return {"first_long": int(over[0]) if over.size else INT_MAX, "longest": int(max(lens.max(), a_lens.max())),
            "fresh": int(absent.size), "first_missing": int(absent[0]) if absent.size else INT_MAX, "kinds": kinds,
            "first_dup": int(dups[0]) if dups else INT_MAX,
            "cap": int(np.maximum(a_lens.reshape(P, M), k[None, :]).sum()),
            "aprev": int((per_part * w)[case["part_kind"] != abi.LIST_ABSENT].sum()), "total": int(a_lens.sum())}


KERNEL_SHAPES = [(1, 1, 1), (1, 2, 3), (85, 3, 2), (128, 2, 4), (257, 1, 59), (300, 3, 7), (3, 16, 3), (1000, 2, 1), (127, 2, 9),
                 (129, 2, 5), (64, 4, 8), (15, 1, 2), (16, 1, 2), (17, 1, 2), (32768, 2, 2)]


def check_kernel_case(o, case, want, tag, slack=3):
    P, M = case["P"], case["M"]
    PM = P * M
    total = int(case["off"][-1])
    res = o["res"]
    r64 = res[4:14].view(np.int64)
    assert (res[0], res[1], res[2], res[3], res[11]) == (want["first_long"], want["longest"], want["fresh"], want["first_missing"],
                                                         want["first_dup"]), (tag, res, want)
    assert int(res[10]) & 0xFFFFFFFF == want["kinds"], tag
    assert (r64[0], r64[2], r64[4]) == (want["cap"], want["aprev"], want["total"]), tag
    assert (res[[6, 7, 14, 15]] == POISON32).all(), tag                  # the words of the block the kernel does not own
    assert np.array_equal(o["p_off"][:PM + 1], case["off"]) and (o["p_off"][PM + 1:] == POISON32).all(), tag
    assert np.array_equal(o["p_nodes"][:total], case["nodes"]) and (o["p_nodes"][total:] == POISON32).all(), tag
    assert np.array_equal(o["p_kind"][:PM], case["kind"]) and (o["p_kind"][PM:] == POISON8).all(), tag
    if case["assign_too"]:
        assert np.array_equal(o["a_off"][:PM + 1], case["off"]) and (o["a_off"][PM + 1:] == POISON32).all(), tag
        assert np.array_equal(o["a_nodes"][:total], case["nodes"]) and (o["a_nodes"][total:] == POISON32).all(), tag
        assert np.array_equal(o["a_kind"][:PM], case["kind"]) and (o["a_kind"][PM:] == POISON8).all(), tag
    else:                                                                # prevMap only: the lists to assign are not touched
        assert (o["a_off"] == POISON32).all() and (o["a_nodes"] == POISON32).all() and (o["a_kind"] == POISON8).all(), tag
    assert np.array_equal(o["in_prev"][:P], case["part_kind"] != 0) and (o["in_prev"][P:] == POISON8).all(), tag
    assert np.array_equal(o["never"][:P], case["part_kind"] == 1) and (o["never"][P:] == POISON8).all(), tag


def run_kernel_cases(ak):
    """Both kernels on documents by hand against kernel_reference; every word they do not own comes back as poison."""
    n, seen = 0, set()
    for i, (P, M, L) in enumerate(KERNEL_SHAPES):
        for assign_too in (1, 0):
            case = kernel_case(i, P, M, L, assign_too, weights=bool(i % 2))
            want = kernel_reference(case)
            for key in ("first_long", "first_missing", "first_dup"):
                if want[key] != INT_MAX:
                    seen.add(key)
            for grids in ([(0, 0), (1, 1), (3, 2)] if P * M < 4000 else [(0, 0)]):
                st, o = ak.run(case, *grids)
                assert st == 0, (P, M, L, grids)
                check_kernel_case(o, case, want, (P, M, L, assign_too, grids))
                n += 1
    assert seen == {"first_long", "first_missing", "first_dup"}
    st, _ = ak.run(dict(kernel_case(0, 4, 2, 3, 1), L=60))
    assert st == -100
    return n


def write_program_input(path):
    """The kernel cases for the stand-alone sanitizer program (tests/simt/wire_adopt_asan_main.cpp), every array as decimal
    words; `want` in the order the program reads."""
    n = 0
    with open(path, "w") as f:
        for i, (P, M, L) in enumerate(KERNEL_SHAPES):
            if P * M > 4000:
                continue
            for assign_too in (1, 0):
                case = kernel_case(i, P, M, L, assign_too, weights=bool(i % 2))
                want = kernel_reference(case)
                f.write("C %d %d %d %d %d\n" % (P, M, L, case["weights_nil"], assign_too))
                for key in ("k", "part_kind", "off", "kind", "nodes", "cur_a_off", "cur_a_kind", "part_weight", "part_has_weight"):
                    f.write(key + " " + " ".join(str(int(v)) for v in case[key]) + "\n")
                f.write("want " + " ".join(str(want[key]) for key in ("first_long", "longest", "fresh", "first_missing", "kinds",
                                                                       "first_dup", "cap", "aprev", "total")) + "\n")
                n += 1
    return n
