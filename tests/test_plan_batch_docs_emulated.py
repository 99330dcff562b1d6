"""blance_plan_batch_docs without a GPU: k_batch_decode and its host driver compiled against the SIMT emulator (tests/simt).
A document problem's result, moves, statistics and document are compared with blance_plan_batch_wire of
problem.wire_adopted_problem(skeleton, lists_of_wire_map(wire.decode(doc)), ..., row_stride=8) -- the host decoder and the
definition in Python --, never with the new call's own output; a sample with the C oracle and with the single route
(upload, adopt_wire, plan_resident).  Refusals are compared with Planner.decode_wire on the same bytes, `why` codes with
the definition's and with adopt_wire's.  The run_* cases are shared with test_plan_batch_docs_gpu.py."""
import ctypes as C
import json
import random

import numpy as np
import pytest

import adopt_cases as A
import wire_adopt_cases as WA
import wire_decode_cases as WD
from blance_amd import abi, hip, planner, problem, synth, wire
from test_plan_batch_stats_emulated import both_classes, fallback_problems, golden_problems, random_problems, same_plan, same_stats
from test_plan_wire_emulated import named
from test_simt_emulated import build_emu

POISON = 0xAB
OUT = abi.BATCH_DOC_OUT


@pytest.fixture(scope="module")
def emu_planner():
    pl = hip.Planner(lib_path=build_emu())
    yield pl
    pl.close()


def _oracle(fp):
    from oracle import loader
    return loader.plan(fp)


def changed(fp, removed=None, added=None, add_nil=None):
    """A copy of fp with another node change (the skeleton's node_removed / node_added / nodes_to_add_nil are the call's)."""
    fp2 = abi.FlatProblem()
    fp2.scalars = dict(fp.scalars)
    for name, a in fp.arrays.items():
        fp2.set(name, a.copy())
    fp2.node_names, fp2.state_names, fp2.part_names = fp.node_names, fp.state_names, fp.part_names
    NX = fp.n_nodes_ext
    fp2.set("node_removed", np.zeros(NX, dtype=np.uint8) if removed is None else np.asarray(removed, dtype=np.uint8))
    fp2.set("node_added", np.zeros(NX, dtype=np.uint8) if added is None else np.asarray(added, dtype=np.uint8))
    fp2.scalars["nodes_to_add_nil"] = int(added is None if add_nil is None else add_nil)
    return fp2


def host_problem(fp, d, doc, assign_too, keep, stride=8):
    """The definition: the host decoder, the carry-over into the dictionary's ids, wire_adopted_problem."""
    wm = wire.decode(bytes(doc))
    try:
        lists = planner.lists_of_wire_map(wm, d)
    finally:
        wm.close()
    new = problem.wire_adopted_problem(fp, lists, fp.node_removed[:fp.n_nodes_ext], fp.node_added[:fp.n_nodes_ext],
                                       bool(fp.nodes_to_add_nil), assign_too, keep, row_stride=stride)
    return new, lists


def is_poison(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == POISON).all())


def same_moves(got, want, tag):
    for g, w in zip(got, want):
        assert np.array_equal(g, w), tag


class Dicts:
    """The dictionaries and the prepared names of a list of problems, closed together."""

    def __init__(self, pl, fps):
        self.dicts = [pl.batch_dict(fp) for fp in fps]
        self.names = [pl.batch_names(fp) for fp in fps]

    def close(self):
        for x in self.dicts + self.names:
            x.close()


def run_batch(pl, fps, docs, assign_too, keep, tag, expect=None, single=2, oracle=2, favor=False, same_tally=True):
    """plan_batch_docs of fps with moves, statistics and documents out.  docs[i] None: no document.  expect: {index: ("refusal",)
    | ("why", code, at)} for the documents that are not planned; every other problem is compared with the host route."""
    expect = expect or {}
    n = len(fps)
    per = lambda v: list(v) if isinstance(v, (list, tuple)) else [v] * n          # noqa: E731
    a_too, keeps = per(assign_too), per(keep)
    ds = Dicts(pl, fps)
    try:
        res, mv, st, out, oc, info = pl.plan_batch_docs(fps, docs, [d if doc is not None else None for d, doc in zip(ds.dicts, docs)],
                                                        assign_too=a_too, keep_prev_only=keeps, names=ds.names, stats=True,
                                                        favor_min_nodes=favor, poison=POISON)
        want_fps, planned = [], []
        for i, fp in enumerate(fps):
            if docs[i] is None:
                assert oc[i] is None, (tag, i)
                want_fps.append(fp)
                planned.append(i)
                continue
            if i in expect:
                assert oc[i]["status"] == abi.ERR_UNSUPPORTED, (tag, i, oc[i])
                for a in (res[i].out_off, res[i].out_nodes, res[i].out_kind, res[i].warn_part, res[i].warn_state, mv[i], out[i]):
                    assert is_poison(a), (tag, i, "a refused problem's buffers are written")
                assert all(is_poison(v) for k, v in st[i].items() if k != "n_nodes_next"), (tag, i)
                if expect[i][0] == "refusal":
                    wd = pl.wire_dict(fps[i])
                    got = pl.decode_wire(wd, docs[i], count_only=True)
                    wd.close()
                    assert got["refusal"] != 0, (tag, i)
                    assert (oc[i]["refusal"], oc[i]["refusal_at"]) == (got["refusal"], got["refusal_at"]), (tag, i, oc[i], got)
                    assert (oc[i]["why"], oc[i]["why_at"]) == (0, -1), (tag, i, oc[i])
                else:
                    assert (oc[i]["refusal"], oc[i]["refusal_at"]) == (0, -1), (tag, i, oc[i])
                    assert (oc[i]["why"], oc[i]["why_at"]) == expect[i][1:3], (tag, i, oc[i])
                    with pytest.raises(problem.Unsupported) as e:
                        host_problem(fps[i], ds.dicts[i], docs[i], a_too[i], keeps[i], expect[i][3] if len(expect[i]) > 3 else 8)
                    assert (e.value.why, e.value.why_at) == expect[i][1:3], (tag, i)
                continue
            assert oc[i]["status"] == 0 and (oc[i]["refusal"], oc[i]["refusal_at"], oc[i]["why"], oc[i]["why_at"]) == (0, -1, 0, -1), \
                (tag, i, oc[i])
            new, lists = host_problem(fp, ds.dicts[i], docs[i], a_too[i], keeps[i])
            assert (oc[i]["n_node_refs"], oc[i]["n_parts_seen"]) == (lists["n_node_refs"], lists["n_parts_seen"]), (tag, i, oc[i])
            want_fps.append(new)
            planned.append(i)
        names = [ds.names[i] for i in planned]
        wres, wmv, wst, wout, winfo = pl.plan_batch_wire(want_fps, names, stats=True, favor_min_nodes=favor)
        for j, i in enumerate(planned):
            same_plan(res[i], wres[j], (tag, "plan", i))
            same_moves(mv[i], wmv[j], (tag, "moves", i))
            same_stats(st[i], wst[j], (tag, "stats", i))
            assert out[i] == wout[j], (tag, "document", i)
        assert info["steps_total"] == winfo["steps_total"], tag
        assert info["n_batched"] + info["n_fallback"] == len(planned), (tag, info)
        if same_tally and not expect:                       # (a skeleton outside the envelope by its own sizes goes the single path)
            assert (info["n_batched"], info["n_fallback"]) == (winfo["n_batched"], winfo["n_fallback"]), (tag, info, winfo)
        if info["n_fallback"] == 0 and winfo["n_fallback"] == 0 and info["n_batched"] > 0 and not expect:
            # the budget: one launch more than the same call without documents, whatever n
            assert info["kernel_launches"] == winfo["kernel_launches"] + (1 if any(d is not None for d in docs) else 0), (tag, info, winfo)
        for j, i in enumerate(planned[:oracle]):
            same_plan(res[i], _oracle(want_fps[j]), (tag, "oracle", i))
        done = 0
        for j, i in enumerate(planned):                     # the single route: upload, adopt_wire, plan_resident
            if done >= single or docs[i] is None:
                continue
            wd = pl.wire_dict(fps[i])
            try:
                pl.upload(fps[i])
                got = pl.adopt_wire(wd, docs[i], fps[i].node_removed[:fps[i].n_nodes_ext], fps[i].node_added[:fps[i].n_nodes_ext],
                                    bool(fps[i].nodes_to_add_nil), a_too[i], keeps[i])
                if got["adopted"]:
                    pl.plan_resident()
                    same_plan(pl.download(), res[i], (tag, "single route", i))
                    done += 1
            finally:
                wd.close()
        return res, out, oc, info, winfo
    finally:
        ds.close()


def planned_documents(pl, fps):
    """The problems that plan with a sweep, and their plans' documents (blance_plan_batch_wire)."""
    fps = [named(fp) for fp in fps if fp.max_iterations > 0]
    names = [pl.batch_names(fp) for fp in fps]
    try:
        res, _, _, docs, _ = pl.plan_batch_wire(fps, names)
    finally:
        for nm in names:
            nm.close()
    keep = [i for i, r in enumerate(res) if r.iterations > 0]
    return [fps[i] for i in keep], [docs[i] for i in keep]


# ---- 1. equality ---------------------------------------------------------------------------------------------------------------

def run_golden(pl, golden_cases, keep):
    fps, docs = planned_documents(pl, golden_problems(pl, golden_cases))
    assert len(fps) >= 60
    sk = []
    for i, fp in enumerate(fps):
        ch = A.golden_change(fp, i, keep)
        fp2 = changed(fp, ch.removed, ch.added, ch.add_nil)
        sk.append(fp2 if pl.validate(fp2) == abi.OK else fp)
    _, _, _, info, _ = run_batch(pl, sk, docs, True, keep, ("golden", keep), single=4, oracle=len(fps))
    assert info["n_batched"] == len(fps) and info["n_fallback"] == 0
    assert sum(bool(fp.node_removed.any()) for fp in sk) >= 10 and sum(bool(fp.node_added.any()) for fp in sk) >= 5


@pytest.mark.parametrize("keep", [False, True])
def test_golden_documents(emu_planner, golden_cases, keep):
    run_golden(emu_planner, golden_cases, keep)


def run_random(pl):
    fps, docs = planned_documents(pl, random_problems())
    assert len(fps) >= 50
    fps, docs = fps[:40], docs[:40]
    sk = []
    for i, fp in enumerate(fps):
        alive = [x for x in range(fp.n_nodes) if not fp.node_removed[x]]
        fp2 = fp
        if len(alive) >= 3 and i % 3:
            fp2 = changed(fp, removed=A.flags(fp, alive[1::3]))
        elif len(alive) >= 3:
            fp2 = changed(fp, added=A.flags(fp, alive[1::3]))
        sk.append(fp2 if pl.validate(fp2) == abi.OK else fp)
    for assign_too in (True, False):
        _, _, _, info, _ = run_batch(pl, sk, docs, assign_too, [bool(i % 2) for i in range(len(sk))], ("random", assign_too))
        assert info["n_batched"] == len(fps) and info["n_fallback"] == 0


def test_random_documents(emu_planner):
    run_random(emu_planner)


def run_both_classes(pl, count=None):
    all16 = both_classes()
    if count:
        small = sorted((fp for fp in all16 if fp.n_nodes_ext <= 64), key=lambda fp: fp.n_parts)[:count]
        large = sorted((fp for fp in all16 if fp.n_nodes_ext > 64), key=lambda fp: fp.n_parts)[:count]
        all16 = [small[0], large[0]] + small[1:] + large[1:]
    fps, docs = planned_documents(pl, all16)
    sk = [changed(fp, removed=A.flags(fp, [x for x in range(fp.n_nodes) if x % 10 == 3])) for fp in fps]
    _, _, _, info, winfo = run_batch(pl, sk, docs, True, False, "classes")
    assert info["n_batched"] == len(fps) and info["kernel_launches"] == winfo["kernel_launches"] + 1 == 2 + 1 + 1 + 2 + 1


def test_both_size_classes(emu_planner):
    run_both_classes(emu_planner, 2)


# ---- 2. documents that are not the plan ----------------------------------------------------------------------------------------

def run_mutants(pl):
    rng = np.random.RandomState(7)
    base = named(WA.mutant_base())
    (fp,), (doc,) = planned_documents(pl, [base])
    planned = json.loads(doc)
    fps, docs, a_too, keeps, expect = [], [], [], [], {}
    for name, m, with_assign, may_remove in WA.mutants(planned, rng):
        for assign_too in (False, True):
            sk = changed(base, removed=A.flags(base, [2])) if may_remove else changed(base, added=A.flags(base, [7]))
            if assign_too and not with_assign:
                why = {"dropped": ("why", abi.WIRE_ADOPT["partition_missing"], 3), "duplicates": ("why", abi.WIRE_ADOPT["duplicate_node"], 1),
                       "empty-document": ("why", abi.WIRE_ADOPT["partition_missing"], 0)}[name]
                expect[len(fps)] = why
            fps.append(sk)
            docs.append(WA.dumps(m))
            a_too.append(assign_too)
            keeps.append(len(fps) % 2 == 0)
    _, _, oc, info, _ = run_batch(pl, fps, docs, a_too, keeps, "mutants", expect=expect, single=len(fps), oracle=len(fps))
    assert info["n_batched"] == len(fps) - len(expect) and info["n_fallback"] == 0 and len(expect) == 3


def test_documents_that_are_not_the_plan(emu_planner):
    run_mutants(emu_planner)


# ---- 3. every refusal reason, 5. seams: the decoder's own documents against a skeleton of its dictionary's names --------------------

def decoder_skeleton(constraints=0):
    """A problem over wire_decode_cases' names (4,121 partitions, 48 nodes, 3 states); constraints 0: nothing is planned, the
    result is the document's lists without the removed nodes -- the decode itself, fast on the emulator."""
    model = {s: {"priority": i, "constraints": constraints} for i, s in enumerate(WD.STATES)}
    parts = WD.PARTS + WD.SPECIAL
    assign = {p: {"name": p, "nodesByState": {}} for p in parts}
    fp = problem.build_problem({}, assign, WD.NODES, [], None, model)
    assert fp.n_parts == len(parts) and fp.n_nodes_ext == len(WD.NODES) and fp.n_states == 3
    return fp


def small_neighbours(pl):
    fps, docs = planned_documents(pl, synth.cbgt_batch(3, seed=41, P_range=(20, 40), N_range=(5, 20)))
    return [changed(fp, removed=A.flags(fp, [1])) for fp in fps], docs


def run_refusals(make_planner, monkeypatch, tile):
    if tile is not None:
        monkeypatch.setenv("BLANCE_WIRE_IN_TILE", str(tile))
    pl = make_planner()
    try:
        T = tile or 256
        cases = WD.refusal_documents(T)
        assert {c[2] for c in cases} == set(abi.WIRE_REFUSALS[1:18])
        sk = decoder_skeleton()
        near, near_docs = small_neighbours(pl)
        # the record that is too long (reason 18) and the rest in lots: one refused document per reason among planned neighbours
        inside, outside = WD.size_limit_documents()
        cases = [c[:3] for c in cases] + [(t, d, "record_too_long") for t, d, _, _ in outside[:2]]
        for lot in range(0, len(cases), 16):
            part = cases[lot:lot + 16]
            fps = [near[0]] + [sk] * len(part) + near[1:]
            docs = [near_docs[0]] + [c[1] for c in part] + near_docs[1:]
            expect = {1 + k: ("refusal",) for k in range(len(part))}
            _, _, oc, info, _ = run_batch(pl, fps, docs, [True] + [k % 2 == 0 for k in range(len(part))] + [True] * (len(near) - 1),
                                          False, ("refusals", tile, lot), expect=expect)
            for k, c in enumerate(part):
                assert oc[1 + k]["refusal"] == abi.WIRE_REFUSED[c[2]], (c[0], oc[1 + k])
            assert info["n_batched"] == len(near) and info["n_fallback"] == 0
    finally:
        pl.close()


@pytest.mark.parametrize("tile", [64, None])
def test_every_refusal_reason(monkeypatch, tile):
    run_refusals(lambda: hip.Planner(lib_path=build_emu()), monkeypatch, tile)


def chunk_documents(T):
    """Documents around the chunk of 256 tiles: just under, at and just over 256 T bytes; a run of backslashes, a string and a
    nested bracket each straddling a tile seam and the chunk seam; every length residue mod 16; whitespace everywhere."""
    out = []
    chunk = 256 * T
    r = lambda i, nbs: WD.record(WD.PARTS[i], nbs)            # noqa: E731
    many = [r(i, {"primary": [WD.NODES[7 + i % 40]], "replica": ["a", "b"][:i % 3]}) for i in range(chunk // 30)]
    body = b"{" + b",".join(many)
    assert len(body) > chunk + 64
    for n in (chunk - 1, chunk, chunk + 1, chunk + 17):
        recs, size = [], 1
        for rec in many:
            if size + len(rec) + 1 + 40 > n:
                break
            recs.append(rec)
            size += len(rec) + 1
        doc = b"{" + b",".join(recs)
        out.append(("length %d" % n, doc + b" " * (n - len(doc) - 1) + b"}"))
    for seam in (8 * T, chunk):
        for what, rec in (("backslash run", WD.record("\\" * 70, {"primary": ["a"]})),
                          ("string", WD.record("p1", {"primary": ["L" * 150, "a"]})),
                          ("bracket", WD.record("p2", {"primary": ["a", "b", "c"], "replica": ["n,1", 'q"']}))):
            for back in (8, len(rec) // 2, len(rec) - 3):
                lead = seam - back - 1
                head, size = [], 1
                for m in many[4:]:                           # (p1, p2 and p3 stand behind)
                    if size + len(m) + 1 > lead - 8:
                        break
                    head.append(m)
                    size += len(m) + 1
                doc = b"{" + b"".join(h + b"," for h in head)
                assert len(doc) <= lead
                doc += b" " * (lead - len(doc)) + rec + b", " + WD.record("p3", None) + b"\n}\n"
                assert doc[lead:lead + len(rec)] == rec and lead < seam < lead + len(rec)
                out.append(("%s over %d, %d back" % (what, seam, back), doc))
    base = WD.document([r(i, {"s\\t": ["c"]}) for i in range(5)])
    for k in range(16):
        out.append(("residue %d" % ((len(base) + k) % 16), base + b" " * k))
    rng = random.Random(5)
    for i in range(6):
        out.append(("written freely %d" % i, WD.render(rng, WD.random_map(rng, 17))))
    out.append(("every special name", WD.render(rng, {s: {"name": s, "nodesByState": {"primary": ["a"]}} for s in WD.SPECIAL})))
    return out


def run_seams(make_planner, monkeypatch, tile, stage=None):
    if tile is not None:
        monkeypatch.setenv("BLANCE_WIRE_IN_TILE", str(tile))
    if stage is not None:
        monkeypatch.setenv("BLANCE_WIRE_IN_STAGE", str(stage))
    pl = make_planner()
    try:
        T = tile or 256
        sk = changed(decoder_skeleton(), removed=A.flags(decoder_skeleton(), [0]))
        cases = WD.seam_documents(T, stage or 32 * 1024) + chunk_documents(T)
        assert len(cases) > 80
        # The record longer than the stage has a list of thousands: more than the batch's rows hold, so it goes the single
        # path, whose rows are the skeleton's own (1 wide) -- LIST_TOO_LONG at that list, as the definition says.
        long_at = sk.part_names.index("p1") * sk.n_states + sk.state_names.index("primary")
        for lot in range(0, len(cases), 24):
            part = cases[lot:lot + 24]
            expect = {k: ("why", abi.WIRE_ADOPT["list_too_long"], long_at, 1) for k, c in enumerate(part) if "longer than the stage" in c[0]}
            # (prevMap alone: a document holds some of the 4,121 partitions; its lists come back as the moves away from them)
            _, _, _, info, _ = run_batch(pl, [sk] * len(part), [c[1] for c in part], False, [k % 2 == 0 for k in range(len(part))],
                                         ("seams", tile, stage, [c[0] for c in part]), expect=expect, single=1, oracle=1)
            assert info["n_batched"] == len(part) - len(expect) and info["n_fallback"] == 0
        return len(cases)
    finally:
        pl.close()


@pytest.mark.parametrize("tile,stage", [(64, None), (None, None), (64, 64), (64, 256)])
def test_seams(monkeypatch, tile, stage):
    run_seams(lambda: hip.Planner(lib_path=build_emu()), monkeypatch, tile, stage)


PART_COUNTS = [0, 1, 2, 255, 256, 257, 513]


def run_partition_counts(pl):
    """The runs of 256 records: P partitions, every one in its document."""
    fps = [named(synth.config_flat(2, P=P, N=16)) if P else
           named(problem.build_problem({}, {}, ["a", "b"], [], None, {"primary": {"priority": 0, "constraints": 1}})) for P in PART_COUNTS]
    docs = []
    for fp in fps:
        if fp.n_parts == 0:
            docs.append(b" {\n} ")
            continue
        (f2,), (doc,) = planned_documents(pl, [fp])
        docs.append(doc)
    sk = [changed(fp, removed=A.flags(fp, [1])) if fp.n_parts else fp for fp in fps]
    _, _, oc, info, _ = run_batch(pl, sk, docs, True, False, "partition counts", single=len(fps), oracle=len(fps))
    assert info["n_batched"] == len(fps)
    assert [o["n_parts_seen"] for o in oc] == PART_COUNTS


def test_partition_counts(emu_planner):
    run_partition_counts(emu_planner)


# ---- 4. the five why codes -----------------------------------------------------------------------------------------------------

def why_base(P=12):
    """Constraints 1 + 7: the skeleton's own rows are 7 wide, the batch's 8."""
    model = {"primary": {"priority": 0, "constraints": 1}, "replica": {"priority": 1, "constraints": 7}}
    nodes = ["n%02d" % i for i in range(12)]
    assign = {"p%02d" % i: {"name": "p%02d" % i, "nodesByState": {"primary": [nodes[i % 12]], "replica": [nodes[(i + 1) % 12]]}} for i in range(P)}
    prev = json.loads(json.dumps(assign))
    return named(problem.build_problem(prev, assign, nodes, [], None, model)), nodes, assign


def run_whys(pl):
    W = abi.WIRE_ADOPT
    base, nodes, assign = why_base()
    assert WA.row_stride(base) == 7
    M = base.n_states
    rep = base.state_names.index("replica")

    def doc(edit):
        m = json.loads(json.dumps(assign))
        edit(m)
        return WA.dumps(m)

    def put(name, state, lst):
        return lambda m: m[name]["nodesByState"].__setitem__(state, lst)

    removed = changed(base, removed=A.flags(base, [3]))
    heavy = named(WA.overflow_base())                       # inside the int32 load bound with lists of one node, beyond it with three
    heavy_doc = WA.dumps({nm: {"name": nm, "nodesByState": {"primary": ["n0"], "replica": ["n1", "n2", "n3"]}} for nm in heavy.part_names})
    cases = [
        # (skeleton, document, assign_too, expectation or None)
        (base, doc(put("p04", "replica", nodes[:8])), True, None),                              # exactly 8: planned on the batch
        (base, doc(put("p04", "replica", nodes[:9])), True, ("why", W["list_too_long"], 4 * M + rep, 7)),   # 9: the single path, its rows
        (base, doc(lambda m: (m.pop("p05"), m.pop("p02"))), True, ("why", W["partition_missing"], 2)),
        (base, doc(lambda m: (put("p07", "replica", ["n01", "n02", "n01"])(m), put("p03", "replica", ["n05", "n05"])(m))), True,
         ("why", W["duplicate_node"], 3 * M + rep)),
        (base, doc(lambda m: (put("p07", "replica", ["n01", "n02", "n01"])(m))), False, None),    # duplicates in prevMap alone are kept
        (removed, doc(lambda m: (m.pop("p09"), m.pop("p06"))), False, ("why", W["removed_without_prev"], 6)),
        (heavy, heavy_doc, True, ("why", W["load_overflow"], -1)),
    ]
    fps = [c[0] for c in cases]
    expect = {i: c[3] for i, c in enumerate(cases) if c[3]}
    _, _, oc, info, _ = run_batch(pl, fps, [c[1] for c in cases], [c[2] for c in cases], False, "whys", expect=expect, single=0)
    assert info["n_batched"] == 2 and info["n_fallback"] == 0
    # ... and equal to adopt_wire's on the same skeleton (where its own rows decide the same)
    for i, c in enumerate(cases):
        if not c[3]:
            continue
        wd = pl.wire_dict(c[0])
        pl.upload(c[0])
        got = pl.adopt_wire(wd, c[1], c[0].node_removed[:c[0].n_nodes_ext], c[0].node_added[:c[0].n_nodes_ext],
                            bool(c[0].nodes_to_add_nil), c[2], False)
        wd.close()
        assert (got["why"], got["why_at"]) == (oc[i]["why"], oc[i]["why_at"]), (i, got, oc[i])
    # a list of 9 on a skeleton whose own rows hold it: the single path plans it
    wide, nodes, assign = why_base()
    wide_assign = json.loads(json.dumps(assign))
    wide_assign["p00"]["nodesByState"]["replica"] = nodes[1:10]
    wide = named(problem.build_problem(wide_assign, wide_assign, nodes, [], None,
                                       {"primary": {"priority": 0, "constraints": 1}, "replica": {"priority": 1, "constraints": 7}}))
    assert WA.row_stride(wide) == 9
    m = json.loads(json.dumps(assign))
    m["p03"]["nodesByState"]["replica"] = nodes[2:11]
    ds = Dicts(pl, [wide])
    try:
        res, mv, st, out, oc, info = pl.plan_batch_docs([wide], [WA.dumps(m)], ds.dicts, names=ds.names, stats=True, favor_min_nodes=True)
        assert oc[0]["status"] == 0 and (info["n_batched"], info["n_fallback"]) == (0, 1), (oc, info)
        new, _ = host_problem(wide, ds.dicts[0], WA.dumps(m), True, False, stride=9)
        wres, wmv, wst, wout, _ = pl.plan_batch_wire([new], ds.names, stats=True, favor_min_nodes=True)
        same_plan(res[0], wres[0], "nine")
        same_plan(res[0], _oracle(new), "nine, oracle")
        same_moves(mv[0], wmv[0], "nine")
        same_stats(st[0], wst[0], "nine")
        assert out[0] == wout[0]
    finally:
        ds.close()


def test_why_codes(emu_planner):
    run_whys(emu_planner)


# ---- 6. mixed batches ---------------------------------------------------------------------------------------------------------

def run_mixed(pl):
    fps, docs = planned_documents(pl, synth.cbgt_batch(7, seed=43, P_range=(20, 60), N_range=(5, 40)))
    sk = [changed(fp, removed=A.flags(fp, [2])) for fp in fps]
    some = [d if i % 3 != 1 else None for i, d in enumerate(docs)]
    _, _, oc, info, _ = run_batch(pl, sk, some, [i % 2 == 0 for i in range(len(sk))], False, "some with documents", favor=True)
    assert info["n_batched"] == len(sk) and sum(o is None for o in oc) >= 2
    # dcs == NULL in effect: no document at all is blance_plan_batch_wire
    _, _, _, info, winfo = run_batch(pl, sk, [None] * len(sk), True, False, "none with documents")
    assert info["kernel_launches"] == winfo["kernel_launches"]


def test_mixed_batch(emu_planner):
    run_mixed(emu_planner)


def run_round_trip(pl, rounds=3):
    """The documents out of call t are the documents in of call t + 1 after a node leaves."""
    fps, docs = planned_documents(pl, synth.cbgt_batch(5, seed=47, P_range=(20, 50), N_range=(8, 30)))
    gone = [np.zeros(fp.n_nodes_ext, dtype=np.uint8) for fp in fps]
    for t in range(rounds):
        for fp, g in zip(fps, gone):
            g[:] = 0
            g[(3 * t + 1) % fp.n_nodes] = 1
        sk = [changed(fp, removed=g) for fp, g in zip(fps, gone)]
        _, docs, _, info, _ = run_batch(pl, sk, docs, True, False, ("round", t), single=1, oracle=1)
        assert info["n_batched"] == len(fps)
        for fp, g, d in zip(fps, gone, docs):
            assert fp.node_names[int(np.flatnonzero(g)[0])].encode() not in d


def test_round_trip(emu_planner):
    run_round_trip(emu_planner)


def run_fallback(pl, P_wide=40, wide_nodes=260):
    inside = synth.cbgt_batch(4, seed=53, P_range=(20, 40), N_range=(5, 20))
    fps, docs = planned_documents(pl, fallback_problems(P_wide, wide_nodes, inside))
    assert len(fps) == 6
    sk = [changed(fp, removed=A.flags(fp, [1])) for fp in fps]
    # (the problem with a list of 9 carries prevMap keys outside the model: with assign_too they are gone, as the definition says)
    _, _, oc, info, winfo = run_batch(pl, sk, docs, True, False, "fallback", single=0, oracle=len(fps), same_tally=False)
    assert (info["n_batched"], info["n_fallback"]) == (4, 2), info


def test_fallback_problems(emu_planner):
    run_fallback(emu_planner)


def run_context_holds_nothing(pl):
    fps, docs = planned_documents(pl, synth.cbgt_batch(2, seed=59, P_range=(20, 30), N_range=(5, 10)))
    pl.plan(fps[0])
    run_batch(pl, fps, docs, True, False, "holds nothing", single=0)
    for call in (pl.plan_resident, pl.download, lambda: pl.plan_stats(fps[0].n_states), lambda: pl.plan_wire(size_only=True)):
        with pytest.raises(hip.BlanceError) as e:
            call()
        assert e.value.status == abi.ERR_BAD_ARG


def test_context_holds_nothing(emu_planner):
    run_context_holds_nothing(emu_planner)


# ---- 7. whole-call refusals ----------------------------------------------------------------------------------------------------

def raw_call(pl, fps, docs, dicts, mutate=None, beg_other_at=None, small=None, names=None):
    """blance_plan_batch_docs through ctypes with poisoned outputs: results, moves and, with names, statistics and documents.
    mutate(dreq): edits the requests; small: an index whose result capacity is too small.  Returns (status, error text,
    every output buffer -- the `need` words of the document requests among them --, the requests, and per index the
    document buffer and its `need` word as views)."""
    n = len(fps)
    structs = [fp.as_struct() for fp in fps]
    dreq = (abi.BatchDoc * n)()
    ptrs = (C.POINTER(abi.BatchDoc) * n)()
    keep = []
    results, wcaps = [], []
    for i in range(n):
        rc = C.c_int64(fps[i].result_capacity())
        wcaps.append(C.c_size_t(int(pl.lib.blance_batch_wire_capacity(C.byref(structs[i]), names[i]._h)) if names else 0))
        if docs[i] is not None:
            buf = C.create_string_buffer(docs[i], len(docs[i]) + 1)
            keep.append(buf)
            dreq[i].dict = dicts[i]._h
            dreq[i].json, dreq[i].len = C.cast(buf, C.c_void_p).value, len(docs[i])
            dreq[i].assign_too = 1
            dreq[i].status = dreq[i].refusal = dreq[i].why = -77
            ptrs[i] = C.pointer(dreq[i])
            pl.lib.blance_batch_doc_bounds(C.byref(structs[i]), C.byref(dreq[i]), names[i]._h if names else None, C.byref(rc), None,
                                           C.byref(wcaps[i]))
        results.append(abi.FlatResult(hip._ResultShape(fps[i], rc.value)))
    if mutate:
        mutate(dreq, ptrs)
    if small is not None:
        results[small].struct.out_capacity = 0
    mv_ptrs, mv_state = pl._moves_requests(fps, results, [True] * n, None,
                                           caps={i: int(len(docs[i]) // 3 + results[i].struct.out_capacity) for i in range(n) if docs[i] is not None})
    if beg_other_at is not None:
        off = np.zeros(fps[beg_other_at].n_parts + 1, dtype=np.int32)
        nodes = np.zeros(1, dtype=np.int32)
        keep += [off, nodes]
        mv_state[6]["beg_other_off"][beg_other_at], mv_state[6]["beg_other_nodes"][beg_other_at] = off.ctypes.data, nodes.ctypes.data
    bufs = []
    for r in results:
        bufs += [r.out_off, r.out_nodes, r.out_kind, r.warn_part, r.warn_state]
    bufs.append(mv_state[5])
    st_ptrs = wr_ptrs = None
    wire = [None] * n
    if names:
        st_arr, st_state = pl._stats_requests(fps, [True] * n)
        base = np.zeros(n + 1, np.int64)
        base[1:] = np.cumsum([w.value for w in wcaps])
        block = np.empty(max(int(base[-1]), 1), dtype=np.uint8)
        wreq = np.zeros(n, dtype=abi.BATCH_WIRE_DTYPE)
        wreq["names"] = [nm._h.value for nm in names]
        wreq["buf"] = block.ctypes.data + base[:-1]
        wreq["cap"] = [w.value for w in wcaps]
        wr_arr = wreq.ctypes.data + wreq.itemsize * np.arange(n, dtype=np.uint64)
        need = wreq["need"]
        keep += [st_state, wreq, wr_arr, st_arr]
        bufs += [st_state[5], block]
        wire = [(block[int(base[i]):int(base[i + 1])], need[i:i + 1]) for i in range(n)]
        st_ptrs = st_arr.ctypes.data_as(C.POINTER(C.POINTER(abi.PlanStats)))
        wr_ptrs = wr_arr.ctypes.data_as(C.POINTER(C.POINTER(abi.BatchWire)))
    for b in bufs:
        b.view(np.uint8)[:] = POISON
    if names:                                            # (a field of the request records: not contiguous)
        need[:] = int.from_bytes(bytes([POISON]) * 8, "little")
        bufs.append(need)
    pbs = (C.POINTER(abi.Problem) * n)(*[C.pointer(s) for s in structs])
    rss = (C.POINTER(abi.Result) * n)(*[C.pointer(r.struct) for r in results])
    info = abi.BatchInfo()
    st = pl.lib.blance_plan_batch_docs(pl._h, n, pbs, rss, mv_ptrs.ctypes.data_as(C.POINTER(C.POINTER(abi.BatchMoves))), st_ptrs, wr_ptrs,
                                       ptrs, C.byref(info))
    return st, pl.lib.blance_last_error().decode(), bufs, dreq, wire


def run_whole_call_refusals(pl):
    fps, docs = planned_documents(pl, synth.cbgt_batch(3, seed=61, P_range=(20, 30), N_range=(5, 10)))
    ds = Dicts(pl, fps)
    other = pl.batch_dict(["x"], ["y"], ["z"])
    try:
        st, _, _, dreq, wire = raw_call(pl, fps, docs, ds.dicts, names=ds.names)
        assert st == 0 and all(d.status == 0 for d in dreq)
        assert all(int(need[0]) == len(doc) > 0 and not is_poison(buf[:len(doc)]) for (buf, need), doc in zip(wire, docs))
        # a document refused on its own: the call is fine, that index's document buffer and its `need` are not written
        bad = [docs[0], docs[1][:-1], docs[2]]
        st, _, _, dreq, wire = raw_call(pl, fps, bad, ds.dicts, names=ds.names)
        assert st == 0 and [d.status for d in dreq] == [0, abi.ERR_UNSUPPORTED, 0] and dreq[1].refusal == abi.WIRE_REFUSED["grammar"]
        assert is_poison(wire[1][0]) and is_poison(wire[1][1]) and not is_poison(wire[0][1]) and not is_poison(wire[2][1])
        zero = changed(fps[1])
        zero.scalars["max_iterations"] = 0

        def set_(i, **kw):
            def f(dreq, ptrs):
                for k, v in kw.items():
                    setattr(dreq[i], k, v)
            return f

        def reserved(dreq, ptrs):
            dreq[2].reserved[1] = 1

        cases = [("dict NULL", dict(mutate=set_(1, dict=None)), 1, abi.ERR_BAD_ARG),
                 ("json NULL", dict(mutate=set_(2, json=None)), 2, abi.ERR_BAD_ARG),
                 ("dict of other sizes", dict(mutate=set_(0, dict=other._h)), 0, abi.ERR_BAD_ARG),
                 ("reserved", dict(mutate=reserved), 2, abi.ERR_BAD_ARG),
                 ("beg_other with a document", dict(beg_other_at=1), 1, abi.ERR_BAD_ARG),
                 ("result capacity", dict(small=2), 2, abi.ERR_CAPACITY)]
        for tag, kw, index, status in cases:
            st, text, bufs, dreq, _ = raw_call(pl, fps, docs, ds.dicts, names=ds.names, **kw)
            assert st == status and text.startswith("problem %d:" % index), (tag, st, text)
            assert all(is_poison(b) for b in bufs), tag
            assert all(d.status == -77 and d.refusal == -77 and d.why == -77 for d in dreq), tag
        st, text, bufs, dreq, _ = raw_call(pl, [fps[0], zero, fps[2]], docs, ds.dicts, names=ds.names)
        assert st == abi.ERR_BAD_ARG and text.startswith("problem 1:") and all(is_poison(b) for b in bufs), (st, text)
    finally:
        other.close()
        ds.close()


def test_whole_call_refusals(emu_planner):
    run_whole_call_refusals(emu_planner)


def test_document_too_long_is_refused_before_anything_runs(emu_planner):
    """len >= 2^31: BLANCE_WIRE_REFUSED_DOCUMENT_TOO_LONG at 0, no byte of the document is read."""
    pl = emu_planner
    fps, docs = planned_documents(pl, synth.cbgt_batch(2, seed=67, P_range=(20, 30), N_range=(5, 10)))
    ds = Dicts(pl, fps)
    try:
        def huge(dreq, ptrs):
            dreq[0].len = 2 ** 31
        rc = C.c_int64()
        st, text, bufs, dreq, _ = raw_call(pl, fps, docs, ds.dicts, mutate=huge, small=0)
        assert st == abi.ERR_CAPACITY                           # (the bounds grow with len: the capacities are checked first)
        n = len(fps)
        structs = [fp.as_struct() for fp in fps]
        big = abi.BatchDoc()
        big.dict, big.json, big.len, big.assign_too = ds.dicts[0]._h, C.cast(C.create_string_buffer(b"{}"), C.c_void_p).value, 2 ** 31, 0
        pl.lib.blance_batch_doc_bounds(C.byref(structs[0]), C.byref(big), None, C.byref(rc), None, None)
        assert rc.value == fps[0].result_capacity()             # (without assign_too the result capacity is the skeleton's)
        results = [abi.FlatResult(fp) for fp in fps]
        for r in results:
            r.out_nodes.view(np.uint8)[:] = POISON
        ptrs = (C.POINTER(abi.BatchDoc) * n)()
        ptrs[0] = C.pointer(big)
        pbs = (C.POINTER(abi.Problem) * n)(*[C.pointer(s) for s in structs])
        rss = (C.POINTER(abi.Result) * n)(*[C.pointer(r.struct) for r in results])
        info = abi.BatchInfo()
        st = pl.lib.blance_plan_batch_docs(pl._h, n, pbs, rss, None, None, None, ptrs, C.byref(info))
        assert st == 0, pl.lib.blance_last_error()
        assert (big.status, big.refusal, big.refusal_at) == (abi.ERR_UNSUPPORTED, abi.WIRE_REFUSED["document_too_long"], 0)
        assert is_poison(results[0].out_nodes) and (info.n_batched, info.n_fallback) == (1, 0)
        same_plan(results[1], _oracle(fps[1]), "the neighbour")
    finally:
        ds.close()


def test_struct_layout_matches_the_header(tmp_path):
    """abi.BatchDoc against include/blance_batch.h, through the C compiler."""
    import os
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    src = tmp_path / "layout.c"
    fields = [f for f, _ in abi.BatchDoc._fields_]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "blance_batch.h"\nint main(void) {\n'
                   + "".join('  printf("%%zu\\n", offsetof(blance_batch_doc, %s));\n' % f for f in fields)
                   + '  printf("%zu\\n", sizeof(blance_batch_doc));\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(here, "..", "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [getattr(abi.BatchDoc, f).offset for f in fields] + [C.sizeof(abi.BatchDoc)]


# ---- the Python route: a plan or the host decoder's error, always ---------------------------------------------------------------

def run_api(pl):
    kws = [synth.cbgt_case(70 + i, P_range=(10, 40), N_range=(4, 20)) for i in range(4)]
    calls, want = [], []
    for i, kw in enumerate(kws):
        first = planner.PlanNextMapEx(kw["prev_map"], kw["partitions_to_assign"], kw["nodes_all"], kw["nodes_to_remove"], kw["nodes_to_add"],
                                      kw["model"], planner=pl)[0]
        stored = {name: {"name": name, "nodesByState": p.NodesByState} for name, p in first.items()}
        doc = WA.dumps(stored)
        if i == 2:                                           # outside the device's subset: an unknown field -- the host route
            doc = doc.replace(b'{"name":', b'{"extra":1,"name":', 1)
        gone = [kw["nodes_all"][1]]
        calls.append(dict(document=doc, partitionsToAssign=stored, nodesAll=kw["nodes_all"], nodesToRemove=gone, nodesToAdd=[], model=kw["model"]))
        prev = {name: planner.Partition(name, p["nodesByState"]) for name, p in json.loads(json.dumps(stored)).items()}
        assign = {name: planner.Partition(name, p["nodesByState"]) for name, p in json.loads(json.dumps(stored)).items()}
        want.append(planner.PlanNextMapEx(prev, assign, kw["nodes_all"], gone, [], kw["model"], planner=pl))
    got = planner.PlanNextMapExBatchDocs(calls, planner=pl)
    routes = [g[2] for g in got]
    assert routes.count("device") == 3 and routes[2] == "host", routes
    for (nm, warn, _), (wnm, wwarn) in zip(got, want):
        assert {k: v.NodesByState for k, v in nm.items()} == {k: v.NodesByState for k, v in wnm.items()}
        assert warn == wwarn
    bad = dict(calls[0], document=b'{"a":')
    with pytest.raises(wire.WireError):
        planner.PlanNextMapExBatchDocs([bad], planner=pl)


def test_plan_next_map_ex_batch_docs(emu_planner):
    run_api(emu_planner)
