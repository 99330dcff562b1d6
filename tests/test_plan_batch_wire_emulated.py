"""blance_plan_batch_wire without a GPU: k_batch_wire_size, k_batch_wire_write and their host driver compiled against the
SIMT emulator (tests/simt).  Every document is checked three ways, never against the batch's own output: its bytes with the
host encoder's (wire.encode of the decoded result, or wire.encode_arrays on raw bytes where a name is no valid UTF-8),
json.loads of it with the decoded result, and -- for a sample -- its bytes with the single path's (blance_plan,
blance_plan_wire_names, blance_plan_wire_get).  The plans themselves are checked against blance_plan_batch and, for a
sample, the C oracle."""
import ctypes as C
import json

import numpy as np
import pytest

from blance_amd import abi, hip, planner, problem, synth, wire
from helpers import build_from_case
from test_plan_batch_stats_emulated import (KEYS, _call_of, _stats_req, both_classes, edge_problems, fallback_problems,
                                            golden_problems, random_problems, same_plan, same_stats)
from test_plan_wire_emulated import encode_raw, escape_strings, named, piece_lengths, renamed, top_keys, unordered_names
from test_simt_emulated import build_emu

POISON = 0xAB


@pytest.fixture(scope="module")
def emu_planner():
    pl = hip.Planner(lib_path=build_emu())
    yield pl
    pl.close()


def _oracle(fp):
    from oracle import loader
    return loader.plan(fp)


def check_document(fp, res, doc, tag):
    """Bytes against the host encoder, json.loads against the decoded result, the keys in byte order."""
    pmap = problem.decode_result(fp, res)[0]
    assert doc == wire.encode(pmap), tag
    assert json.loads(doc) == pmap, tag
    keys = top_keys(doc)
    assert keys == sorted(keys), tag
    return pmap


def single_document(pl, fp):
    """The single path: blance_plan, blance_plan_wire_names, blance_plan_wire_get."""
    res = pl.plan(fp)
    pl.set_wire_names(fp)
    return res, pl.plan_wire()[0]


def run_docs(pl, fps, tag, single=3, oracle=2, names=None, plans=None, check=True):
    """plan_batch_wire with a document for every problem (no moves, no statistics): the documents three ways (the single
    path for the first `single`), the plans against plan_batch (`plans`: its (results, info) computed before) and the first
    `oracle` against the C oracle, the launch count.  Problems whose plan makes no map ask for nothing."""
    fps = [named(fp) for fp in fps]
    own = names is None
    if own:
        names = [pl.batch_names(fp) if fp.max_iterations > 0 else None for fp in fps]
    try:
        got, moves, stats, docs, info = pl.plan_batch_wire(fps, names)
        caps = [None if nm is None else int(pl.lib.blance_batch_wire_capacity(C.byref(fp.as_struct()), nm._h))
                for fp, nm in zip(fps, names)]
    finally:
        if own:
            for nm in names:
                if nm is not None:
                    nm.close()
    want, winfo = plans if plans is not None else pl.plan_batch(fps)
    assert moves == [None] * len(fps) and stats == [None] * len(fps), tag
    for i, (g, w) in enumerate(zip(got, want)):
        same_plan(g, w, (tag, "plan", i))
    for i in range(min(oracle, len(fps))):
        same_plan(got[i], _oracle(fps[i]), (tag, "oracle", i))
    assert info["steps_total"] == winfo["steps_total"], tag
    assert (info["n_batched"], info["n_fallback"]) == (winfo["n_batched"], winfo["n_fallback"]), tag
    asked = sum(nm is not None and fp.n_parts > 0 for fp, nm in zip(fps, names))
    if info["n_fallback"] == 0 and info["n_batched"] > 0:
        assert info["kernel_launches"] == winfo["kernel_launches"] + (2 if asked else 0) <= 6, tag
    pmaps = []
    for i, (fp, g, doc, nm, cap) in enumerate(zip(fps, got, docs, names, caps)):
        if nm is None:
            assert doc is None, (tag, i)
            pmaps.append(None)
            continue
        assert len(doc) <= cap, (tag, i, len(doc), cap)
        pmaps.append(check_document(fp, g, doc, (tag, i)) if check else None)
        if i < single:
            sres, sdoc = single_document(pl, fp)
            same_plan(sres, g, (tag, "single plan", i))
            assert doc == sdoc, (tag, "single path", i)
    return got, docs, pmaps, info, winfo


def list_shapes(fps, pmaps):
    missing = empty = full = null = 0
    for fp, pmap in zip(fps, pmaps):
        for part in (pmap or {}).values():
            nbs = part["nodesByState"]
            missing += sum(1 for s in fp.state_names if s not in nbs)
            empty += sum(1 for v in nbs.values() if v == [])
            full += sum(1 for v in nbs.values() if v)
            null += sum(1 for v in nbs.values() if v is None)
    return missing, empty, full, null


def run_golden(pl, golden_cases):
    fps = golden_problems(pl, golden_cases)
    assert len(fps) >= 60
    _, docs, pmaps, info, _ = run_docs(pl, fps, "golden", single=6, oracle=len(fps))
    assert info["n_batched"] == len(fps) and info["n_fallback"] == 0
    missing, empty, full, null = list_shapes(fps, pmaps)
    assert missing > 0 and empty > 0 and full > 0           # (no golden plan has a nil list: test_plan_wire_kernels_emulated)
    assert sum(d is not None for d in docs) >= 60


def test_golden_cases_one_batch(emu_planner, golden_cases):
    run_golden(emu_planner, golden_cases)


def test_random_cases_one_batch(emu_planner):
    fps = random_problems()
    assert len(fps) >= 60
    _, _, _, info, _ = run_docs(emu_planner, fps, "random")
    assert info["n_batched"] == len(fps) and info["n_fallback"] == 0


def test_edge_cases_one_batch(emu_planner):
    fps = edge_problems()
    _, docs, _, info, _ = run_docs(emu_planner, fps, "edge", single=len(fps))
    assert info["n_batched"] + info["n_fallback"] == len(fps)


def test_both_size_classes(emu_planner):
    all16 = both_classes()
    small = sorted((fp for fp in all16 if fp.n_nodes_ext <= 64), key=lambda fp: fp.n_parts)[:3]
    large = sorted((fp for fp in all16 if fp.n_nodes_ext > 64), key=lambda fp: fp.n_parts)[:2]
    assert len(small) >= 2 and len(large) >= 2
    fps = [small[0], large[0]] + small[1:] + large[1:]
    _, _, _, info, winfo = run_docs(emu_planner, fps, "classes")
    assert info["n_batched"] == len(fps) and winfo["kernel_launches"] == 2 and info["kernel_launches"] == 4


SEAM_SIZES = [1, 2, 255, 256, 257, 513]


def seam_problems():
    """Partition counts at the seams of the 256-rank run and of the scan's chunks, names whose id order is not their byte
    order (the empty name among them), node names of very different lengths."""
    fps = []
    for P in SEAM_SIZES:
        fp = synth.config_flat(2, P=P, N=16)
        fp.node_names = ["n%d" % i + "z" * (37 * (i % 5)) for i in range(fp.n_nodes_ext)]
        fps.append(renamed(fp, unordered_names(P)))
    return fps


def run_seams(pl):
    fps = seam_problems()
    _, docs, _, info, _ = run_docs(pl, fps, "seams", single=len(fps), oracle=len(fps))
    assert info["n_batched"] == len(fps)
    for fp, doc in zip(fps, docs):
        keys = top_keys(doc)
        assert len(keys) == fp.n_parts and keys == sorted(n.encode() for n in fp.part_names)
    assert len({len(n) for n in fps[0].node_names}) >= 5


def test_partition_counts_at_the_seams(emu_planner):
    run_seams(emu_planner)


def run_escapes(pl):
    """Every hard string as a partition name, a node name and a state name, names as raw bytes (one is no valid UTF-8)."""
    strs = escape_strings()
    P = len(strs)
    fp = synth.config_flat(2, P=P, N=P)
    M, NX = fp.n_states, fp.n_nodes_ext
    nodes = [strs[i % P] for i in range(NX)]
    lots = [[strs[(k + j) % P] for j in range(M)] for k in range(0, P, M)]
    fps = [fp] * len(lots)
    names = [pl.batch_names(strs, nodes, states) for states in lots]
    got, _, _, docs, info = pl.plan_batch_wire(fps, names)
    assert info["n_batched"] == len(fps)
    same_plan(got[0], _oracle(fp), "escapes")
    for res, doc, states in zip(got, docs, lots):
        assert doc == encode_raw(res, P, M, strs, nodes, states), states
    pl.plan(fp)
    pl.set_wire_names(strs, nodes, lots[0])
    assert docs[0] == pl.plan_wire()[0]
    both = b"".join(docs)
    assert b"\\ufffd" in both and b"\\u2028" in both and b"\\u003c" in both and b'"\\""' in both and b"\\u0001" in both
    for nm in names:
        nm.close()


def test_escapes(emu_planner):
    run_escapes(emu_planner)


def stage_problems():
    """Three problems for a small stage: one-byte names (a partition is 44 or 45 bytes: it fits a stage of 64 bytes, two do
    not), one name that alone is larger than any small stage, and 255 partitions with node names of very different lengths."""
    keys = list("abcdefghijklmnopqrstuvwxyz0123456789ABCD")
    fresh = {k: {"name": k, "nodesByState": {}} for k in keys}
    a = problem.build_problem({}, fresh, ["n", "m"], [], ["n", "m"], {"p": {"priority": 0, "constraints": 1}})
    b = renamed(synth.config_flat(2, P=9, N=8), ["b", "L" * 700, "c"] + ["q%d" % i for i in range(6)])
    return [a, b, seam_problems()[2]]


STAGES = [64, 256]


def run_small_stage(make_planner, monkeypatch, default_planner, stage):
    fps = stage_problems()
    _, want, pmaps, _, _ = run_docs(default_planner, fps, "default stage")
    monkeypatch.setenv("BLANCE_WIRE_STAGE", str(stage))
    pl = make_planner()
    try:
        _, docs, _, info, _ = run_docs(pl, fps, ("stage", stage), single=3)
    finally:
        pl.close()
    assert docs == want and info["n_batched"] == 3
    budget = stage - 16
    assert max(piece_lengths(pmaps[0])) <= budget                                        # staged ...
    if stage == 64:
        assert budget < 2 * min(piece_lengths(pmaps[0]))                                 # ... one partition a sub-run
    assert max(piece_lengths(pmaps[1])) > budget                                         # the first-wave path
    if stage == 256:                                        # sub-runs of several partitions, cut at every alignment
        lens = piece_lengths(pmaps[2])
        assert sum(lens) > 20 * budget and min(lens) * 2 <= budget < max(lens)


@pytest.mark.parametrize("stage", STAGES)
def test_small_stage(monkeypatch, emu_planner, stage):
    run_small_stage(lambda: hip.Planner(lib_path=build_emu()), monkeypatch, emu_planner, stage)


def residue_problems():
    """16 problems that differ by one byte of a partition name: the name is written twice, a node name differs too, so the
    documents' lengths take every residue mod 16."""
    fps = []
    for k in range(16):
        fp = synth.config_flat(2, P=5, N=4)
        fp.node_names = ["n" + "y" * (k % 2), "n1", "n2", "n3"] + ["x%d" % i for i in range(fp.n_nodes_ext - 4)]
        fps.append(renamed(fp, ["a", "b", "c", "d", "e" * (1 + k // 2)]))
    return fps


def run_residues(pl):
    fps = residue_problems()
    _, docs, _, info, _ = run_docs(pl, fps, "residues", single=2)
    assert info["n_batched"] == 16
    assert {len(d) % 16 for d in docs} == set(range(16)), sorted(len(d) for d in docs)


def test_every_length_residue(emu_planner):
    run_residues(emu_planner)


# ---- the C contract ------------------------------------------------------------------------------------------------

def _raw_call(pl, fps, names, caps=None, bufs=None, moves=False, stats=False, null_names=()):
    """blance_plan_batch_wire through ctypes with everything poisoned first.  names[i] None: no request for problem i."""
    n = len(fps)
    results = [abi.FlatResult(fp) for fp in fps]
    for r in results:
        r.out_off[:] = -7
    cap = [0 if nm is None else int(pl.lib.blance_batch_wire_capacity(C.byref(fp.as_struct()), nm._h))
           for fp, nm in zip(fps, names)]
    if caps is not None:
        cap = [c if o is None else o for c, o in zip(cap, caps)]
    own = [np.full(max(c, 1) + 64, POISON, np.uint8) for c in cap]
    reqs = []
    for i, nm in enumerate(names):
        w = abi.BatchWire()
        w.names = None if i in null_names else (nm._h if nm is not None else None)
        w.buf = own[i].ctypes.data if bufs is None or bufs[i] else None
        w.cap, w.need = cap[i], 12345
        reqs.append(w)
    wrs = (C.POINTER(abi.BatchWire) * n)(*[C.pointer(w) if nm is not None else None for w, nm in zip(reqs, names)])
    pbs = (C.POINTER(abi.Problem) * n)(*[C.pointer(fp.as_struct()) for fp in fps])
    rss = (C.POINTER(abi.Result) * n)(*[C.pointer(r.struct) for r in results])
    sreqs = [_stats_req(fp.n_states) for fp in fps] if stats else None
    sts = (C.POINTER(abi.PlanStats) * n)(*[C.pointer(s) for s, _ in sreqs]) if stats else None
    mvs, mstate = None, None
    if moves:
        ptrs, mstate = pl._moves_requests(fps, results, False, None)
        mstate[5][:] = -7                                     # the moves block
        mvs = ptrs.ctypes.data_as(C.POINTER(C.POINTER(abi.BatchMoves)))
    info = abi.BatchInfo()
    st = pl.lib.blance_plan_batch_wire(pl._h, n, pbs, rss, mvs, sts, wrs, C.byref(info))
    return st, results, reqs, own, cap, sreqs, mstate, info


def run_untouched_tails(pl):
    fps = [named(fp) for fp in synth.cbgt_batch(5, seed=51, P_range=(20, 60), N_range=(5, 90))]
    names = [pl.batch_names(fp) for fp in fps]
    st, results, reqs, own, cap, _, _, info = _raw_call(pl, fps, names)
    assert st == abi.OK and info.n_batched == 5
    for i, (fp, r, w, buf) in enumerate(zip(fps, results, reqs, own)):
        assert 0 < w.need <= cap[i]
        check_document(fp, r, buf[:w.need].tobytes(), ("tails", i))
        assert (buf[w.need:] == POISON).all(), i
    for nm in names:
        nm.close()


def test_untouched_tails(emu_planner):
    run_untouched_tails(emu_planner)


def run_some_ask(pl):
    fps = [named(fp) for fp in synth.cbgt_batch(7, seed=41, P_range=(20, 60), N_range=(5, 40))]
    shared = pl.batch_names(fps[0])
    names = [None if i % 3 == 0 else pl.batch_names(fp) for i, fp in enumerate(fps)]
    got, docs, _, info, winfo = run_docs(pl, fps, "some", names=names)
    assert [d is not None for d in docs] == [i % 3 != 0 for i in range(7)]
    assert info["kernel_launches"] == winfo["kernel_launches"] + 2
    # nobody asks: what plan_batch_stats returns, no launch more
    got0, _, _, docs0, info0 = pl.plan_batch_wire(fps, [None] * 7)
    sres, _, _, sinfo = pl.plan_batch_stats(fps, False)
    assert docs0 == [None] * 7 and info0["kernel_launches"] == sinfo["kernel_launches"] == winfo["kernel_launches"]
    for i, (g, w) in enumerate(zip(got0, sres)):
        same_plan(g, w, ("none", i))
    # one names object for two problems of one batch, and for two batches in a row
    twice = [fps[0], fps[4], fps[0]]
    for _ in range(2):
        _, docs2, _, _, _ = run_docs(pl, twice, "shared", names=[shared, names[4], shared], single=1)
        assert docs2[0] == docs2[2]
    shared.close()


def test_some_ask_some_do_not(emu_planner):
    run_some_ask(emu_planner)


def run_with_moves_and_stats(pl):
    fps = [named(fp) for fp in synth.cbgt_batch(5, seed=43, P_range=(20, 60), N_range=(5, 80))]
    favor = [bool(i % 2) for i in range(len(fps))]
    names = [pl.batch_names(fp) for fp in fps]
    got, moves, stats, docs, info = pl.plan_batch_wire(fps, names, True, favor)
    _, mmoves, sstats, sinfo = pl.plan_batch_stats(fps, True, favor)
    _, wdocs, _, winfo_docs, _ = run_docs(pl, fps, "docs only", names=names, single=0)
    want, winfo = pl.plan_batch(fps)
    for i, (g, w) in enumerate(zip(got, want)):
        same_plan(g, w, ("all", i))
        assert all(np.array_equal(a, b) for a, b in zip(moves[i], mmoves[i])), i
        same_stats(stats[i], sstats[i], ("all", i))
        check_document(fps[i], g, docs[i], ("all", i))
    assert docs == wdocs
    assert sum(int(m[0][-1]) for m in moves) > 0
    assert info["kernel_launches"] == winfo["kernel_launches"] + 1 + 1 + 2 <= 6
    assert sinfo["kernel_launches"] == winfo["kernel_launches"] + 2
    assert winfo_docs["kernel_launches"] == winfo["kernel_launches"] + 2
    for nm in names:
        nm.close()


def test_with_moves_and_statistics_in_the_same_call(emu_planner):
    run_with_moves_and_stats(emu_planner)


def run_fallback(pl, P_wide, wide_nodes, inside):
    fps = fallback_problems(P_wide, wide_nodes, inside)
    got, docs, _, info, _ = run_docs(pl, fps, "fallback", single=len(fps))
    assert info["n_fallback"] >= 2 and info["n_batched"] == len(inside)
    assert all(d is not None and len(d) > 2 for d in docs)
    return info


def test_envelope_fallback(emu_planner):
    run_fallback(emu_planner, 30, 257, synth.cbgt_batch(2, seed=7, P_range=(20, 60), N_range=(30, 60)))


def empty_problem():
    return problem.build_problem({}, {}, ["a", "b"], [], ["a", "b"], {"primary": {"priority": 0, "constraints": 1}})


def run_empty_map(pl):
    fps = [named(empty_problem())] + [named(fp) for fp in synth.cbgt_batch(1, seed=3, P_range=(20, 30), N_range=(5, 9))]
    assert fps[0].n_parts == 0
    _, docs, _, _, _ = run_docs(pl, fps, "empty", single=2)
    assert docs[0] == b"{}"
    _, docs, _, _, _ = run_docs(pl, fps[:1], "empty alone", single=1)
    assert docs == [b"{}"]


def test_empty_map(emu_planner):
    run_empty_map(emu_planner)


REFUSALS = ["names_null", "buf_null", "sizes_parts", "sizes_nodes", "sizes_states", "cap_short", "no_iterations"]


@pytest.mark.parametrize("bad", REFUSALS)
def test_contract_refusals(emu_planner, bad):
    pl = emu_planner
    fps = [named(fp) for fp in synth.cbgt_batch(4, seed=47, P_range=(20, 40), N_range=(5, 20))]
    if bad == "no_iterations":
        fps[2].scalars["max_iterations"] = 0
        fps[2]._struct = None
    names = [pl.batch_names(fp) for fp in fps]
    caps, bufs, null_names = [None] * 4, None, ()
    want = abi.ERR_BAD_ARG
    if bad == "names_null":
        null_names = (2,)
    elif bad == "buf_null":
        bufs = [True, True, False, True]
    elif bad.startswith("sizes_"):
        fp = fps[2]
        lists = {"parts": (fp.part_names + ["extra"], fp.node_names, fp.state_names),
                 "nodes": (fp.part_names, fp.node_names + ["extra"], fp.state_names),
                 "states": (fp.part_names, fp.node_names, fp.state_names[:-1])}[bad[6:]]
        caps[2] = 1 << 20                                    # (ample: the sizes are what is wrong)
        names[2] = pl.batch_names(*lists)
    elif bad == "cap_short":
        caps[2] = int(pl.lib.blance_batch_wire_capacity(C.byref(fps[2].as_struct()), names[2]._h)) - 1
        want = abi.ERR_CAPACITY
    st, results, reqs, own, _, sreqs, mstate, _ = _raw_call(pl, fps, names, caps=caps, bufs=bufs, moves=True, stats=True,
                                                            null_names=null_names)
    assert st == want
    with pytest.raises(hip.BlanceError) as e:
        pl._check(st)
    assert e.value.status == want and "problem 2" in str(e.value)
    assert all((r.out_off == -7).all() and r.iterations == 0 for r in results)
    assert all((b == POISON).all() for b in own) and all(w.need == 12345 for w in reqs)
    assert all((a == -7).all() for _, arr in sreqs for a in arr.values()) and all(s.n_nodes_next == -7 for s, _ in sreqs)
    assert (mstate[5] == -7).all()
    # the same planner answers a valid call
    run_docs(pl, [fps[0], fps[1]], ("after refusal", bad), single=0, oracle=0)


def _names_create(pl, part, node, state, sizes=None, part_off=None, null=None, out=True):
    nm, keep = hip.wire_names_struct(part, node, state)
    if part_off is not None:
        off = np.asarray(part_off, np.int64)
        keep.append(off)
        nm.part_off = off.ctypes.data
    if null is not None:
        setattr(nm, null, None)
    h = C.c_void_p()
    sizes = sizes or (len(part), len(node), len(state))
    st = pl.lib.blance_batch_names_create(C.byref(nm) if null != "names" else None, sizes[0], sizes[1], sizes[2],
                                          C.byref(h) if out else None)
    return st, h


NAMES_REFUSALS = {
    "null_names": (dict(null="names"), abi.ERR_BAD_ARG),
    "null_out": (dict(out=False), abi.ERR_BAD_ARG),
    "null_offsets": (dict(null="node_off"), abi.ERR_BAD_ARG),
    "negative_size": (dict(sizes=(-1, 2, 2)), abi.ERR_BAD_ARG),
    "offsets_start": (dict(part_off=[1, 2, 3]), abi.ERR_BAD_ARG),
    "offsets_monotone": (dict(part_off=[0, 2, 1]), abi.ERR_BAD_ARG),
    "two_states": (dict(state=["s", "s"]), abi.ERR_BAD_ARG),
    "two_partitions": (dict(part=["p", "p"]), abi.ERR_UNSUPPORTED),
}


@pytest.mark.parametrize("bad", sorted(NAMES_REFUSALS))
def test_names_refusals(emu_planner, bad):
    kw, want = NAMES_REFUSALS[bad]
    kw = dict(kw)
    part, node, state = kw.pop("part", ["p", "q"]), ["n", "m"], kw.pop("state", ["s", "t"])
    st, h = _names_create(emu_planner, part, node, state, **kw)
    assert st == want and not h.value
    assert emu_planner.lib.blance_last_error()
    st, h = _names_create(emu_planner, ["p", "q"], node, ["s", "t"])
    assert st == abi.OK and h.value
    emu_planner.lib.blance_batch_names_destroy(h)
    emu_planner.lib.blance_batch_names_destroy(None)         # NULL is fine


def run_context_holds_nothing(pl):
    fps = [named(fp) for fp in synth.cbgt_batch(2, seed=49, P_range=(20, 40), N_range=(5, 20))]
    pl.plan(fps[0])
    pl.set_wire_names(fps[0])
    pl.plan_wire()                                           # (a plan and names are held here)
    run_docs(pl, fps, "holds nothing", single=0, oracle=0)
    with pytest.raises(hip.BlanceError) as e:
        pl.plan_wire()
    assert e.value.status == abi.ERR_BAD_ARG
    run_docs(pl, fallback_problems(30, 257, [])[:1], "holds nothing, single path", single=0, oracle=0)
    with pytest.raises(hip.BlanceError) as e:
        pl.plan_wire()
    assert e.value.status == abi.ERR_BAD_ARG
    with pytest.raises(hip.BlanceError):
        pl.set_wire_names(fps[0])


def test_context_holds_no_problem_and_no_names_afterwards(emu_planner):
    run_context_holds_nothing(emu_planner)


def test_null_requests_is_plan_batch_stats(emu_planner):
    pl = emu_planner
    fps = synth.cbgt_batch(4, seed=53, P_range=(20, 40), N_range=(5, 80))
    n = len(fps)
    out = []
    for with_wire in (True, False):
        results = [abi.FlatResult(fp) for fp in fps]
        sreqs = [_stats_req(fp.n_states) for fp in fps]
        pbs = (C.POINTER(abi.Problem) * n)(*[C.pointer(fp.as_struct()) for fp in fps])
        rss = (C.POINTER(abi.Result) * n)(*[C.pointer(r.struct) for r in results])
        sts = (C.POINTER(abi.PlanStats) * n)(*[C.pointer(s) for s, _ in sreqs])
        info = abi.BatchInfo()
        if with_wire:
            st = pl.lib.blance_plan_batch_wire(pl._h, n, pbs, rss, None, sts, None, C.byref(info))
        else:
            st = pl.lib.blance_plan_batch_stats(pl._h, n, pbs, rss, None, sts, C.byref(info))
        assert st == abi.OK
        out.append((results, sreqs, info.kernel_launches, info.n_batched, info.steps_total))
    (ra, sa, *ia), (rb, sb, *ib) = out
    assert ia == ib
    for i in range(n):
        same_plan(ra[i], rb[i], i)
        assert sa[i][0].n_nodes_next == sb[i][0].n_nodes_next
        assert all(np.array_equal(sa[i][1][k], sb[i][1][k]) for k in KEYS)


def test_plan_next_map_ex_batch_wire(emu_planner, golden_cases):
    ok = [c for c in golden_cases if emu_planner.validate(build_from_case(c)) == abi.OK]
    calls_a, calls_b = [_call_of(c) for c in ok], [_call_of(c) for c in ok]
    want = [planner.PlanNextMapEx(*c, planner=emu_planner) for c in calls_a]
    got = planner.PlanNextMapExBatchWire(calls_b, planner=emu_planner)
    assert len(got) == len(ok) >= 60
    n_docs = 0
    for i, ((nm, w, doc), (wnm, ww)) in enumerate(zip(got, want)):
        assert (nm, w) == (wnm, ww), i
        if wnm is None:
            assert doc is None
            continue
        n_docs += 1
        assert doc == wire.encode({k: {"name": v.Name, "nodesByState": v.NodesByState} for k, v in wnm.items()}), i
    assert n_docs >= 60
    for ca, cb in zip(calls_a, calls_b):          # the write-back into each call's own input maps
        assert ca[0] == cb[0] and ca[1] == cb[1]


def test_library_exports_the_symbols():
    import __graft_entry__ as g
    g.build_hip()
    lib = hip.load_library()
    for name in ("blance_plan_batch_wire", "blance_batch_names_create", "blance_batch_names_destroy", "blance_batch_wire_capacity"):
        assert hasattr(lib, name), name
    assert lib.blance_abi_version() == 6
