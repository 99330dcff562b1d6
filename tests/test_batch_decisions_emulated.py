"""The batch driver's decisions, pinned: for a few small calls of blance_plan_batch* under
the SIMT emulator, who was batched and who went the single path, the launches and steps the call counted, what every
document was told, and which problem a refused call names -- the numbers a restructuring of BatchCall (blance_hip.hip) must
leave alone.  The expected values were printed by this file, run as a program, against the library of the commit before
the driver became a record of steps; they are not taken from the code they check.

Run as a program it prints the rows (an argument: the library to load; none: the emulator build of this tree).

Left out: a document beyond the byte limits of one call (2^28 a document, 2^31 a call) -- no test here reaches them without
a quarter of a gigabyte of document."""
import copy
import ctypes as C
import json
import sys

import pytest

import wire_adopt_cases as WA
from blance_amd import abi, hip, problem, synth
from test_plan_wire_emulated import named

INFO = ("n_batched", "n_fallback", "kernel_launches", "steps_total")
MODEL = {"primary": {"priority": 0, "constraints": 1}, "replica": {"priority": 1, "constraints": 2}}


def _mixed_problems():
    """A 64-class problem, a 256-class one (65 node names), an envelope fallback (a list of 9), one with max_iterations 0,
    one without partitions (its document is the host's "{}")."""
    small = synth.cbgt_batch(1, seed=3, P_range=(20, 30), N_range=(5, 20))[0]
    wide = problem.build_problem(**synth.cbgt_case(8, P_range=(30, 30), N_range=(65, 65), rebalance=False))
    assert small.n_nodes_ext <= 64 and wide.n_nodes_ext == 65
    nodes = ["n%02d" % i for i in range(12)]
    long_prev = {"a": {"name": "a", "nodesByState": {"primary": nodes[:1], "replica": nodes[1:10]}},
                 "b": {"name": "b", "nodesByState": {"primary": nodes[2:3]}}}
    list9 = problem.build_problem(long_prev, copy.deepcopy(long_prev), nodes, [], [], MODEL)
    zero = synth.cbgt_batch(1, seed=4, P_range=(20, 30), N_range=(5, 20))[0]
    zero.scalars["max_iterations"] = 0
    zero._struct = None
    empty = problem.build_problem({}, {}, ["a", "b"], [], None, {"primary": {"priority": 0, "constraints": 1}})
    return [named(fp) for fp in (small, wide, list9, zero, empty)]


# moves, statistics and documents on alternating problems (neither moves nor a document may be asked of max_iterations 0)
FAVOR = [True, None, True, None, True]
STATS = [False, True, False, True, False]
WIRE = [True, False, True, False, True]


def _info(info):
    return tuple(int(info[k]) for k in INFO)


def mixed_rows(pl):
    fps = _mixed_problems()
    every = [pl.batch_names(fp) for fp in fps]
    names = [nm if w else None for nm, w in zip(every, WIRE)]
    try:
        yield "mixed/plan_batch", _info(pl.plan_batch(fps)[-1])
        yield "mixed/plan_batch_moves", _info(pl.plan_batch_moves(fps, FAVOR)[-1])
        yield "mixed/plan_batch_stats", _info(pl.plan_batch_stats(fps, stats=STATS, favor_min_nodes=FAVOR)[-1])
        yield "mixed/plan_batch_wire", _info(pl.plan_batch_wire(fps, names, stats=STATS, favor_min_nodes=FAVOR)[-1])
        yield "mixed/plan_batch_docs", _info(pl.plan_batch_docs(fps, [None] * len(fps), [None] * len(fps), names=names, stats=STATS,
                                                                 favor_min_nodes=FAVOR)[-1])
        # ... and everything asked of every problem that has a map
        yield "mixed/all_ask", _info(pl.plan_batch_wire(fps[:3] + fps[4:], every[:3] + every[4:], stats=True, favor_min_nodes=False)[-1])
    finally:
        for nm in every:
            nm.close()


def _doc_base(P=12, wide=False):
    """Constraints 1 + 7; wide: a list of 9 to assign, so that the skeleton's own rows hold a document's list of 9."""
    model = {"primary": {"priority": 0, "constraints": 1}, "replica": {"priority": 1, "constraints": 7}}
    nodes = ["n%02d" % i for i in range(12)]
    assign = {"p%02d" % i: {"name": "p%02d" % i, "nodesByState": {"primary": [nodes[i % 12]], "replica": [nodes[(i + 1) % 12]]}}
              for i in range(P)}
    mine = json.loads(json.dumps(assign))
    if wide:
        mine["p00"]["nodesByState"]["replica"] = nodes[1:10]
    return named(problem.build_problem(json.loads(json.dumps(mine)), mine, nodes, [], None, model)), nodes, assign


def docs_rows(pl):
    """A batched document, one the parser refuses, one refused with a why (a partition missing, assign_too), one with a list of
    9 (the single path, which plans it on the skeleton's rows of 9), one with a list of 9 on rows of 7 (the single path, which
    refuses it), and a problem without a document."""
    base, nodes, assign = _doc_base()
    wide, _, _ = _doc_base(wide=True)

    def doc(edit=None):
        m = json.loads(json.dumps(assign))
        if edit:
            edit(m)
        return WA.dumps(m)

    def nine(m):
        m["p03"]["nodesByState"]["replica"] = nodes[2:11]

    fps = [base, base, base, wide, base, base]
    docs = [doc(), doc()[:-1] + b"]", doc(lambda m: m.pop("p02")), doc(nine), doc(nine), None]
    dicts = [pl.batch_dict(fp) for fp in fps]
    names = [pl.batch_names(fp) for fp in fps]
    try:
        *_, oc, info = pl.plan_batch_docs(fps, docs, [d if doc_ is not None else None for d, doc_ in zip(dicts, docs)],
                                          assign_too=True, names=names, stats=True, favor_min_nodes=[True] * 5 + [None])
    finally:
        for x in dicts + names:
            x.close()
    yield "docs/info", _info(info)
    for i, o in enumerate(oc):
        yield "docs/outcome%d" % i, None if o is None else tuple(o[k] for k in ("status", "refusal", "refusal_at", "why", "why_at"))


def refused_rows(pl):
    """Problems 1 and 3 both fail their checks: problem 1 is the one reported."""
    fps = synth.cbgt_batch(5, seed=5, P_range=(20, 40), N_range=(5, 20))
    fps[1].arrays["part_order"][0] = fps[1].arrays["part_order"][1]          # not a permutation
    fps[1]._struct = None
    results = [abi.FlatResult(fp) for fp in fps]
    results[3].struct.out_capacity = fps[3].result_capacity() - 1
    pbs = (C.POINTER(abi.Problem) * 5)(*[C.pointer(fp.as_struct()) for fp in fps])
    rss = (C.POINTER(abi.Result) * 5)(*[C.pointer(r.struct) for r in results])
    st = pl.lib.blance_plan_batch(pl._h, 5, pbs, rss, None)
    yield "refused/1_and_3", (int(st), pl.lib.blance_last_error().decode().split(":")[0])
    pbs = (C.POINTER(abi.Problem) * 2)(*[C.pointer(fp.as_struct()) for fp in (fps[0], fps[3])])
    rss = (C.POINTER(abi.Result) * 2)(*[C.pointer(r.struct) for r in (results[0], results[3])])
    st = pl.lib.blance_plan_batch(pl._h, 2, pbs, rss, None)
    yield "refused/capacity", (int(st), pl.lib.blance_last_error().decode().split(":")[0])


def all_rows(pl):
    for rows in (mixed_rows, docs_rows, refused_rows):
        yield from rows(pl)


# INFO of the call; a document's (status, refusal, refusal_at, why, why_at); (status, the problem the error names)
EXPECTED = {
    'mixed/plan_batch': (4, 1, 36, 648),
    'mixed/plan_batch_moves': (4, 1, 40, 648),
    'mixed/plan_batch_stats': (4, 1, 41, 648),
    'mixed/plan_batch_wire': (4, 1, 46, 648),
    'mixed/plan_batch_docs': (4, 1, 46, 648),
    'mixed/all_ask': (3, 1, 48, 648),
    'docs/info': (2, 1, 74, 240),
    'docs/outcome0': (0, 0, -1, 0, -1),
    'docs/outcome1': (-2, 1, 888, 0, -1),
    'docs/outcome2': (-2, 0, -1, 2, 2),
    'docs/outcome3': (0, 0, -1, 0, -1),
    'docs/outcome4': (-2, 0, -1, 1, 7),
    'docs/outcome5': None,
    'refused/1_and_3': (-1, 'problem 1'),
    'refused/capacity': (-3, 'problem 1'),
}


@pytest.fixture(scope="module")
def rows():
    from test_simt_emulated import build_emu
    pl = hip.Planner(lib_path=build_emu())
    try:
        return dict(all_rows(pl))
    finally:
        pl.close()


def test_every_row_is_pinned(rows):
    assert sorted(rows) == sorted(EXPECTED)


@pytest.mark.parametrize("name", list(EXPECTED))
def test_decisions(rows, name):
    assert rows[name] == EXPECTED[name], (name, rows[name])


if __name__ == "__main__":
    if len(sys.argv) > 1:
        lib_ = sys.argv[1]
    else:
        from test_simt_emulated import build_emu
        lib_ = build_emu()
    pl_ = hip.Planner(lib_path=lib_)
    for name_, value_ in all_rows(pl_):
        print("    %r: %r," % (name_, value_), flush=True)
    pl_.close()
