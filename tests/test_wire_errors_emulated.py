"""What a caller is told, pinned: for the entry points whose checks live in host/wire_names.hpp or were
folded into one function each, the status and the text of blance_last_error() for every bad input -- the words a move of those
checks must leave alone.  The expected values were printed by this file, run as a program, against the emulator library of
the commit before the checks moved; they are not taken from the code they check.

Run as a program it prints the rows (an argument: the library to load; none: the emulator build of this tree).

The four creators (blance_plan_wire_names, blance_wire_dict_create, blance_batch_names_create, blance_batch_dict_create) cross
each blob cause on each blob, a duplicate partition, node and state -- the names encoder ACCEPTS two nodes with one name, the
dictionaries refuse them: kept as it is --, negative sizes (blance_plan_wire_names takes none: its sizes are the context's),
and the dictionaries' two bounds that need no gigabytes: n_parts * n_states of 2^31 - 1, and names whose last offset says 2^31
bytes.  The readers: blance_plan_moves_get and blance_plan_batch_moves on each beg_other fault, blance_plan_stats_get and
blance_plan_batch_stats on a short and on a missing array, blance_plan_adopt and blance_wire_adopt on a context with a
communicator (blance_comm_set with a host callback and one rank reaches that refusal under the emulator).

Left out: the encoder's "the escaped names take 2^31 bytes or more" (gigabytes of names), and every text that carries a
source line number."""
import ctypes as C
import sys

import numpy as np
import pytest

from blance_amd import abi, hip, problem

MODEL = {"primary": {"priority": 0, "constraints": 1}, "replica": {"priority": 1, "constraints": 1}}
PARTS, NODES, STATES = ["p1", "p0"], ["n0", "n1", "n2"], ["primary", "replica"]
SIZES = (len(PARTS), len(NODES), len(STATES))
BLOBS = ("part", "node", "state")
INT_MAX = 2 ** 31 - 1


def _problem():
    prev = {p: {"name": p, "nodesByState": {"primary": [NODES[i]], "replica": [NODES[i + 1]]}} for i, p in enumerate(PARTS)}
    fp = problem.build_problem(prev, {p: dict(v) for p, v in prev.items()}, NODES, [], None, MODEL)
    assert (fp.n_parts, fp.n_nodes_ext, fp.n_states) == SIZES
    return fp


def _names(lists=None, bad=None):
    """abi.WireNames of three lists of names; bad: (blob index, cause) spoils that blob."""
    nm, keep = hip.wire_names_struct(*(lists or (PARTS, NODES, STATES)))
    if bad:
        k, cause = bad
        off = keep[2 * k + 1]
        if cause == "null_offsets":
            setattr(nm, BLOBS[k] + "_off", None)
        elif cause == "first_offset":
            off[0] = 1
        elif cause == "not_monotone":
            off[1], off[2] = off[2], off[1] - 1
        elif cause == "null_bytes":
            setattr(nm, BLOBS[k] + "_bytes", None)
        elif cause == "2^31_bytes":
            off[-1] = 2 ** 31
    return nm, keep


def _told(pl, st):
    return int(st), pl.lib.blance_last_error().decode() if st else ""


def _creators(pl):
    """name -> a call (names, sizes) -> status; what it made is destroyed at once."""
    lib, h = pl.lib, pl._h

    def wire_names(nm, sizes):
        return lib.blance_plan_wire_names(h, C.byref(nm))

    def wire_dict(nm, sizes):
        out = C.c_void_p()
        st = lib.blance_wire_dict_create(h, C.byref(nm), *sizes, C.byref(out))
        if out.value:
            lib.blance_wire_dict_destroy(h, out)
        return st

    def batch_names(nm, sizes):
        out = C.c_void_p()
        st = lib.blance_batch_names_create(C.byref(nm), *sizes, C.byref(out))
        if st == 0:
            lib.blance_batch_names_destroy(out)
        return st

    def batch_dict(nm, sizes):
        out = C.c_void_p()
        st = lib.blance_batch_dict_create(C.byref(nm), *sizes, C.byref(out))
        if st == 0:
            lib.blance_batch_dict_destroy(out)
        return st
    return {"plan_wire_names": wire_names, "wire_dict_create": wire_dict, "batch_names_create": batch_names,
            "batch_dict_create": batch_dict}


def creator_rows(pl):
    pl.upload(_problem())                                              # blance_plan_wire_names wants a problem on the context
    calls = _creators(pl)
    for who, call in calls.items():
        nm, keep = _names()
        yield "%s/good" % who, _told(pl, call(nm, SIZES))
        for cause in ("null_offsets", "first_offset", "not_monotone", "null_bytes"):
            for k in range(3):
                nm, keep = _names(bad=(k, cause))
                yield "%s/%s/%s" % (who, cause, BLOBS[k]), _told(pl, call(nm, SIZES))
        for k in range(3):
            lists = [PARTS, NODES, STATES]
            lists[k] = [lists[k][0]] * len(lists[k])
            nm, keep = _names(lists)
            yield "%s/duplicate/%s" % (who, BLOBS[k]), _told(pl, call(nm, SIZES))
        nm, keep = _names((["p", "p"], NODES, ["s", "s"]))               # a partition and a state twice: who is named
        yield "%s/duplicate/part_and_state" % who, _told(pl, call(nm, SIZES))
        if who == "plan_wire_names":
            continue
        nm, keep = _names()
        for k in range(3):
            sizes = list(SIZES)
            sizes[k] = -1
            yield "%s/negative/%s" % (who, BLOBS[k]), _told(pl, call(nm, sizes))
    for who in ("wire_dict_create", "batch_dict_create"):
        nm, keep = _names()
        yield "%s/lists_2^31" % who, _told(pl, calls[who](nm, (INT_MAX, 3, 1)))
        for k in range(3):
            nm, keep = _names(bad=(k, "2^31_bytes"))
            yield "%s/2^31_bytes/%s" % (who, BLOBS[k]), _told(pl, calls[who](nm, SIZES))
    del keep


OTHER_FAULTS = {   # name -> (offsets [P + 1], node ids) of a bad beg_other for P = 2, NX = 3
    "first_offset": ([1, 1, 1], [0]),
    "not_monotone": ([0, 2, 1], [0, 1]),
    "node_negative": ([0, 1, 2], [0, -1]),
    "node_too_large": ([0, 1, 2], [3, 0]),
    "one_array_only": ([0, 1, 2], None),
}


def _batch_call(pl, fp, other=None, stats_edit=None):
    """blance_plan_batch_stats of one problem with its moves (other: beg_other arrays) or its statistics (stats_edit spoils the
    request); the status."""
    res = abi.FlatResult(fp)
    pbs = (C.POINTER(abi.Problem) * 1)(C.pointer(fp.as_struct()))
    rss = (C.POINTER(abi.Result) * 1)(C.pointer(res.struct))
    mv_ptrs, mv_state = pl._moves_requests([fp], [res], True if other is not None else None, None)
    keep = []
    if other is not None:
        req = mv_state[6]
        keep = [np.asarray(other[0], np.int32), np.asarray(other[1] if other[1] is not None else [0], np.int32)]
        req["beg_other_off"][0] = keep[0].ctypes.data
        req["beg_other_nodes"][0] = keep[1].ctypes.data if other[1] is not None else 0
    st_ptrs, st_state = pl._stats_requests([fp], [stats_edit is not None])
    if stats_edit is not None:
        stats_edit(st_state[6])
    st = pl.lib.blance_plan_batch_stats(pl._h, 1, pbs, rss, mv_ptrs.ctypes.data_as(C.POINTER(C.POINTER(abi.BatchMoves))),
                                        st_ptrs.ctypes.data_as(C.POINTER(C.POINTER(abi.PlanStats))), None)
    del keep, mv_state, st_state
    return st


def _short(req):
    req["n_states"][0] = SIZES[2] - 1


def _missing(name):
    def edit(req):
        req[name][0] = 0
    return edit


STATS_FAULTS = dict([("short", _short)] + [("no_" + a, _missing(a)) for a in abi.PLAN_STATS_ARRAYS])


def reader_rows(pl):
    fp = _problem()
    pl.plan(fp)
    for name, (off, nodes) in OTHER_FAULTS.items():
        mv = abi.PlanMoves()                                           # a count: no buffers
        keep = [np.asarray(off, np.int32), np.asarray(nodes if nodes is not None else [0], np.int32)]
        mv.beg_other_off = keep[0].ctypes.data_as(C.POINTER(C.c_int32))
        if nodes is not None:
            mv.beg_other_nodes = keep[1].ctypes.data_as(C.POINTER(C.c_int32))
        yield "plan_moves_get/" + name, _told(pl, pl.lib.blance_plan_moves_get(pl._h, C.byref(mv)))
    for name in STATS_FAULTS:
        a = {k: np.zeros(SIZES[2], np.int64) for k in abi.PLAN_STATS_ARRAYS}
        st = abi.PlanStats()
        st.n_states = SIZES[2]
        for k, v in a.items():
            setattr(st, k, v.ctypes.data_as(C.POINTER(C.c_int32 if k == "nodes_used" else C.c_int64)))
        if name == "short":
            st.n_states = SIZES[2] - 1
        else:
            setattr(st, name[3:], None)
        yield "plan_stats_get/" + name, _told(pl, pl.lib.blance_plan_stats_get(pl._h, C.byref(st)))
    for name, other in OTHER_FAULTS.items():
        yield "plan_batch_moves/" + name, _told(pl, _batch_call(pl, fp, other=other))
    for name, edit in STATS_FAULTS.items():
        yield "plan_batch_stats/" + name, _told(pl, _batch_call(pl, fp, stats_edit=edit))


def comm_rows(pl):
    """A planned context with a dictionary, then a communicator of one rank with a host callback: both adoptions refuse."""
    fp = _problem()
    pl.plan(fp)
    wdict = pl.wire_dict(PARTS, NODES, STATES)
    pl.comm_set_callback(0, 1, lambda ptr, count: None)
    zeros = np.zeros(SIZES[1], np.uint8)
    z = zeros.ctypes.data_as(C.POINTER(C.c_uint8))
    ad = abi.Adopt()
    ad.node_removed, ad.node_added, ad.nodes_to_add_nil = z, z, 1
    yield "plan_adopt/communicator", _told(pl, pl.lib.blance_plan_adopt(pl._h, C.byref(ad)))
    doc = b"{}"
    buf = C.create_string_buffer(doc, len(doc))
    wa = abi.WireAdopt()
    wa.dict, wa.json, wa.len = wdict._h, C.cast(buf, C.c_void_p).value, len(doc)
    wa.node_removed, wa.node_added, wa.nodes_to_add_nil = z, z, 1
    yield "wire_adopt/communicator", _told(pl, pl.lib.blance_wire_adopt(pl._h, C.byref(wa)))
    pl.comm_clear()
    wdict.close()


def all_rows(pl):
    for rows in (creator_rows, reader_rows, comm_rows):
        yield from rows(pl)


# (status, blance_last_error()); a call that succeeds: (0, "")
EXPECTED = {
    'plan_wire_names/good': (0, ''),
    'plan_wire_names/null_offsets/part': (-1, 'null offsets'),
    'plan_wire_names/null_offsets/node': (-1, 'null offsets'),
    'plan_wire_names/null_offsets/state': (-1, 'null offsets'),
    'plan_wire_names/first_offset/part': (-1, 'name offsets must start at 0'),
    'plan_wire_names/first_offset/node': (-1, 'name offsets must start at 0'),
    'plan_wire_names/first_offset/state': (-1, 'name offsets must start at 0'),
    'plan_wire_names/not_monotone/part': (-1, 'name offsets not monotone'),
    'plan_wire_names/not_monotone/node': (-1, 'name offsets not monotone'),
    'plan_wire_names/not_monotone/state': (-1, 'name offsets not monotone'),
    'plan_wire_names/null_bytes/part': (-1, 'null name bytes'),
    'plan_wire_names/null_bytes/node': (-1, 'null name bytes'),
    'plan_wire_names/null_bytes/state': (-1, 'null name bytes'),
    'plan_wire_names/duplicate/part': (-2, "two partitions with one name (the reference's map would keep one of them)"),
    'plan_wire_names/duplicate/node': (0, ''),
    'plan_wire_names/duplicate/state': (-1, 'two states with one name'),
    'plan_wire_names/duplicate/part_and_state': (-1, 'two states with one name'),
    'wire_dict_create/good': (0, ''),
    'wire_dict_create/null_offsets/part': (-1, 'null offsets'),
    'wire_dict_create/null_offsets/node': (-1, 'null offsets'),
    'wire_dict_create/null_offsets/state': (-1, 'null offsets'),
    'wire_dict_create/first_offset/part': (-1, 'name offsets must start at 0'),
    'wire_dict_create/first_offset/node': (-1, 'name offsets must start at 0'),
    'wire_dict_create/first_offset/state': (-1, 'name offsets must start at 0'),
    'wire_dict_create/not_monotone/part': (-1, 'name offsets not monotone'),
    'wire_dict_create/not_monotone/node': (-1, 'name offsets not monotone'),
    'wire_dict_create/not_monotone/state': (-1, 'name offsets not monotone'),
    'wire_dict_create/null_bytes/part': (-1, 'null name bytes'),
    'wire_dict_create/null_bytes/node': (-1, 'null name bytes'),
    'wire_dict_create/null_bytes/state': (-1, 'null name bytes'),
    'wire_dict_create/duplicate/part': (-2, "two partitions with one name (the reference's map would keep one of them)"),
    'wire_dict_create/duplicate/node': (-1, 'two nodes with one name'),
    'wire_dict_create/duplicate/state': (-1, 'two states with one name'),
    'wire_dict_create/duplicate/part_and_state': (-2, "two partitions with one name (the reference's map would keep one of them)"),
    'wire_dict_create/negative/part': (-1, 'negative count'),
    'wire_dict_create/negative/node': (-1, 'negative count'),
    'wire_dict_create/negative/state': (-1, 'negative count'),
    'batch_names_create/good': (0, ''),
    'batch_names_create/null_offsets/part': (-1, 'null offsets'),
    'batch_names_create/null_offsets/node': (-1, 'null offsets'),
    'batch_names_create/null_offsets/state': (-1, 'null offsets'),
    'batch_names_create/first_offset/part': (-1, 'name offsets must start at 0'),
    'batch_names_create/first_offset/node': (-1, 'name offsets must start at 0'),
    'batch_names_create/first_offset/state': (-1, 'name offsets must start at 0'),
    'batch_names_create/not_monotone/part': (-1, 'name offsets not monotone'),
    'batch_names_create/not_monotone/node': (-1, 'name offsets not monotone'),
    'batch_names_create/not_monotone/state': (-1, 'name offsets not monotone'),
    'batch_names_create/null_bytes/part': (-1, 'null name bytes'),
    'batch_names_create/null_bytes/node': (-1, 'null name bytes'),
    'batch_names_create/null_bytes/state': (-1, 'null name bytes'),
    'batch_names_create/duplicate/part': (-2, "two partitions with one name (the reference's map would keep one of them)"),
    'batch_names_create/duplicate/node': (0, ''),
    'batch_names_create/duplicate/state': (-1, 'two states with one name'),
    'batch_names_create/duplicate/part_and_state': (-1, 'two states with one name'),
    'batch_names_create/negative/part': (-1, 'negative size'),
    'batch_names_create/negative/node': (-1, 'negative size'),
    'batch_names_create/negative/state': (-1, 'negative size'),
    'batch_dict_create/good': (0, ''),
    'batch_dict_create/null_offsets/part': (-1, 'null offsets'),
    'batch_dict_create/null_offsets/node': (-1, 'null offsets'),
    'batch_dict_create/null_offsets/state': (-1, 'null offsets'),
    'batch_dict_create/first_offset/part': (-1, 'name offsets must start at 0'),
    'batch_dict_create/first_offset/node': (-1, 'name offsets must start at 0'),
    'batch_dict_create/first_offset/state': (-1, 'name offsets must start at 0'),
    'batch_dict_create/not_monotone/part': (-1, 'name offsets not monotone'),
    'batch_dict_create/not_monotone/node': (-1, 'name offsets not monotone'),
    'batch_dict_create/not_monotone/state': (-1, 'name offsets not monotone'),
    'batch_dict_create/null_bytes/part': (-1, 'null name bytes'),
    'batch_dict_create/null_bytes/node': (-1, 'null name bytes'),
    'batch_dict_create/null_bytes/state': (-1, 'null name bytes'),
    'batch_dict_create/duplicate/part': (-2, "two partitions with one name (the reference's map would keep one of them)"),
    'batch_dict_create/duplicate/node': (-1, 'two nodes with one name'),
    'batch_dict_create/duplicate/state': (-1, 'two states with one name'),
    'batch_dict_create/duplicate/part_and_state': (-2, "two partitions with one name (the reference's map would keep one of them)"),
    'batch_dict_create/negative/part': (-1, 'negative count'),
    'batch_dict_create/negative/node': (-1, 'negative count'),
    'batch_dict_create/negative/state': (-1, 'negative count'),
    'wire_dict_create/lists_2^31': (-1, 'n_parts * n_states of 2^31 - 1 or more'),
    'wire_dict_create/2^31_bytes/part': (-2, 'names of 2^31 bytes or more'),
    'wire_dict_create/2^31_bytes/node': (-2, 'names of 2^31 bytes or more'),
    'wire_dict_create/2^31_bytes/state': (-2, 'names of 2^31 bytes or more'),
    'batch_dict_create/lists_2^31': (-1, 'n_parts * n_states of 2^31 - 1 or more'),
    'batch_dict_create/2^31_bytes/part': (-2, 'names of 2^31 bytes or more'),
    'batch_dict_create/2^31_bytes/node': (-2, 'names of 2^31 bytes or more'),
    'batch_dict_create/2^31_bytes/state': (-2, 'names of 2^31 bytes or more'),
    'plan_moves_get/first_offset': (-1, 'beg_other offsets must start at 0'),
    'plan_moves_get/not_monotone': (-1, 'beg_other offsets not monotone'),
    'plan_moves_get/node_negative': (-1, 'beg_other node id outside [0, n_nodes_ext)'),
    'plan_moves_get/node_too_large': (-1, 'beg_other node id outside [0, n_nodes_ext)'),
    'plan_moves_get/one_array_only': (-1, 'beg_other_off and beg_other_nodes: both or neither'),
    'plan_stats_get/short': (-1, 'stats arrays missing or shorter than n_states'),
    'plan_stats_get/no_load_min': (-1, 'stats arrays missing or shorter than n_states'),
    'plan_stats_get/no_load_max': (-1, 'stats arrays missing or shorter than n_states'),
    'plan_stats_get/no_load_sum': (-1, 'stats arrays missing or shorter than n_states'),
    'plan_stats_get/no_load_sumsq': (-1, 'stats arrays missing or shorter than n_states'),
    'plan_stats_get/no_nodes_used': (-1, 'stats arrays missing or shorter than n_states'),
    'plan_stats_get/no_unmet_slots': (-1, 'stats arrays missing or shorter than n_states'),
    'plan_stats_get/no_rule_violations': (0, ''),
    'plan_batch_moves/first_offset': (-1, 'problem 0: beg_other offsets must start at 0'),
    'plan_batch_moves/not_monotone': (-1, 'problem 0: beg_other offsets not monotone'),
    'plan_batch_moves/node_negative': (-1, 'problem 0: beg_other node id outside [0, n_nodes_ext)'),
    'plan_batch_moves/node_too_large': (-1, 'problem 0: beg_other node id outside [0, n_nodes_ext)'),
    'plan_batch_moves/one_array_only': (-1, 'problem 0: beg_other_off and beg_other_nodes: both or neither'),
    'plan_batch_stats/short': (-1, 'problem 0: stats arrays missing or shorter than n_states'),
    'plan_batch_stats/no_load_min': (-1, 'problem 0: stats arrays missing or shorter than n_states'),
    'plan_batch_stats/no_load_max': (-1, 'problem 0: stats arrays missing or shorter than n_states'),
    'plan_batch_stats/no_load_sum': (-1, 'problem 0: stats arrays missing or shorter than n_states'),
    'plan_batch_stats/no_load_sumsq': (-1, 'problem 0: stats arrays missing or shorter than n_states'),
    'plan_batch_stats/no_nodes_used': (-1, 'problem 0: stats arrays missing or shorter than n_states'),
    'plan_batch_stats/no_unmet_slots': (-1, 'problem 0: stats arrays missing or shorter than n_states'),
    'plan_batch_stats/no_rule_violations': (0, ''),
    'plan_adopt/communicator': (-2, 'blance_plan_adopt on a context with a communicator'),
    'wire_adopt/communicator': (-2, 'blance_wire_adopt on a context with a communicator'),
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


def test_no_line_numbers_pinned():
    assert not any(": line " in text for _, text in EXPECTED.values())


@pytest.mark.parametrize("name", list(EXPECTED))
def test_told(rows, name):
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
