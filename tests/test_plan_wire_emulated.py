"""blance_plan_wire_names / blance_plan_wire_get without a GPU: k_wire_size, k_wire_write and their host driver compiled
against the SIMT emulator (tests/simt).  Every document is compared twice, independently: its bytes with the host encoder's
(wire.encode of the decoded result, or wire.encode_arrays on raw bytes where a name is no valid UTF-8), and json.loads of it
with the decoded result.  The plans themselves are checked against the C oracle's digest."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from blance_amd import abi, hip, problem, synth, wire
from helpers import build_from_case
from test_plan_batch_moves_emulated import _mixed
from test_plan_moves_emulated import _rebalance, same_moves
from test_simt_emulated import build_emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN, STAGE_SKEW = 256, 16            # k_plan_wire.h: ranks of a workgroup's run; the stage keeps 16 bytes for its alignment


def _oracle(fp):
    from oracle import loader
    return loader.plan(fp)


@pytest.fixture(scope="module")
def emu_planner():
    pl = hip.Planner(lib_path=build_emu())
    yield pl
    pl.close()


def pmap_of(fp, res):
    return problem.decode_result(fp, res)[0]


def top_keys(doc):
    """The document's keys in document order, as bytes."""
    pairs = json.JSONDecoder(object_pairs_hook=lambda kv: kv).decode(doc.decode("utf-8"))
    return [k.encode("utf-8") for k, _ in pairs]


def check_document(fp, res, doc, tag=""):
    """The two comparisons of every checked plan, and the key order."""
    pmap = pmap_of(fp, res)
    assert doc == wire.encode(pmap), tag
    assert json.loads(doc) == pmap, tag
    keys = top_keys(doc)
    assert keys == sorted(keys), tag
    return pmap


def plan_and_check(pl, fp, tag, vs_oracle=True):
    res = pl.plan(fp)
    if vs_oracle:
        assert res.digest() == _oracle(fp).digest(), tag
    if res.iterations == 0:
        return None
    pl.set_wire_names(fp)
    doc, info = pl.plan_wire()
    assert info["need"] == len(doc)
    return res, doc, check_document(fp, res, doc, tag)


def run_golden(pl, golden_cases):
    n = missing = empty = full = null = 0
    for c in golden_cases:
        fp = build_from_case(c)
        if pl.validate(fp) != abi.OK:
            continue
        got = plan_and_check(pl, fp, c["source"])
        if got is None:
            continue
        n += 1
        for part in got[2].values():
            nbs = part["nodesByState"]
            missing += sum(1 for s in fp.state_names if s not in nbs)
            empty += sum(1 for v in nbs.values() if v == [])
            full += sum(1 for v in nbs.values() if v)
            null += sum(1 for v in nbs.values() if v is None)
    return n, missing, empty, full, null


def test_golden_cases(emu_planner, golden_cases):
    n, missing, empty, full, null = run_golden(emu_planner, golden_cases)
    assert n >= 60
    assert missing > 0 and empty > 0 and full > 0


@pytest.mark.parametrize("seed", [0, 100])
def test_random_cases(emu_planner, seed):
    pairs = [(fp, prev) for fp, prev in _mixed(seed) if emu_planner.validate(fp) == abi.OK]
    sweeps = []
    for i, (fp, _) in enumerate(pairs):
        res, _, _ = plan_and_check(emu_planner, fp, ("mixed", seed, i))
        sweeps.append(res.iterations if fp.n_prev > 0 else 0)
    assert max(sweeps) >= 2


def unordered_names(P):
    """P partition names whose id order is not their byte order: "10" < "9" < "a" < "ab", the empty name, and numbers of
    mixed width ("0000013" < "12")."""
    names = ["9", "10", "a", "ab", ""][:P]
    names += [str(i + 11) if i % 3 else "%07d" % (i + 11) for i in range(P - len(names))]
    assert len(set(names)) == P
    return names


def named(fp, part_names=None):
    """A synthetic problem carries ids only: give it names.  The plan goes by ids, only the document (and decode_result)
    reads the names, so any unique partition names will do."""
    fp.part_names = list(part_names) if part_names is not None else (fp.part_names or [str(p) for p in range(fp.n_parts)])
    fp.node_names = fp.node_names or ["n%04d" % i for i in range(fp.n_nodes_ext)]
    fp.state_names = fp.state_names or ["primary", "replica", "spare", "dead"][:fp.n_states]
    assert len(fp.part_names) == fp.n_parts and len(fp.node_names) == fp.n_nodes_ext and len(fp.state_names) == fp.n_states
    return fp


def renamed(fp, part_names):
    return named(fp, part_names)


ORDER_SIZES = [1, 2, 255, 256, 257, 1000, 4099]


@pytest.mark.parametrize("P", ORDER_SIZES)
def test_order(emu_planner, P):
    fp = renamed(synth.config_flat(2, P=P, N=16), unordered_names(P))
    res, doc, _ = plan_and_check(emu_planner, fp, ("order", P))
    keys = top_keys(doc)
    assert len(keys) == P and keys == sorted(n.encode() for n in fp.part_names)
    if P > 1:
        assert keys != [n.encode() for n in fp.part_names]               # the permutation is not the identity


# ---- escapes: names as raw bytes ------------------------------------------------------------------------------------

def escape_strings():
    """Every string of the nine marshal vectors of tests/golden/wire_cases.json, and the hard ones by hand."""
    with open(os.path.join(ROOT, "tests", "golden", "wire_cases.json")) as f:
        cases = json.load(f)
    assert len(cases["marshal"]) + len(cases["marshal_raw"]) == 9
    found = []

    def walk(v):
        if isinstance(v, str):
            found.append(v.encode("utf-8"))
        elif isinstance(v, dict):
            for k, x in v.items():
                walk(k)
                walk(x)
        elif isinstance(v, list):
            for x in v:
                walk(x)

    for c in cases["marshal"]:
        walk(c["value"])
    for c in cases["marshal_raw"]:
        found += [bytes.fromhex(c["key_hex"]), bytes.fromhex(c["name_hex"])]
    found += [b'"', b"\\", b"<>&", b"\x01", b"\t", "\u2028".encode("utf-8"), "\u2029".encode("utf-8"), b"\xff", b"\xe2\x82", b""]
    out = []
    for s in found:
        if s not in out:
            out.append(s)
    return out


def encode_raw(res, P, M, part_names, node_names, state_names):
    """The host encoder on a downloaded result with names as raw bytes (wire.encode_arrays): key = name = the partition's
    name, one entry per (partition, state) that is not ABSENT."""
    part_off, entry_state, entry_kind, entry_off, entry_nodes = [0], [], [], [0], []
    for p, lists in enumerate(res.lists()):
        for m, (kind, ids) in enumerate(lists):
            if kind == abi.LIST_ABSENT:
                continue
            entry_state.append(m)
            entry_kind.append(wire.NIL if kind == abi.LIST_NIL else wire.LIST)
            entry_nodes += ids.tolist()
            entry_off.append(len(entry_nodes))
        part_off.append(len(entry_state))
    return wire.encode_arrays(list(part_names), list(part_names), [wire.LIST] * P, part_off, list(state_names),
                              list(node_names), entry_state, entry_kind, entry_off, entry_nodes)


def run_escapes(pl):
    strs = escape_strings()
    assert len(strs) >= 20
    P = len(strs)
    fp = synth.config_flat(2, P=P, N=P)
    M, NX = fp.n_states, fp.n_nodes_ext
    assert M == 2 and NX >= P
    res = pl.plan(fp)
    assert res.digest() == _oracle(fp).digest()
    nodes = [strs[i % P] for i in range(NX)]
    used_nodes = {nodes[i] for i in res.out_nodes[:int(res.out_off[P * M])].tolist()}
    assert used_nodes == set(strs)                                        # every string is written as a node name
    seen_states = set()
    for k in range(0, P, M):
        states = [strs[(k + j) % P] for j in range(M)]
        pl.set_wire_names(strs, nodes, states)
        doc, _ = pl.plan_wire()
        assert doc == encode_raw(res, P, M, strs, nodes, states), states
        seen_states |= set(states)
    assert seen_states == set(strs)
    assert b"\\ufffd" in doc and b"\\u2028" in doc and b"\\u003c" in doc and b'"\\""' in doc and b"\\u0001" in doc
    return doc


def test_escapes(emu_planner):
    run_escapes(emu_planner)


# ---- the LDS stage: sub-runs, the oversize path, every alignment ------------------------------------------------------------

def stage_names(P=300):
    """Names of lengths 0 .. 40 (every residue mod 16 of a rank's first byte comes about), and two names that alone are
    larger than a stage of 256 bytes."""
    names = []
    for i in range(P):
        n = i % 41
        tag = "%x" % i
        name = (tag + "_" * n)[:n] if n >= len(tag) + 1 else tag + "!" * 3
        names.append(name)
    names[7], names[150] = "L" * 150, "M" * 500
    assert len(set(names)) == P
    return names


def piece_lengths(pmap):
    """Bytes of every rank's piece of the document: the separator, the partition, the closing brace behind the last."""
    keys = sorted(pmap, key=lambda k: k.encode("utf-8"))
    lens = [len(wire.encode({k: pmap[k]})) - 1 for k in keys]
    lens[-1] += 1
    return lens


def sub_runs(lens, stage):
    """k_wire_write's cuts: [(first byte, last byte + 1, ranks, oversize)] of every sub-run."""
    off = np.concatenate([[0], np.cumsum(lens)]).tolist()
    out = []
    for r0 in range(0, len(lens), RUN):
        r1 = min(r0 + RUN, len(lens))
        a = r0
        while a < r1:
            b = a
            while b < r1 and off[b + 1] - off[a] <= stage - STAGE_SKEW:
                b += 1
            if b == a:
                out.append((off[a], off[a + 1], 1, True))
                a += 1
            else:
                out.append((off[a], off[b], b - a, False))
                a = b
    return out


def run_small_stage(make_planner, monkeypatch):
    monkeypatch.setenv("BLANCE_WIRE_STAGE", "256")
    pl = make_planner()
    try:
        fp = synth.config_flat(2, P=300, N=16)
        fp.node_names = ["n%d" % i + "y" * (i % 4) for i in range(fp.n_nodes_ext)]   # (a name counts twice: the nodes make odd lengths)
        fp = renamed(fp, stage_names())
        res, doc, pmap = plan_and_check(pl, fp, "stage 256")
    finally:
        pl.close()
    lens = piece_lengths(pmap)
    assert sum(lens) == len(doc)
    runs = sub_runs(lens, 256)
    staged = [r for r in runs if not r[3]]
    assert sum(r[3] for r in runs) >= 2                                   # partitions on the oversize path
    assert len(staged) > 2 * ((300 + RUN - 1) // RUN)                     # sub-run cuts inside a workgroup's run
    assert {r[0] % 16 for r in staged} == set(range(16)) == {r[1] % 16 for r in staged}
    return doc


def test_small_stage(monkeypatch):
    run_small_stage(lambda: hip.Planner(lib_path=build_emu()), monkeypatch)


def run_long_name(pl):
    """The default stage and one partition larger than it."""
    names = ["b", "a" * 100000, "c"]
    fp = renamed(synth.config_flat(2, P=3, N=8), names)
    res, doc, pmap = plan_and_check(pl, fp, "long name")
    assert len(doc) > 200000 and max(piece_lengths(pmap)) > 65536


def test_long_name(emu_planner):
    run_long_name(emu_planner)


def test_result_encoder_is_the_host_route(emu_planner):
    """wire.ResultEncoder (the route plan_wire replaces, as tools/plan_wire_gpu.py times it) is wire.encode of the result."""
    fp = named(_rebalance(emu_planner, 300, 20))
    res = emu_planner.plan(fp)
    enc = wire.ResultEncoder(fp.part_names, fp.node_names, fp.state_names)
    assert enc.encode(res) == wire.encode(pmap_of(fp, res))


# ---- the C contract ---------------------------------------------------------------------------------------------------------

SENTINEL = 0xAB


def _get(pl, buf, cap):
    need = C.c_size_t(12345)
    st = pl.lib.blance_plan_wire_get(pl._h, None if buf is None else buf.ctypes.data, cap, C.byref(need), None)
    return st, int(need.value)


def run_size_only_and_capacity(pl):
    fp = named(_rebalance(pl, 300, 20))
    pl.plan(fp)
    pl.set_wire_names(fp)
    doc, info = pl.plan_wire()
    none, sized = pl.plan_wire(size_only=True)
    assert none is None and sized["need"] == len(doc) == info["need"] > 0
    need = len(doc)
    assert _get(pl, None, 0) == (abi.OK, need)
    buf = np.full(need + 64, SENTINEL, np.uint8)
    assert _get(pl, buf, need) == (abi.OK, need)                                     # exactly the document: enough
    assert buf[:need].tobytes() == doc and (buf[need:] == SENTINEL).all()
    exact, _ = pl.plan_wire(capacity=need)
    assert exact == doc
    buf = np.full(need + 64, SENTINEL, np.uint8)
    assert _get(pl, buf, need - 1) == (abi.ERR_CAPACITY, need) and pl.lib.blance_last_error()
    assert (buf == SENTINEL).all()                                                   # one short: nothing is written
    with pytest.raises(hip.BlanceError) as e:
        pl.plan_wire(capacity=need - 1)
    assert e.value.status == abi.ERR_CAPACITY and e.value.info["need"] == need
    assert pl.plan_wire()[0] == doc                                                  # and the context answers as before


def test_size_only_and_capacity(emu_planner):
    run_size_only_and_capacity(emu_planner)


def _names_struct(part, node, state, part_off=None):
    keep, nm = [], abi.WireNames()
    for field, strs in (("part", part), ("node", node), ("state", state)):
        raw = [s if isinstance(s, bytes) else s.encode() for s in strs]
        off = np.zeros(len(raw) + 1, np.int64)
        off[1:] = np.cumsum([len(s) for s in raw]) if raw else 0
        if field == "part" and part_off is not None:
            off = np.asarray(part_off, np.int64)
        buf = C.create_string_buffer(b"".join(raw) + b"\0")
        keep += [buf, off]
        setattr(nm, field + "_bytes", C.cast(buf, C.c_void_p).value)
        setattr(nm, field + "_off", off.ctypes.data)
    nm._keep = keep
    return nm


def _refused(pl, status=abi.ERR_BAD_ARG):
    with pytest.raises(hip.BlanceError) as e:
        pl.plan_wire()
    return e.value.status == status and len(str(e.value)) > 0


def test_lifetime(emu_planner):
    pl = hip.Planner(lib_path=build_emu())
    try:
        fp = named(_rebalance(emu_planner, 64, 10))
        P = fp.n_parts
        lib = pl.lib
        assert lib.blance_plan_wire_names(None, C.byref(abi.WireNames())) == abi.ERR_BAD_ARG
        assert lib.blance_plan_wire_names(pl._h, None) == abi.ERR_BAD_ARG
        good = _names_struct(fp.part_names, fp.node_names, fp.state_names)
        assert lib.blance_plan_wire_names(pl._h, C.byref(good)) == abi.ERR_BAD_ARG   # no problem on the context
        need = C.c_size_t(0)
        assert lib.blance_plan_wire_get(None, None, 0, C.byref(need), None) == abi.ERR_BAD_ARG
        assert lib.blance_plan_wire_get(pl._h, None, 0, None, None) == abi.ERR_BAD_ARG
        assert lib.blance_plan_wire_get(pl._h, None, 8, C.byref(need), None) == abi.ERR_BAD_ARG   # no buffer, a capacity
        pl.upload(fp)
        pl.set_wire_names(fp)
        assert _refused(pl)                                                          # uploaded, not planned
        pl.plan_resident()
        doc = pl.plan_wire()[0]
        check_document(fp, pl.download(), doc)
        pl.plan_resident()                                                           # the names stay across plan_resident
        assert pl.plan_wire()[0] == doc
        pl.upload(fp)                                                                # a second upload, no new names
        pl.plan_resident()
        assert _refused(pl)
        pl.set_wire_names(fp)
        assert pl.plan_wire()[0] == doc
        pl.plan(fp)                                                                  # blance_plan replaces the problem too
        assert _refused(pl)
        pl.set_wire_names(fp)
        pl.plan_batch([fp])
        assert _refused(pl)                                                          # after a batch: no problem, no names
        with pytest.raises(hip.BlanceError) as e:
            pl.set_wire_names(fp)
        assert e.value.status == abi.ERR_BAD_ARG
        # names that are refused leave the ones set before as they were
        pl.plan(fp)
        assert _refused(pl)                                                          # planned, no names yet
        pl.set_wire_names(fp)
        dup = list(fp.part_names)
        dup[5] = dup[P - 1]
        with pytest.raises(hip.BlanceError) as e:
            pl.set_wire_names(dup, fp.node_names, fp.state_names)
        assert e.value.status == abi.ERR_UNSUPPORTED                                 # two partitions with one name
        with pytest.raises(hip.BlanceError) as e:
            pl.set_wire_names(fp.part_names, fp.node_names, [fp.state_names[0]] * fp.n_states)
        assert e.value.status == abi.ERR_BAD_ARG                                     # two states with one name
        off = np.zeros(P + 1, np.int64)
        off[1:] = np.cumsum([len(n) for n in fp.part_names])
        bad = off.copy()
        bad[3] = bad[4] + 1
        assert lib.blance_plan_wire_names(pl._h, C.byref(_names_struct(fp.part_names, fp.node_names, fp.state_names, bad))) \
            == abi.ERR_BAD_ARG                                                       # offsets not monotone
        bad = off.copy()
        bad[0] = 1
        assert lib.blance_plan_wire_names(pl._h, C.byref(_names_struct(fp.part_names, fp.node_names, fp.state_names, bad))) \
            == abi.ERR_BAD_ARG                                                       # offsets that do not start at 0
        nm = _names_struct(fp.part_names, fp.node_names, fp.state_names)
        nm.node_off = None
        assert lib.blance_plan_wire_names(pl._h, C.byref(nm)) == abi.ERR_BAD_ARG     # a NULL array
        assert pl.plan_wire()[0] == doc
        zero = named(_rebalance(pl, 64, 10))
        zero.scalars["max_iterations"] = 0
        zero._struct = None
        assert pl.plan(zero).iterations == 0
        pl.set_wire_names(zero)
        assert _refused(pl)                                                          # PlanNextMapEx returned no map
    finally:
        pl.close()


def run_context_undisturbed(pl, P, N):
    fp = named(_rebalance(pl, P, N))
    pl.upload(fp)
    pl.plan_resident()
    pl.set_wire_names(fp)
    before = pl.download()
    stats0 = pl.plan_stats(fp.n_states)
    mv0, _ = pl.plan_moves(False)
    doc1, _ = pl.plan_wire()
    assert pl.download().digest() == before.digest() == _oracle(fp).digest()
    stats1 = pl.plan_stats(fp.n_states)
    assert all(np.array_equal(stats0[k], stats1[k]) for k in stats0)
    same_moves(mv0, pl.plan_moves(False)[0], "moves after plan_wire")
    pl.plan_resident()                               # the begin map is still the upload, the names are still the problem's
    doc2, _ = pl.plan_wire()
    assert doc1 == doc2
    assert pl.download().digest() == before.digest()
    same_moves(mv0, pl.plan_moves(False)[0], "moves after the second plan")
    check_document(fp, before, doc2, "resident")


def test_context_undisturbed(emu_planner):
    run_context_undisturbed(emu_planner, 300, 20)


def test_empty_map(emu_planner):
    model = {"primary": {"priority": 0, "constraints": 1}}
    fp = problem.build_problem({}, {}, ["n0", "n1"], [], [], model)
    res = emu_planner.plan(fp)
    if res.iterations > 0:
        emu_planner.set_wire_names(fp)
        assert emu_planner.plan_wire()[0] == b"{}" == wire.encode({})
        assert emu_planner.plan_wire(size_only=True)[1]["need"] == 2


def test_symbols_and_struct_layout(tmp_path):
    """abi.WireNames matches include/blance_hip.h, and the gfx950 library exports both new symbols."""
    import subprocess
    import __graft_entry__ as g
    header = os.path.join(ROOT, "include", "blance_hip.h")
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\n'
                    'int main(){printf("%%zu %%zu %%zu\\n", sizeof(blance_wire_names), offsetof(blance_wire_names, node_off), '
                    'offsetof(blance_wire_names, state_bytes));return 0;}\n' % header)
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-o", str(exe), str(prog)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(abi.WireNames), abi.WireNames.node_off.offset, abi.WireNames.state_bytes.offset]
    g.build_hip()
    lib = hip.load_library()
    assert hasattr(lib, "blance_plan_wire_names") and hasattr(lib, "blance_plan_wire_get")
    assert lib.blance_abi_version() == 6
