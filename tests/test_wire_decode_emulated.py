"""blance_wire_dict_create / blance_wire_decode_device without a GPU: the kernels of blance_amd/csrc/k_wire_decode.h and their
host driver compiled against the SIMT emulator (tests/simt).  What a decode is compared with is never the code under test:
the host decoder (blance_amd.wire.decode) carried over to the dictionary's ids, json.loads carried over in plain Python, the
arrays problem.build_problem makes of the same map, and the downloaded plan (tests/wire_decode_cases.py has the documents and
the checks; tests/test_wire_decode_gpu.py runs the same on the device).  One test builds the stand-alone sanitizer program
(tests/simt/wire_decode_asan_main.cpp) and runs it on the seam documents and the mutants."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import wire_decode_cases as W
from blance_amd import abi, hip, planner, wire
from helpers import build_from_case
from test_plan_batch_moves_emulated import _mixed
from test_plan_moves_emulated import _rebalance, same_moves
from test_plan_wire_emulated import named
from test_simt_emulated import HERE, _deps, build_emu

ROOT = os.path.dirname(HERE)


def _oracle(fp):
    from oracle import loader
    return loader.plan(fp)


@pytest.fixture(scope="module")
def emu_planner():
    pl = hip.Planner(lib_path=build_emu())
    yield pl
    pl.close()


@pytest.fixture(scope="module")
def wire_cases():
    with open(os.path.join(ROOT, "tests", "golden", "wire_cases.json")) as f:
        return json.load(f)


# ---- the problem's own arrays ---------------------------------------------------------------------------------------------

def expected_refusal(pmap, fp):
    """Why the device must refuse wire.encode(pmap) against fp's names (None: it must accept): the first thing outside the
    names in the order of the document -- keys sorted bytewise, name in front of nodesByState, states sorted."""
    if pmap is None:
        return "null_document"
    parts, states = set(fp.part_names), set(fp.state_names)
    for key in sorted(pmap, key=lambda k: k.encode("utf-8")):
        part = pmap[key]
        if key not in parts:
            return "unknown_partition"
        if part is None:
            return "null_partition"
        if part["name"] != key:
            return "name_differs"
        for s in sorted(part.get("nodesByState") or {}, key=lambda k: k.encode("utf-8")):
            if s not in states:
                return "unknown_state"
    return None


def run_problem_arrays(pl, golden_cases):
    """wire.encode(prevMap) decodes to fp's prev_* and part_in_prev, wire.encode(partitionsToAssign) to its assign_*."""
    accepted = 0
    reasons = {}
    for c in golden_cases:
        fp = build_from_case(c)
        if pl.validate(fp) != abi.OK:
            continue
        P, M = fp.n_parts, fp.n_states
        wdict = pl.wire_dict(fp)
        prev = c["prevMap"]
        both = True
        for which, pmap in (("prev", prev), ("assign", prev if c.get("aliased") else c["partitionsToAssign"])):
            why = expected_refusal(pmap, fp)
            got = pl.decode_wire(wdict, wire.encode(pmap))
            assert abi.WIRE_REFUSALS[got["refusal"]] == (why or "accepted"), (c["source"], which, got["refusal_at"])
            if why:
                reasons[why] = reasons.get(why, 0) + 1
                both = False
                continue
            n = int(fp.arrays[which + "_off"][P * M])
            assert got["n_node_refs"] == n, (c["source"], which)
            assert np.array_equal(got["off"], fp.arrays[which + "_off"][:P * M + 1]), (c["source"], which)
            assert np.array_equal(got["nodes"], fp.arrays[which + "_nodes"][:n]), (c["source"], which)
            assert np.array_equal(got["kind"], fp.arrays[which + "_kind"][:P * M]), (c["source"], which)
            if which == "prev":
                assert np.array_equal(got["part_kind"] != abi.LIST_ABSENT, fp.arrays["part_in_prev"][:P] != 0), c["source"]
            else:
                assert (got["part_kind"] != abi.LIST_ABSENT).all(), c["source"]
        accepted += both
        wdict.close()
    # (no golden case has a map outside its problem's names: all 69 that validate are accepted twice)  The random problems
    # bring prevMaps with partitions that are not assigned and with state keys outside the model: refused, with the reason.
    for i, (fp, prev) in enumerate(_mixed(0)):
        if pl.validate(fp) != abi.OK or not fp.part_names:
            continue
        prev = {k: (v if isinstance(v, dict) else {"name": v.Name, "nodesByState": v.NodesByState}) for k, v in (prev or {}).items()}
        why = expected_refusal(prev, fp)
        wdict = pl.wire_dict(fp)
        got = pl.decode_wire(wdict, wire.encode(prev))
        wdict.close()
        assert abi.WIRE_REFUSALS[got["refusal"]] == (why or "accepted"), ("mixed", i, got["refusal_at"])
        if why:
            reasons[why] = reasons.get(why, 0) + 1
            continue
        P, M = fp.n_parts, fp.n_states
        n = int(fp.arrays["prev_off"][P * M])
        assert np.array_equal(got["off"], fp.arrays["prev_off"][:P * M + 1]) and np.array_equal(got["nodes"], fp.arrays["prev_nodes"][:n]), i
        assert np.array_equal(got["kind"], fp.arrays["prev_kind"][:P * M]), i
        assert np.array_equal(got["part_kind"] != abi.LIST_ABSENT, fp.arrays["part_in_prev"][:P] != 0), i
    return accepted, reasons


def test_problem_arrays(emu_planner, golden_cases):
    accepted, reasons = run_problem_arrays(emu_planner, golden_cases)
    assert accepted >= 40, (accepted, reasons)
    assert reasons, "no case exercises a refusal"


# ---- round trip -----------------------------------------------------------------------------------------------------------

def round_trip(pl, fp, tag):
    """The document plan_wire() composes decodes to the downloaded result."""
    res = pl.plan(fp)
    if res.iterations == 0:
        return False
    pl.set_wire_names(fp)
    doc, _ = pl.plan_wire()
    wdict = pl.wire_dict(fp)
    got = pl.decode_wire(wdict, doc)
    wdict.close()
    PM = fp.n_parts * fp.n_states
    n = int(res.out_off[PM])
    assert got["refusal"] == 0, (tag, abi.WIRE_REFUSALS[got["refusal"]], got["refusal_at"])
    assert got["n_node_refs"] == n and got["n_parts_seen"] == fp.n_parts, tag
    assert np.array_equal(got["off"], res.out_off[:PM + 1]) and np.array_equal(got["nodes"], res.out_nodes[:n]), tag
    assert np.array_equal(got["kind"], res.out_kind[:PM]) and (got["part_kind"] == abi.LIST_SET).all(), tag
    return True


def run_round_trip(pl, golden_cases):
    n = 0
    for c in golden_cases:
        fp = build_from_case(c)
        if pl.validate(fp) == abi.OK:
            n += round_trip(pl, fp, c["source"])
    for i, (fp, _) in enumerate(_mixed(0)):
        if pl.validate(fp) == abi.OK:
            n += round_trip(pl, named(fp), ("mixed", i))
    return n


def test_round_trip(emu_planner, golden_cases):
    assert run_round_trip(emu_planner, golden_cases) >= 60


# ---- inside the subset, seams, outside --------------------------------------------------------------------------------------

def run_subset(pl):
    wdict = W.make_dict(pl)
    docs = W.subset_documents()
    for tag, doc in docs:
        W.check_accepted(pl, wdict, doc, tag)
    joined = b"".join(d for _, d in docs)
    for token in (b"\\u0041", b"\\/", b"\\ud83d\\uDE00", "\U0001F600".encode(), b"null", b"[]", b"\\u0022"):
        assert token in joined or token.lower() in joined.lower(), token           # the generator reaches every form it names
    wdict.close()
    return len(docs)


def test_subset(emu_planner):
    assert run_subset(emu_planner) > 60


def own_planner(make_planner, monkeypatch, tile):
    """BLANCE_WIRE_IN_TILE is read when a context is made: a planner of its own (tile None: the default tile)."""
    if tile is not None:
        monkeypatch.setenv("BLANCE_WIRE_IN_TILE", str(tile))
    return make_planner(), (tile or W_DEFAULT_TILE)


W_DEFAULT_TILE, W_DEFAULT_STAGE = 256, 32 * 1024        # k_wire_decode.h: kWdTileDefault, kWdStageDefault


def run_seams(make_planner, monkeypatch, tile):
    pl, T = own_planner(make_planner, monkeypatch, tile)
    try:
        wdict = W.make_dict(pl)
        docs = W.seam_documents(T, W_DEFAULT_STAGE)
        for tag, doc in docs:
            got = W.check_accepted(pl, wdict, doc, (T, tag))
            if tag.endswith("records"):
                assert got["n_parts_seen"] == int(tag.split()[0])
        assert max(len(d) for _, d in docs) > W_DEFAULT_STAGE
        return len(docs)
    finally:
        pl.close()


@pytest.mark.parametrize("tile", [64, None])
def test_seams(monkeypatch, tile):
    assert run_seams(lambda: hip.Planner(lib_path=build_emu()), monkeypatch, tile) > 30


def test_small_stage(monkeypatch):
    """Most workgroups read global memory: a stage of 256 bytes holds two or three records."""
    monkeypatch.setenv("BLANCE_WIRE_IN_STAGE", "256")
    assert run_seams(lambda: hip.Planner(lib_path=build_emu()), monkeypatch, 64) > 30


def run_refusals(make_planner, monkeypatch, tile, wire_cases):
    pl, T = own_planner(make_planner, monkeypatch, tile)
    try:
        wdict = W.make_dict(pl)
        seen = set()
        for tag, doc, reason, lo, hi in W.refusal_documents(T):
            W.check_refused(pl, wdict, doc, reason, lo, hi, (T, tag))
            seen.add(reason)
        gdict = W.golden_dict(pl)
        for tag, doc, reason in W.golden_vector_documents(wire_cases):
            W.check_refused(pl, gdict, doc, reason, tag=(T, tag))
            seen.add(reason)
        # the limit of size: a record, the bytes in front of the first and the space behind the document, each below 1 MiB
        inside, outside = W.size_limit_documents()
        for tag, doc in inside:
            W.check_accepted(pl, wdict, doc, (T, tag))
        for tag, doc, lo, hi in outside:
            W.check_refused(pl, wdict, doc, "record_too_long", lo, hi, (T, tag))
        # A length of 2^31 is refused before a byte is read, and ONLY therefore may this call hand the library a buffer of
        # three bytes beside it: a library that read first would read outside the buffer instead of failing an assertion.
        st, wl, arrays = W.raw_decode(pl, wdict, b"{}", 64, length=1 << 31)
        assert st == abi.ERR_UNSUPPORTED and abi.WIRE_REFUSALS[wl.refusal] == "document_too_long" and W.untouched(arrays)
        seen |= {"record_too_long", "document_too_long"}
        assert seen == set(abi.WIRE_REFUSALS[1:]), set(abi.WIRE_REFUSALS[1:]) - seen
        W.check_accepted(pl, wdict, W.document([W.record("p0", {"primary": ["a"]})]), "and the planner still decodes")
    finally:
        pl.close()


@pytest.mark.parametrize("tile", [64, None])
def test_refusals(monkeypatch, tile, wire_cases):
    run_refusals(lambda: hip.Planner(lib_path=build_emu()), monkeypatch, tile, wire_cases)


def test_host_decoder_accepts_what_the_subset_allows():
    """On the CPU alone, before anything relies on it: the host decoder takes every document of the two accepting families.
    (This checks the references, not the feature: it runs no new code and passes without the decoder.)"""
    for tag, doc in W.subset_documents() + W.seam_documents(64) + W.seam_documents(256):
        wm = wire.decode(doc)
        want = {k: {"name": p["name"], "nodesByState": p.get("nodesByState")} for k, p in json.loads(doc).items()}   # (missing: nil)
        assert wm.to_dict() == want, tag
        wm.close()


# ---- the C contract ---------------------------------------------------------------------------------------------------------

def run_capacity_and_memory(pl, arena):
    wdict = W.make_dict(pl)
    doc = dict(W.seam_documents(64))["4099 records"]
    full = W.check_accepted(pl, wdict, doc, "pageable")
    n = full["n_node_refs"]
    assert n > 4099
    counted = pl.decode_wire(wdict, doc, count_only=True)
    assert counted["nodes"] is None and counted["n_node_refs"] == n and counted["n_parts_seen"] == 4099 and counted["refusal"] == 0
    exact = pl.decode_wire(wdict, doc, capacity=n)
    W.same_lists(exact, full, "capacity = n_node_refs")
    st, wl, arrays = W.raw_decode(pl, wdict, doc, n - 1)
    assert st == abi.ERR_CAPACITY and wl.n_node_refs == n and wl.n_parts_seen == 4099 and W.untouched(arrays)
    with pytest.raises(hip.BlanceError) as e:
        pl.decode_wire(wdict, doc, capacity=n - 1)
    assert e.value.status == abi.ERR_CAPACITY and e.value.info["n_node_refs"] == n
    st, wl, arrays = W.raw_decode(pl, wdict, doc, n + 7)
    assert st == abi.OK and wl.n_node_refs == n and (arrays[3][n:] == 0x2B2B2B2B).all() and np.array_equal(arrays[3][:n], full["nodes"])
    # the document in page-locked memory (read by DMA where it lies), the arrays in page-locked memory
    pinned_doc = arena.copy_of(np.frombuffer(doc, np.uint8))
    W.same_lists(pl.decode_wire(wdict, pinned_doc), full, "page-locked document")
    W.same_lists(pl.decode_wire(wdict, pinned_doc, arena=arena), full, "page-locked arrays")
    W.same_lists(pl.decode_wire(wdict, np.frombuffer(doc, np.uint8).copy()), full, "numpy document")
    # bad arguments: nothing launched
    lib = pl.lib
    wl = abi.WireLists()
    buf = C.create_string_buffer(doc)
    assert lib.blance_wire_decode_device(None, wdict._h, buf, len(doc), C.byref(wl)) == abi.ERR_BAD_ARG
    assert lib.blance_wire_decode_device(pl._h, None, buf, len(doc), C.byref(wl)) == abi.ERR_BAD_ARG
    assert lib.blance_wire_decode_device(pl._h, wdict._h, None, len(doc), C.byref(wl)) == abi.ERR_BAD_ARG
    assert lib.blance_wire_decode_device(pl._h, wdict._h, buf, len(doc), None) == abi.ERR_BAD_ARG
    wl.capacity = 5                                                                  # a capacity and no nodes
    assert lib.blance_wire_decode_device(pl._h, wdict._h, buf, len(doc), C.byref(wl)) == abi.ERR_BAD_ARG
    wdict.close()
    wdict.close()                                                                    # (twice is harmless)


def test_capacity_and_memory(emu_planner):
    run_capacity_and_memory(emu_planner, hip.HostArena(lib_path=build_emu()))


def run_dictionary(pl, other):
    """What blance_wire_dict_create refuses, and whose a dictionary is."""
    for names, status in (((["p", "p"], ["a"], ["s"]), abi.ERR_UNSUPPORTED), ((["p"], ["a"], ["s", "s"]), abi.ERR_BAD_ARG),
                          ((["p"], ["a", "a"], ["s"]), abi.ERR_BAD_ARG)):
        with pytest.raises(hip.BlanceError) as e:
            pl.wire_dict(*names)
        assert e.value.status == status, names
    h = C.c_void_p()
    nm, keep = hip.wire_names_struct(["p"], ["a"], ["s"])
    assert pl.lib.blance_wire_dict_create(None, C.byref(nm), 1, 1, 1, C.byref(h)) == abi.ERR_BAD_ARG
    assert pl.lib.blance_wire_dict_create(pl._h, None, 1, 1, 1, C.byref(h)) == abi.ERR_BAD_ARG
    assert pl.lib.blance_wire_dict_create(pl._h, C.byref(nm), 1, 1, 1, None) == abi.ERR_BAD_ARG
    assert pl.lib.blance_wire_dict_create(pl._h, C.byref(nm), -1, 1, 1, C.byref(h)) == abi.ERR_BAD_ARG
    nm.node_off = None
    assert pl.lib.blance_wire_dict_create(pl._h, C.byref(nm), 1, 1, 1, C.byref(h)) == abi.ERR_BAD_ARG
    empty = pl.wire_dict([], [], [])                                                 # no names at all: `{}` and nothing else
    assert pl.decode_wire(empty, b"{}")["refusal"] == 0
    assert abi.WIRE_REFUSALS[pl.decode_wire(empty, b'{"p":{"name":"p"}}')["refusal"]] == "unknown_partition"
    mine = pl.wire_dict(["p"], ["a"], ["s"])
    with pytest.raises(hip.BlanceError) as e:
        other.decode_wire(mine, b"{}")                                               # a dictionary of another context
    assert e.value.status == abi.ERR_BAD_ARG
    other.lib.blance_wire_dict_destroy(other._h, mine._h)                            # ... which that context does not destroy
    got = pl.decode_wire(mine, b'{"p":{"name":"p","nodesByState":{"s":["a","a"]}}}')
    assert got["refusal"] == 0 and got["nodes"].tolist() == [0, 0] and got["kind"].tolist() == [abi.LIST_SET]
    mine.close()
    empty.close()


def test_dictionary(emu_planner):
    other = hip.Planner(lib_path=build_emu())
    try:
        run_dictionary(emu_planner, other)
    finally:
        other.close()


def run_context_undisturbed(pl, P, N):
    """A resident plan's download, statistics, moves and JSON are the same before and after a decode and after creating and
    destroying a dictionary; the dictionary outlives upload and plan."""
    fp = named(_rebalance(pl, P, N))
    pl.upload(fp)
    pl.plan_resident()
    pl.set_wire_names(fp)
    before = pl.download()
    assert before.digest() == _oracle(fp).digest()
    stats0 = pl.plan_stats(fp.n_states)
    mv0, _ = pl.plan_moves(False)
    doc0, _ = pl.plan_wire()
    wdict = pl.wire_dict(fp)
    PM = fp.n_parts * fp.n_states

    def decode_is_the_plan(tag):
        got = pl.decode_wire(wdict, doc0)
        n = int(before.out_off[PM])
        assert got["refusal"] == 0 and np.array_equal(got["off"], before.out_off[:PM + 1]), tag
        assert np.array_equal(got["nodes"], before.out_nodes[:n]) and np.array_equal(got["kind"], before.out_kind[:PM]), tag

    def context_answers_as_before(tag):
        assert pl.download().digest() == before.digest(), tag
        stats1 = pl.plan_stats(fp.n_states)
        assert all(np.array_equal(stats0[k], stats1[k]) for k in stats0), tag
        same_moves(mv0, pl.plan_moves(False)[0], tag)
        assert pl.plan_wire()[0] == doc0, tag

    decode_is_the_plan("first decode")
    context_answers_as_before("after a decode")
    assert pl.decode_wire(wdict, b'{"nobody":null}')["refusal"] != 0
    context_answers_as_before("after a refusal")
    pl.wire_dict(["x"], ["y"], ["z"]).close()
    context_answers_as_before("after creating and destroying a dictionary")
    pl.plan_resident()                                   # the begin map is still the upload
    context_answers_as_before("after the second plan")
    pl.upload(fp)                                        # the dictionary is independent of the problem the context holds
    decode_is_the_plan("after an upload")
    pl.plan(fp)
    decode_is_the_plan("after a plan")
    wdict.close()


def test_context_undisturbed(emu_planner):
    run_context_undisturbed(emu_planner, 300, 20)


def run_fallback(pl):
    """planner.decode_partition_map: the device's lists, or the host decoder's for what the device refuses."""
    wdict = W.make_dict(pl)
    doc = W.document([W.record("p0", {"primary": ["a"]}), W.record("p1", None)])
    got = planner.decode_partition_map(pl, wdict, doc)
    assert got["route"] == "device" and not got["names_differ"].any()
    # outside the subset, inside Go's semantics: a field in another case, an unknown field, a repeated key that replaces
    odd = b'{"p0":{"NAME":"p0","extra":[1,2],"nodesByState":{"primary":["b"]}},"p1":{"name":"p1"},"p1":{"name":"zz","nodesByState":{"replica":["a","c"]}}}'
    host = planner.decode_partition_map(pl, wdict, odd)
    assert host["route"] == "host" and abi.WIRE_REFUSALS[host["refusal"]] == "unknown_field"
    want = W.lists_of_python_map({"p0": {"name": "p0", "nodesByState": {"primary": ["b"]}},
                                  "p1": {"name": "p1", "nodesByState": {"replica": ["a", "c"]}}}, wdict.part_names, wdict.node_names, wdict.state_names)
    W.same_lists(host, want, "fallback")
    assert host["names_differ"].tolist().count(True) == 1 and host["names_differ"][1]
    with pytest.raises(planner.problem.Unsupported):
        planner.decode_partition_map(pl, wdict, b'{"nobody":{"name":"nobody"}}')     # a name outside the dictionary raises there
    with pytest.raises(wire.WireError):
        planner.decode_partition_map(pl, wdict, b'{"p0":{"name":"p0"')                # and the host decoder reports syntax errors
    wdict.close()


def test_fallback(emu_planner):
    run_fallback(emu_planner)


# ---- mutants ----------------------------------------------------------------------------------------------------------------

def run_mutants(pl):
    wdict = W.make_dict(pl)
    docs = W.mutants()
    both = device_only_refused = 0
    for tag, doc in docs:
        dev, host = W.check_mutant(pl, wdict, doc, tag)
        both += dev
        device_only_refused += host and not dev
    assert W.check_mutant(pl, wdict, W.mutant_base(), "base") == (True, True)
    assert both >= 10 and device_only_refused >= 10, (both, device_only_refused)     # the family reaches both sides of the contract
    wdict.close()
    return len(docs)


def test_mutants(emu_planner):
    assert run_mutants(emu_planner) >= 400


# ---- bindings -----------------------------------------------------------------------------------------------------------------

def test_symbols_and_struct_layout(tmp_path):
    """abi.WireLists matches include/blance_hip.h, the reason codes match, and the gfx950 library exports the new symbols."""
    import __graft_entry__ as g
    header = os.path.join(ROOT, "include", "blance_hip.h")
    fields = ["part_kind", "off", "kind", "nodes", "capacity", "n_node_refs", "n_parts_seen", "refusal", "refusal_at", "device_ms", "total_ms"]
    codes = [n.upper() for n in abi.WIRE_REFUSALS[1:]]
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu", sizeof(blance_wire_lists));\n' % header +
                    "".join('printf(" %%zu", offsetof(blance_wire_lists, %s));\n' % f for f in fields) +
                    "".join('printf(" %%d", BLANCE_WIRE_REFUSED_%s);\n' % c for c in codes) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-o", str(exe), str(prog)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(abi.WireLists)] + [getattr(abi.WireLists, f).offset for f in fields] + list(range(1, len(codes) + 1))
    g.build_hip()
    lib = hip.load_library()
    for name in ("blance_wire_dict_create", "blance_wire_dict_destroy", "blance_wire_decode_device"):
        assert hasattr(lib, name), name
    assert lib.blance_abi_version() == 6


def test_library_without_the_symbols():
    """Against a library from before the decoder, wire_dict and decode_wire raise ERR_UNSUPPORTED, as set_wire_names does."""
    pl = hip.Planner(lib_path=build_emu())
    real = pl.lib

    class Before:
        def __getattr__(self, name):
            if name.startswith("blance_wire_dict_") or name == "blance_wire_decode_device":
                raise AttributeError(name)
            return getattr(real, name)

    wdict = W.make_dict(pl)
    pl.lib = Before()
    try:
        for call in (lambda: pl.wire_dict(["p"], ["a"], ["s"]), lambda: pl.decode_wire(wdict, b"{}"),
                     lambda: planner.decode_partition_map(pl, wdict, b"{}")):
            with pytest.raises(hip.BlanceError) as e:
                call()
            assert e.value.status == abi.ERR_UNSUPPORTED
    finally:
        pl.lib = real
        wdict.close()
        pl.close()


# ---- the stand-alone sanitizer program ------------------------------------------------------------------------------------------

ASAN_SRC = os.path.join(HERE, "simt", "wire_decode_asan_main.cpp")
ASAN_EXE = os.path.join(HERE, "simt", "_build", "wire_decode_asan")


SANITIZE = ["-fsanitize=address,undefined", "-static-libasan", "-static-libubsan"]     # the runtimes inside the program: nothing it
#                                                                                        meets in the process's library list matters


def build_asan_program():
    """The program, or None with the linker's or the runtime's words when a sanitized program does not link or start here."""
    import fcntl
    deps = _deps() + [ASAN_SRC, os.path.join(HERE, "kernels", "wire_decode_cases.inc")]
    os.makedirs(os.path.dirname(ASAN_EXE), exist_ok=True)
    with open(ASAN_EXE + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not os.path.exists(ASAN_EXE) or any(os.path.getmtime(d) > os.path.getmtime(ASAN_EXE) for d in deps):
            probe = subprocess.run(["g++"] + SANITIZE + ["-x", "c++", "-", "-o", ASAN_EXE + ".probe"],
                                   input="int main(){return 0;}\n", capture_output=True, text=True)
            if probe.returncode != 0:
                return None, probe.stderr[-400:]
            started = subprocess.run([ASAN_EXE + ".probe"], capture_output=True, text=True)      # (in the environment as it is)
            os.remove(ASAN_EXE + ".probe")
            if started.returncode != 0:
                return None, "the program does not start: " + started.stderr[-400:]
            tmp = "%s.%d.tmp" % (ASAN_EXE, os.getpid())
            subprocess.check_call(["g++", "-x", "c++", "-std=c++17", "-O1", "-g1"] + SANITIZE + ["-fno-sanitize-recover=undefined",
                                   "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wno-unknown-pragmas", "-o", tmp, ASAN_SRC])
            os.replace(tmp, ASAN_EXE)
    return ASAN_EXE, ""


@pytest.mark.parametrize("tile,stage", [(64, 256), (256, 32 * 1024)])
def test_sanitized_program(tmp_path, monkeypatch, tile, stage):
    """The seam documents, the refusals and the mutants through the stand-alone program under AddressSanitizer and UBSan, every
    buffer of exactly its documented size; its answers are the emulator library's."""
    exe, why = build_asan_program()
    if exe is None:
        pytest.skip("-fsanitize=address does not link or start on this machine: " + why)
    docs = [d for _, d in W.seam_documents(tile, stage)] + [d for _, d in W.mutants()] + [d for _, d, _, _, _ in W.refusal_documents(tile)]
    path = tmp_path / "input.txt"
    W.write_program_input(str(path), W.PARTS + W.SPECIAL, W.NODES, W.STATES, docs, tile, stage)
    env = dict(os.environ)                                                           # as it is, plus the two sanitizers' options
    env["ASAN_OPTIONS"] = "detect_leaks=0:detect_stack_use_after_return=0:abort_on_error=1"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=1500, env=env)
    assert out.returncode == 0, out.stdout[-1000:] + out.stderr[-4000:]
    assert "AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
    lines = out.stdout.strip().split("\n")
    assert lines[-1] == "decoded %d documents, 0 disagreements" % len(docs)
    monkeypatch.setenv("BLANCE_WIRE_IN_TILE", str(tile))
    monkeypatch.setenv("BLANCE_WIRE_IN_STAGE", str(stage))
    pl = hip.Planner(lib_path=build_emu())
    try:
        wdict = W.make_dict(pl)
        for i, doc in enumerate(docs):
            got = pl.decode_wire(wdict, doc, count_only=True)
            assert lines[i].split() == [str(i), str(got["refusal"]), str(got["refusal_at"]), str(got["n_node_refs"])], (i, lines[i], got)
    finally:
        pl.close()
