"""Documents, references and checks of the device decoder's tests (blance_wire_decode_device, blance_amd/csrc/k_wire_decode.h):
shared by tests/test_wire_decode_emulated.py, tests/test_wire_decode_gpu.py, the two test_wire_decode_kernels_* modules and
the stand-alone sanitizer program (tests/simt/wire_decode_asan_main.cpp reads the file write_program_input makes).

What a decode is compared with is never the code under test: the host decoder (blance_amd.wire.decode, pinned by
tests/golden/wire_cases.json) carried over to the dictionary's ids, and json.loads carried over in plain Python."""
import ctypes as C
import json
import random

import numpy as np

from blance_amd import abi, planner, wire

FILL = 0xAB


# ---- the two references ----------------------------------------------------------------------------------------------------

def lists_of_python_map(pmap, parts, nodes, states):
    """json.loads's dict in the layout of prev_* / assign_*: plain loops."""
    P, M = len(parts), len(states)
    pid, nid, sid = ({x: i for i, x in enumerate(names)} for names in (parts, nodes, states))
    part_kind, kind, lists = np.zeros(P, np.uint8), np.zeros(P * M, np.uint8), {}
    for key, part in pmap.items():
        p = pid[key]
        assert part["name"] == key
        nbs = part.get("nodesByState")
        part_kind[p] = abi.LIST_NIL if nbs is None else abi.LIST_SET
        for s, lst in (nbs or {}).items():
            idx = p * M + sid[s]
            kind[idx] = abi.LIST_NIL if lst is None else abi.LIST_SET
            lists[idx] = [nid[x] for x in (lst or [])]
    off, flat = np.zeros(P * M + 1, np.int32), []
    for idx in range(P * M):
        flat += lists.get(idx, [])
        off[idx + 1] = len(flat)
    return {"part_kind": part_kind, "off": off, "kind": kind, "nodes": np.asarray(flat, np.int32)}


def same_lists(got, want, tag=""):
    for k in ("part_kind", "off", "kind", "nodes"):
        assert np.array_equal(got[k], want[k]), (tag, k, got[k][:40], want[k][:40])


def check_accepted(pl, wdict, doc, tag=""):
    """The device accepts `doc` and its lists are the host decoder's and json.loads's."""
    got = pl.decode_wire(wdict, doc)
    assert got["refusal"] == 0 and got["refusal_at"] == -1, (tag, abi.WIRE_REFUSALS[got["refusal"]], got["refusal_at"], doc[:200])
    wm = wire.decode(doc)
    try:
        host = planner.lists_of_wire_map(wm, wdict)
    finally:
        wm.close()
    assert not host["names_differ"].any(), tag
    same_lists(got, host, (tag, "host decoder"))
    same_lists(got, lists_of_python_map(json.loads(doc), wdict.part_names, wdict.node_names, wdict.state_names), (tag, "json.loads"))
    assert got["n_node_refs"] == len(got["nodes"]) == host["n_node_refs"] and got["n_parts_seen"] == host["n_parts_seen"], tag
    return got


def raw_decode(pl, wdict, doc, capacity, length=None):
    """blance_wire_decode_device with arrays of this function's, filled with FILL: (status, abi.WireLists, arrays)."""
    P, M = wdict.n_parts, wdict.n_states
    arrays = [np.full(max(P, 1), FILL, np.uint8), np.full(P * M + 1, 0x2B2B2B2B, np.int32),
              np.full(max(P * M, 1), FILL, np.uint8), np.full(max(capacity, 1), 0x2B2B2B2B, np.int32)]
    wl = abi.WireLists()
    wl.part_kind, wl.off, wl.kind, wl.nodes = [a.ctypes.data for a in arrays]
    wl.capacity = capacity
    buf = C.create_string_buffer(doc, len(doc) + 1)
    st = pl.lib.blance_wire_decode_device(pl._h, wdict._h, C.cast(buf, C.c_void_p), len(doc) if length is None else length, C.byref(wl))
    return st, wl, arrays


def untouched(arrays):
    return (arrays[0] == FILL).all() and (arrays[1] == 0x2B2B2B2B).all() and (arrays[2] == FILL).all() and (arrays[3] == 0x2B2B2B2B).all()


def check_refused(pl, wdict, doc, reason, lo=0, hi=None, tag=""):
    """The device refuses `doc` with `reason` at an offset in [lo, hi), and writes none of the caller's arrays."""
    st, wl, arrays = raw_decode(pl, wdict, doc, 64)
    hi = len(doc) + 1 if hi is None else hi
    assert st == abi.ERR_UNSUPPORTED, (tag, st, doc[:200])
    assert abi.WIRE_REFUSALS[wl.refusal] == reason and lo <= wl.refusal_at < hi, \
        (tag, abi.WIRE_REFUSALS[wl.refusal], wl.refusal_at, reason, lo, hi, doc[:300])
    assert untouched(arrays), tag
    assert pl.lib.blance_last_error()


# ---- stage 1 in twenty lines -----------------------------------------------------------------------------------------------

def split_reference(doc, tile):
    """The definition k_wd_tail .. k_wd_walk are compared with: one sequential walk over the bytes.  Returns (bit per byte:
    an unescaped quote, unescaped quotes per tile, change of bracket depth outside strings per tile, offsets of the opening
    quotes at depth 1)."""
    n_tiles = (len(doc) + tile - 1) // tile
    bits, quotes, depth, starts = [0] * len(doc), [0] * n_tiles, [0] * n_tiles, []
    esc = in_str = False
    d = 0
    for i, ch in enumerate(doc):
        t = i // tile
        if esc:
            esc = False
        elif ch == 0x5C:
            esc = True
        elif ch == 0x22:
            bits[i] = 1
            quotes[t] += 1
            if not in_str and d == 1:
                starts.append(i)
            in_str = not in_str
            continue
        if not in_str and ch in b"{[":
            d += 1
            depth[t] += 1
        elif not in_str and ch in b"}]":
            d -= 1
            depth[t] -= 1
    return bits, quotes, depth, starts


# ---- writing documents -----------------------------------------------------------------------------------------------------

def jstr(s):
    return json.dumps(s, ensure_ascii=False).encode("utf-8")


def record(name, nbs="missing", key=None):
    """Compact bytes of one record; nbs: "missing", None (null) or {state: None | [nodes]}."""
    out = jstr(name if key is None else key) + b':{"name":' + jstr(name)
    if nbs != "missing":
        out += b',"nodesByState":'
        if nbs is None:
            out += b"null"
        else:
            out += b"{" + b",".join(jstr(s) + b":" + (b"null" if l is None else b"[" + b",".join(jstr(x) for x in l) + b"]")
                                    for s, l in nbs.items()) + b"}"
    return out + b"}"


def document(records):
    return b"{" + b",".join(records) + b"}"


PARTS = ["p%d" % i for i in range(4099)]
# names that look like JSON, escapes of every kind, and runs of backslashes of every parity (a name of k backslashes is written
# as 2k, a quote behind them makes the run odd)
SPECIAL = ['a"b', "c\\d", "{x", "[y", ",z", ":w", "/s", "A", "t\tb", "ü", "日本", "\U0001F600x", "",
           '"', "\\", '\\"', "\\\\", '\\\\"', "\\" * 70, "\\" * 70 + '"', "\\" * 300, "\\" * 300 + '"']
NODES = ["a", "b", "c", "n,1", 'q"', "L" * 150, "W" * 700] + ["n%04d" % i for i in range(40)] + ["n1"]
STATES = ["primary", "replica", "s\\t"]


def make_dict(pl):
    return pl.wire_dict(PARTS + SPECIAL, NODES, STATES)


def lead(doc_records, first_quote_at):
    """A document whose first record's opening quote lies at byte first_quote_at (whitespace behind the brace)."""
    assert first_quote_at >= 1
    return b"{" + b" " * (first_quote_at - 1) + b",".join(doc_records) + b"}"


def seam_documents(T, stage=32 * 1024):
    """[(tag, document)]: every one inside the subset.  T: the tile of the record split."""
    out = []
    base = document([record("p0", {"primary": ["a"]})])
    assert len(base) < T - 1
    for n in (T - 1, T, T + 1, 2 * T + 1):
        out.append(("length %d" % n, base[:-1] + b" " * (n - len(base)) + b"}"))
        out.append(("length %d, space behind" % n, base + b"\n" * (n - len(base))))
    # an escaped quote whose backslash is a tile's last byte: the key "a\"b", backslash at T - 1 and at 2T - 1
    for at in (T - 1, 2 * T - 1):
        out.append(("backslash at %d" % at, lead([record('a"b', None), record("p1", {"replica": ["b"]})], at - 2)))
    # backslash runs of 1 .. 5 with the seam at every place inside and beside them
    for name in ('"', "\\", '\\"', "\\\\", '\\\\"'):
        run = len(jstr(name)) - 2 - (1 if name.endswith('"') else 0)
        for cut in range(run + 1):
            out.append(("run %d cut %d" % (run, cut), lead([record(name, {"primary": []}), record("p2")], T - 1 - cut)))
    # runs longer than a tile, even and odd
    for name in ("\\" * 70, "\\" * 70 + '"', "\\" * 300, "\\" * 300 + '"'):
        if 2 * len(name) > T:
            for first in (1, 7, T - 3):
                out.append(("long run %d at %d" % (len(name), first), lead([record(name, None), record("p3", {"s\\t": None})], first)))
    # a record start on a tile's first and last byte
    r0 = record("p0", {"primary": ["a", "b"]})
    for at in (T, T - 1, 2 * T, 2 * T - 1):
        pad = at - (1 + len(r0) + 1)
        if pad >= 0:
            out.append(("record start at %d" % at, b"{" + r0 + b"," + b" " * pad + record("p1") + b"}"))
    # a string longer than two tiles
    long_node = "L" * 150 if T <= 64 else "W" * 700
    assert len(long_node) > 2 * T
    out.append(("long string", document([record("p0", {"primary": [long_node, "a"]}), record("p1", {"replica": [long_node]})])))
    # 0, 1, 255, 256, 257 and 4,099 records; every partition, every third
    for n in (0, 1, 255, 256, 257, 4099):
        out.append(("%d records" % n, document([record(PARTS[i], {"primary": [NODES[7 + i % 40]], "replica": [NODES[7 + (i + 1) % 40], "a"][:i % 3]})
                                                for i in range(n)])))
    out.append(("every third", document([record(PARTS[i], {"replica": ["c"]}) for i in range(0, 4099, 3)])))
    names = PARTS + SPECIAL                                 # every name of the dictionary, the 22 that look like JSON included
    out.append(("every name", document([record(names[i], {"s\\t": [NODES[i % 7]]}) for i in range(len(names))])))
    # one record longer than the LDS stage (the workgroup reads global memory), with short ones around it
    n_refs = stage // 8 + 64
    big = record("p1", {"primary": [NODES[7 + i % 40] for i in range(n_refs)]})
    assert len(big) > stage
    out.append(("record longer than the stage", document([record("p0", {"primary": ["a"]}), big, record("p2", {"replica": ["b"]})])))
    return out


MAX_RECORD = 1 << 20                                        # k_wire_decode.h: kWdMaxRecord


def size_limit_documents():
    """([(tag, document)] just inside the limit of size, [(tag, document, lo, hi)] refused as record_too_long at an offset in
    [lo, hi)).  The limit is part of the subset (include/blance_hip.h): a record, the bytes in front of the first record and
    the whitespace behind the closing brace are each shorter than 1 MiB."""
    r0, r1 = record("p0", {"primary": ["a"]}), record("p1", {"replica": ["b", "c"]})
    two = document([r0, r1])
    last = two.index(b'"p1"')
    inside = [("first record at 1 MiB", lead([r0, r1], MAX_RECORD)),
              ("1 MiB behind the brace", two + b"\n" * MAX_RECORD)]
    # a run of backslashes of more than 1 MiB in a key: the record split stops walking back over it, the record is too long
    run = jstr("\\" * (MAX_RECORD // 2 + 64)) + b':{"name":"x"}'
    outside = [("nothing but space", b"{" + b" " * (MAX_RECORD + 5) + b"}", 0, 1),
               ("space in front of the document", b" " * MAX_RECORD + two, 0, 1),
               ("first record behind 1 MiB", lead([r0, r1], MAX_RECORD + 1), 0, 1),
               ("more than 1 MiB behind the brace", two + b"\n" * (MAX_RECORD + 1), last, last + 1),
               ("a backslash run of more than 1 MiB", document([r0, run, r1]), 1 + len(r0) + 1, 1 + len(r0) + 2)]
    return inside, outside


# ---- inside the subset by construction ---------------------------------------------------------------------------------------

def _esc(rng, s):
    """One permitted way to write the string s."""
    out = [b'"']
    for ch in s:
        cp = ord(ch)
        short = {'"': b'\\"', "\\": b"\\\\", "/": b"\\/", "\b": b"\\b", "\f": b"\\f", "\n": b"\\n", "\r": b"\\r", "\t": b"\\t"}
        how = rng.randrange(4)
        if cp >= 0x10000 and how == 0:
            v = cp - 0x10000
            out.append(b"\\u%04x\\u%04X" % (0xD800 + (v >> 10), 0xDC00 + (v & 0x3FF)))
        elif cp < 0x10000 and (how == 0 or (cp < 0x20 and ch not in short)):
            out.append((b"\\u%04x" if rng.randrange(2) else b"\\u%04X") % cp)
        elif ch in short and (how == 1 or ch in '"\\' or cp < 0x20):
            out.append(short[ch])
        else:
            out.append(ch.encode("utf-8"))
    return b"".join(out) + b'"'


def _ws(rng):
    return rng.choice([b"", b"", b" ", b"\n", b"\t \r", b"  \n  "])


def render(rng, pmap):
    """pmap ({key: {"name", "nodesByState"}}) written a random permitted way: whitespace, order, escapes, null or missing
    nodesByState."""
    w = lambda: _ws(rng)                                                                    # noqa: E731
    recs = []
    keys = list(pmap)
    rng.shuffle(keys)
    for key in keys:
        nbs = pmap[key]["nodesByState"]
        fields = [_esc(rng, "name") + w() + b":" + w() + _esc(rng, key)]
        if nbs is not None or rng.randrange(2):
            if nbs is None:
                val = b"null"
            else:
                states = list(nbs)
                rng.shuffle(states)
                val = b"{" + w() + (w() + b"," + w()).join(
                    _esc(rng, s) + w() + b":" + w() + (b"null" if nbs[s] is None else
                                                       b"[" + w() + (w() + b"," + w()).join(_esc(rng, x) for x in nbs[s]) + w() + b"]")
                    for s in states) + w() + b"}"
            fields.append(_esc(rng, "nodesByState") + w() + b":" + w() + val)
        rng.shuffle(fields)
        recs.append(_esc(rng, key) + w() + b":" + w() + b"{" + w() + (w() + b"," + w()).join(fields) + w() + b"}")
    return w() + b"{" + w() + (w() + b"," + w()).join(recs) + w() + b"}" + w()


def random_map(rng, n_parts):
    names = rng.sample(SPECIAL[:18] + PARTS[:40], n_parts)
    pmap = {}
    for name in names:
        nbs = None
        if rng.randrange(5):
            nbs = {}
            for s in rng.sample(STATES, rng.randrange(len(STATES) + 1)):
                k = rng.randrange(5)
                nbs[s] = None if k == 0 else [rng.choice(NODES[:5] + NODES[7:12]) for _ in range(0 if k == 1 else rng.randrange(1, 5))]
        pmap[name] = {"name": name, "nodesByState": nbs}
    return pmap


def subset_documents(n=60, seed=1):
    rng = random.Random(seed)
    docs = [("{}", b"{}"), ("{} in whitespace", b" \n{\t}\r ")]
    for i in range(n):
        docs.append(("subset %d" % i, render(rng, random_map(rng, rng.choice([1, 2, 5, 17, 30])))))
    docs.append(("every special name", render(rng, {s: {"name": s, "nodesByState": {"primary": ["a"]}} for s in SPECIAL})))
    return docs


# ---- outside by construction -----------------------------------------------------------------------------------------------

def bad_records(name):
    """{reason: the bytes of a record for partition `name` that must be refused with it}."""
    k = jstr(name)
    return {
        "grammar": k + b':{"name":' + k + b' "nodesByState":{}}',
        "type": k + b':{"name":' + k + b',"nodesByState":{"primary":"a"}}',
        "unknown_partition": record("nobody", {"primary": ["a"]}),
        "unknown_state": record(name, {"primary": ["a"], "tertiary": []}),
        "unknown_node": record(name, {"primary": ["a", "stranger"]}),
        "repeated_state": k + b':{"name":' + k + b',"nodesByState":{"primary":["a"],"replica":null,"primary":[]}}',
        "repeated_field": k + b':{"name":' + k + b',"nodesByState":{},"name":' + k + b"}",
        "unknown_field": k + b':{"Name":' + k + b',"nodesByState":{}}',
        "null_partition": k + b":null",
        "name_missing": k + b':{"nodesByState":{"primary":["a"]}}',
        "name_differs": k + b':{"name":"p4000","nodesByState":{"primary":["a"]}}',
        "null_element": record(name, {"primary": ["a"]}).replace(b'["a"]', b'["a",null]'),
        "invalid_utf8": record(name, {"primary": ["a"]}).replace(b'["a"]', b'["a\xff"]'),
        "unpaired_surrogate": record(name, {"primary": ["a"]}).replace(b'["a"]', b'["\\ud83dx"]'),
        "control_character": record(name, {"primary": ["a"]}).replace(b'["a"]', b'["a\x01"]'),
    }


def refusal_documents(T):
    """[(tag, document, reason, lo, hi)]: each reason in the first record, in one that straddles a tile seam and in the last."""
    good = [record(PARTS[i], {"primary": [NODES[7 + i]], "replica": ["a", "b"]}) for i in range(6)]
    out = []
    for reason in bad_records("x"):
        for where in ("first", "seam", "last"):
            at = {"first": 0, "seam": 3, "last": 5}[where]
            bad = bad_records(PARTS[at])[reason]
            recs = list(good)
            recs[at] = bad
            pad = b""
            if where == "seam":                              # the seam at the bad record's eighth byte
                before = 1 + sum(len(r) + 1 for r in recs[:at])
                pad = b" " * ((-(before + 8)) % T)
            doc = b"{" + b",".join(recs[:at]) + (b"," if at else b"") + pad + b",".join(recs[at:]) + b"}"
            lo = doc.index(bad)
            if where == "seam":
                assert lo // T != (lo + len(bad) - 1) // T
            out.append(("%s in the %s record" % (reason, where), doc, reason, lo, lo + len(bad)))
    # a repeated partition: the second of the two is the one reported
    for where, (i, j) in (("first", (0, 1)), ("seam", (1, 3)), ("last", (0, 5))):
        recs = list(good)
        recs[j] = record(PARTS[i], None)
        doc = document(recs)
        lo = len(document(recs[:j]))                         # (`{...}` is as long as `{...,`)
        out.append(("repeated_partition, %s" % where, doc, "repeated_partition", lo, lo + len(recs[j])))
    out.append(("three records with one key", document([good[0], good[1], record("p0"), record("p0", None)]), "repeated_partition",
                len(document(good[:2])), len(document(good[:2])) + len(record("p0"))))
    out += [("null", b"null", "null_document", 0, 1), ("null in whitespace", b" \n null\t", "null_document", 3, 4),
            ("nothing", b"", "grammar", 0, 1), ("whitespace", b"  ", "grammar", 0, 3), ("an array", b"[]", "type", 0, 1),
            ("a number", b"12", "type", 0, 1), ("an open brace", b"{", "grammar", 1, 2), ("null and more", b"null {}", "grammar", 0, 8)]
    return out


def golden_vector_documents(cases):
    """The vectors of tests/golden/wire_cases.json the device must refuse, with the reason: the eight errors, the null document,
    the repeated state key, invalid UTF-8 -- against the dictionary golden_dict() makes."""
    # (the reason is that of the smallest offset: two vectors carry the name "x" under the key "p" in front of their error, and
    # the trailing comma stands behind a null partition)
    want = {"wrong-type-name": "type", "wrong-type-list": "name_differs", "wrong-type-document": "type", "trailing-data": "grammar",
            "truncated": "name_differs", "control-in-string": "control_character", "bad-escape": "grammar",
            "trailing-comma": "null_partition"}
    out = [(c["id"], bytes.fromhex(c["hex"]), want[c["id"]]) for c in cases["errors"]]
    assert len(out) == 8
    by_id = {c["id"]: bytes.fromhex(c["hex"]) for c in cases["unmarshal"] + cases["unmarshal_raw"]}
    out += [("null-document", by_id["null-document"], "null_document"), ("array-resets", by_id["array-resets"], "repeated_state"),
            ("invalid-utf8-in", by_id["invalid-utf8-in"], "invalid_utf8"),
            ("case-insensitive-fields", by_id["case-insensitive-fields"], "unknown_field"),
            ("unknown-fields-ignored", by_id["unknown-fields-ignored"], "unknown_field"),
            ("missing-fields-zero", by_id["missing-fields-zero"], "name_missing"), ("null-members", by_id["null-members"], "null_partition"),
            ("repeated-map-key", by_id["repeated-map-key"], "name_differs")]
    return out


def golden_dict(pl):
    return pl.wire_dict(["p", "q", "k", "kA"], ["a", "b", "c"], ["s", "t"])


# ---- mutants ---------------------------------------------------------------------------------------------------------------

def mutant_base():
    return b' {"p0":{"name":"p0","nodesByState":{"primary":["a"],"replica":["b","n1"]}},\n "a\\"b" : {"nodesByState":null,"name":"a\\u0022b"},' \
           b'"\xc3\xbc":{"name":"\\u00fc","nodesByState":{"replica":[],"primary":null}},"\\\\":{"name":"\\\\"},"p1":{"name":"p1","nodesByState":{}}} '


def mutants(seed=7, n_sub=300, n_del=80):
    """[(tag, document)]: single byte substitutions and deletions at fixed seeds, every record duplicated, every truncation of
    one small document."""
    rng = random.Random(seed)
    base = mutant_base()
    alphabet = b'"\\{}[],: anul0p1\x00\x1f\x7f\x80\xc3\xbc\xff/utbf-9eE.'
    out = [("base", base)]
    for i in range(n_sub):
        at = rng.randrange(len(base))
        out.append(("substitute %d at %d" % (i, at), base[:at] + bytes([rng.choice(alphabet)]) + base[at + 1:]))
    for i in range(n_del):
        at = rng.randrange(len(base))
        out.append(("delete %d" % at, base[:at] + base[at + 1:]))
    recs = [record("p0", {"primary": ["a"]}), record('a"b', None), record("p1", {"replica": ["b", "b"]})]
    for i in range(3):
        for j in range(4):
            dup = list(recs)
            dup.insert(j, recs[i])
            out.append(("record %d again at %d" % (i, j), document(dup)))
    small = document(recs[:2]) + b" "
    out += [("cut at %d" % n, small[:n]) for n in range(len(small) + 1)]
    return out


def check_mutant(pl, wdict, doc, tag):
    """Device OK => the host decodes it and the results are equal; a host error => the device refuses.  Returns (device
    accepted, host accepted)."""
    got = pl.decode_wire(wdict, doc)
    try:
        wm = wire.decode(doc)
    except wire.WireError:
        assert got["refusal"] != 0, (tag, "the host decoder rejects what the device accepts", doc)
        return False, False
    try:
        if got["refusal"] == 0:
            host = planner.lists_of_wire_map(wm, wdict)                   # (raises for a name outside the dictionary)
            assert not host["names_differ"].any(), (tag, doc)
            same_lists(got, host, (tag, doc))
        else:
            assert got["nodes"] is None and 0 <= got["refusal_at"] <= len(doc), (tag, got)
    finally:
        wm.close()
    return got["refusal"] == 0, True


# ---- the stand-alone sanitizer program's input --------------------------------------------------------------------------------

def write_program_input(path, parts, nodes, states, docs, tile, stage):
    """One line per item, strings as hex: T <tile> <stage>; P / N / S <name>; D <document>."""
    with open(path, "w") as f:
        f.write("T %d %d\n" % (tile, stage))
        for tag, names in (("P", parts), ("N", nodes), ("S", states)):
            for x in names:
                f.write("%s %s\n" % (tag, x.encode("utf-8").hex()))
        for d in docs:
            f.write("D %s\n" % d.hex())


# ---- stage 1 alone (tests/kernels/wire_decode_cases.inc) ----------------------------------------------------------------------

class SplitCases:
    """blance_case_wd_split of a case library: the emulator's or the device's."""

    def __init__(self, lib_path):
        self.lib = C.CDLL(lib_path)
        self.lib.blance_case_wd_split.restype = C.c_int
        self.lib.blance_case_wd_split.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_int]

    def split(self, doc, tile, rec_cap=None):
        n_tiles = (len(doc) + tile - 1) // tile
        qbits = np.full(n_tiles * tile // 32 + 1, 0x5A5A5A5A, np.uint32)
        quotes, depth = np.full(n_tiles + 1, -7, np.int32), np.full(n_tiles + 1, -7, np.int32)
        cap = len(doc) if rec_cap is None else rec_cap
        rec = np.full(cap + 1, -7, np.int32)
        buf = C.create_string_buffer(doc, len(doc) + 1)
        n = self.lib.blance_case_wd_split(C.cast(buf, C.c_void_p), len(doc), tile, qbits.ctypes.data, quotes.ctypes.data,
                                          depth.ctypes.data, rec.ctypes.data, cap)
        assert qbits[-1] == 0x5A5A5A5A and quotes[-1] == -7 and depth[-1] == -7 and rec[-1] == -7     # nothing behind the arrays
        return n, qbits[:-1], quotes[:-1], depth[:-1], rec[:-1]


def check_split(sc, doc, tile, tag=""):
    """The kernels' unescaped-quote bits, per-tile quote counts and depth changes and the record offsets are the definition's."""
    n, qbits, quotes, depth, rec = sc.split(doc, tile)
    bits, want_quotes, want_depth, starts = split_reference(doc, tile)
    assert n == len(starts), (tag, n, len(starts))
    got_bits = np.unpackbits(qbits.view(np.uint8), bitorder="little")
    assert got_bits[:len(doc)].tolist() == bits and not got_bits[len(doc):].any(), tag
    assert quotes.tolist() == want_quotes and depth.tolist() == want_depth, tag
    assert rec[:n].tolist() == starts, tag
    return n


def random_split_documents(n=200, seed=3):
    """Byte strings over the alphabet of the split: quotes, backslashes, brackets, separators, a letter."""
    rng = random.Random(seed)
    alphabet = b'"\\{}[],: a'
    return [bytes(rng.choice(alphabet) for _ in range(rng.choice([0, 1, 63, 64, 65, 127, 128, 129, 200, 333, 1000]))) for _ in range(n)]


def run_split_cases(sc):
    n = 0
    for tile in (64, 256):
        for tag, doc in seam_documents(tile):
            n += check_split(sc, doc, tile, (tile, tag)) > 0
    for i, doc in enumerate(random_split_documents()):
        for tile in (64, 128):
            check_split(sc, doc, tile, ("random", i, tile))
    # a run of backslashes over many tiles in front of a quote, odd and even; a document of backslashes only
    for k in (64, 65, 640, 641, 4097):
        check_split(sc, b'{"' + b"\\" * k + b'"":1}', 64, ("backslashes", k))
    check_split(sc, b"\\" * 300, 64, "backslashes only")
    return n


def check_split_refusals(sc):
    """The entry refuses a tile that is no multiple of 64 or outside [64, 4096]; too small a record array is not written."""
    doc = document([record("p0"), record("p1"), record("p2")])
    for tile in (0, 32, 96, 8192):
        qb = np.zeros(64, np.uint32)
        assert sc.lib.blance_case_wd_split(doc, len(doc), tile, qb.ctypes.data, qb.ctypes.data, qb.ctypes.data, qb.ctypes.data, 8) == -100
    n, _, _, _, rec = sc.split(doc, 64, rec_cap=2)
    assert n == 3 and (rec == -7).all()
