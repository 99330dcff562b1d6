"""The host tables of the wire paths alone (blance_amd/csrc/host/wire_names.hpp): the partitions' document order, the escaped
names, the blob checks, the decoder's hash tables, the names block and the dictionary block of a batch, and the capacities of a
batch's documents -- through a stand-alone program (tests/simt/wire_names_main.cpp, plain g++, no HIP), built twice -- plain, and
under AddressSanitizer and UBSan -- and compared with references written here from the definitions: Go's byte-wise order of
map keys (sorted() over bytes), json.Marshal's escaping (oracle/wire_ref.py: go_string), FNV-1a with the length folded in and
the device's probe (tests/batch_decode_cases.py: fnv; k_wire_decode.h: hash, mask, linear probe, every byte compared), and the
two block layouts as the kernel-alone tests spell them (tests/batch_wire_cases.py: names_block; tests/batch_decode_cases.py:
dict_block) -- so the host's builders and the tests' builders are compared word for word.

k_wire_*, k_wd_parse, k_batch_wire_* and k_batch_decode follow these ranks and offsets blindly: a wrong rank or an unaligned
table corrupts a document silently.  The cases are each the smallest input where one decision can go wrong.

Left out: the encoder's refusal of escaped names of 2^31 bytes or more (wire_escape would have to write them).  The same
refusal of a block of 2^31 words is tested through wire_block_layout, which takes the sizes; the dictionaries' refusal of names
of 2^31 bytes is tested with an offset that says so and one byte behind it (nothing is read before the refusal).

Mutants of wire_names.hpp applied by hand (the plain build), and what failed then:
  wire_block_layout without its rounding `(words[i] + 3) & ~(size_t)3`  -> test_block_layout, test_names_block and
                                                                          test_dict_block in every world
  wire_cmp's length tie-break inverted (`xn < yn ? 1 : ...`)            -> test_sort[a_and_a_nul], [differ_behind_byte_8],
                                                                          test_names_block[escapes] (not [prefix_of_the_other]
                                                                          or [empty_name]: their 8-byte prefixes differ)
  wd_build_table's capacity loop `cap <= 2 * n` for `cap < 2 * n`       -> test_table_capacity, test_table_probe_wraps,
                                                                          test_dict_block[plain], [P_0], [M_0], [NX_0]
  the probe without its wrap (`at = at + 1`)                            -> test_table_probe_wraps, test_dict_block[escapes]
  the signed `char` in the 8-byte prefix (no `(unsigned char)` cast)    -> test_sort[high_byte_in_the_prefix],
                                                                          test_names_block[escapes] (not
                                                                          [high_bytes_after_ascii]: the sign bits of a
                                                                          name's first byte are shifted out of the word)
(the other tests passed under each mutant)
"""
import fcntl
import os
import subprocess

import numpy as np
import pytest

from batch_decode_cases import dict_block, fnv
from batch_wire_cases import names_block
from oracle.wire_ref import go_string

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "simt", "wire_names_main.cpp")
CSRC = os.path.join(HERE, "..", "blance_amd", "csrc")
HDRS = [os.path.join(CSRC, "host", "wire_names.hpp"), os.path.join(CSRC, "host", "json_escape.hpp"), os.path.join(CSRC, "blance_kernels.h"),
        os.path.join(HERE, "..", "include", "blance_hip.h"), os.path.join(HERE, "..", "include", "blance_batch.h")]
EXE = os.path.join(HERE, "simt", "_build", "wire_names")
SANITIZE = ["-fsanitize=address,undefined", "-static-libasan", "-static-libubsan"]     # the runtimes inside the program
INT_MAX = 2 ** 31 - 1
NAMES_HDR, DICT_HDR = 8, 16                                                            # kBatchNamesHdr, kBatchDictHdr
# WireErr
NONE, NEGATIVE, TOO_MANY_LISTS, NULL_OFFSETS, FIRST_OFFSET, NOT_MONOTONE, NULL_BYTES, DUP_PART, DUP_NODE, DUP_STATE, TOO_LONG = range(11)


# ---- the two builds ---------------------------------------------------------------------------------------------------------

def build_program(sanitized):
    """The program, or (None, why) when a sanitized program does not link or start here."""
    exe = EXE + ("_asan" if sanitized else "")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    with open(exe + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if os.path.exists(exe) and all(os.path.getmtime(d) <= os.path.getmtime(exe) for d in [SRC] + HDRS):
            return exe, ""
        flags = []
        if sanitized:
            probe = subprocess.run(["g++"] + SANITIZE + ["-x", "c++", "-", "-o", exe + ".probe"], input="int main(){return 0;}\n",
                                   capture_output=True, text=True)
            if probe.returncode != 0:
                return None, probe.stderr[-400:]
            started = subprocess.run([exe + ".probe"], capture_output=True, text=True)
            os.remove(exe + ".probe")
            if started.returncode != 0:
                return None, "the program does not start: " + started.stderr[-400:]
            flags = ["-g1"] + SANITIZE + ["-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
        tmp = "%s.%d.tmp" % (exe, os.getpid())
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", tmp, SRC])
        os.replace(tmp, exe)
    return exe, ""


def run(commands, tmp_path, sanitized):
    """The program's answers: per command a dict of its lines."""
    exe, why = build_program(sanitized)
    if exe is None:
        pytest.skip("-fsanitize=address does not link or start on this machine: " + why)
    cases, answers = tmp_path / "commands.txt", tmp_path / "answers.txt"
    cases.write_text("\n".join(commands) + "\n")
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=1"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    got = subprocess.run([exe, str(cases), str(answers)], capture_output=True, text=True, timeout=300, env=env)
    assert got.returncode == 0, got.stderr[-4000:]
    assert "AddressSanitizer" not in got.stderr and "runtime error" not in got.stderr, got.stderr[-4000:]
    out = []
    lines = answers.read_text().strip().split("\n")
    assert lines[-1] == "ran %d commands" % len(commands)
    for ln in lines[:-1]:
        name, *vals = ln.split()
        if name == "answer":
            out.append({})
        else:
            out[-1][name] = [int(v) for v in vals]
    assert len(out) == len(commands)
    return out


BUILDS = [pytest.param(False, id="plain"), pytest.param(True, id="sanitized")]


# ---- blobs ------------------------------------------------------------------------------------------------------------------

def raw(names):
    return [x if isinstance(x, bytes) else x.encode("utf-8") for x in names]


def blob(names, off=True, data=True):
    """A blob's words.  off / data: True -- as the names say; None -- a null pointer; a list / bytes -- these instead."""
    names = raw(names)
    if off is True:
        off = [sum(len(x) for x in names[:i]) for i in range(len(names) + 1)]
    if data is True:
        data = b"".join(names)
    w = [0] if off is None else [1, len(off) - 1] + list(off)
    w += [0] if data is None else [1, len(data)] + list(data)
    return " ".join(str(int(x)) for x in w)


def names_cmd(cmd, parts, nodes, states, sizes=None, blobs=None):
    sizes = sizes or (len(parts), len(nodes), len(states))
    blobs = blobs or [blob(parts), blob(nodes), blob(states)]
    return "%s %d %d %d %s" % (cmd, *sizes, " ".join(blobs))


def words_of(data):
    data = data + b"\0" * (-len(data) % 4)
    return np.frombuffer(data, np.int32).tolist()


def r4(n):
    return (n + 3) & ~3


# ---- wire_sort --------------------------------------------------------------------------------------------------------------

SORTS = {   # name -> (names, two of them are equal)
    "sorted_strictly": (["a", "b", "c"], False),
    "sorted_with_an_equal_pair": (["a", "b", "b", "c"], True),
    "reversed": (["d", "c", "b", "a"], False),
    "unsorted_with_an_equal_pair": (["b", "a", "b"], True),
    "differ_behind_byte_8": (["12345678b", "12345678a", "12345678", "12345678ab"], False),
    "equal_behind_byte_8": (["12345678b", "12345678a", "12345678b"], True),
    "prefix_of_the_other": (["ab", "a", "abc"], False),
    "a_and_a_nul": ([b"a\0", b"a", b"a\0\0"], False),                  # one zero-padded prefix: the length decides
    "empty_name": (["b", "", "a"], False),
    "two_empty_names": (["", "a", ""], True),
    "high_bytes_after_ascii": ([b"\x80", b"z", b"\xff", b"A"], False),    # unsigned order
    "high_byte_in_the_prefix": ([b"b", b"a\x80", b"a", b"a\x7f"], False),    # ... of every byte of the 8-byte prefix
    "n_0": ([], False),
    "n_1": (["only"], False),
}


@pytest.fixture(scope="module")
def sort_answers(tmp_path_factory):
    got = {}

    def answers(sanitized):
        if sanitized not in got:
            got[sanitized] = dict(zip(SORTS, run(["sort " + blob(n) for n, _ in SORTS.values()], tmp_path_factory.mktemp("sort"), sanitized)))
        return got[sanitized]
    return answers


@pytest.mark.parametrize("sanitized", BUILDS)
@pytest.mark.parametrize("name", list(SORTS))
def test_sort(sort_answers, name, sanitized):
    """The ids in Go's order of map keys (bytes, unsigned, the shorter of a prefix pair first); a duplicate is reported."""
    names, dup = SORTS[name]
    names = raw(names)
    got = sort_answers(sanitized)[name]
    assert got["ok"] == [int(not dup)], name
    assert dup == (len(set(names)) < len(names))
    if not dup:
        assert got["order"] == sorted(range(len(names)), key=lambda i: names[i]), name


# ---- wire_escape ------------------------------------------------------------------------------------------------------------

SPECIAL = [b'q"q', b"b\\s", b"\x00\x01\x1f", b"\b\f\n\r\t", b"<", b">", b"&", " ".encode(), "x y".encode(), b"\xff", b"\xe2\x82",
           b"\xc0\x80", b"\xed\xa0\x80", "é漢\U0001F600".encode(), b"", b"plain/name 7"]


@pytest.mark.parametrize("sanitized", BUILDS)
def test_escape(tmp_path, sanitized):
    """Every class json_escape.hpp treats specially, in a given order, as they lie (a null order), and with the states' tail:
    the bytes are json.Marshal's, offset i + 1 is the byte count behind string i."""
    order = list(reversed(range(len(SPECIAL))))
    cases = [(SPECIAL, None, b""), (SPECIAL, order, b""), (SPECIAL[:5], [4, 0, 2, 1, 3], b":"), ([], None, b":"), ([b""], None, b":")]
    cmds = []
    for names, o, tail in cases:
        cmds.append("escape %s %s %d %s" % (blob(names), "0" if o is None else "1 " + " ".join(map(str, o)), len(tail),
                                          " ".join(str(x) for x in tail)))
    for (names, o, tail), got in zip(cases, run(cmds, tmp_path, sanitized)):
        want = [go_string(names[i]) + tail for i in (o if o is not None else range(len(names)))]
        assert got["ok"] == [1]
        assert bytes(got["bytes"]) == b"".join(want)
        assert got["off"] == [sum(len(x) for x in want[:i]) for i in range(len(want) + 1)]
    assert go_string(b"<") == b'"\\u003c"' and go_string(b"\xff") == b'"\\ufffd"' and go_string(b"\x1f") == b'"\\u001f"'


# ---- the blob checks --------------------------------------------------------------------------------------------------------

GOOD = (["p1", "p0"], ["n0", "n1", "n2"], ["s"])
BAD_BLOBS = {   # cause -> (off, data) of a blob of two names "ab", "c"
    NULL_OFFSETS: (None, True),
    FIRST_OFFSET: ([1, 2, 3], True),
    NOT_MONOTONE: ([0, 2, 1], True),
    NULL_BYTES: (True, None),
}


@pytest.mark.parametrize("sanitized", BUILDS)
def test_blob_checks(tmp_path, sanitized):
    """Each of the four causes for each of the three blobs, through the encoder's and through the dictionaries' builder (one
    copy of the checks: the same cause from both); the first bad blob is the one reported; off[n] == 0 with null bytes passes."""
    cmds, want = [], []
    for cause, (off, data) in BAD_BLOBS.items():
        bad = blob(["ab", "c"], off, data)
        cmds.append("check " + bad)
        want.append(cause)
        for k in range(3):
            blobs = [blob(x) for x in GOOD]
            blobs[k] = bad
            sizes = [len(x) for x in GOOD]
            sizes[k] = 2
            for cmd in ("names", "dict"):
                cmds.append(names_cmd(cmd, *GOOD, sizes=sizes, blobs=blobs))
                want.append(cause)
    # two bad blobs: the partitions' cause, then the nodes'
    two = [blob(["ab", "c"], *BAD_BLOBS[NOT_MONOTONE]), blob(["ab", "c"], *BAD_BLOBS[NULL_OFFSETS]), blob(GOOD[2])]
    for cmd in ("names", "dict"):
        cmds.append(names_cmd(cmd, *GOOD, sizes=(2, 2, 1), blobs=two))
        want.append(NOT_MONOTONE)
    # nothing to point at: two empty names, no names at all -- null bytes are fine
    empty = [blob(["", ""], True, None), blob([], True, None), blob([""], True, None)]
    cmds += ["check " + empty[0], "check " + empty[1]]
    want += [NONE, NONE]
    cmds.append(names_cmd("dict", [], [], [], sizes=(0, 0, 0), blobs=[empty[1]] * 3))
    want.append(NONE)
    cmds.append(names_cmd("names", [], [], [], sizes=(0, 0, 0), blobs=[empty[1]] * 3))
    want.append(NONE)
    got = run(cmds, tmp_path, sanitized)
    assert [g["err"][0] for g in got] == want


@pytest.mark.parametrize("sanitized", BUILDS)
def test_sizes_refused(tmp_path, sanitized):
    """A negative count of each kind (before a blob is looked at: null blobs); P * M of 2^31 - 1 for the dictionaries alone;
    names of 2^31 bytes by their last offset."""
    null = [blob([], None, None)] * 3
    cmds, want = [], []
    for sizes in ((-1, 0, 0), (0, -1, 0), (0, 0, -1)):
        for cmd in ("names", "dict"):
            cmds.append(names_cmd(cmd, [], [], [], sizes=sizes, blobs=null))
            want.append(NEGATIVE)
    cmds.append(names_cmd("dict", [], [], [], sizes=(INT_MAX, 0, 1), blobs=null))
    want.append(TOO_MANY_LISTS)
    cmds.append(names_cmd("dict", [], [], [], sizes=(INT_MAX - 1, 0, 1), blobs=null))     # one below: on to the blobs
    want.append(NULL_OFFSETS)
    huge = blob(["x"], [0, 2 ** 31], b"x")
    for k in range(3):
        blobs = [blob(x) for x in GOOD]
        blobs[k] = huge
        sizes = [len(x) for x in GOOD]
        sizes[k] = 1
        cmds.append(names_cmd("dict", *GOOD, sizes=sizes, blobs=blobs))
        want.append(TOO_LONG)
    cmds.append("table %s %d" % (huge, DUP_NODE))
    want.append(TOO_LONG)
    got = run(cmds, tmp_path, sanitized)
    assert [g["err"][0] for g in got] == want


# ---- wd_build_table ---------------------------------------------------------------------------------------------------------

def probe(slots, mask, names, name):
    """k_wire_decode.h's lookup: the id of `name`, -1 when an empty slot ends the probe; and the slots visited."""
    h = fnv(name)
    at = h & mask
    seen = []
    for _ in range(mask + 2):
        seen.append(at)
        i = slots[2 * at]
        if i < 0:
            return -1, seen
        if slots[2 * at + 1] & 0xFFFFFFFF == h and names[i] == name:
            return i, seen
        at = (at + 1) & mask
    raise AssertionError("the probe does not end")


def check_table(got, names):
    names = raw(names)
    (mask,), slots = got["mask"], got["slots"]
    cap = mask + 1
    assert cap >= 2 and cap & mask == 0 and cap >= 2 * len(names) and (cap == 2 or cap < 4 * len(names)), (cap, len(names))
    assert len(slots) == 2 * cap
    assert sorted(i for i in slots[0::2] if i >= 0) == list(range(len(names)))
    for i, nm in enumerate(names):
        assert probe(slots, mask, names, nm)[0] == i, nm
    assert probe(slots, mask, names, b"not a name of the table")[0] == -1
    assert got["off32"] == [sum(len(x) for x in names[:i]) for i in range(len(names) + 1)]


def search(want, cap):
    """The first names "k<i>" whose home slots (hash & (cap - 1)) are want[0], want[1], ..."""
    out, i = [], 0
    for slot in want:
        while fnv(b"k%d" % i) & (cap - 1) != slot:
            i += 1
        out.append(b"k%d" % i)
        i += 1
    return out


@pytest.mark.parametrize("sanitized", BUILDS)
def test_table_capacity(tmp_path, sanitized):
    """n = 0 .. 5, 8 and 9: the capacity is the smallest power of two >= max(2, 2 n) (load <= 1/2), every id is found."""
    sizes = [0, 1, 2, 3, 4, 5, 8, 9]
    worlds = [["name%d" % i for i in range(n)] for n in sizes]
    got = run(["table %s %d" % (blob(w), DUP_NODE) for w in worlds], tmp_path, sanitized)
    assert [g["mask"][0] + 1 for g in got] == [2, 2, 4, 8, 8, 16, 16, 32]
    for w, g in zip(worlds, got):
        assert g["err"] == [NONE]
        check_table(g, w)


@pytest.mark.parametrize("sanitized", BUILDS)
def test_table_collision(tmp_path, sanitized):
    """Three names with one home slot (cap 8): they lie one behind the other from it, each found by the device's probe."""
    names = search([5, 5, 5], 8)
    (got,) = run(["table %s %d" % (blob(names), DUP_NODE)], tmp_path, sanitized)
    check_table(got, names)
    assert [got["slots"][2 * s] for s in (5, 6, 7)] == [0, 1, 2]
    assert probe(got["slots"], 7, names, names[2])[1] == [5, 6, 7]


@pytest.mark.parametrize("sanitized", BUILDS)
def test_table_probe_wraps(tmp_path, sanitized):
    """Two names whose home is the last slot (cap 4): the second lies in slot 0."""
    names = search([3, 3], 4)
    (got,) = run(["table %s %d" % (blob(names), DUP_NODE)], tmp_path, sanitized)
    check_table(got, names)
    assert got["slots"][2 * 3] == 0 and got["slots"][0] == 1
    assert probe(got["slots"], 3, names, names[1])[1] == [3, 0]


@pytest.mark.parametrize("sanitized", BUILDS)
def test_table_duplicates(tmp_path, sanitized):
    """A duplicate name of each kind with the cause its kind reports; the encoder refuses two partitions or two states with one
    name and ACCEPTS two nodes with one name (kept as it is: DESIGN.md 4.12)."""
    cmds, want = [], []
    for k, cause in enumerate((DUP_PART, DUP_NODE, DUP_STATE)):
        world = [list(x) for x in GOOD]
        world[k] = ["same", "other", "same"]
        cmds.append(names_cmd("dict", *world))
        want.append(cause)
        cmds.append(names_cmd("names", *world))
        want.append(NONE if cause == DUP_NODE else cause)
    # both a state and a partition twice: the encoder names the states, the dictionaries the partitions
    world = (["p", "p"], ["n"], ["s", "s"])
    cmds += [names_cmd("names", *world), names_cmd("dict", *world)]
    want += [DUP_STATE, DUP_PART]
    # equal hashes are not equal names: two names of one home slot are no duplicate
    cmds.append("table %s %d" % (blob(search([1, 1], 4)), DUP_STATE))
    want.append(NONE)
    cmds.append("table %s %d" % (blob(["x", "x"]), DUP_STATE))
    want.append(DUP_STATE)
    got = run(cmds, tmp_path, sanitized)
    assert [g["err"][0] for g in got] == want


# ---- the two blocks ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sanitized", BUILDS)
def test_block_layout(tmp_path, sanitized):
    """wire_block_layout: every table at a multiple of 4 words, one behind the other; 2^31 - 1 words pass, 2^31 do not."""
    cases = [(8, [0, 1, 4, 5, 3]), (16, [7]), (8, []), (8, [INT_MAX - 8 - 3]), (8, [INT_MAX - 8 - 2]), (16, [2 ** 31, 2 ** 31])]
    got = run(["layout %d %d %s" % (first, len(w), " ".join(map(str, w))) for first, w in cases], tmp_path, sanitized)
    for (first, w), g in zip(cases, got):
        at, total = [], first
        for n in w:
            at.append(total)
            total += r4(n)
        assert g["at"] == at and g["total"] == [total] and g["ok"] == [int(total <= INT_MAX)], (first, w)
        assert all(a % 4 == 0 for a in g["at"])
    assert [g["ok"][0] for g in got] == [1, 1, 1, 1, 0, 0]


def check_regions(regions, total):
    """(start, words): each 4-word aligned, inside [0, total), no two overlapping."""
    for a, n in regions:
        assert a % 4 == 0 and a >= 0 and a + n <= total, (regions, total)
    spans = sorted((a, a + n) for a, n in regions if n > 0)
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
        assert a1 <= b0, regions


def ref_names_block(parts, nodes, states):
    """names_block's layout (tests/batch_wire_cases.py) with json.Marshal's escaping in place of its plain quotes."""
    parts, nodes, states = raw(parts), raw(nodes), raw(states)
    order = sorted(range(len(parts)), key=lambda p: parts[p])
    sorder = sorted(range(len(states)), key=lambda m: states[m])
    quoted = [[go_string(parts[p]) for p in order], [go_string(n) for n in nodes], [go_string(states[m]) + b":" for m in sorder]]
    offs = [[sum(len(x) for x in q[:i]) for i in range(len(q) + 1)] for q in quoted]
    tables = [order, offs[0], offs[1], offs[2], sorder] + [words_of(b"".join(q)) for q in quoted]
    at, words = [], NAMES_HDR
    for t in tables:
        at.append(words)
        words += r4(len(t))
    block = [0] * words
    block[:NAMES_HDR] = at
    for a, t in zip(at, tables):
        block[a:a + len(t)] = t
    nbytes = [4 * len(order), 4 * len(offs[0]), 4 * len(offs[1]), 4 * len(offs[2]), 4 * len(sorder)] + [len(b"".join(q)) for q in quoted]
    sums = [len(b"".join(quoted[0])), len(b"".join(quoted[2])), max([0] + [len(x) for x in quoted[1]])]
    return block, at, nbytes, sums


WORLDS = {
    "escapes": ([b'p"2', b"p<1>", "p ".encode(), b"p\xff", b"p", b"p\0", b""], [b"n&0", b"n\\1", b"n\t2", b"", b"n3n3n3n3n3"], ["replica", "primary", "a\"b"]),
    "plain": (["p%d" % ((p * 7919) % 10007) for p in range(9)], ["n%d" % i for i in range(5)], ["replica", "primary"]),
    "P_0": ([], ["n0"], ["s"]),
    "M_0": (["p0", "p1"], ["n0"], []),
    "NX_0": (["p0"], [], ["s"]),
    "all_0": ([], [], []),
}


@pytest.mark.parametrize("sanitized", BUILDS)
@pytest.mark.parametrize("world", list(WORLDS))
def test_names_block(tmp_path, world, sanitized):
    """The names block word for word; every header word a multiple of 4, the tables disjoint and inside the block, the words no
    table owns zero; the three sums of blance_batch_wire_capacity; the single path's tables inside the block, by name."""
    parts, nodes, states = WORLDS[world]
    (got,) = run([names_cmd("names", parts, nodes, states)], tmp_path, sanitized)
    assert got["err"] == [NONE]
    block, at, nbytes, sums = ref_names_block(parts, nodes, states)
    assert got["block"] == block
    hdr = got["block"][:NAMES_HDR]
    assert all(a % 4 == 0 for a in hdr)
    check_regions([(0, NAMES_HDR)] + [(a, (n + 3) // 4) for a, n in zip(hdr, nbytes)], len(got["block"]))
    owned = np.zeros(len(block), bool)
    owned[:NAMES_HDR] = True
    for a, n in zip(hdr, nbytes):
        owned[a:a + (n + 3) // 4] = True
    assert not np.asarray(got["block"])[~owned].any()
    assert got["sums"] == sums
    # WireTables' fields: order, part_esc, part_off, node_esc, node_off, state_esc, state_off, state_id -> kNames*
    to_block = [0, 5, 1, 6, 2, 7, 3, 4]
    assert got["tables"] == [x for k in to_block for x in (4 * at[k], nbytes[k])]
    if world == "plain":                                                   # the kernel-alone tests' builder, as it is
        theirs, order = names_block(parts, nodes, states)
        assert got["block"] == theirs.tolist() and got["block"][at[0]:at[0] + len(parts)] == order


@pytest.mark.parametrize("sanitized", BUILDS)
@pytest.mark.parametrize("world", list(WORLDS))
def test_dict_block(tmp_path, world, sanitized):
    """The dictionary block word for word against the kernel-alone tests' builder (names that need escaping are raw bytes
    here: the decoder compares unescaped bytes); alignment, disjointness, zero padding; afterwards the tables' names lie in the
    block, and each table alone answers the device's probe."""
    parts, nodes, states = (raw(x) for x in WORLDS[world])
    (got,) = run([names_cmd("dict", parts, nodes, states)], tmp_path, sanitized)
    assert got["err"] == [NONE]

    class Raw(bytes):                                                      # (dict_block encodes str names: these are bytes already)
        def encode(self, *_):
            return bytes(self)
    want = dict_block(*[[Raw(x) for x in names] for names in (parts, nodes, states)])
    assert got["block"] == want
    b = got["block"]
    regions, owned = [(0, DICT_HDR)], np.zeros(len(b), bool)
    owned[:DICT_HDR] = True
    for k, names in enumerate((parts, nodes, states)):
        slots, mask, at_bytes, off = b[4 * k:4 * k + 4]
        assert b[12 + k] == len(names) and all(x % 4 == 0 for x in (slots, at_bytes, off))
        nb = sum(len(x) for x in names)
        for a, n in ((slots, 2 * (mask + 1)), (off, len(names) + 1), (at_bytes, (nb + 3) // 4)):
            regions.append((a, n))
            owned[a:a + n] = True
        assert got["bytes_at"][k] == 4 * at_bytes                          # the single path's names: in the block
        table = dict(mask=[mask], slots=b[slots:slots + 2 * (mask + 1)], off32=b[off:off + len(names) + 1])
        check_table(table, names)
        assert np.asarray(b[at_bytes:at_bytes + (nb + 3) // 4], np.int32).tobytes()[:nb] == b"".join(names)
        assert got["slots%d" % k] == table["slots"] and got["off32_%d" % k] == table["off32"]       # the single path's copies
    assert b[15] == 0
    check_regions(regions, len(b))
    assert not np.asarray(b)[~owned].any()
    assert got["n"] == [len(parts), len(nodes), len(states)]


# ---- capacities -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sanitized", BUILDS)
def test_capacities(tmp_path, sanitized):
    """batch_wire_cap_of and the three bounds of a document against the formulas of include/blance_batch.h: with and without
    assign_too, with a zero and a negative constraint, without names, P = 0, a document shorter than 3 bytes."""
    cases = [  # P, M, k, len, assign_too, names?, part_esc, state_esc, node_max, skeleton, result_cap of the plain formula
        (5, 2, [1, 2], 100, 0, 1, 40, 19, 7, 23, 23),
        (5, 2, [1, 2], 100, 1, 1, 40, 19, 7, 23, 23),
        (5, 3, [1, 0, 2], 101, 1, 1, 40, 19, 7, 23, 0),
        (5, 3, [1, -1, 2], 102, 1, 1, 40, 19, 7, 23, 1),
        (5, 2, [1, 2], 100, 1, 0, 40, 19, 7, 23, 23),
        (0, 0, [], 2, 1, 1, 0, 0, 0, 0, 0),
        (16384, 16, [8] * 16, 2 ** 28, 1, 1, 2 ** 20, 200, 300, 10 ** 6, 10 ** 6),
    ]
    got = run(["bounds %d %d %s %d %d %d %d %d %d %d %d" % (P, M, " ".join(map(str, k)), ln, a, nm, pe, se, nmax, sk, rc)
               for P, M, k, ln, a, nm, pe, se, nmax, sk, rc in cases], tmp_path, sanitized)
    for (P, M, k, ln, a, nm, pe, se, nmax, sk, rc), g in zip(cases, got):
        def wire_cap(result_cap):
            return 2 + 29 * P + 2 * pe + P * (se + 5 * M) + result_cap * (nmax + 1)
        result = P * sum(max(x, 0) for x in k) + ln // 3 if a else sk
        assert g["bounds"] == [result, ln // 3 + result, wire_cap(result) if nm else 0], (P, M, k, ln, a)
        assert g["wire_cap"] == [wire_cap(rc)]
