"""The batch's host arithmetic alone (blance_amd/csrc/host/batch_layout.hpp): batch_layout, the four optional region sets,
batch_head, batch_pack, the documents' verdict with the refusal order and the load bound it shares with blance_wire_adopt, and
the unpacking of an output slice -- through a stand-alone program (tests/simt/batch_layout_main.cpp, plain g++, no HIP), built
twice -- plain, and under AddressSanitizer and UBSan -- and compared with references written here from the definitions
(blance_kernels.h's comments on the slices, blance_hip.h on blance_wire_adopt, blance_batch.h), in plain Python.

The kernels trust these offsets blindly: a region that overlaps its neighbour corrupts a plan silently, and could so far only
be seen through whole plans.  The cases are each the smallest world where one decision can go wrong.

Mutants of batch_layout.hpp applied by hand (the plain build), and what failed then:
  batch_take without its rounding `(n_words + 3) & ~3ll`            -> test_layout_regions (the pack tests read through the
                                                                      descriptor and follow it wherever it points)
  `NX >= kBatchMaxNX` for `NX > kBatchMaxNX` in batch_layout         -> test_envelope_edges[nx_256]
  adopt_refusal: DUPLICATE_NODE tested before PARTITION_MISSING      -> test_refusal_order, test_verdict[missing_before_duplicate]
  adopt_load_bound_exceeded with `>=` for `>`                        -> test_load_bound, test_verdict[load_exactly_at_the_bound] and
                                                                      [kept_loads_at_the_bound]
  batch_unpack_moves without the `- 1` of the state                  -> test_unpack_moves
(the other tests passed under each mutant)
"""
import fcntl
import itertools
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "simt", "batch_layout_main.cpp")
HDRS = [os.path.join(HERE, "..", "blance_amd", "csrc", "host", "batch_layout.hpp"),
        os.path.join(HERE, "..", "blance_amd", "csrc", "blance_kernels.h"), os.path.join(HERE, "..", "include", "blance_hip.h"),
        os.path.join(HERE, "..", "include", "blance_batch.h")]
EXE = os.path.join(HERE, "simt", "_build", "batch_layout")
SANITIZE = ["-fsanitize=address,undefined", "-static-libasan", "-static-libubsan"]     # the runtimes inside the program
# blance_kernels.h
MAX_NX, MAX_P, MAX_L, MAX_STATES, HDR, STATS_ARRAYS = 256, 16384, 8, 16, 8, 7
BD = dict(refusal=0, records=2, refs=3, longest=4, fresh=5, first_missing=6, first_dup=7, first_long=8, cap=10, prev_load=12, words=16)
INT_MAX = 2 ** 31 - 1
POISON = 0x5A5A5A5A
# blance_hip.h: BLANCE_WIRE_ADOPT_*
MISSING, DUPLICATE, REMOVED_WITHOUT_PREV, LOAD_OVERFLOW = 2, 3, 4, 5
# DocVerdict::Kind, ::Which
PARSER_REFUSED, WHY_REFUSED, SINGLE_PATH, INCONSISTENT, PLAN = range(5)
LENGTHS_OVERFLOW, LONGEST_DISAGREES, CAP_ABOVE_BOUND = range(3)


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
    """The program's answers: per command that answers a dict of its lines."""
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
    n = sum(not c.startswith("problem") for c in commands)
    assert lines[-1] == "ran %d commands" % n
    for ln in lines[:-1]:
        name, *vals = ln.split()
        if name == "answer":
            out.append({})
        else:
            out[-1][name] = [int(v) for v in vals]
    assert len(out) == n
    return out


BUILDS = [pytest.param(False, id="plain"), pytest.param(True, id="sanitized")]


# ---- problems ---------------------------------------------------------------------------------------------------------------

class Prob:
    """A blance_problem as arrays.  assign / prev: PM lists of node ids; loads: (state, node, weight, first sweep only);
    hierarchy: (parent, lo, hi, empty) over the vertices, rules: (state, include level, exclude level)."""

    def __init__(self, P=1, M=1, NX=1, N=None, k=None, assign=None, prev=None, loads=(), rules=(), hierarchy=None, n_prev=None,
                 in_prev=None, part_weight=None, weights_nil=1, removed=(), max_it=10, seed=1):
        rng = np.random.RandomState(seed)
        self.P, self.M, self.NX, self.N = P, M, NX, NX if N is None else N
        PM = P * M
        self.k = list(k) if k is not None else [1] * M
        self.prio = list(range(M))
        self.stick = [int(x) for x in rng.randint(1, 1000, M)]
        self.hstick = [int(x) for x in rng.randint(0, 2, M)]
        self.removed = [int(n in removed) for n in range(NX)]
        self.added = [int(x) for x in rng.randint(0, 2, NX)]
        self.nweight = [int(x) for x in rng.randint(-5, 1000, NX)]
        self.hweight = [int(x) for x in rng.randint(0, 2, NX)]
        self.leaf = [int(x) for x in rng.permutation(NX)]
        self.order = [int(x) for x in rng.permutation(P)]
        self.pweight = list(part_weight) if part_weight is not None else [int(x) for x in rng.randint(1, 50, P)]
        self.phweight = [1] * P if part_weight is not None else [int(x) for x in rng.randint(0, 2, P)]
        self.in_prev = list(in_prev) if in_prev is not None else [1] * P
        self.never = [int(x) for x in rng.randint(0, 2, P)]
        self.assign = [list(a) for a in assign] if assign is not None else [[int(rng.randint(0, NX))] for _ in range(PM)]
        self.prev = [list(a) for a in prev] if prev is not None else [[int(x) for x in rng.randint(0, NX, i % 3)] for i in range(PM)]
        self.akind = [int(x) for x in rng.randint(0, 3, PM)]
        self.pkind = [int(x) for x in rng.randint(0, 3, PM)]
        self.loads = [tuple(l) for l in loads]
        self.rules = [tuple(r) for r in rules]
        self.hierarchy = hierarchy
        self.n_prev = P if n_prev is None else n_prev
        self.weights_nil, self.max_it = weights_nil, max_it
        self.add_nil, self.booster, self.top = int(rng.randint(0, 2)), int(rng.randint(0, 3)), 0

    def rule_off(self):
        return [sum(r[0] < m for r in self.rules) for m in range(self.M + 1)]

    def text(self):
        parent, lo, hi, empty = self.hierarchy if self.hierarchy else ([], [], [], 0)
        csr = lambda ls: [sum(len(x) for x in ls[:i]) for i in range(len(ls) + 1)]          # noqa: E731
        flat = lambda ls: [x for l in ls for x in l]                                        # noqa: E731
        w = [self.N, self.NX, self.M, self.P, self.n_prev, len(self.loads), len(self.rules), len(parent), self.max_it,
             self.weights_nil, self.add_nil, int(not self.rules), self.booster, self.top]
        w += self.prio + self.k + self.stick + self.hstick
        w += self.removed + self.added + self.nweight + self.hweight + self.leaf
        w += self.order + self.pweight + self.phweight + self.in_prev + self.never
        w += csr(self.assign) + flat(self.assign) + self.akind + csr(self.prev) + flat(self.prev) + self.pkind
        for j in range(4):
            w += [l[j] for l in self.loads]
        w += self.rule_off() + [r[1] for r in self.rules] + [r[2] for r in self.rules]
        w += [empty] + list(parent) + list(lo) + list(hi)
        return "problem " + " ".join(str(int(x)) for x in w)

    def longest(self):
        return max([1] + self.k + [len(a) for a in self.assign] + [len(a) for a in self.prev])

    def passes(self):
        return sum(k > 0 for k in self.k)


def layout_cmd(result_cap, doc=0, doc_loads=0, moves=None, stats=False, wire=None, docd=None, pack=None):
    """moves: (favor, other offsets or None, cap); wire: (names words, bound); docd: (len, dict words, assign_too);
    pack: (doc, keep)."""
    w = [result_cap, doc, doc_loads]
    if moves is None:
        w += [0]
    else:
        w += [1, int(moves[0])] + ([0] if moves[1] is None else [1] + list(moves[1])) + [moves[2]]
    w += [int(stats)]
    w += [0] if wire is None else [1, wire[0], wire[1]]
    w += [0] if docd is None else [1, docd[0], docd[1], docd[2]]
    w += [0] if pack is None else [1, pack[0], int(pack[1])]
    return "layout " + " ".join(str(int(x)) for x in w)


def r4(n):
    return (n + 3) // 4 * 4


# ---- layout -----------------------------------------------------------------------------------------------------------------

IN_FIELDS = ("i_state", "i_rule_off", "i_node", "i_order", "i_part", "i_alist", "i_ahdr", "i_plist", "i_phdr", "i_loads", "i_anch")
SC_FIELDS = ("s_live", "s_lhdr", "s_prv", "s_phdr", "s_pflag", "s_order", "s_cat", "s_ntn")
OUT_FIELDS = ("o_off", "o_kind", "o_nodes", "o_wp", "o_ws")


def plan_region_sizes(p, L, n_loads, cap):
    """The words of every region of the plan, by BatchDesc's comments (blance_kernels.h)."""
    P, M, NX, N, PM = p.P, p.M, p.NX, p.N, p.P * p.M
    wcap = P * p.passes()
    return ([4 * M, M + 1, 4 * NX, P, 2 * P, PM * L, PM, PM * L, PM, 4 * n_loads, 4 * len(p.rules) * (NX + 1)],
            [PM * L, PM, PM * L, PM, P, P, P, (NX + 1) * max(N, 1)],
            [PM + 1, PM, cap, wcap, wcap])


def check_regions(regions, total, tag):
    """regions: (start, words) of one slice: each 4-word aligned, inside [0, total), no two overlapping."""
    for a, n in regions:
        assert a % 4 == 0 and a >= 0 and a + n <= total, (tag, regions, total)
    spans = sorted((a, a + n) for a, n in regions if n > 0)
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
        assert a1 <= b0, (tag, regions)


SHAPES = [dict(P=1, M=1, NX=1, k=[1]), dict(P=3, M=2, NX=5, k=[1, 2], rules=[(1, 2, 1)]),
          dict(P=3, M=2, NX=5, N=0, k=[0, 3], loads=[(0, 1, 5, 0), (2, 0, 7, 1)])]
MOVES = [None, "plain", "other"]
DOCS = [None, 0, 1]
HIER5 = ([5, 5, 6, 6, 8, 7, 7, 8, 8], [0, 1, 2, 3, 4, 0, 2, 0, 5], [1, 2, 3, 4, 5, 2, 4, 4, 6], 8)      # two racks in a zone, a loose node, ""


@pytest.mark.parametrize("sanitized", BUILDS)
def test_layout_regions(tmp_path, sanitized):
    """Every combination of the optional region sets on three shapes: each region where the definition puts it, aligned,
    inside its slice, overlapping none; the statistics 8-byte aligned."""
    cases, commands = [], []
    for shape, moves, stats, wire, docd in itertools.product(SHAPES, MOVES, (False, True), (False, True), DOCS):
        p = Prob(hierarchy=HIER5 if shape.get("rules") else None, **shape)
        other = None
        if moves == "other":                                         # one partition with an empty other-list
            other = [0, 2, 2, 3][:p.P + 1] if p.P > 1 else [0, 1]
        cap = 11 if docd is None else 23
        c = dict(p=p, cap=cap, doc=docd is not None, doc_loads=1 if docd is not None and p.loads else 0,
                 moves=None if moves is None else (True, other, 17), stats=stats, wire=(24, 1001) if wire else None,
                 docd=None if docd is None else (37, 40, docd))
        cases.append(c)
        commands += [p.text(), layout_cmd(c["cap"], int(c["doc"]), c["doc_loads"], c["moves"], stats, c["wire"], c["docd"])]
    for c, got in zip(cases, run(commands, tmp_path, sanitized)):
        p = c["p"]
        tag = (p.P, p.M, p.NX, c["moves"], c["stats"], c["wire"], c["docd"])
        assert got["ok"] == [1], tag
        L = MAX_L if c["doc"] else p.longest()
        n_loads = c["doc_loads"] if c["doc"] else len(p.loads)
        sizes = plan_region_sizes(p, L, n_loads, c["cap"])
        slices = [list(zip(got["in"], sizes[0])), list(zip(got["sc"], sizes[1])), [(0, HDR)] + list(zip(got["out"], sizes[2]))]
        # the plan's regions one behind the other, from the definition
        for sl, first in zip(slices, (0, 0, 0)):
            at = first
            for a, n in sl:
                assert a == at, (tag, sl)
                at += r4(n)
        plan_words = [sum(r4(n) for _, n in sl) for sl in slices]
        assert got["plan_words"] == plan_words + [64 if p.NX <= 64 else 256], tag
        assert got["sizes"] == [p.N, p.NX, p.M, p.P, L], tag
        words = list(plan_words)
        if c["moves"]:
            other = c["moves"][1]
            n_other = other[p.P] if other else 0
            other_len = max([0] + [other[i + 1] - other[i] for i in range(p.P)]) if other else 0
            stride = min(2 * p.M * L + other_len, p.NX)
            desc, favor, i_ooff, i_onodes, s_cnt, s_mv, got_stride, o_moff, o_mops, mcap = got["moves"]
            assert (desc, favor, got_stride, mcap) == (5, 1, stride, 17), tag
            assert [i_ooff, i_onodes] == [words[0], words[0] + r4(p.P + 1)], tag
            assert [s_cnt, s_mv] == [words[1], words[1] + r4(p.P)], tag
            assert [o_moff, o_mops] == [words[2], words[2] + r4(p.P + 1)], tag
            slices[0] += [(i_ooff, p.P + 1), (i_onodes, n_other)]
            slices[1] += [(s_cnt, p.P), (s_mv, p.P * stride)]
            slices[2] += [(o_moff, p.P + 1), (o_mops, 17)]
            words = [words[0] + r4(p.P + 1) + r4(n_other), words[1] + r4(p.P) + r4(p.P * stride), words[2] + r4(p.P + 1) + r4(17)]
        if c["stats"]:
            assert got["stats"] == [5, words[2]] and got["stats"][1] * 4 % 8 == 0, tag
            slices[2].append((words[2], 2 * (1 + STATS_ARRAYS * p.M)))
            words[2] += r4(2 * (1 + STATS_ARRAYS * p.M))
        if c["wire"]:
            assert got["wire"] == [5, words[0], words[1], words[2]], tag
            slices[0].append((words[0], 24)); slices[1].append((words[1], p.P + 1)); slices[2].append((words[2], 1))
            words = [words[0] + 24, words[1] + r4(p.P + 1), words[2] + 4]
        if c["docd"]:
            ln, dict_words, a_too = c["docd"]
            PM = p.P * p.M
            rec_cap = (ln + 1) // 2 + 1
            sc = [(p.P, None), ((p.P + 3) // 4, None), ((PM + 3) // 4, None), (PM + 1, None), (rec_cap, None)]
            starts, at = [], words[1]
            for n, _ in sc:
                starts.append(at)
                at += r4(n)
            assert got["docd"] == [5, ln, 3 * 16, words[0], a_too] + starts + [rec_cap], tag
            slices[0].append((words[0], dict_words))
            slices[1] += [(s, n) for s, (n, _) in zip(starts, sc)]
            words = [words[0] + dict_words, at, words[2]]
        assert got["bytes"] == [7 * 16 + (1008 if c["wire"] else 0), 3 * 16 + (48 if c["docd"] else 0)], tag
        assert got["words"] == words, tag
        for sl, total, name in zip(slices, got["words"], ("in", "sc", "out")):
            check_regions(sl, total, (tag, name))


@pytest.mark.parametrize("sanitized", BUILDS)
def test_head(tmp_path, sanitized):
    """BatchHead for 0 and 1 of each kind (and a few more): every array on a 256-byte multiple, one behind the other, head_bytes
    the sum."""
    counts = list(itertools.product((0, 1), repeat=5)) + [(3, 2, 40, 17, 5), (1000, 0, 1, 0, 999)]
    got = run(["head %d %d %d %d %d" % c for c in counts], tmp_path, sanitized)
    for c, g in zip(counts, got):
        sizes = g["sizeof"]
        at, want = 0, []
        for n, size in zip(c, sizes):
            want.append(at)
            at += (n * size + 255) // 256 * 256
        assert g["head"] == want + [at], (c, g)
        assert all(x % 256 == 0 for x in g["head"]), (c, g)


def envelope_cases():
    """name -> (problem, layout arguments, inside the envelope?, size class)"""
    out = {}
    for NX, ok in ((256, 1), (257, 0)):
        out["nx_%d" % NX] = (Prob(P=1, M=1, NX=NX), dict(result_cap=5), ok, 256)
    for P, ok in ((16384, 1), (16385, 0)):
        out["p_%d" % P] = (Prob(P=P, M=1, NX=1, prev=[[]] * P), dict(result_cap=P), ok, 64)
    for n, ok in ((8, 1), (9, 0)):
        out["assign_list_%d" % n] = (Prob(P=1, M=1, NX=9, assign=[list(range(n))], prev=[[]]), dict(result_cap=20), ok, 64)
        out["prev_list_%d" % n] = (Prob(P=1, M=1, NX=9, assign=[[]], prev=[list(range(n))]), dict(result_cap=20), ok, 64)
        out["constraint_%d" % n] = (Prob(P=1, M=1, NX=9, k=[n], assign=[[]], prev=[[]]), dict(result_cap=20), ok, 64)
    for M, ok in ((MAX_STATES, 1), (MAX_STATES + 1, 0)):
        out["states_%d" % M] = (Prob(P=1, M=M, NX=2), dict(result_cap=40), ok, 64)
    for cap, ok in ((INT_MAX // 2, 1), (INT_MAX // 2 + 1, 0)):
        out["doc_bound_%d" % cap] = (Prob(P=1, M=1, NX=2), dict(result_cap=cap, doc=1), ok, 64)
    for NX, cls in ((64, 64), (65, 256)):
        out["class_nx_%d" % NX] = (Prob(P=2, M=1, NX=NX), dict(result_cap=5), 1, cls)
    return out


ENVELOPE = envelope_cases()


@pytest.fixture(scope="module")
def envelope_answers(tmp_path_factory):
    got = {}

    def answers(sanitized):
        if sanitized not in got:
            commands = []
            for p, kw, _, _ in ENVELOPE.values():
                commands += [p.text(), layout_cmd(**kw)]
            got[sanitized] = dict(zip(ENVELOPE, run(commands, tmp_path_factory.mktemp("envelope"), sanitized)))
        return got[sanitized]
    return answers


@pytest.mark.parametrize("sanitized", BUILDS)
@pytest.mark.parametrize("name", list(ENVELOPE))
def test_envelope_edges(envelope_answers, name, sanitized):
    _, _, ok, cls = ENVELOPE[name]
    got = envelope_answers(sanitized)[name]
    assert got["ok"] == [ok], name
    if ok:
        assert got["plan_words"][3] == cls, name


# ---- pack -------------------------------------------------------------------------------------------------------------------

def unpack_words(p, d, w, doc, n_loads):
    """Reads the packed words back through the descriptor (d: in offsets by name, L) and checks them against the problem."""
    P, M, NX, L, PM = p.P, p.M, p.NX, d["L"], p.P * p.M
    at = lambda name, n: [int(x) for x in w[d[name]:d[name] + n]]          # noqa: E731
    assert at("i_state", 4 * M) == [x for m in range(M) for x in (p.prio[m], p.k[m], p.stick[m], p.hstick[m])]
    assert at("i_rule_off", M + 1) == (p.rule_off() if p.rules else [0] * (M + 1))
    assert at("i_node", 4 * NX) == [x for n in range(NX) for x in
                                    (p.nweight[n], p.removed[n] | p.added[n] << 1 | p.hweight[n] << 2, p.leaf[n], 0)]
    assert at("i_order", P) == p.order
    assert at("i_part", 2 * P) == [x for i in range(P) for x in (p.pweight[i], p.phweight[i] | p.in_prev[i] << 1 | p.never[i] << 2)]
    for lists, kinds, rows, hdr, mine in ((p.assign, p.akind, "i_alist", "i_ahdr", doc < 2), (p.prev, p.pkind, "i_plist", "i_phdr", doc < 1)):
        if not mine:                                                   # k_batch_decode's to write: untouched
            assert at(rows, PM * L) == [POISON] * (PM * L) and at(hdr, PM) == [POISON] * PM, rows
            continue
        for idx in range(PM):
            row = w[d[rows] + idx * L:d[rows] + (idx + 1) * L]
            assert [int(x) for x in row[:len(lists[idx])]] == lists[idx], (rows, idx)
            assert all(int(x) == POISON for x in row[len(lists[idx]):]), (rows, idx)
            assert int(w[d[hdr] + idx]) == len(lists[idx]) | kinds[idx] << 16, (hdr, idx)
    return at("i_loads", 4 * n_loads)


def desc_of(got):
    d = dict(zip(IN_FIELDS, got["in"]))
    d["L"] = got["sizes"][4]
    return d


@pytest.mark.parametrize("sanitized", BUILDS)
def test_pack_round_trip(tmp_path, sanitized):
    """Every array of the problem recovered from the packed words; what k_batch_decode writes keeps the poison; the load
    filter of keep_prev_only."""
    loads = [(0, 1, 5, 1), (1, 0, -7, 0), (2, 3, 9, 0), (0, 2, 4, 1), (1, 4, 6, 0)]
    later = [l for l in loads if not l[3]]
    p = Prob(P=3, M=2, NX=5, k=[1, 2], loads=loads, rules=[(1, 2, 1)], hierarchy=HIER5, seed=3)
    runs = [  # (doc of batch_pack, keep, doc_loads of batch_layout, the load entries expected)
        (0, False, 0, loads),
        (1, False, 0, []),
        (1, True, 3, later),
        (2, True, 3, later),
        (2, True, 2, later[:2]),                                     # d.n_loads respected
        (2, False, 0, []),
    ]
    commands = [p.text()] + [layout_cmd(30, int(doc > 0), dl, pack=(doc, keep)) for doc, keep, dl, _ in runs]
    for (doc, keep, dl, want), got in zip(runs, run(commands, tmp_path, sanitized)):
        assert got["ok"] == [1] and got["kept_loads"] == [3, 0]
        w = np.array(got["packed"], dtype=np.int64)
        assert len(w) == got["words"][0]
        got_loads = unpack_words(p, desc_of(got), w, doc, len(want))
        assert got_loads == [x for l in want for x in l], (doc, keep, dl)


@pytest.mark.parametrize("sanitized", BUILDS)
def test_pack_anchor_table(tmp_path, sanitized):
    """One rule with include level 2 and exclude level 1: every anchor's two leaf intervals against a walk of vertex_parent here,
    the "" vertex (anchor NX) included."""
    parent, lo, hi, empty = HIER5
    p = Prob(P=3, M=2, NX=5, k=[1, 2], rules=[(1, 2, 1)], hierarchy=HIER5, seed=4)
    (got,) = run([p.text(), layout_cmd(30, pack=(0, False))], tmp_path, sanitized)
    d = desc_of(got)
    want = []
    for a in range(p.NX + 1):
        v = empty if a == p.NX else a
        vi = ve = v
        for _ in range(2):
            vi = parent[vi]
        for _ in range(1):
            ve = parent[ve]
        want += [lo[vi], hi[vi], lo[ve], hi[ve]]
    assert got["packed"][d["i_anch"]:d["i_anch"] + 4 * (p.NX + 1)] == want
    assert want[:4] == [0, 4, 0, 2] and want[16:20] == [5, 6, 5, 6] and want[20:] == [5, 6, 5, 6]     # a rack's node; the loose node; ""


# ---- the verdict ------------------------------------------------------------------------------------------------------------

def summary(refusal=None, records=3, refs=6, longest=2, fresh=0, first_missing=INT_MAX, first_dup=INT_MAX, first_long=INT_MAX,
            cap=9, prev_load=10):
    """k_batch_decode's summary words of one document (blance_kernels.h kBd*)."""
    v = [0] * BD["words"]

    def put64(at, x):
        x &= 2 ** 64 - 1
        for j in range(2):
            h = (x >> (32 * j)) & 0xffffffff
            v[at + j] = h - 2 ** 32 if h >= 2 ** 31 else h
    put64(BD["refusal"], 2 ** 64 - 1 if refusal is None else refusal[1] << 8 | refusal[0])
    put64(BD["cap"], cap)
    put64(BD["prev_load"], prev_load)
    for name, x in (("records", records), ("refs", refs), ("longest", longest), ("fresh", fresh), ("first_missing", first_missing),
                    ("first_dup", first_dup), ("first_long", first_long)):
        v[BD[name]] = x
    return v


def ref_verdict(p, s, v, assign_too, keep, result_cap):
    """What the host decides of a document (blance_batch.h on blance_plan_batch_docs; blance_hip.h on blance_wire_adopt's
    refusals "the first of them in the order below" and blance_validate's load bound for P'), from the keyword form s of the
    summary.  Returns the program's line."""
    none = (0, -1, 0, -1)
    if s.get("refusal") is not None:
        return [PARSER_REFUSED, s["refusal"][0], s["refusal"][1], 0, -1, -1, 0, 0, 0, 0, 0]
    g = dict(records=3, refs=6, longest=2, fresh=0, first_missing=INT_MAX, first_dup=INT_MAX, first_long=INT_MAX, cap=9, prev_load=10)
    g.update(s)
    if g["refs"] < 0:
        return [INCONSISTENT, *none, LENGTHS_OVERFLOW, 0, 0, 0, 0, 0]
    if (g["longest"] > MAX_L) != (g["first_long"] != INT_MAX):
        return [INCONSISTENT, *none, LONGEST_DISAGREES, 0, 0, 0, 0, 0]
    if g["longest"] > MAX_L:
        return [SINGLE_PATH, *none, -1, 0, 0, 0, 0, 0]
    seen = [g["refs"], g["records"]]
    any_removed, any_pass = any(p.removed), any(k > 0 for k in p.k)
    ksum = sum(k for k in p.k if k > 0)
    sumw = sum(abs(p.pweight[i]) if (not p.weights_nil and p.phweight[i]) else 1 for i in range(p.P))
    kept = sum(abs(l[2]) for l in p.loads if not l[3]) if keep else 0
    why = None
    if assign_too and g["first_missing"] != INT_MAX:
        why = (MISSING, g["first_missing"])
    elif assign_too and g["first_dup"] != INT_MAX:
        why = (DUPLICATE, g["first_dup"])
    elif g["first_missing"] != INT_MAX and any_removed and any_pass:
        why = (REMOVED_WITHOUT_PREV, g["first_missing"])
    elif g["prev_load"] + kept + sumw * max(ksum, 1) * 2 > INT_MAX:
        why = (LOAD_OVERFLOW, -1)
    if why:
        return [WHY_REFUSED, 0, -1, why[0], why[1], -1, 0, 0, 0] + seen
    if assign_too and g["cap"] > result_cap:
        return [INCONSISTENT, *none, CAP_ABOVE_BOUND, 0, 0, 0] + seen
    n_prev = g["records"] + (p.n_prev - sum(p.in_prev) if keep else 0)
    return [PLAN, *none, -1, n_prev, g["fresh"], g["cap"] if assign_too else result_cap] + seen


def verdict_cases():
    """name -> (problem, summary keywords, assign_too, keep, result_cap, the kind expected, its why or which)"""
    plain = Prob(P=3, M=2, NX=4, k=[1, 2], n_prev=7, in_prev=[1, 0, 1], loads=[(0, 1, -2, 0), (1, 2, 3, 0), (0, 0, 100, 1)], seed=5)
    removed = Prob(P=3, M=2, NX=4, k=[1, 2], removed=[2], seed=5)
    removed_no_pass = Prob(P=3, M=2, NX=4, k=[0, 0], removed=[2], seed=5)
    # P = 3 without weights, constraints 1 + 2: a plan can add 3 * 3 * 2 = 18; the kept load entries weigh 2 + 3
    edge, edge_kept = INT_MAX - 18, INT_MAX - 18 - 5
    bad = dict(refusal=(7, 123456789012))
    c = {
        "plans": (plain, {}, 1, 0, 20, PLAN, None),
        "parser_refusal_wins_over_everything": (removed, dict(refs=-1, longest=9, first_missing=0, first_dup=0, prev_load=2 ** 40, **bad),
                                                1, 0, 20, PARSER_REFUSED, None),
        "refs_negative": (plain, dict(refs=-1, longest=9, first_long=4, first_missing=0), 1, 0, 20, INCONSISTENT, LENGTHS_OVERFLOW),
        "longest_without_first_long": (plain, dict(longest=9), 1, 0, 20, INCONSISTENT, LONGEST_DISAGREES),
        "first_long_without_longest": (plain, dict(longest=8, first_long=4), 1, 0, 20, INCONSISTENT, LONGEST_DISAGREES),
        "longest_8_plans": (plain, dict(longest=8), 1, 0, 20, PLAN, None),
        "longest_9_single_path": (plain, dict(longest=9, first_long=4, first_missing=1), 1, 0, 20, SINGLE_PATH, None),
        "missing_without_assign_too": (plain, dict(first_missing=1), 0, 0, 20, PLAN, None),
        "missing_removed_but_no_pass": (removed_no_pass, dict(first_missing=1), 0, 0, 20, PLAN, None),
        "missing_pass_but_none_removed": (plain, dict(first_missing=1), 0, 0, 20, PLAN, None),
        "missing_removed_and_pass": (removed, dict(first_missing=1), 0, 0, 20, WHY_REFUSED, REMOVED_WITHOUT_PREV),
        "missing_with_assign_too": (plain, dict(first_missing=2), 1, 0, 20, WHY_REFUSED, MISSING),
        "duplicate_with_assign_too": (plain, dict(first_dup=5), 1, 0, 20, WHY_REFUSED, DUPLICATE),
        "duplicate_without_assign_too": (plain, dict(first_dup=5), 0, 0, 20, PLAN, None),
        "missing_before_duplicate": (removed, dict(first_missing=2, first_dup=1), 1, 0, 20, WHY_REFUSED, MISSING),
        "duplicate_before_removed_without_prev": (removed, dict(first_dup=1, prev_load=2 ** 40), 1, 0, 20, WHY_REFUSED, DUPLICATE),
        "removed_without_prev_before_load": (removed, dict(first_missing=1, prev_load=2 ** 40), 0, 0, 20, WHY_REFUSED, REMOVED_WITHOUT_PREV),
        "load_exactly_at_the_bound": (plain, dict(prev_load=edge), 1, 0, 20, PLAN, None),
        "load_one_above_the_bound": (plain, dict(prev_load=edge + 1), 1, 0, 20, WHY_REFUSED, LOAD_OVERFLOW),
        "kept_loads_at_the_bound": (plain, dict(prev_load=edge_kept), 1, 1, 20, PLAN, None),
        "kept_loads_one_above": (plain, dict(prev_load=edge_kept + 1), 1, 1, 20, WHY_REFUSED, LOAD_OVERFLOW),
        "kept_loads_not_counted_without_keep": (plain, dict(prev_load=edge_kept + 1), 1, 0, 20, PLAN, None),
        "load_before_the_capacity": (plain, dict(prev_load=edge + 1, cap=21), 1, 0, 20, WHY_REFUSED, LOAD_OVERFLOW),
        "capacity_above_its_bound": (plain, dict(cap=21), 1, 0, 20, INCONSISTENT, CAP_ABOVE_BOUND),
        "capacity_equal_to_its_bound": (plain, dict(cap=20), 1, 0, 20, PLAN, None),
        "capacity_not_read_without_assign_too": (plain, dict(cap=2 ** 40), 0, 0, 20, PLAN, None),
        "n_prev_keeps_the_keys_outside": (plain, dict(records=3, fresh=2), 1, 1, 20, PLAN, None),
        "n_prev_without_keep": (plain, dict(records=3, fresh=2), 1, 0, 20, PLAN, None),
    }
    return c


VERDICTS = verdict_cases()


@pytest.fixture(scope="module")
def verdict_answers(tmp_path_factory):
    got = {}

    def answers(sanitized):
        if sanitized not in got:
            commands = []
            for p, s, a_too, keep, cap, _, _ in VERDICTS.values():
                commands += [p.text(), "verdict %s %d %d %d" % (" ".join(str(x) for x in summary(**s)), a_too, keep, cap)]
            got[sanitized] = dict(zip(VERDICTS, run(commands, tmp_path_factory.mktemp("verdict"), sanitized)))
        return got[sanitized]
    return answers


@pytest.mark.parametrize("sanitized", BUILDS)
@pytest.mark.parametrize("name", list(VERDICTS))
def test_verdict(verdict_answers, name, sanitized):
    p, s, a_too, keep, cap, kind, detail = VERDICTS[name]
    got = verdict_answers(sanitized)[name]["verdict"]
    want = ref_verdict(p, s, summary(**s), a_too, keep, cap)
    assert want[0] == kind and (detail is None or detail == (want[3] if kind == WHY_REFUSED else want[5])), (name, want)
    assert got == want, name
    if name == "n_prev_keeps_the_keys_outside":
        assert got[6:9] == [3 + 7 - 2, 2, 9]
    if name == "n_prev_without_keep":
        assert got[6:9] == [3, 2, 9]
    if name == "missing_without_assign_too":
        assert got[8] == 20                                            # (without assign_too the capacity is the skeleton's)
    if name == "parser_refusal_wins_over_everything":
        assert got[1:3] == [7, 123456789012]


@pytest.mark.parametrize("sanitized", BUILDS)
def test_refusal_order(tmp_path, sanitized):
    """adopt_refusal over every combination of its inputs: the first that applies of PARTITION_MISSING, DUPLICATE_NODE,
    REMOVED_WITHOUT_PREV, LOAD_OVERFLOW (blance_hip.h: "the first of them in the order below")."""
    table = list(itertools.product((0, 1), (INT_MAX, 4), (INT_MAX, 9), (0, 1), (0, 1), (0, 1)))
    got = run(["refusal %d %d %d %d %d %d" % t for t in table], tmp_path, sanitized)
    for (a_too, missing, dup, removed, any_pass, load), g in zip(table, got):
        conditions = [(MISSING, missing, a_too and missing != INT_MAX), (DUPLICATE, dup, a_too and dup != INT_MAX),
                      (REMOVED_WITHOUT_PREV, missing, missing != INT_MAX and removed and any_pass), (LOAD_OVERFLOW, -1, load)]
        want = next(([why, at] for why, at, applies in conditions if applies), [0, -1])
        assert g["refusal"] == want, (a_too, missing, dup, removed, any_pass, load)


@pytest.mark.parametrize("sanitized", BUILDS)
def test_load_bound(tmp_path, sanitized):
    """aprev + kept + sumw * max(ksum, 1) * 2 > INT32_MAX, at the edge through each term."""
    table = [(INT_MAX - 18, 0, 3, 3), (INT_MAX - 17, 0, 3, 3), (INT_MAX - 23, 5, 3, 3), (INT_MAX - 22, 5, 3, 3),
             (INT_MAX - 2, 0, 1, 0), (INT_MAX - 1, 0, 1, 0), (1, 0, (INT_MAX - 1) // 2, 1), (2, 0, (INT_MAX - 1) // 2, 1),
             (0, 0, 0, 5), (0, INT_MAX, 0, 5), (0, INT_MAX + 1, 0, 5), (2 ** 40, 0, 0, 0)]
    got = run(["load_bound %d %d %d %d" % t for t in table], tmp_path, sanitized)
    for (aprev, kept, sumw, ksum), g in zip(table, got):
        assert g["load_bound"] == [int(aprev + kept + sumw * max(ksum, 1) * 2 > INT_MAX)], (aprev, kept, sumw, ksum)
    assert [g["load_bound"][0] for g in got] == [0, 1, 0, 1, 0, 1, 0, 1, 0, 0, 1, 1]


# ---- unpack -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sanitized", BUILDS)
def test_planned(tmp_path, sanitized):
    """batch_planned: done == 1 and no error word, whatever the other header words say."""
    table = [(3, 1, 0, 5, 0, 1, 99, 0), (3, 1, 0, 5, 0, 0, 99, 0), (3, 1, 0, 5, 2, 1, 99, 0), (0, 0, 0, 0, 0, 1, 0, 0),
             (3, 1, 0, 5, 0, 2, 99, 0), (1, 1, 1, 1, -1, 1, 1, 1)]
    got = run(["planned " + " ".join(str(x) for x in t) for t in table], tmp_path, sanitized)
    assert [g["planned"][0] for g in got] == [1, 0, 0, 1, 0, 0]


@pytest.mark.parametrize("sanitized", BUILDS)
def test_unpack_result(tmp_path, sanitized):
    """A result with lists and warnings, and one with neither (its buffers hold nothing: a byte written is the sanitizer's)."""
    p = Prob(P=2, M=2, NX=4, k=[1, 0], seed=6)                    # one state with a pass
    PM = 4
    o_off, o_kind, o_nodes, o_wp, o_ws = 8, 16, 20, 28, 32
    full = [3, 1, 2, 5, 0, 1, 77, 0] + [0, 2, 2, 4, 5, 0, 0, 0] + [2, 0, 1, 2] + [3, 1, 0, 2, 1, -9, -9, -9] + [1, 0, -9, -9] + [0, 1, -9, -9]
    none = [4, 0, 0, 0, 0, 1, 0, 0] + [0, 0, 0, 0, 0, 0, 0, 0] + [1, 1, 0, 2] + [-9] * 16
    cmds = [p.text()] + ["unpack_result 2 2 %d %d %d %d %d %d %s" % (o_off, o_kind, o_nodes, o_wp, o_ws, len(o), " ".join(map(str, o)))
                         for o in (full, none)]
    a, b = run(cmds, tmp_path, sanitized)
    assert a["out_off"] == [0, 2, 2, 4, 5] and a["out_kind"] == [2, 0, 1, 2] and a["out_nodes"] == [3, 1, 0, 2, 1]
    assert a["warn_part"] == [1, 0] and a["warn_state"] == [0, 1]
    # warnings, sweeps, converged, steps = sweeps * P * passes; the single path's counters zero; the times as given
    assert a["counters"] == [2, 3, 1, 3 * 2 * 1, 0, 0, 0, 0, 0, 0, 0, 0, 3, 5, 0]
    assert b["out_off"] == [0] * (PM + 1) and b["out_kind"] == [1, 1, 0, 2] and b["out_nodes"] == [] and b["warn_part"] == []
    assert b["counters"] == [0, 4, 0, 4 * 2 * 1, 0, 0, 0, 0, 0, 0, 0, 0, 3, 5, 0]


@pytest.mark.parametrize("sanitized", BUILDS)
def test_unpack_moves(tmp_path, sanitized):
    """node | (state + 1) << 16 | kind << 24: state -1 is encoded 0, the highest state kMaxStates - 1; a problem without moves."""
    moves = [(255, -1, 1), (0, MAX_STATES - 1, 3), (17, 0, 0), (64, 7, 2)]
    words = [n | (s + 1) << 16 | k << 24 for n, s, k in moves]
    o = [0] * 4 + [0, 1, 1, 4] + words
    quiet = [0] * 4 + [0, 0, 0, 0]
    a, b = run(["unpack_moves 3 4 8 %d %s" % (len(o), " ".join(map(str, o))),
                "unpack_moves 3 4 8 %d %s" % (len(quiet), " ".join(map(str, quiet)))], tmp_path, sanitized)
    assert a["op_off"] == [0, 1, 1, 4]
    assert (a["op_node"], a["op_state"], a["op_kind"]) == ([m[0] for m in moves], [m[1] for m in moves], [m[2] for m in moves])
    assert b["op_off"] == [0, 0, 0, 0] and b["op_node"] == []


@pytest.mark.parametrize("sanitized", BUILDS)
def test_unpack_stats(tmp_path, sanitized):
    """1 + 7 M int64 values, with and without rule_violations (NULL: not written)."""
    M = 2
    vals = [5] + [-3, 4, 2 ** 40, 7, 2 ** 33 + 1, 9, 2 ** 50, -2 ** 50, 3, 1, 0, 2 ** 35, 11, 12]
    words = [0] * 4
    for v in vals:
        v &= 2 ** 64 - 1
        for j in range(2):
            h = (v >> (32 * j)) & 0xffffffff
            words.append(h - 2 ** 32 if h >= 2 ** 31 else h)
    a, b = run(["unpack_stats %d 4 %d %d %s" % (M, rv, len(words), " ".join(map(str, words))) for rv in (1, 0)], tmp_path, sanitized)
    for g in (a, b):
        assert g["n_nodes_next"] == [5]
        assert [g[k] for k in ("load_min", "load_max", "load_sum", "load_sumsq", "nodes_used", "unmet_slots")] == \
            [vals[1:3], vals[3:5], vals[5:7], vals[7:9], vals[9:11], vals[11:13]]
    assert a["rule_violations"] == vals[13:15] and "rule_violations" not in b
