"""The sweep's record, category, bit-map, region-chain, list-edit and tail kernels one at a time: binding, tables, references and checks
shared by tests/test_sweep_cases_emulated.py (the SIMT emulator) and tests/test_sweep_cases_gpu.py (the device).  Both run
the same tables through the entries of tests/kernels/sweep_cases.inc; only the library differs.

The references are plain Python over lists of ints, written from what plan.go does with a partition's NodesByState:
  * a step record is the partition, its weight (plan.go:269-275), its stickiness (plan.go:104-115: the partition's weight, else
    the state's stickiness, else 1.5 -- and 1.5 whenever there are no partition weights at all) and a copy of its lists;
  * the category is partitionSorter's (plan.go:542-561);
  * a step's choices are applied as plan.go:290-299 does: the state's old nodes and the chosen nodes leave every other state,
    every other state that is present becomes a non-nil slice, the state takes the chosen nodes;
  * the convergence test is reflect.DeepEqual per partition (plan.go:36-45: a nil and an empty slice differ, a missing key and
    a present one differ), followed by prevMap[name] = nextMap[name] (plan.go:49-52);
  * the next sweep's opening counts the new prevMap (countStateNodes, plan.go:374-399) and makes every present list a non-nil
    slice (plan.go:418).
  * a chain pass gives every step the region of its top priority node; a node the partition holds in the pass's state outside
    that region leaves it whatever the step decides (plan.go:290-293) -- an event for the region that owns it, or an orphan;
    the compact record (blance_kernels.h has its layout) names the step's nodes by leaf inside the region.  A step the record
    cannot hold is compared by its header and the flag it raises: no pass runs on such a record.
Everything is integers; stickiness is compared as the bit pattern of the double.  Every comparison is exact.

A list's slots at and behind its length mean nothing and are not compared; the tables fill them with valid node ids, so that a
kernel that reads them computes something wrong without indexing outside a table.  Where the product keeps an invariant (an
absent or nil list has length 0) the convergence and tail tables keep it too; the record and category tables break it on
purpose where the kernels say they do not rely on it (an absent list with stale contents)."""
import copy
import ctypes
import struct

import numpy as np

import kernel_case_tables as T
from kernel_case_tables import BAD_ARG, GUARD, LIST_ABSENT, LIST_NIL, LIST_SET, _i32, _p, _rng, _u8

REC_HEAD = 4                                         # kRecHead
GATE_WORDS = 32                                      # kGateWords
GUARD8 = 0x5A
CNT_FILL = 0x33                                      # what the binding fills cnt_next with before a call
GEOM_P = [1, 63, 64, 65, 255, 256, 257, 513, 1000]


# ---- binding ----------------------------------------------------------------------------------------------------------------

_PB_ARRAYS = ["live", "live_len", "live_kind", "prv", "prv_len", "prv_kind", "in_prev", "never_equal", "node_removed", "node_added",
              "part_weight", "part_has_weight"]
_PB_U8 = {"live_kind", "prv_kind", "in_prev", "never_equal", "node_removed", "node_added", "part_has_weight"}


class _CProblem(ctypes.Structure):                   # KSweepProblem
    _fields_ = [(n, ctypes.c_int32) for n in ("N", "NX", "M", "L", "P", "weights_nil")] + [(n, ctypes.c_void_p) for n in _PB_ARRAYS]


def _cproblem(pb):
    """-> (the struct, a copy of pb whose arrays the struct points at: the entry writes what it copied back into them)"""
    q = {k: pb[k] for k in ("N", "NX", "M", "L", "P", "weights_nil")}
    for k in _PB_ARRAYS:
        q[k] = np.array(pb[k], dtype=np.uint8 if k in _PB_U8 else np.int32, order="C", copy=True)
    c = _CProblem(**{k: q[k] for k in ("N", "NX", "M", "L", "P", "weights_nil")},
                  **{k: q[k].ctypes.data for k in _PB_ARRAYS})
    return c, q


class SweepCases(T.KernelCases):
    def __init__(self, path):
        super().__init__(path)
        vp, ci, cu = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint
        for name, args in {
            "kcase_category": [vp, ci, ci, ci, vp],
            "kcase_gather": [vp, ci, ci, vp, vp, vp, ci, vp, vp],
            "kcase_ntn_bits_words": [ci],
            "kcase_ntn_bits": [ci, ci, ci, vp, vp],
            "kcase_invert": [ci, vp, vp],
            "kcase_sweep_end": [vp, ci, ci, ci, vp, vp, ci, ci, vp, vp, cu, vp],
        }.items():
            f = getattr(self.lib, name)
            f.argtypes, f.restype = args, ci
        self.calls = 0

    def category(self, pb, m, any_removed, add_nil, check=True, fill=0):
        c, q = _cproblem(pb)
        cat = np.full(pb["P"] + 1, fill, np.uint8)
        self.calls += 1
        rc = self._ok(self.lib.kcase_category(ctypes.addressof(c), m, any_removed, add_nil, _p(cat)), check)
        return rc, q, cat

    def gather(self, pb, m, top_state, order, ss, hs, with_rows, check=True, fill=0):
        c, q = _cproblem(pb)
        RW = REC_HEAD + pb["M"] * (1 + pb["L"])
        rec, rows = np.full(pb["P"] * RW + 1, fill, np.int32), np.full(pb["NX"] + 2, fill, np.int32)
        order, ss, hs = _i32(order), _i32(ss), _u8(hs)
        self.calls += 1
        rc = self._ok(self.lib.kcase_gather(ctypes.addressof(c), m, top_state, _p(order), _p(ss), _p(hs), int(with_rows), _p(rec),
                                            _p(rows)), check)
        return rc, q, rec, rows

    def ntn_bits_words(self, NX):
        return self.lib.kcase_ntn_bits_words(NX)

    def ntn_bits(self, N, NX, rows, ntn, BW, check=True, fill=0):
        ntn = _i32(ntn)
        bits = np.full(rows * BW + 1, fill, np.uint32)
        self.calls += 1
        rc = self._ok(self.lib.kcase_ntn_bits(N, NX, rows, _p(ntn), _p(bits)), check)
        return rc, bits

    def invert(self, perm, check=True, fill=0):
        perm = _i32(perm)
        inv = np.full(len(perm) + 1, fill, np.int32)
        self.calls += 1
        rc = self._ok(self.lib.kcase_invert(len(perm), _p(perm), _p(inv)), check)
        return rc, inv

    def sweep_end(self, pb, mode, m, order, out, with_out, with_cnt, word, gate_words=None, gate_mask=0, check=True):
        """-> rc, the problem as the kernels left it, the three words (sentinel, not_match, sentinel), cnt_next[M NX + 1]"""
        c, q = _cproblem(pb)
        order, out = _i32(order), _i32(out)
        words = np.array([T.SENTINEL_A, word, T.SENTINEL_B], np.int32)
        gw = _i32(np.zeros(GATE_WORDS) if gate_words is None else gate_words)
        cnt = np.full(pb["M"] * pb["NX"] + 1, CNT_FILL, np.int32)
        self.calls += 1
        rc = self._ok(self.lib.kcase_sweep_end(ctypes.addressof(c), mode, m, out.shape[1], _p(order), _p(out), int(with_out),
                                               int(with_cnt), _p(words), _p(gw), gate_mask, _p(cnt)), check)
        return rc, q, words, cnt


# ---- problems ---------------------------------------------------------------------------------------------------------------

def blank_problem(P, M, L, N, NX, seed, weights_nil=0):
    """Every list absent, nothing removed or added, no weights; the list slots hold valid node ids that mean nothing."""
    r = _rng(40, seed, P, M, L)
    return dict(N=N, NX=NX, M=M, L=L, P=P, weights_nil=weights_nil,
                live=r.integers(0, NX, (P, M, L)).astype(np.int32), live_len=np.zeros((P, M), np.int32), live_kind=np.zeros((P, M), np.uint8),
                prv=r.integers(0, NX, (P, M, L)).astype(np.int32), prv_len=np.zeros((P, M), np.int32), prv_kind=np.zeros((P, M), np.uint8),
                in_prev=np.ones(P, np.uint8), never_equal=np.zeros(P, np.uint8), node_removed=np.zeros(NX, np.uint8),
                node_added=np.zeros(NX, np.uint8), part_weight=np.zeros(P, np.int32), part_has_weight=np.zeros(P, np.uint8))


def set_list(pb, which, p, t, nodes, kind=LIST_SET):
    """nodes: a list of node ids; kind LIST_NIL / LIST_ABSENT with nodes given: stale contents under a list that is not there"""
    pb[which][p, t, :len(nodes)] = nodes
    pb[which + "_len"][p, t] = len(nodes)
    pb[which + "_kind"][p, t] = kind


def get_list(pb, which, p, t):
    """None: absent; else (is_nil, nodes)"""
    k = int(pb[which + "_kind"][p, t])
    if k == LIST_ABSENT:
        return None
    return (k == LIST_NIL, [int(x) for x in pb[which][p, t, :int(pb[which + "_len"][p, t])]])


def random_problem(P, M, L, N, NX, seed, stale=False, weights_nil=0):
    """Random lists of every kind.  A partition's nodes are distinct inside a list; now and then a node sits in two states.
    stale: absent lists keep a length and contents (the record and category kernels must not look at them)."""
    pb = blank_problem(P, M, L, N, NX, seed, weights_nil)
    r = _rng(41, seed, P, M, L)
    for which in ("live", "prv"):
        for p in range(P):
            for t in range(M):
                k = int(r.integers(0, 8))
                n = int(r.integers(0, L + 1)) if k < 6 else L
                nodes = [int(x) for x in r.choice(NX, size=min(n, NX), replace=False)]
                if k == 0:
                    set_list(pb, which, p, t, nodes if stale else [], LIST_ABSENT)
                elif k == 1:
                    set_list(pb, which, p, t, [], LIST_NIL)
                else:
                    set_list(pb, which, p, t, nodes)
    pb["in_prev"] = (r.integers(0, 6, P) > 0).astype(np.uint8)
    pb["never_equal"] = (r.integers(0, 6, P) == 0).astype(np.uint8)
    pb["node_removed"] = (r.integers(0, 5, NX) == 0).astype(np.uint8)
    pb["node_added"] = (r.integers(0, 5, NX) == 0).astype(np.uint8)
    pb["part_has_weight"] = (r.integers(0, 2, P)).astype(np.uint8)
    pb["part_weight"] = r.integers(-3, 6, P).astype(np.int32)
    return pb


def part_w(pb, p):
    return int(pb["part_weight"][p]) if not pb["weights_nil"] and pb["part_has_weight"][p] else 1


def assert_problem(got, want, what, lists_whole=False):
    """Every array of the problem as the reference has it.  Lists: the slots below their length (an absent list has none),
    or whole (lists_whole: nothing may have been written at all)."""
    for k in _PB_ARRAYS:
        if k in ("live", "prv") and not lists_whole:
            continue
        assert np.array_equal(got[k], np.asarray(want[k], got[k].dtype)), (what, k, np.flatnonzero(np.ravel(got[k] != want[k]))[:8])
    if not lists_whole:
        for which in ("live", "prv"):
            for p in range(want["P"]):
                for t in range(want["M"]):
                    assert get_list(got, which, p, t) == get_list(want, which, p, t), (what, which, p, t)


# ---- 1. k_category ----------------------------------------------------------------------------------------------------------

def ref_category(pb, m, any_removed, add_nil):
    cat = []
    for p in range(pb["P"]):
        c = 2
        lp = get_list(pb, "prv", p, m)
        if any_removed and pb["in_prev"][p] and lp is not None and not lp[0] and any(pb["node_removed"][x] for x in lp[1]):
            c = 0                                    # on a node that is being removed
        elif not add_nil:
            held = [x for t in range(pb["M"]) for x in (get_list(pb, "live", p, t) or (0, []))[1]]
            if not any(pb["node_added"][x] for x in held):
                c = 1                                # not yet on any added node
        cat.append(c)
    return cat


CAT_M, CAT_L, CAT_NX, CAT_STATE = 3, 3, 12, 1
CAT_REMOVED, CAT_ADDED = 10, 11


def category_table():
    """[(name, any_removed, add_nil, want)]: partition i of the table's problem is case i under ITS OWN (any_removed, add_nil);
    the check runs the problem once per pair of flags and compares every partition, the table's `want` is asserted on the
    reference for the named pair."""
    P = 12
    pb = blank_problem(P, CAT_M, CAT_L, CAT_NX, CAT_NX, 1)
    pb["node_removed"][CAT_REMOVED] = 1
    pb["node_added"][CAT_ADDED] = 1
    for p in range(P):                               # calm defaults: one plain node everywhere
        for t in range(CAT_M):
            set_list(pb, "live", p, t, [t])
            set_list(pb, "prv", p, t, [t])
    rows = []

    def case(name, any_removed, add_nil, want):
        rows.append((name, any_removed, add_nil, want))
        return len(rows) - 1

    p = case("removed node in prevMap's list of the state", 1, 0, 0)
    set_list(pb, "prv", p, CAT_STATE, [1, CAT_REMOVED])
    p = case("the same with any_removed = 0", 0, 0, 1)
    set_list(pb, "prv", p, CAT_STATE, [1, CAT_REMOVED])
    p = case("the same, partition not in prevMap", 1, 0, 1)
    set_list(pb, "prv", p, CAT_STATE, [1, CAT_REMOVED])
    pb["in_prev"][p] = 0
    p = case("removed node only in ANOTHER state of prevMap", 1, 0, 1)
    set_list(pb, "prv", p, 0, [CAT_REMOVED])
    p = case("prevMap's list nil", 1, 0, 1)
    set_list(pb, "prv", p, CAT_STATE, [], LIST_NIL)
    p = case("prevMap's list absent, stale contents name the removed node", 1, 0, 1)
    set_list(pb, "prv", p, CAT_STATE, [CAT_REMOVED], LIST_ABSENT)
    p = case("on an added node", 1, 0, 2)
    set_list(pb, "live", p, 0, [CAT_ADDED])
    p = case("added node only in an absent list's stale contents", 1, 0, 1)
    set_list(pb, "live", p, 2, [CAT_ADDED], LIST_ABSENT)
    p = case("on no added node, add_nil = 1", 1, 1, 2)
    p = case("removed wins over added", 1, 0, 0)
    set_list(pb, "prv", p, CAT_STATE, [CAT_REMOVED])
    set_list(pb, "live", p, 0, [CAT_ADDED])
    p = case("the added node at the last slot of the last state", 1, 0, 2)
    set_list(pb, "live", p, CAT_M - 1, [3, 4, CAT_ADDED])
    p = case("the removed node at the last slot of prevMap's list", 1, 0, 0)
    set_list(pb, "prv", p, CAT_STATE, [3, 4, CAT_REMOVED])
    assert len(rows) == P
    return pb, rows


def check_category_table(kc):
    pb, rows = category_table()
    seen = set()
    for any_removed in (0, 1):
        for add_nil in (0, 1):
            want = ref_category(pb, CAT_STATE, any_removed, add_nil)
            for i, (name, ar, an, w) in enumerate(rows):
                if (ar, an) == (any_removed, add_nil):
                    assert want[i] == w, name        # the table says what it means
                    seen.add(w)
            rc, q, cat = kc.category(pb, CAT_STATE, any_removed, add_nil)
            assert [int(x) for x in cat[:-1]] == want, (any_removed, add_nil)
            assert cat[-1] == GUARD8
            assert_problem(q, pb, "k_category writes nothing", lists_whole=True)
    assert seen == {0, 1, 2}


def check_category_geometry(kc, P):
    pb = random_problem(P, 3, 3, 20, 24, 2, stale=True)
    seen = set()
    for m, any_removed, add_nil in [(0, 1, 0), (2, 1, 0), (1, 0, 0), (1, 1, 1)]:
        want = ref_category(pb, m, any_removed, add_nil)
        seen |= set(want)
        rc, q, cat = kc.category(pb, m, any_removed, add_nil)
        assert [int(x) for x in cat[:-1]] == want, (m, any_removed, add_nil)
        assert cat[-1] == GUARD8
        assert_problem(q, pb, "k_category writes nothing", lists_whole=True)
    assert P < 63 or seen == {0, 1, 2}


# ---- 5. k_gather ------------------------------------------------------------------------------------------------------------

def stick_words(x):
    lo, hi = struct.unpack("<ii", struct.pack("<d", float(x)))
    return [lo, hi]


def ref_weight_stick(pb, p, m, ss, hs):
    w, stick = 1, 1.5
    if not pb["weights_nil"]:
        if pb["part_has_weight"][p]:
            w = int(pb["part_weight"][p])
            stick = float(w)
        elif hs[m]:
            stick = float(int(ss[m]))
    return w, stick


def ref_gather(pb, m, order, ss, hs):
    """-> the records as one flat list of ints, the tops (node, -1: no list for the top state... see ref_tops)"""
    rec = []
    for p in order:
        w, stick = ref_weight_stick(pb, p, m, ss, hs)
        rec += [int(p), w] + stick_words(stick)
        for t in range(pb["M"]):
            l = get_list(pb, "live", p, t)
            nodes = [] if l is None else l[1]
            rec += [len(nodes) | (int(pb["live_kind"][p, t]) << 16)] + nodes + [-1] * (pb["L"] - len(nodes))
    return rec


def ref_tops(pb, top_state, order):
    """Per step: its top priority node, -1 (no list for the top state) or -2 (an empty one) -- kcase_flat_row_count's input."""
    tops = []
    for p in order:
        l = get_list(pb, "live", p, top_state)
        tops.append(-1 if l is None else (l[1][0] if l[1] else -2))
    return tops


def ref_row_count(tops, NX):
    rows = [0] * (NX + 1)
    for x in tops:
        rows[x if x >= 0 else NX] += 1
    return rows


def _perm(P, *seed):
    return [int(x) for x in _rng(42, P, *seed).permutation(P)]


def run_gather(kc, pb, m, top_state, order, ss, hs, what):
    """With and without row_count: records word for word, the guards, the rows; the problem untouched."""
    want = ref_gather(pb, m, order, ss, hs)
    tops = ref_tops(pb, top_state, order)
    want_rows = ref_row_count(tops, pb["NX"])
    for with_rows in (1, 0):
        rc, q, rec, rows = kc.gather(pb, m, top_state, order, ss, hs, with_rows)
        got = [int(x) for x in rec[:-1]]
        if got != want:
            bad = [i for i in range(len(want)) if got[i] != want[i]]
            RW = REC_HEAD + pb["M"] * (1 + pb["L"])
            raise AssertionError("%s: %d record words differ, first at step %d word %d: %d, not %d" %
                                 (what, len(bad), bad[0] // RW, bad[0] % RW, got[bad[0]], want[bad[0]]))
        assert int(rec[-1]) == GUARD, what
        assert [int(x) for x in rows[:-1]] == (want_rows if with_rows else [0] * (pb["NX"] + 1)), (what, with_rows)
        assert int(rows[-1]) == GUARD, what
        assert_problem(q, pb, what, lists_whole=True)
    return tops, want_rows


GATHER_SHAPES = [(1, 1), (2, 1), (3, 2), (4, 3), (2, 5)]           # RW 6, 8, 13, 20, 16: odd and even (the LDS stride is RW | 1)
GATHER_WIDE = [(1, 58), (4, 14), (2, 29), (10, 5)]                 # RW 63, then 64 three ways: the widest blance_validate admits
GATHER_WIDE_P = [1, 256, 257]


def gather_problem(P, M, L, seed):
    """Random lists with stale absent ones; partitions 4 t + v force state t to be full, empty, nil and absent."""
    NX = 9
    pb = random_problem(P, M, L, NX - 2, NX, seed, stale=True)
    for t in range(M):
        for v in range(4):
            p = 4 * t + v
            if p < P:
                nodes = [(p + j) % NX for j in range(L)]
                if v == 0:
                    set_list(pb, "live", p, t, nodes)
                elif v == 1:
                    set_list(pb, "live", p, t, [])
                elif v == 2:
                    set_list(pb, "live", p, t, [], LIST_NIL)
                else:
                    set_list(pb, "live", p, t, nodes, LIST_ABSENT)
    return pb


def gather_states_covered(pb, t):
    """which of full / empty / nil / absent state t's list is somewhere in the problem"""
    seen = set()
    for p in range(pb["P"]):
        l = get_list(pb, "live", p, t)
        seen.add("absent" if l is None else "nil" if l[0] else "full" if len(l[1]) == pb["L"] else "empty" if not l[1] else "some")
    return seen


def check_gather_geometry(kc, P):
    for M, L in GATHER_SHAPES:
        pb = gather_problem(P, M, L, 3)
        if P >= 4 * M:
            for t in range(M):
                assert {"full", "empty", "nil", "absent"} <= gather_states_covered(pb, t), (M, L, t)
        order = _perm(P, M, L)
        ss, hs = [7 + t for t in range(M)], [t & 1 for t in range(M)]
        run_gather(kc, pb, M - 1, 0, order, ss, hs, "k_gather P %d M %d L %d" % (P, M, L))


def check_gather_wide(kc, M, L, P):
    """The widest records: at RW = 64 a workgroup of 256 stages 66,624 bytes of LDS."""
    pb = gather_problem(P, M, L, 4)
    for p in range(0, P, 3):                         # and many lists full to the last slot
        for t in range(M):
            set_list(pb, "live", p, t, [int(x) for x in _rng(43, p, t).choice(9, size=min(L, 9), replace=False)] +
                     [(p + t + j) % 9 for j in range(max(0, L - 9))])
    order = _perm(P, M, L, 1)
    run_gather(kc, pb, M - 1, 0, order, [5] * M, [1] * M, "k_gather RW %d P %d" % (REC_HEAD + M * (1 + L), P))


def check_gather_header(kc):
    """Weight and stickiness: from the partition's weight (positive, zero, negative), from the state's stickiness, the 1.5
    default, and weights_nil over all of them."""
    P, M, L, m = 70, 2, 2, 1
    base = gather_problem(P, M, L, 5)
    base["part_has_weight"][:] = 0
    for p, w in [(0, 3), (1, 0), (2, -4), (63, 9), (64, 1), (69, -1)]:
        base["part_has_weight"][p], base["part_weight"][p] = 1, w
    base["part_weight"][5] = 1234                     # a weight the partition does not have
    order = list(range(P))
    seen = set()
    for weights_nil, hs in [(0, [1, 1]), (0, [1, 0]), (1, [1, 1])]:
        pb = dict(base, weights_nil=weights_nil)
        ss = [11, 6]
        run_gather(kc, pb, m, 0, order, ss, hs, "k_gather header weights_nil %d has_stick %s" % (weights_nil, hs))
        for p in (0, 1, 2, 5):
            seen.add(ref_weight_stick(pb, p, m, ss, hs))
    # each outcome shows in a compared word: (weight, stickiness) of partitions 0, 1, 2 and 5 over the three runs
    assert seen == {(3, 3.0), (0, 0.0), (-4, -4.0), (1, 6.0), (1, 1.5)}


def check_gather_row_count(kc, P):
    """row_count equals k_flat_row_count's for the same tops, the "" row included; steps without a top priority node at
    lanes 0 and 63, in a last partial wave, and nowhere at all."""
    NX = 5
    for holes in T.ROW_COUNT_HOLES:
        r = _rng(44, P, T.ROW_COUNT_HOLES.index(holes))
        top = [int(x) for x in r.integers(0, NX, P)]
        if holes == "lane_0":
            top[0::64] = [-1] * len(top[0::64])
        elif holes == "lane_63":
            top[63::64] = [-2] * len(top[63::64])
            top[0] = -1 if P == 1 else top[0]
        elif holes == "last_wave":
            top[P - 1] = -1
            top[((P - 1) // 64) * 64] = -2
        elif holes == "many":
            top = [(-1 if x == 0 else -2 if x == 1 else x) for x in top]
        order = _perm(P, 7)
        pb = blank_problem(P, 2, 2, NX, NX, 6)
        for oi, p in enumerate(order):
            set_list(pb, "live", p, 0, [1, 2])
            if top[oi] >= 0:
                set_list(pb, "live", p, 1, [top[oi], (top[oi] + 1) % NX])
            elif top[oi] == -2:
                set_list(pb, "live", p, 1, [], LIST_NIL if oi & 1 else LIST_SET)
            else:
                set_list(pb, "live", p, 1, [3], LIST_ABSENT)
        tops, rows = run_gather(kc, pb, 0, 1, order, [0, 0], [0, 0], "k_gather rows P %d %s" % (P, holes))
        assert tops == top
        rc, flat_rows = kc.flat_row_count(top, NX)
        assert [int(x) for x in flat_rows] == rows, (P, holes)
        assert rows[NX] == sum(1 for x in top if x < 0) and (holes != "nowhere" or rows[NX] == 0)
        assert holes not in ("lane_0", "last_wave") or rows[NX] > 0


# ---- 6. k_ntn_bits ----------------------------------------------------------------------------------------------------------

BITS_N = [1, 63, 64, 65, 127, 128, 129, 4031, 4095, 4096]
BITS_ROWS = [1, 3, 4, 5, 9]
BITS_KINDS = ["zero", "nonzero", "col_0", "col_63", "col_64", "col_last", "negative", "random"]


def bits_matrix(N, rows, kind, seed):
    r = _rng(45, N, rows, seed)
    a = np.zeros((rows, N), np.int64)
    if kind == "nonzero":
        a = r.integers(1, 9, (rows, N))
    elif kind.startswith("col_"):
        col = N - 1 if kind == "col_last" else int(kind[4:])
        if col >= N:
            return None
        a[rows - 1, col] = 7
    elif kind == "negative":
        a = -(r.integers(0, 3, (rows, N)) == 0).astype(np.int64) * r.integers(1, 2 ** 31, (rows, N))
    elif kind == "random":
        a = r.integers(0, 4, (rows, N)) * (r.integers(0, 3, (rows, N)) == 0)
    if kind in ("negative", "random"):               # (never all zero, however small)
        a[0, N - 1] = -5 if kind == "negative" else 2
    return a


def ref_bits(a, BW):
    out = []
    for row in a.tolist():
        v = sum(1 << i for i, x in enumerate(row) if x != 0)         # the row as one long integer, bit i = column i
        out += [(v >> (32 * w)) & 0xFFFFFFFF for w in range(BW)]
    return out


def check_ntn_bits(kc, N):
    for NX in (N, N + 1, N + 70):
        if NX > 4096:
            continue
        BW = kc.ntn_bits_words(NX)
        assert BW >= 1 and 32 * BW >= NX and BW <= 128
        for rows in BITS_ROWS:
            if rows > NX + 1:
                continue
            for ki, kind in enumerate(BITS_KINDS):
                a = bits_matrix(N, rows, kind, NX)
                if a is None:
                    continue
                want = ref_bits(a, BW)
                assert kind in ("zero",) or any(want)
                rc, bits = kc.ntn_bits(N, NX, rows, a.ravel(), BW)
                assert [int(x) for x in bits[:-1]] == want, (N, NX, rows, kind)
                assert int(bits[-1]) == GUARD, (N, NX, rows, kind)


# ---- k_invert ---------------------------------------------------------------------------------------------------------------

def check_invert(kc, n):
    for perm in (list(range(n)), list(range(n - 1, -1, -1)), _perm(n, 9)):
        rc, inv = kc.invert(perm)
        want = [0] * n
        for i, x in enumerate(perm):
            want[x] = i
        assert [int(x) for x in inv[:-1]] == want
        assert int(inv[-1]) == GUARD


# ---- 7. the sweep's end -----------------------------------------------------------------------------------------------------

def ref_apply_step(pb, m, p, nil, chosen):
    """plan.go:290-299 on partition p: pb is edited in place (lists as get_list / set_list see them)"""
    old = get_list(pb, "live", p, m)
    gone = set(chosen) | set(old[1] if old else [])
    for t in range(pb["M"]):
        l = get_list(pb, "live", p, t)
        if t == m or l is None:
            continue
        keep = [x for x in l[1] if x not in gone]
        pb["live_len"][p, t] = 0
        set_list(pb, "live", p, t, keep)
    pb["live_len"][p, m] = 0
    set_list(pb, "live", p, m, list(chosen), LIST_NIL if nil else LIST_SET)


def ref_differs(pb, p):
    if not pb["in_prev"][p] or pb["never_equal"][p]:
        return True
    return any(get_list(pb, "live", p, t) != get_list(pb, "prv", p, t) for t in range(pb["M"]))


def ref_sweep_end(pb, m, order, out, apply, converge, count, refresh, word, closed):
    """-> the problem afterwards, the not_match word, cnt_next[M NX]"""
    q = copy.deepcopy(pb)
    cnt = [0] * (pb["M"] * pb["NX"])
    if closed:
        return q, word, cnt
    if apply:
        for oi, p in enumerate(order):
            o = [int(x) for x in out[oi]]
            ref_apply_step(q, m, p, o[0] >> 16, o[1:1 + (o[0] & 0xffff)])
    if converge:
        for p in range(q["P"]):
            if ref_differs(q, p):
                word = 1 if word == 0 else word
            for t in range(q["M"]):
                l = get_list(q, "live", p, t)
                q["prv_kind"][p, t] = q["live_kind"][p, t]
                q["prv_len"][p, t] = q["live_len"][p, t]
                if l is not None:
                    q["prv"][p, t, :len(l[1])] = l[1]
            q["in_prev"][p], q["never_equal"][p] = 1, 0
    if count:
        for p in range(q["P"]):
            if q["in_prev"][p]:
                for t in range(q["M"]):
                    for x in (get_list(q, "prv", p, t) or (0, []))[1]:
                        cnt[t * q["NX"] + x] += part_w(q, p)
    if refresh:
        q["live_kind"][q["live_kind"] != LIST_ABSENT] = LIST_SET
    return q, word, cnt


def out_rows(P, OW, order, choices):
    """choices[p] = (nil, nodes) -> out[P OW] in pass order; unused words hold a valid node id"""
    out = np.full((P, OW), 1, np.int32)
    for oi, p in enumerate(order):
        nil, nodes = choices[p]
        out[oi, 0] = len(nodes) | (int(nil) << 16)
        out[oi, 1:1 + len(nodes)] = nodes
    return out


END_M, END_L, END_NX, END_STATE = 3, 3, 40, 1


def run_sweep_end(kc, pb, order, choices, word, what, gate=None):
    """Every mode over one scenario; the fused tail's arrays equal the unfused sequence's and the reference's.
    -> the reference's word after a full tail."""
    m, OW = END_STATE, 1 + pb["L"]
    out = out_rows(pb["P"], OW, order, choices)
    gate_words, gate_mask, closed = (None, 0, False) if gate is None else gate
    full_word = None
    #            mode, with_out, with_cnt | apply, converge, count, refresh
    plans = [(0, 1, 1, 1, 1, 1, 1), (0, 1, 0, 1, 1, 0, 0), (0, 0, 1, 0, 1, 1, 1), (0, 0, 0, 0, 1, 0, 0),
             (1, 1, 1, 1, 1, 1, 1), (1, 0, 1, 0, 1, 1, 1), (2, 1, 0, 1, 0, 0, 0), (3, 1, 0, 1, 1, 0, 0), (3, 0, 0, 0, 1, 0, 0)]
    got_by_plan = {}
    for mode, with_out, with_cnt, apply, converge, count, refresh in plans:
        want, want_word, want_cnt = ref_sweep_end(pb, m, order, out, apply, converge, count, refresh, word, closed)
        rc, q, words, cnt = kc.sweep_end(pb, mode, m, order, out, with_out, with_cnt, word, gate_words, gate_mask)
        tag = "%s: mode %d out %d cnt %d" % (what, mode, with_out, with_cnt)
        assert_problem(q, want, tag, lists_whole=closed)
        assert [int(x) for x in words] == [T.SENTINEL_A, want_word, T.SENTINEL_B], tag
        assert [int(x) for x in cnt[:-1]] == want_cnt, tag
        assert int(cnt[-1]) == GUARD, tag
        got_by_plan[(mode, with_out, with_cnt)] = (q, [int(x) for x in words], [int(x) for x in cnt])
        if (mode, with_out, with_cnt) == (0, 1, 1):
            full_word = want_word
    for out_on in (1, 0):                            # fused against unfused, array for array (beyond what the reference compares)
        a, b = got_by_plan[(0, out_on, 1)], got_by_plan[(1, out_on, 1)]
        for k in _PB_ARRAYS:
            assert np.array_equal(a[0][k], b[0][k]), (what, "fused / unfused", k)
        assert a[1:] == b[1:], (what, "fused / unfused words, counters")
    return full_word


def calm_world(P, seed, weights=True):
    """Every partition equal to its prevMap entry, its step choosing what it holds: nothing changes, nothing differs."""
    pb = blank_problem(P, END_M, END_L, END_NX, END_NX, seed)
    r = _rng(46, P, seed)
    choices = {}
    for p in range(P):
        nodes = [int(x) for x in r.choice(END_NX - 10, size=4, replace=False)]
        for t, l in enumerate([nodes[:1], nodes[1:3], nodes[3:]]):
            set_list(pb, "live", p, t, l)
            set_list(pb, "prv", p, t, l)
        choices[p] = (0, nodes[1:3])
    if weights:
        pb["part_has_weight"] = (r.integers(0, 3, P) > 0).astype(np.uint8)
        pb["part_weight"] = r.integers(-3, 7, P).astype(np.int32)
    return pb, choices


A, B, C, D, E = 30, 31, 32, 33, 34                   # nodes no calm partition holds

# name -> (live lists, prevMap lists, in_prev, never_equal, choice); a list: None absent, "nil", or nodes.  Each differs from
# its prevMap entry in exactly the way named, whether or not the step's choice (which changes nothing) is applied.
DIFF_CASES = {
    "kind_only": ({0: [A], 1: "nil", 2: [B]}, {0: [A], 1: [], 2: [B]}, 1, 0, (1, [])),
    "length_only": ({0: [A], 1: [B, C], 2: [D]}, {0: [A], 1: [B, C, E], 2: [D]}, 1, 0, (0, [B, C])),
    "last_element": ({0: [A], 1: [B, C, D], 2: None}, {0: [A], 1: [B, C, E], 2: None}, 1, 0, (0, [B, C, D])),
    "last_element_last_state": ({0: [A], 1: [B], 2: [C, D, E]}, {0: [A], 1: [B], 2: [C, D, A]}, 1, 0, (0, [B])),
    "absent_against_nil": ({0: [A], 1: [B], 2: None}, {0: [A], 1: [B], 2: "nil"}, 1, 0, (0, [B])),
    "not_in_prev": ({0: [A], 1: [B], 2: [C]}, {0: [A], 1: [B], 2: [C]}, 0, 0, (0, [B])),
    "never_equal": ({0: [A], 1: [B], 2: [C]}, {0: [A], 1: [B], 2: [C]}, 1, 1, (0, [B])),
}
# list edits: name -> (live lists, choice, live lists afterwards); prevMap = the live lists before
EDIT_CASES = {
    "none_chosen_nil": ({0: [A], 1: [B], 2: [C]}, (1, []), {0: [A], 1: "nil", 2: [C]}),
    "none_chosen_set": ({0: [A], 1: [B], 2: [C]}, (0, []), {0: [A], 1: [], 2: [C]}),
    "all_slots_chosen": ({0: [A], 1: [B], 2: [C]}, (0, [D, E, B]), {0: [A], 1: [D, E, B], 2: [C]}),
    "chosen_leaves_other_state": ({0: [A, D], 1: [B], 2: [C, E, D]}, (0, [D]), {0: [A], 1: [D], 2: [C, E]}),
    "old_leaves_other_state": ({0: [B, A], 1: [B], 2: [C, B]}, (0, [D]), {0: [A], 1: [D], 2: [C]}),
    "other_nil_becomes_set": ({0: "nil", 1: [B], 2: [C]}, (0, [D]), {0: [], 1: [D], 2: [C]}),
    "other_absent_stays": ({0: None, 1: [B], 2: [C]}, (0, [D]), {0: None, 1: [D], 2: [C]}),
    "state_absent_becomes_set": ({0: [A], 1: None, 2: [C]}, (0, [D]), {0: [A], 1: [D], 2: [C]}),
    "nothing_changes": ({0: [A], 1: [B, C], 2: [D]}, (0, [B, C]), {0: [A], 1: [B, C], 2: [D]}),
}


def put_lists(pb, which, p, lists):
    for t, l in lists.items():
        pb[which + "_len"][p, t] = 0
        if l is None:
            set_list(pb, which, p, t, [], LIST_ABSENT)
        elif l == "nil":
            set_list(pb, which, p, t, [], LIST_NIL)
        else:
            set_list(pb, which, p, t, l)


def lists_of(pb, which, p):
    out = {}
    for t in range(pb["M"]):
        l = get_list(pb, which, p, t)
        out[t] = None if l is None else "nil" if l[0] else l[1]
    return out


def put_diff_case(pb, choices, p, name):
    live, prv, in_prev, never, choice = DIFF_CASES[name]
    put_lists(pb, "live", p, live)
    put_lists(pb, "prv", p, prv)
    pb["in_prev"][p], pb["never_equal"][p] = in_prev, never
    choices[p] = choice


def check_converge_case(kc, name):
    """One partition differs from prevMap in exactly one way, alone among calm ones (check_converge_all_equal: the same world without it)."""
    P, p = 65, 5
    pb, choices = calm_world(P, 1)
    order = _perm(P, 11)
    put_diff_case(pb, choices, p, name)
    assert ref_differs(pb, p) and sum(ref_differs(pb, x) for x in range(P)) == 1
    assert run_sweep_end(kc, pb, order, choices, 0, name) == 1


CONVERGE_SEAMS = [(64, 0), (64, 63), (257, 256), (257, 255), (257, 64), (1, 0)]


def check_converge_seam(kc, P, p):
    """The single differing partition at a chosen lane: lane 0, lane 63, and p = 256 of 257, whose wave has no other lane
    in range."""
    pb, choices = calm_world(P, 2)
    put_diff_case(pb, choices, p, "last_element")
    order = _perm(P, 12)
    assert run_sweep_end(kc, pb, order, choices, 0, "differs at %d of %d" % (p, P)) == 1


def check_converge_all_equal(kc):
    pb, choices = calm_world(65, 1)
    assert run_sweep_end(kc, pb, _perm(65, 11), choices, 0, "all equal") == 0


def check_converge_word_set_on_entry(kc):
    pb, choices = calm_world(65, 3)
    order = _perm(65, 13)
    assert run_sweep_end(kc, pb, order, choices, 1, "word 1 on entry, all equal") == 1
    put_diff_case(pb, choices, 7, "length_only")
    assert run_sweep_end(kc, pb, order, choices, 1, "word 1 on entry, one differs") == 1


def edit_world():
    names = sorted(EDIT_CASES)
    P = 70
    pb, choices = calm_world(P, 4)
    at = {}
    for i, name in enumerate(names):
        p = [0, 1, 31, 62, 63, 64, 65, 68, 69][i]
        live, choice, after = EDIT_CASES[name]
        put_lists(pb, "live", p, live)
        put_lists(pb, "prv", p, live)
        choices[p] = choice
        at[name] = p
    return pb, choices, at


def check_list_edits(kc):
    pb, choices, at = edit_world()
    order = _perm(pb["P"], 14)
    out = out_rows(pb["P"], 1 + END_L, order, choices)
    want, _, _ = ref_sweep_end(pb, END_STATE, order, out, 1, 0, 0, 0, 0, False)
    for name, p in at.items():                       # the table says what it means, on the reference
        assert lists_of(want, "live", p) == EDIT_CASES[name][2], name
    run_sweep_end(kc, pb, order, choices, 0, "list edits")


def check_sweep_end_geometry(kc, P):
    """Random partitions of every kind (an absent or nil list is empty, as in the product), weights of both signs, random
    choices; with weights_nil on the odd sizes."""
    pb = random_problem(P, END_M, END_L, END_NX - 4, END_NX, 7, weights_nil=P & 1)
    r = _rng(47, P)
    choices = {}
    for p in range(P):
        n = int(r.integers(0, END_L + 1))
        nodes = [int(x) for x in r.choice(END_NX, size=n, replace=False)]
        choices[p] = (int(r.integers(0, 4) == 0) if n == 0 else 0, nodes)
    order = _perm(P, 15)
    run_sweep_end(kc, pb, order, choices, 0, "random P %d" % P)
    if P >= 63:
        w = {part_w(pb, p) for p in range(P)}
        assert (w == {1}) if P & 1 else (min(w) < 0 and 0 in w and max(w) > 1)


def check_sweep_end_gate(kc):
    """A closed Gate: nothing at all is written, the counter buffer included; an open one with other words set runs."""
    pb, choices, at = edit_world()
    put_diff_case(pb, choices, 10, "last_element")
    order = _perm(pb["P"], 16)
    gw = np.zeros(GATE_WORDS, np.int32)
    gw[7] = 1
    assert run_sweep_end(kc, pb, order, choices, 0, "closed Gate", (gw, (1 << 7) | (1 << 0), True)) == 0
    assert run_sweep_end(kc, pb, order, choices, 0, "open Gate", (gw, (1 << 6) | (1 << 0), False)) == 1


# ---- refusals ---------------------------------------------------------------------------------------------------------------

def check_sweep_refusals(kc):
    """Whatever a kernel would index with is checked first: kCaseBadArg, no launch, the outputs as the caller filled them."""
    FILL = 0x3C
    pb, choices = calm_world(10, 5)
    order = list(range(10))
    out = out_rows(10, 1 + END_L, order, choices)

    def broken(how):
        q = copy.deepcopy(pb)
        if how == "node":
            q["live"][4, 1, 0] = END_NX
        elif how == "prv_node":
            q["prv"][4, 1, 0] = -1
        elif how == "long":
            q["live_len"][3, 0] = END_L + 1
        elif how == "kind":
            q["prv_kind"][3, 0] = 3
        return q

    for how in ("node", "prv_node", "long", "kind"):
        q = broken(how)
        rc, _, cat = kc.category(q, 0, 1, 0, check=False, fill=FILL)
        assert rc == BAD_ARG and (cat == FILL).all(), how
        rc, _, rec, rows = kc.gather(q, 0, 0, order, [0] * END_M, [0] * END_M, 1, check=False, fill=FILL)
        assert rc == BAD_ARG and (rec == FILL).all() and (rows == FILL).all(), how
        rc, q2, words, cnt = kc.sweep_end(q, 0, END_STATE, order, out, 1, 1, 0, check=False)
        assert rc == BAD_ARG and words[1] == 0 and (cnt == CNT_FILL).all(), how
        assert_problem(q2, q, how, lists_whole=True)
    rc, _, cat = kc.category(pb, END_M, 1, 0, check=False, fill=FILL)
    assert rc == BAD_ARG and (cat == FILL).all()
    for bad_order in ([0] * 10, list(range(1, 11)), [-1] + list(range(1, 10))):
        if bad_order != [0] * 10:                    # (k_gather takes any partition ids below P)
            rc, _, rec, rows = kc.gather(pb, 0, 0, bad_order, [0] * END_M, [0] * END_M, 1, check=False, fill=FILL)
            assert rc == BAD_ARG and (rec == FILL).all()
        rc, _, words, cnt = kc.sweep_end(pb, 0, END_STATE, bad_order, out, 1, 1, 0, check=False)
        assert rc == BAD_ARG and (cnt == CNT_FILL).all()
        rc, inv = kc.invert(bad_order, check=False, fill=FILL)
        assert rc == BAD_ARG and (inv == FILL).all()
    for bad in ("node", "count", "nil"):
        o = out.copy()
        if bad == "node":
            o[2, 1] = END_NX
        elif bad == "count":
            o[2, 0] = END_L + 1
        else:
            o[2, 0] |= 2 << 16
        for mode in (0, 1, 2, 3):
            rc, _, words, cnt = kc.sweep_end(pb, mode, END_STATE, order, o, 1, 1, 0, check=False)
            assert rc == BAD_ARG and (cnt == CNT_FILL).all(), (bad, mode)
    wide = blank_problem(2, 4, 15, 5, 5, 1)          # RW = 68: wider than validation admits
    rc, _, rec, rows = kc.gather(wide, 0, 0, [0, 1], [0] * 4, [0] * 4, 1, check=False, fill=FILL)
    assert rc == BAD_ARG and (rec == FILL).all()
    for N, NX, rows in [(5, 4, 1), (4097, 4097, 1), (5, 5, 7), (5, 5, 0)]:
        rc, bits = kc.ntn_bits(N, NX, rows, np.zeros(max(rows, 1) * N), 1, check=False, fill=FILL)
        assert rc == BAD_ARG and (bits == FILL).all(), (N, NX, rows)


# ---- 2. to 4. region chains: k_chain_classify, k_chain_ev_fill, k_chain_orphans, k_gather_chain ------------------------------

CW, C_OWN, C_HIGH, C_LOW, C_LOW_STATE = 24, 7, 11, 15, 19          # kCW, kCOwn, kCHigh, kCLow, kCLowState
CHAIN_OWN, CHAIN_HIGH, CHAIN_LOW = 4, 4, 4                          # kChainOwn, kChainHigh, kChainLow
FLAG_NOT_LOCAL, FLAG_ORPHANS, FLAG_EVENTS = 0, 6, 7                 # kFlagNotLocal, kFlagOrphans, kFlagEvents


class ChainCases(SweepCases):
    def __init__(self, path):
        super().__init__(path)
        vp, ci, cu = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint
        for name, args in {
            "kcase_chain_events": [vp, ci, ci, vp, vp, vp, vp, ci, ci, vp, cu, ci, vp, vp, ci, vp, vp, vp, vp, vp, vp],
            "kcase_gather_chain": [vp, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, vp, cu, ci, vp, vp],
        }.items():
            f = getattr(self.lib, name)
            f.argtypes, f.restype = args, ci

    def chain_events(self, pb, R, m, top_state, order, flags0, gate_mask, stage, ev_cap, cnt=None, check=True, fill=0):
        """stage 0: k_chain_classify; 1: + the scan of n_ev and k_chain_ev_fill, as ChainPass::events launches them (only when
        no step is NotLocal and some event was flagged); cnt given: k_chain_orphans on it.
        -> rc, problem, flags[GATE_WORDS + 1], regid[P + 1], n_ev[P + 2], n_events, (ev_key, ev_oi, ev_leaf, ev_w)[ev_cap + 1], cnt"""
        c, q = _cproblem(pb)
        P = pb["P"]
        flags = _i32(list(flags0) + [GUARD])
        regid, n_ev, n_events = np.full(P + 1, fill, np.int32), np.full(P + 2, fill, np.int32), np.full(1, fill, np.int32)
        ev = [np.full(ev_cap + 1, fill, np.int32) for _ in range(4)]
        cnt = None if cnt is None else _i32(list(cnt) + [GUARD])
        self.calls += 1
        rc = self._ok(self.lib.kcase_chain_events(ctypes.addressof(c), m, top_state, _p(_i32(order)), _p(_i32(R["node_region"])),
                                                  _p(_i32(R["node_leaf_pos"])), _p(_i32(R["reg_lo"])), len(R["reg_lo"]), R["n_leaves"],
                                                  _p(flags), gate_mask, stage, _p(regid), _p(n_ev), ev_cap, _p(n_events), _p(ev[0]),
                                                  _p(ev[1]), _p(ev[2]), _p(ev[3]), _p(cnt)), check)
        return rc, q, flags, regid, n_ev, int(n_events[0]), ev, cnt

    def gather_chain(self, pb, R, m, top_state, higher_mask, order, chain_oi, ss, hs, flat, classify, flags0, gate_mask, with_topkey,
                     check=True, fill=0):
        """-> rc, problem, crec[P CW + 1], flags[GATE_WORDS + 1], topkey[P + 1]"""
        c, q = _cproblem(pb)
        P = pb["P"]
        flags = _i32(list(flags0) + [GUARD])
        crec, topkey = np.full(P * CW + 1, fill, np.int32), np.full(P + 1, fill, np.int32)
        oi = None if chain_oi is None else _i32(chain_oi)
        self.calls += 1
        rc = self._ok(self.lib.kcase_gather_chain(ctypes.addressof(c), m, top_state, higher_mask, _p(_i32(order)), _p(oi), _p(_i32(ss)),
                                                  _p(_u8(hs)), _p(_i32(R["node_region"])), _p(_i32(R["node_leaf_pos"])),
                                                  _p(_i32(R["reg_lo"])), _p(_i32(R["leaf_cls"])), _p(_i32(R["cls_size"])),
                                                  len(R["reg_lo"]), R["n_leaves"], flat, classify, _p(flags), gate_mask, int(with_topkey),
                                                  _p(crec), _p(topkey)), check)
        return rc, q, crec, flags, topkey


# Three regions of 5, 1 and 8 leaves; node x < 14 sits at leaf 13 - x, nodes 14 .. 19 lie in no region.  Exclude classes: leaf 0
# alone (region 0), leaves 6, 7, 8 together and leaf 9 alone (region 2).
CH_NX, CH_M, CH_L, CH_STATE, CH_TOP, CH_MASK = 20, 4, 6, 1, 0, 0b0001      # state 0 has priority over state 1; 2 and 3 come after it
REG_LO, REG_SIZE = [0, 5, 6], [5, 1, 8]


def chain_regions():
    n_leaves = 14
    leaf_region = [0] * 5 + [1] + [2] * 8
    node_leaf = [13 - x if x < 14 else 0 for x in range(CH_NX)]
    leaf_cls, cls_size = [-1] * n_leaves, [0] * n_leaves
    leaf_cls[0] = 0
    cls_size[0 + 0] = 1
    for lp in (6, 7, 8):
        leaf_cls[lp] = 0
    leaf_cls[9] = 1
    cls_size[6 + 0], cls_size[6 + 1] = 3, 1
    return dict(node_region=[leaf_region[13 - x] if x < 14 else -1 for x in range(CH_NX)], node_leaf_pos=node_leaf, reg_lo=list(REG_LO),
                n_leaves=n_leaves, leaf_cls=leaf_cls, cls_size=cls_size)


def flat_regions(NX):
    """What the flat single chain passes: every node in region 0 at leaf = node id, no class."""
    return dict(node_region=[0] * NX, node_leaf_pos=list(range(NX)), reg_lo=[0], n_leaves=NX, leaf_cls=list(range(NX)), cls_size=[1] * NX)


def node_at(leaf):
    return 13 - leaf


def ref_top(pb, p, top_state):
    l = get_list(pb, "live", p, top_state)
    return l[1][0] if l and l[1] else None


def ref_classify(pb, R, m, top_state, order):
    """-> regid[P], n_ev[P + 1], the flag words raised, the event rows (key, oi, leaf, w) in pass order"""
    regid, n_ev, raised, events = [], [], set(), []
    for oi, p in enumerate(order):
        top = ref_top(pb, p, top_state)
        rg = R["node_region"][top] if top is not None else -1
        ne = 0
        if rg < 0:
            raised.add(FLAG_NOT_LOCAL)
            rg = 0
        else:
            for x in (get_list(pb, "live", p, m) or (0, []))[1]:
                r2 = R["node_region"][x]
                if r2 == rg:
                    continue
                raised.add(FLAG_EVENTS)
                if r2 < 0:
                    raised.add(FLAG_ORPHANS)
                else:
                    ne += 1
                    events.append((r2, oi, R["node_leaf_pos"][x] - R["reg_lo"][r2], part_w(pb, p)))
        regid.append(rg)
        n_ev.append(ne)
    return regid, n_ev + [0], raised, events


def ref_orphans(pb, R, m, cnt):
    cnt = list(cnt)
    for p in range(pb["P"]):
        for x in (get_list(pb, "live", p, m) or (0, []))[1]:
            if R["node_region"][x] < 0:
                cnt[m * pb["NX"] + x] -= part_w(pb, p)
    return cnt


def ref_chain_record(pb, R, m, top_state, higher_mask, p, oi, ss, hs, flat, classify):
    """-> (the record's CW words or, for a step the compact record cannot hold, its four header words; the flag words it
    raises; its top key).  blance_kernels.h has the layout."""
    NX, M = pb["NX"], pb["M"]
    region, leaf = R["node_region"], R["node_leaf_pos"]
    w, stick = ref_weight_stick(pb, p, m, ss, hs)
    r = [-1] * CW
    r[0:4] = [oi, w] + stick_words(stick)
    top = ref_top(pb, p, top_state)
    rg = 0 if flat else (region[top] if top is not None else -1)
    if rg < 0:                                       # blanked: no region, nothing to hold
        r[4], r[5], r[6] = 0, 0, -1
        return r, {FLAG_NOT_LOCAL}, 0
    lo = R["reg_lo"][rg]
    if flat:
        r[4], r[6], r[23] = (top if top is not None else NX), -1, 0
    else:
        r[4] = leaf[top] - lo
        r[6] = R["leaf_cls"][leaf[top]]
        r[23] = R["cls_size"][lo + r[6]] if r[6] >= 0 else 0
    raised, fits = set(), True
    own = get_list(pb, "live", p, m)
    own_nodes = own[1] if own else []
    if classify:                                     # k_chain_classify's two words, for every node of the list
        for x in own_nodes:
            if region[x] != rg:
                raised.add(FLAG_EVENTS)
                if region[x] < 0:
                    raised.add(FLAG_ORPHANS)
    if len(own_nodes) > CHAIN_OWN:
        fits = False
    inside = [leaf[x] - lo for x in own_nodes if region[x] == rg]
    remote = any(region[x] != rg for x in own_nodes)
    high, low = [], []
    for t in range(M):
        l = get_list(pb, "live", p, t)
        if t == m or l is None:
            continue
        for x in l[1]:
            if x in own_nodes:
                fits = False                         # a node held in two states
            if region[x] != rg:
                continue
            if (higher_mask >> t) & 1:
                if r[6] >= 0 and R["leaf_cls"][leaf[x]] == r[6]:
                    continue                         # inside the top priority node's exclude class: excluded anyway
                high.append(leaf[x] - lo)
            else:
                low.append((leaf[x] - lo, t))
    if len(high) > CHAIN_HIGH or len(low) > CHAIN_LOW:
        fits = False
    if not fits:
        return r[:4], raised | {FLAG_NOT_LOCAL}, (0 if flat else lo + r[4])
    r[C_OWN:C_OWN + len(inside)] = inside
    r[C_HIGH:C_HIGH + len(high)] = high
    r[C_LOW:C_LOW + len(low)] = [x for x, _ in low]
    r[C_LOW_STATE:C_LOW_STATE + len(low)] = [t for _, t in low]
    r[5] = len(inside) | (len(high) << 8) | (len(low) << 16) | ((1 if own else 0) << 24) | ((1 if remote else 0) << 25)
    return r, raised, (0 if flat else lo + r[4])


# ---- the tables: a step is {state: list}, placed among filler steps

def chain_filler(i):
    """A calm step of region 2: top priority node, one own node, one lower node, all inside the region, no class involved."""
    return {0: [node_at(10 + i % 4)], 1: [node_at(10 + (i + 1) % 4)], 2: [node_at(10 + (i + 2) % 4)], 3: None}


T2 = node_at(11)                                     # a top priority node of region 2 without an exclude class
TC = node_at(6)                                      # one inside the class of leaves 6, 7, 8
ORPH, ORPH2 = 15, 17                                 # nodes in no region
# name -> lists (state -> nodes, None absent, "nil")
CHAIN_STEPS = {
    "own_0": {0: [T2], 1: [], 2: [node_at(12)]},
    "own_1": {0: [T2], 1: [node_at(12)], 2: []},
    "own_4": {0: [T2], 1: [node_at(12), node_at(13), node_at(10), node_at(9)], 2: []},
    "own_5": {0: [T2], 1: [node_at(12), node_at(13), node_at(10), node_at(9), node_at(8)], 2: []},
    "own_5th_remote": {0: [T2], 1: [node_at(12), node_at(13), node_at(10), node_at(9), node_at(2)], 2: []},
    "own_5th_orphan": {0: [T2], 1: [node_at(12), node_at(13), node_at(10), node_at(9), ORPH], 2: []},
    # (a node behind the fifth: only a gather that classifies walks on to it)
    "own_6th_remote": {0: [T2], 1: [node_at(12), node_at(13), node_at(10), node_at(9), node_at(8), node_at(2)], 2: []},
    "own_6th_orphan": {0: [T2], 1: [node_at(12), node_at(13), node_at(10), node_at(9), node_at(8), ORPH], 2: []},
    "high_0": {0: [TC], 1: [node_at(12)], 2: []},    # (the top priority node lies in its own exclude class: not listed)
    "high_4": {0: [T2, node_at(12), node_at(13), node_at(10)], 1: [node_at(9)], 2: []},
    "high_5": {0: [T2, node_at(12), node_at(13), node_at(10), node_at(9)], 1: [node_at(8)], 2: []},
    "high_in_top_class": {0: [TC, node_at(7), node_at(8), node_at(9)], 1: [node_at(12)], 2: []},
    "high_class_no_anchor": {0: [T2, node_at(7), node_at(8), node_at(9)], 1: [node_at(12)], 2: []},
    "low_4": {0: [T2], 1: [node_at(12)], 2: [node_at(13), node_at(10)], 3: [node_at(9), node_at(8)]},
    "low_5": {0: [T2], 1: [node_at(12)], 2: [node_at(13), node_at(10), node_at(6)], 3: [node_at(9), node_at(8)]},
    "two_states": {0: [T2], 1: [node_at(12)], 2: [node_at(12)]},
    "two_states_remote": {0: [T2], 1: [node_at(2)], 3: [node_at(2)]},
    "remote_own": {0: [T2], 1: [node_at(2), node_at(12)], 2: []},
    "two_foreign_regions": {0: [T2], 1: [node_at(2), node_at(12), node_at(5)], 2: []},
    "orphan_only": {0: [T2], 1: [ORPH, node_at(12)], 2: []},
    "own_absent": {0: [T2], 1: None, 2: [node_at(12)]},
    "own_nil": {0: [T2], 1: "nil", 2: [node_at(12)]},
    "all_foreign": {0: [T2], 1: [node_at(0), node_at(1), node_at(2), node_at(3), node_at(4), node_at(5)], 2: []},
    "top_in_no_region": {0: [ORPH2], 1: [node_at(12)], 2: []},
    "no_top_absent": {0: None, 1: [node_at(12)], 2: []},
    "no_top_empty": {0: [], 1: [node_at(2)], 2: []},
    "lower_foreign_ignored": {0: [T2], 1: [node_at(12)], 2: [node_at(2), ORPH]},
    "region_of_one_leaf": {0: [node_at(5)], 1: [node_at(12)], 2: [node_at(5)]},      # (its own node belongs to region 2)
    "top_class_of_one": {0: [node_at(0), node_at(1)], 1: [node_at(2)], 2: [node_at(3)]},
}
CHAIN_LANES = [0, 1, 31, 62, 63]


def chain_world(P, steps_at, weights_nil=0):
    """steps_at: {partition: name}; every other partition is a filler"""
    pb = blank_problem(P, CH_M, CH_L, CH_NX, CH_NX, 8, weights_nil)
    pb["part_has_weight"] = np.array([(p % 3) != 0 for p in range(P)], np.uint8)
    pb["part_weight"] = np.array([(p % 5) - 1 for p in range(P)], np.int32)
    for p in range(P):
        put_lists(pb, "live", p, {t: None for t in range(CH_M)})
        put_lists(pb, "live", p, CHAIN_STEPS[steps_at[p]] if p in steps_at else chain_filler(p))
    return pb


def run_chain_world(kc, pb, order, what, expect=None):
    """classify, events and orphans, then k_gather_chain every way, on one world.  -> the flag words the classification raises"""
    R = chain_regions()
    P, NX = pb["P"], pb["NX"]
    regid, n_ev, raised, events = ref_classify(pb, R, CH_STATE, CH_TOP, order)
    assert sum(n_ev) == len(events)
    flags0 = [0] * GATE_WORDS
    flags0[3], flags0[20] = 77, -5                   # the caller's words stay
    want_flags = list(flags0)
    for b in raised:
        want_flags[b] = 1
    cnt0 = [int(x) for x in _rng(48, P).integers(-50, 50, (CH_M + 1) * NX)]
    cap = len(events) + 3
    rc, q, flags, g_regid, g_nev, n_events, ev, cnt = kc.chain_events(pb, R, CH_STATE, CH_TOP, order, flags0, 0, 1, cap, cnt0)
    assert_problem(q, pb, what, lists_whole=True)
    assert [int(x) for x in flags] == want_flags + [GUARD], what
    assert [int(x) for x in g_regid] == regid + [GUARD], what
    assert [int(x) for x in g_nev] == n_ev + [GUARD], what
    filled = FLAG_NOT_LOCAL not in raised and FLAG_EVENTS in raised
    assert n_events == (len(events) if filled else 0), what
    for j, col in enumerate(ev):
        assert [int(x) for x in col] == ([e[j] for e in events] if filled else []) + [GUARD] * (cap + 1 - (len(events) if filled else 0)), (what, j)
    assert [int(x) for x in cnt] == ref_orphans(pb, R, CH_STATE, cnt0) + [GUARD], what
    for e in events:                                 # a leaf local to the region that owns it
        assert 0 <= e[2] < REG_SIZE[e[0]]
    # classify alone gives the same words; and behind a closed Gate nothing is written
    rc, q, flags, g_regid, g_nev, _, _, _ = kc.chain_events(pb, R, CH_STATE, CH_TOP, order, flags0, 0, 0, 0)
    assert [int(x) for x in flags] == want_flags + [GUARD] and [int(x) for x in g_nev] == n_ev + [GUARD], what
    # k_gather_chain
    ss, hs = [3, 8, 2, 2], [1, 1, 0, 0]
    oi_given = [int(x) for x in _rng(49, P).permutation(P)]
    for classify, chain_oi, with_topkey in [(0, None, 1), (1, oi_given, 0), (1, None, 1)]:
        want_rec, g_raised, want_top = [], set(), []
        fits_at = []
        for i, p in enumerate(order):
            r, fl, tk = ref_chain_record(pb, R, CH_STATE, CH_TOP, CH_MASK, p, chain_oi[i] if chain_oi else i, ss, hs, 0, classify)
            want_rec.append(r)
            g_raised |= fl
            want_top.append(tk)
        gflags = list(flags0)
        for b in g_raised:
            gflags[b] = 1
        rc, q, crec, flags, topkey = kc.gather_chain(pb, R, CH_STATE, CH_TOP, CH_MASK, order, chain_oi, ss, hs, 0, classify, flags0, 0,
                                                     with_topkey)
        tag = "%s: k_gather_chain classify %d" % (what, classify)
        assert_problem(q, pb, tag, lists_whole=True)
        assert [int(x) for x in flags] == gflags + [GUARD], tag
        assert int(crec[-1]) == GUARD, tag
        for i, r in enumerate(want_rec):             # (a step that does not fit: its header only, the pass is not run on it)
            assert [int(x) for x in crec[i * CW:i * CW + len(r)]] == r, (tag, "step", i, "partition", order[i])
        assert [int(x) for x in topkey] == (want_top + [GUARD] if with_topkey else [0] * (P + 1)), tag
        if classify:                                 # the two words equal k_chain_classify's
            assert {b for b in g_raised if b != FLAG_NOT_LOCAL} == {b for b in raised if b != FLAG_NOT_LOCAL}, tag
    if expect is not None:
        assert raised == expect, (what, raised)
    return raised


# what the classification raises for a world of fillers and this one step
CHAIN_EXPECT = {
    "own_5th_remote": {FLAG_EVENTS}, "own_5th_orphan": {FLAG_EVENTS, FLAG_ORPHANS}, "own_6th_remote": {FLAG_EVENTS},
    "own_6th_orphan": {FLAG_EVENTS, FLAG_ORPHANS}, "two_states_remote": {FLAG_EVENTS},
    "remote_own": {FLAG_EVENTS}, "two_foreign_regions": {FLAG_EVENTS}, "orphan_only": {FLAG_EVENTS, FLAG_ORPHANS},
    "all_foreign": {FLAG_EVENTS}, "top_in_no_region": {FLAG_NOT_LOCAL}, "no_top_absent": {FLAG_NOT_LOCAL},
    "no_top_empty": {FLAG_NOT_LOCAL}, "top_class_of_one": set(), "region_of_one_leaf": {FLAG_EVENTS},
}
# ... and whether the compact record holds it
CHAIN_UNFIT = {"own_5", "own_5th_remote", "own_5th_orphan", "own_6th_remote", "own_6th_orphan", "high_5", "low_5", "two_states", "two_states_remote", "all_foreign",
               "top_in_no_region", "no_top_absent", "no_top_empty"}


def check_chain_step(kc, name):
    """The step alone among fillers, at one of lanes 0, 1, 31, 62, 63 of the second wave of three."""
    i = sorted(CHAIN_STEPS).index(name)
    P, p = 150, 64 + CHAIN_LANES[i % len(CHAIN_LANES)]
    pb = chain_world(P, {p: name}, weights_nil=i % 4 == 3)
    order = _perm(P, 20 + i)
    R = chain_regions()
    oi = order.index(p)
    # the table says what it means: on the references, before any kernel runs
    r, fl, _ = ref_chain_record(pb, R, CH_STATE, CH_TOP, CH_MASK, p, oi, [0] * 4, [0] * 4, 0, 1)
    assert (FLAG_NOT_LOCAL in fl) == (name in CHAIN_UNFIT), name
    if name in ("remote_own", "two_foreign_regions", "orphan_only"):
        assert r[5] >> 25 == 1 and (r[5] & 0xff) == 1
    if name == "own_absent":
        assert r[5] >> 24 == 0
    if name == "own_nil":
        assert r[5] >> 24 == 1 and (r[5] & 0xff) == 0
    if name == "high_0":
        assert (r[5] >> 8) & 0xff == 0 and r[6] == 0
    if name == "own_0":
        assert r[5] & 0xff == 0 and r[5] >> 24 == 1
    if name == "high_in_top_class":
        assert (r[5] >> 8) & 0xff == 1 and r[6] == 0 and r[23] == 3
    if name == "high_class_no_anchor":
        assert (r[5] >> 8) & 0xff == 4 and r[6] == -1
    if name in ("own_4", "high_4", "low_4"):
        assert 4 in ((r[5] & 0xff), (r[5] >> 8) & 0xff, (r[5] >> 16) & 0xff)
    # (the lane the step sits at in the gather and in the classification is its place in the pass order)
    order[oi], order[64 + CHAIN_LANES[i % 5]] = order[64 + CHAIN_LANES[i % 5]], order[oi]
    run_chain_world(kc, pb, order, name, CHAIN_EXPECT.get(name, set()))
    if name == "two_foreign_regions":
        _, n_ev, _, events = ref_classify(pb, R, CH_STATE, CH_TOP, order)
        assert sorted(e[0] for e in events) == [0, 1] and max(n_ev) == 2


def check_chain_geometry(kc, P):
    """Every fitting table step somewhere among fillers, events from many steps: rows in pass order, their sum the count."""
    names = [n for n in sorted(CHAIN_STEPS) if n not in CHAIN_UNFIT]
    steps_at = {}
    for j, p in enumerate(range(0, P, 7)):
        steps_at[p] = names[j % len(names)]
    if P > 1:
        steps_at[P - 1] = "two_foreign_regions"
    pb = chain_world(P, steps_at)
    order = _perm(P, 30)
    raised = run_chain_world(kc, pb, order, "chain geometry P %d" % P)
    assert P < 63 or raised == {FLAG_EVENTS, FLAG_ORPHANS}
    R = chain_regions()
    _, n_ev, _, events = ref_classify(pb, R, CH_STATE, CH_TOP, order)
    assert [e[1] for e in events] == sorted(e[1] for e in events)
    assert P < 63 or {0, 2} <= set(n_ev)


def check_chain_events_counts(kc):
    """Steps with 0, 1 and L events in one pass."""
    P = 70
    pb = chain_world(P, {3: "remote_own", 64: "all_foreign", 65: "two_foreign_regions"})
    order = list(range(P))
    R = chain_regions()
    _, n_ev, raised, events = ref_classify(pb, R, CH_STATE, CH_TOP, order)
    assert {0, 1, 2, CH_L} <= set(n_ev) and raised == {FLAG_EVENTS}
    run_chain_world(kc, pb, order, "0, 1 and L events")


def check_chain_flat(kc):
    """flat = 1: one region, r[4] the top priority node itself or NX without one, no anchor class, no top key."""
    P, NX = 70, CH_NX
    pb = chain_world(P, {0: "no_top_absent", 63: "no_top_empty", 64: "own_4", 5: "own_5", 6: "own_nil", 7: "own_absent"})
    R = flat_regions(NX)
    order = _perm(P, 31)
    ss, hs = [3, 8, 2, 2], [1, 1, 0, 0]
    flags0 = [0] * GATE_WORDS
    want, raised = [], set()
    for i, p in enumerate(order):
        r, fl, tk = ref_chain_record(pb, R, CH_STATE, CH_TOP, CH_MASK, p, i, ss, hs, 1, 0)
        assert tk == 0
        want.append(r)
        raised |= fl
    assert raised == {FLAG_NOT_LOCAL}                # own_5 does not fit
    assert {want[order.index(0)][4], want[order.index(63)][4]} == {NX} and want[order.index(64)][4] == T2
    for with_topkey in (1, 0):
        rc, q, crec, flags, topkey = kc.gather_chain(pb, R, CH_STATE, CH_TOP, CH_MASK, order, None, ss, hs, 1, 0, flags0, 0, with_topkey)
        assert [int(x) for x in flags] == [1] + [0] * (GATE_WORDS - 1) + [GUARD]
        for i, r in enumerate(want):
            assert [int(x) for x in crec[i * CW:i * CW + len(r)]] == r, i
        assert int(crec[-1]) == GUARD
        assert [int(x) for x in topkey] == ([0] * P + [GUARD] if with_topkey else [0] * (P + 1))


def check_chain_gate(kc):
    """Closed: k_chain_classify writes nothing; k_gather_chain leaves crec as filled and zeroes topkey; no word is raised."""
    P = 70
    pb = chain_world(P, {3: "orphan_only", 9: "no_top_empty"})
    R = chain_regions()
    order = _perm(P, 32)
    flags0 = [0] * GATE_WORDS
    flags0[22] = 1
    mask = (1 << 22) | 1
    rc, q, flags, regid, n_ev, n_events, ev, cnt = kc.chain_events(pb, R, CH_STATE, CH_TOP, order, flags0, mask, 1, 4, [0] * ((CH_M + 1) * CH_NX))
    assert [int(x) for x in flags] == flags0 + [GUARD]
    assert (regid == GUARD).all() and (n_ev == GUARD).all() and n_events == 0 and all((c == GUARD).all() for c in ev)
    assert [int(x) for x in cnt] == [0] * ((CH_M + 1) * CH_NX) + [GUARD]
    for with_topkey in (1, 0):
        rc, q, crec, flags, topkey = kc.gather_chain(pb, R, CH_STATE, CH_TOP, CH_MASK, order, None, [0] * 4, [0] * 4, 0, 1, flags0, mask, with_topkey)
        assert [int(x) for x in flags] == flags0 + [GUARD]
        assert (crec == GUARD).all()
        assert [int(x) for x in topkey] == ([0] * P + [GUARD] if with_topkey else [0] * (P + 1))
    # the same mask over a clear word: open
    flags0[22] = 0
    rc, q, flags, regid, n_ev, n_events, ev, cnt = kc.chain_events(pb, R, CH_STATE, CH_TOP, order, flags0, mask, 0, 0)
    assert flags[FLAG_NOT_LOCAL] == 1 and flags[FLAG_ORPHANS] == 1 and flags[FLAG_EVENTS] == 1


def check_chain_refusals(kc):
    FILL = 0x3C
    P = 10
    pb = chain_world(P, {})
    R = chain_regions()
    order = list(range(P))
    flags0 = [0] * GATE_WORDS

    def both(pb, R, order, what):
        rc, _, flags, regid, n_ev, _, ev, _ = kc.chain_events(pb, R, CH_STATE, CH_TOP, order, flags0, 0, 1, 4, check=False, fill=FILL)
        assert rc == BAD_ARG and (regid == FILL).all() and (n_ev == FILL).all(), what
        rc, _, crec, flags, topkey = kc.gather_chain(pb, R, CH_STATE, CH_TOP, CH_MASK, order, None, [0] * 4, [0] * 4, 0, 0, flags0, 0, 1,
                                                     check=False, fill=FILL)
        assert rc == BAD_ARG and (crec == FILL).all() and (topkey == FILL).all(), what

    for key, i, v in [("node_region", 3, 3), ("node_region", 3, -2), ("node_leaf_pos", 3, 14), ("node_leaf_pos", 13, -1), ("reg_lo", 2, 14),
                      ("node_leaf_pos", 0, 4)]:       # (the last: a leaf below its region's first)
        R2 = copy.deepcopy(R)
        R2[key][i] = v
        both(pb, R2, order, (key, i, v))
    both(pb, R, [0] * P, "order not a permutation")
    both(pb, R, list(range(1, P + 1)), "partition id P")
    q = copy.deepcopy(pb)
    q["live"][2, 1, 0] = CH_NX
    both(q, R, order, "node id NX")
    R2 = copy.deepcopy(R)
    R2["leaf_cls"][12] = 8                            # class 8 of region 2: its size would be read at leaf 14
    rc, _, crec, flags, topkey = kc.gather_chain(pb, R2, CH_STATE, CH_TOP, CH_MASK, order, None, [0] * 4, [0] * 4, 0, 0, flags0, 0, 1,
                                                 check=False, fill=FILL)
    assert rc == BAD_ARG and (crec == FILL).all()
