"""k_period_verify, k_period_segments, k_period_judge and k_period_replicate one at a time, and the periodic form as a whole
against one sequential walk (blance_amd/csrc/k_period.h): the cases, the references in plain Python and the
checks, shared by tests/test_period_cases_emulated.py (SIMT emulator), tests/test_period_cases_gpu.py (device) and the
stand-alone sanitizer program (tests/simt/period_cases_asan_main.cpp reads the file write_program_input makes).

The references follow the definitions, not the kernels: verify's limit is the first step whose words 1..23 differ from the step
one period back, found by comparing whole rows; the judge's counters behind the copied stretch are found by REPLAYING every
copied step's picks with that step's own weight, one by one, where the kernel adds d per full period in closed form.

Every buffer a kernel may write goes in full of POISON but for the words the case sets, carries one guard word behind its last,
and comes back whole: what the kernel does not own must still be as it went in."""
import ctypes as C

import numpy as np

import period_case_tables as PT
from period_case_tables import BAD_ARG, CAP, INT_MAX, INT_MIN, KCW, POISON

K_T, K_LIMIT, K_OK, K_D, K_BEG1, K_END1, K_BEG2, K_END2, K_BEG3, K_END3 = range(10)
WORDS = 10                       # kPWords
CHAIN_FLAGS, FLAG_ESCAPED = 8, 1  # kChainFlags, kFlagEscaped
MIN_ROUNDS = 4                   # kPeriodMinRounds
P32 = np.int32(POISON)


def i32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int64).astype(np.int32))


def new_pb(B):
    return np.full(WORDS * B + 1, POISON, dtype=np.int32)


def rows(pb):
    """pb[kPWords][B], a view (the guard word is pb[-1])."""
    return pb[:-1].reshape(WORDS, -1)


def joins(T, limit):
    return 1 <= T <= CAP and limit >= MIN_ROUNDS * T


class PeriodKernels:
    """The entries of tests/kernels/period_cases.inc.  Arrays are changed in place; every call returns the entry's status."""

    def __init__(self, lib_path):
        lib = self.lib = C.CDLL(lib_path)
        lib.blance_case_period_words.restype = C.c_int
        for name, n_int, n_ptr in (("find", 7, 7), ("verify", 3, 3), ("segments", 4, 2), ("judge", 9, 11), ("replicate", 4, 3)):
            fn = getattr(lib, "blance_case_period_" + name)
            fn.restype = C.c_int
            fn.argtypes = [C.c_int] * n_int + [C.c_void_p] * n_ptr
        assert lib.blance_case_period_words() == WORDS

    @staticmethod
    def _p(a):
        assert a.flags["C_CONTIGUOUS"]
        return a.ctypes.data

    def find(self, w, pb, known, threads):
        leaves = w.leaf_node if w.leaf_node.size else np.zeros(1, dtype=np.int32)
        keep = w.crec if w.crec.size else np.zeros(1, dtype=np.int32)
        return self.lib.blance_case_period_find(w.B, int(known), threads, w.N, w.NX, w.n_steps, len(w.leaf_node), self._p(w.reg_off),
                                                self._p(w.reg_lo), self._p(w.reg_hi), self._p(leaves), self._p(w.alive), self._p(keep),
                                                self._p(pb))

    def verify(self, reg_off, crec, pb, threads=256):
        keep = crec if crec.size else np.zeros(1, dtype=np.int32)
        return self.lib.blance_case_period_verify(len(reg_off) - 1, threads, crec.size // KCW, self._p(reg_off), self._p(keep), self._p(pb))

    def segments(self, reg_off, n_steps, cut, pb, threads=64):
        return self.lib.blance_case_period_segments(len(reg_off) - 1, threads, cut, n_steps, self._p(reg_off), self._p(pb))

    def judge(self, w, s, n_states, OW, out, flags, cnt1, cnt, pb, threads=128):
        leaves = w.leaf_node if w.leaf_node.size else np.zeros(1, dtype=np.int32)
        keep = w.crec if w.crec.size else np.zeros(1, dtype=np.int32)
        return self.lib.blance_case_period_judge(w.B, threads, s, n_states, w.N, w.NX, OW, w.n_steps, len(w.leaf_node), self._p(w.reg_off),
                                                 self._p(w.reg_lo), self._p(w.reg_hi), self._p(leaves), self._p(w.alive), self._p(keep),
                                                 self._p(out), self._p(flags), self._p(cnt1), self._p(cnt), self._p(pb))

    def replicate(self, reg_off, n_steps, OW, pb, out, threads=256):
        return self.lib.blance_case_period_replicate(len(reg_off) - 1, threads, OW, n_steps, self._p(reg_off), self._p(pb), self._p(out))


# =============================================================================================================================
# k_period_verify
# =============================================================================================================================

def periodic_records(period, length, seed, breaks=()):
    """`length` records that repeat with `period` in words 1..23 (word 4 tells the steps of a period apart) and never in word 0;
    breaks: (step, word) whose value is changed to one no other record has."""
    rng = np.random.RandomState(seed)
    base = rng.randint(0, 1 << 20, size=(period, KCW))
    base[:, 4] = np.arange(period)
    rec = base[np.arange(length) % period] if length else np.zeros((0, KCW), dtype=np.int64)
    rec = np.array(rec, dtype=np.int64)
    rec[:, 0] = 100000 + 7 * np.arange(length) + seed
    for t, w in breaks:
        rec[t, w] += 1 << 21
    return rec


def verify_reference(reg_off, crec, T_row, limit_row):
    """limit per region: the first t >= T whose words 1..23 differ from step t - T's, else what came in (k_period_find leaves the
    chain's length there); what came in, too, where T is no candidate or no step lies T behind another."""
    rec = crec.reshape(-1, KCW)
    want = []
    for r in range(len(reg_off) - 1):
        T, mine = int(T_row[r]), rec[reg_off[r]:reg_off[r + 1]]
        limit = int(limit_row[r])
        if 1 <= T <= CAP:
            for t in range(T, len(mine)):
                if list(mine[t][1:]) != list(mine[t - T][1:]):
                    limit = min(limit, t)
                    break
        want.append(limit)
    return want


def _seam_break(qi):
    """(step, word) inside the 16-byte piece qi of a chain (a record is six pieces; word 0 is not compared)."""
    piece = qi % 6
    return qi // 6, piece * 4 + (1 + qi % 3 if piece == 0 else qi % 4)


def _verify_cases():
    """name -> ([(T set in pb, length, period of the records, breaks, limit that comes in or None for the length)], expected
    limits where the case knows them by hand (None: the reference alone), workgroup sizes)."""
    c = {}
    for w in range(1, KCW):                                       # every compared word: every piece, every lane of the int4
        c["break_in_word_%d" % w] = ([(7, 60, 7, [(33, w)], None)], [33], (256, 64))
    c["word_0_differs_only"] = ([(7, 60, 7, [(20, 0)], None)], [60], (256, 64))
    c["break_at_T"] = ([(7, 60, 7, [(7, 5)], None)], [7], (256, 64))
    c["break_at_the_last_step"] = ([(7, 60, 7, [(59, 9)], None)], [59], (256, 64))
    # a break in [1, T) is not compared where it lies: the step one period on differs from it.  (T is set by hand: the search
    # does not return 7 for such records -- here it would, the first record is unchanged, but nothing rests on that)
    c["break_inside_the_first_period"] = ([(7, 60, 7, [(3, 2)], None)], [10], (256, 64))
    c["two_breaks"] = ([(7, 60, 7, [(40, 3), (25, 17)], None)], [25], (256, 64))
    for j in (1, 2, 3):                                           # the seams of the 256-thread workgroups
        for delta in (-1, 0, 1):
            t, w = _seam_break(256 * j + delta)
            c["seam_%d%+d" % (256 * j, delta)] = ([(5, 200, 5, [(t, w)], None)], [t], (256,))
    c["period_of_one"] = ([(1, 40, 1, [], None)], [40], (256, 64))
    c["period_of_one_broken"] = ([(1, 40, 1, [(17, 23)], None)], [17], (256, 64))
    c["period_at_the_cap"] = ([(CAP, 4 * CAP + 5, CAP, [], None)], [4 * CAP + 5], (256,))
    c["period_at_the_cap_broken"] = ([(CAP, 4 * CAP + 5, CAP, [(4 * CAP + 3, 22)], None)], [4 * CAP + 3], (256,))
    c["three_chains_middle_empty"] = ([(4, 50, 4, [(30, 6)], None), (3, 0, 3, [], None), (6, 13, 6, [], None)], [30, 0, 13], (256, 64))
    c["three_chains_longest_last"] = ([(4, 9, 4, [(8, 1)], None), (3, 300, 3, [(299, 20)], None), (5, 700, 5, [(650, 12)], None)],
                                      [8, 299, 650], (256, 64))
    # T no candidate: nothing is written, although the records break
    c["no_candidate"] = ([(INT_MAX, 30, 3, [(10, 2)], POISON), (CAP + 1, 30, 3, [(10, 2)], POISON), (0, 30, 3, [(10, 2)], POISON),
                          (-1, 30, 3, [(10, 2)], POISON), (31, 30, 3, [(10, 2)], POISON), (30, 30, 3, [(10, 2)], POISON)],
                         [POISON] * 6, (256, 64))
    # records with ANOTHER period than the one in pb: limit = T (here step 4 differs from step 0)
    c["not_the_period"] = ([(4, 40, 5, [], None)], [4], (256, 64))
    return c


VERIFY_CASES = _verify_cases()


def check_verify(pk, name):
    chains, expect, sizes = VERIFY_CASES[name]
    B = len(chains)
    reg_off = i32(np.concatenate([[0], np.cumsum([ch[1] for ch in chains])]))
    recs = [periodic_records(period, length, 11 + r, breaks) for r, (_, length, period, breaks, _) in enumerate(chains)]
    crec = i32(np.concatenate(recs).reshape(-1))
    pb0 = new_pb(B)
    for r, (T, length, _, _, limit_in) in enumerate(chains):
        rows(pb0)[K_T, r] = T
        rows(pb0)[K_LIMIT, r] = length if limit_in is None else limit_in
    want = verify_reference(reg_off, crec, rows(pb0)[K_T], rows(pb0)[K_LIMIT])
    assert want == expect, (name, want, expect)                   # (the reference agrees with what the case says by hand)
    for threads in sizes:
        pb = pb0.copy()
        assert pk.verify(reg_off, crec, pb, threads) == 0, (name, threads)
        assert [int(x) for x in rows(pb)[K_LIMIT]] == want, (name, threads, rows(pb)[K_LIMIT], want)
        pb[:-1].reshape(WORDS, B)[K_LIMIT] = rows(pb0)[K_LIMIT]
        assert (pb == pb0).all(), (name, threads, "a word outside the limits was written")


# =============================================================================================================================
# k_period_segments
# =============================================================================================================================

def segments_reference(reg_off, pb_rows, cut):
    """The ten words per region: a positive cut ends the stretch, the region joins with a candidate period and four periods in
    front of the limit; [0, T) and [T, 2T) of one that joins, the whole chain and nothing of one that does not; nothing third."""
    want = pb_rows.copy()
    for r in range(pb_rows.shape[1]):
        cbeg, cend = int(reg_off[r]), int(reg_off[r + 1])
        T, limit = int(pb_rows[K_T, r]), int(pb_rows[K_LIMIT, r])
        if cut > 0:
            limit = min(limit, cut)
        j = joins(T, limit)
        want[K_LIMIT, r] = limit
        want[K_OK, r] = int(j)
        want[K_BEG1:, r] = [cbeg, cbeg + T, cbeg + T, cbeg + 2 * T, cend, cend] if j else [cbeg, cend, cend, cend, cend, cend]
    return want


# (T, limit, chain length)
SEGMENT_REGIONS = [(10, 39, 39), (10, 40, 40), (10, 41, 50), (1, 4, 4), (1, 3, 3), (INT_MAX, 25, 25), (INT_MAX, 0, 0), (3, 0, 0),
                   (CAP, 4 * CAP, 4 * CAP + 1), (CAP, 4 * CAP - 1, 4 * CAP), (CAP + 1, 5 * CAP, 5 * CAP), (0, 30, 30), (-4, 30, 30),
                   (4, 17, 90), (5, 200, 200)]
# cut: off, off (negative), above every limit, below some limits (regions that still join, one that no longer does: 4 * 5 > 17),
# and low enough that only T = 1 joins
SEGMENT_CUTS = [0, -3, 10 ** 6, 40, 17, 4]


def check_segments(pk, B, cut, threads):
    regions = [SEGMENT_REGIONS[(r * 7) % len(SEGMENT_REGIONS)] for r in range(B)] if B != len(SEGMENT_REGIONS) else SEGMENT_REGIONS
    reg_off = i32(np.concatenate([[0], np.cumsum([g[2] for g in regions])]))
    pb0 = new_pb(B)
    for r, (T, limit, _) in enumerate(regions):
        rows(pb0)[K_T, r], rows(pb0)[K_LIMIT, r] = T, limit
    want = segments_reference(reg_off, rows(pb0), cut)
    assert (want[K_D] == P32).all()
    pb = pb0.copy()
    assert pk.segments(reg_off, int(reg_off[-1]), cut, pb, threads) == 0
    assert (rows(pb) == want).all(), (B, cut, threads, np.argwhere(rows(pb) != want)[:4])
    assert pb[-1] == P32
    return want


# =============================================================================================================================
# k_period_judge
# =============================================================================================================================

class World:
    """Regions of leaves with their chains: what every kernel of the form reads."""

    def __init__(self, N, NX, reg_off, reg_lo, reg_hi, leaf_node, alive, crec, leaf_cls=None, k=1):
        self.N, self.NX, self.reg_off, self.reg_lo, self.reg_hi = N, NX, i32(reg_off), i32(reg_lo), i32(reg_hi)
        self.leaf_node, self.alive, self.crec = i32(leaf_node), np.ascontiguousarray(alive, dtype=np.uint8), i32(crec)
        self.B, self.n_steps = len(self.reg_lo), len(self.crec) // KCW
        self.leaf_cls, self.k = leaf_cls, k

    def live(self, r):
        """The region's candidate nodes in leaf order: a node of the cluster's first N ids that is alive."""
        return [int(n) for n in self.leaf_node[self.reg_lo[r]:self.reg_hi[r]] if 0 <= n < self.N and self.alive[n]]

    def others(self, r):
        return [int(n) for n in self.leaf_node[self.reg_lo[r]:self.reg_hi[r]] if n >= 0 and not (n < self.N and self.alive[n])]


def judge_reference(w, s, OW, out, flags, cnt1, cnt, pb):
    """(counters, pb) behind the judge, by the definition: a region that joins is ok when its live leaves all grew by one d >= 0
    between cnt1 and cnt, no other leaf's node moved, and no chain has escaped; then the third segment starts behind the limit
    and every step t of [2T, limit) adds its own weight to what step T + (t - T) % T picked; else it starts behind 2T and no
    counter changes.  A region that does not join keeps every word."""
    cnt, pb = cnt.copy(), pb.copy()
    P = rows(pb)
    rec = w.crec.reshape(-1, KCW)
    verdicts = []
    for r in range(w.B):
        cbeg, cend, T, limit = int(w.reg_off[r]), int(w.reg_off[r + 1]), int(P[K_T, r]), int(P[K_LIMIT, r])
        if not joins(T, limit):
            verdicts.append(None)
            continue
        diff = lambda n: int(cnt[s * w.NX + n]) - int(cnt1[s * w.NX + n])    # noqa: E731
        live = w.live(r)
        d = max([diff(n) for n in live], default=INT_MIN)
        ok = bool(live) and all(diff(n) == d for n in live) and d >= 0 and all(diff(n) == 0 for n in w.others(r)) and flags[FLAG_ESCAPED] == 0
        P[K_D, r], P[K_OK, r], P[K_BEG3, r], P[K_END3, r] = d, int(ok), cbeg + (limit if ok else 2 * T), cend
        verdicts.append(ok)
        if ok:
            for t in range(2 * T, limit):
                o = out[(cbeg + T + (t - T) % T) * OW:][:OW]
                for c in range(int(o[0]) & 0xffff):
                    if 0 <= o[1 + c] < w.NX:
                        cnt[s * w.NX + o[1 + c]] += rec[cbeg + t, 1]
    return cnt, pb, verdicts


class JRegion:
    def __init__(self, leaves, T, k, rest, full=2, weight=1, tail=3, wrong=None, joined=True, bad_picks=False):
        """leaves: a string, one letter per leaf: l a live node, d a dead one, o one outside the cluster's ids, - none.
        The region's steps pick its live nodes in turn, k a step; limit = (2 + full) * T + rest; weight: a number or a function
        of the step's place in the period; wrong: what is done to the counters behind the second walk."""
        self.leaves, self.T, self.k, self.rest, self.full, self.tail = leaves, T, k, rest, full, tail
        self.weight = weight if callable(weight) else (lambda j, w=weight: w)
        self.wrong, self.joined, self.bad_picks = wrong, joined, bad_picks


def build_judge(regions, s, n_states, OW, escaped=0, seed=5):
    """The arrays of one table as the second walk leaves them: (world, out, flags, cnt1, cnt, pb)."""
    rng = np.random.RandomState(seed)
    N = max(1, sum(sum(1 for ch in g.leaves if ch in "ld") for g in regions))
    NX = N + sum(g.leaves.count("o") for g in regions) + 1
    alive = np.zeros(NX, dtype=np.uint8)
    leaf_node, reg_off, reg_lo, reg_hi = [], [0], [], []
    nxt_in, nxt_out = 0, N
    for g in regions:
        reg_lo.append(len(leaf_node))
        for ch in g.leaves:
            if ch == "-":
                leaf_node.append(-1)
            elif ch == "o":
                leaf_node.append(nxt_out)
                alive[nxt_out] = 1
                nxt_out += 1
            else:
                leaf_node.append(nxt_in)
                alive[nxt_in] = ch == "l"
                nxt_in += 1
        reg_hi.append(len(leaf_node))
        limit = (2 + g.full) * g.T + g.rest if g.joined else 4 * g.T - 1
        g.limit = limit
        reg_off.append(reg_off[-1] + limit + g.tail)
    n_steps = reg_off[-1]
    crec = np.full((n_steps, KCW), -1, dtype=np.int64)
    crec[:, 0] = 5000 + np.arange(n_steps)
    w = World(N, NX, reg_off, reg_lo, reg_hi, leaf_node, alive, crec.reshape(-1))
    out = np.full(n_steps * OW + 1, POISON, dtype=np.int32)
    cnt1 = np.full(n_states * NX + 1, POISON, dtype=np.int32)
    cnt1[s * NX:(s + 1) * NX] = rng.randint(0, 50, size=NX)
    cnt = cnt1.copy()
    pb = new_pb(len(regions))
    P = rows(pb)
    for r, g in enumerate(regions):
        cbeg, cend, live = reg_off[r], reg_off[r + 1], w.live(r)
        for t in range(cbeg, cend):
            crec[t, 1] = g.weight((t - cbeg) % g.T)
        # the two walks wrote [0, 2T) of a region that joins (every step of one that does not); the rest is nobody's yet
        for t in range(cbeg, cbeg + 2 * g.T if g.joined else cend):
            j = (t - cbeg) % g.T
            first = t < cbeg + g.T                                # (the first period starts from another state: other picks)
            picks = [live[(j * g.k + c + first) % len(live)] for c in range(g.k)] if live else []
            if g.bad_picks and j % 3 != 1:                         # (ids the kernel must skip: no node, the first id past the counters)
                picks.insert(j % (len(picks) + 1), -1 if j % 2 else NX)
            assert len(picks) <= OW - 1
            o = out[t * OW:(t + 1) * OW]
            o[:] = -7
            o[0] = len(picks) | ((1 + t % 0x7ffe) << 16)           # (bits above 0xffff: the kernel masks them)
            o[1:1 + len(picks)] = picks
            if cbeg + g.T <= t < cbeg + 2 * g.T:
                for n in picks:
                    if 0 <= n < NX:
                        cnt[s * NX + n] += crec[t, 1]
        diffs = set(int(cnt[s * NX + n] - cnt1[s * NX + n]) for n in live)
        assert len(diffs) <= 1, "the case's picks are not uniform over its live leaves"
        kind, at = g.wrong or (None, None)
        if kind == "live":                                        # one live leaf off by `at`
            cnt[s * NX + live[len(live) // 2]] += at
        elif kind == "other":                                     # a leaf that is no candidate moved: the at-th of them
            cnt[s * NX + w.others(r)[at]] += 1
        elif kind == "negative":
            for n in live:
                cnt[s * NX + n] -= max(diffs) + 1
        P[K_T, r], P[K_LIMIT, r], P[K_OK, r], P[K_D, r] = g.T, g.limit, int(g.joined), INT_MIN
        P[K_BEG1:, r] = [cbeg, cbeg + g.T, cbeg + g.T, cbeg + 2 * g.T, cend, cend] if g.joined else [cbeg, cend, cend, cend, cend, cend]
    w.crec = i32(crec.reshape(-1))
    flags = np.full(CHAIN_FLAGS + 1, 0, dtype=np.int32)
    flags[FLAG_ESCAPED], flags[-1] = escaped, POISON
    return w, out, flags, cnt1, cnt, pb


def _mixed(n):
    """n leaves: mostly live, with leaves of every other kind between them."""
    return "".join("-" if i % 23 == 7 else "d" if i % 29 == 11 else "o" if i % 31 == 13 else "l" for i in range(n))


L6 = "llllll"
# name -> (regions, expected verdicts with the flag clear, s, states, OW)
JUDGE_TABLES = {
    # the last, partial period: none, one step, all but one; limit = 4T exactly is the first of them
    "rests": ([JRegion(L6, 12, 2, 0), JRegion(L6, 12, 2, 1), JRegion(L6, 12, 2, 11), JRegion(L6, 12, 2, 5, full=7)], [True] * 4, 1, 2, 3),
    # more counted steps than threads, on 128 and on 64
    "rest_over_the_threads": ([JRegion("l" * 100, 300, 1, 299), JRegion("l" * 100, 300, 1, 257), JRegion("l" * 60, 300, 1, 129, full=3)],
                              [True] * 3, 1, 2, 2),
    # more leaves than threads; leaves with no node, a dead node, a node outside the ids
    "wide": ([JRegion("l" * 192, 192, 1, 100), JRegion("l" * 256, 128, 2, 77), JRegion(_mixed(256), _mixed(256).count("l"), 1, 50),
              JRegion(_mixed(192), _mixed(192).count("l"), 3, 9)], [True] * 4, 1, 2, 4),
    # each refusal in turn, between regions that pass and one that does not join
    "refusals": ([JRegion(L6, 6, 1, 2),
                  JRegion("l" * 200, 200, 1, 3, wrong=("live", 1)),
                  JRegion("l" * 200, 200, 1, 3, wrong=("live", -1)),
                  JRegion(L6, 6, 1, 2, wrong=("live", 1)),
                  JRegion("lldlldl-", 5, 1, 2, wrong=("other", 1)),
                  JRegion("lldl" + "l" * 150 + "d", 153, 1, 2, wrong=("other", 1)),
                  JRegion("lloll", 4, 1, 2, wrong=("other", 0)),
                  JRegion("lldlol-", 4, 1, 2),                     # the same kinds of leaves, none moved: passes
                  JRegion("dd-o", 3, 1, 2),                        # no live leaf
                  JRegion(L6, 6, 1, 2, wrong=("negative", None)),
                  JRegion(L6, 6, 1, 2, joined=False),
                  JRegion(L6, 6, 1, 4)],
                 [True, False, False, False, False, False, False, True, False, False, None, True], 1, 2, 2),
    "picks_to_skip": ([JRegion(L6, 12, 2, 7, bad_picks=True), JRegion("l" * 9, 9, 1, 8, bad_picks=True)], [True] * 2, 1, 2, 4),
    "widest_records": ([JRegion("l" * 8, 8, 4, 5), JRegion("l" * 8, 8, 3, 5, bad_picks=True)], [True] * 2, 0, 1, 5),
    "partition_weight_3": ([JRegion(L6, 12, 2, 7, weight=3), JRegion("l" * 9, 9, 1, 4, weight=2)], [True] * 2, 1, 2, 3),
    "state_0_of_1": ([JRegion(L6, 12, 2, 7)], [True], 0, 1, 3),
    "state_2_of_3": ([JRegion(L6, 12, 2, 7), JRegion(L6, 6, 1, 2, wrong=("live", 1))], [True, False], 2, 3, 3),
    # THE WEIGHT OF THE COUNTED STEPS: weights that differ inside a period while d is uniform -- 64 leaves picked in turn, 64
    # steps of weight 1 and 64 of weight 2, d = 3; 70 counted steps, the last six of the other weight than the chain's first
    "weights_differ_inside_a_period": ([JRegion("l" * 64, 128, 1, 70, weight=lambda j: 1 if j < 64 else 2),
                                        JRegion("l" * 64, 128, 1, 70, weight=lambda j: 2 if j < 64 else 1),
                                        JRegion("l" * 4, 8, 1, 7, weight=lambda j: (5, 1, 1, 1, 1, 5, 5, 5)[j])], [True] * 3, 1, 2, 2),
}
_judge_built = {}


def judge_table(name, escaped=0):
    if (name, escaped) not in _judge_built:
        regions, verdicts, s, n_states, OW = JUDGE_TABLES[name]
        arrays = build_judge(regions, s, n_states, OW, escaped)
        w, out, flags, cnt1, cnt, pb = arrays
        want = judge_reference(w, s, OW, out, flags, cnt1, cnt, pb)
        assert want[2] == ([v if v is None else False for v in verdicts] if escaped else verdicts), (name, want[2])
        _judge_built[(name, escaped)] = (arrays, want)
    return _judge_built[(name, escaped)]


def check_judge(pk, name, threads, escaped=0):
    (w, out0, flags0, cnt10, cnt0, pb0), (want_cnt, want_pb, verdicts) = judge_table(name, escaped)
    _, _, s, n_states, OW = JUDGE_TABLES[name]
    out, flags, cnt1, cnt, pb = out0.copy(), flags0.copy(), cnt10.copy(), cnt0.copy(), pb0.copy()
    assert pk.judge(w, s, n_states, OW, out, flags, cnt1, cnt, pb, threads) == 0, (name, threads)
    P, W = rows(pb), rows(want_pb)
    for r, v in enumerate(verdicts):
        assert (P[:, r] == W[:, r]).all(), (name, threads, r, v, P[:, r], W[:, r])
    assert pb[-1] == P32
    bad = np.flatnonzero(cnt != want_cnt)
    assert bad.size == 0, (name, threads, bad[:6], cnt[bad[:6]], want_cnt[bad[:6]])
    if not any(verdicts):
        assert (cnt == cnt0).all()                                # (refused: no counter changed)
    assert (cnt1 == cnt10).all() and (out == out0).all() and (flags == flags0).all(), (name, threads)
    return verdicts


# =============================================================================================================================
# k_period_replicate
# =============================================================================================================================

def replicate_reference(reg_off, pb_rows, OW, out):
    want = out.copy()
    o = want[:-1].reshape(-1, OW)
    for r in range(pb_rows.shape[1]):
        if pb_rows[K_OK, r]:
            cbeg, T, limit = int(reg_off[r]), int(pb_rows[K_T, r]), int(pb_rows[K_LIMIT, r])
            for t in range(2 * T, limit):
                o[cbeg + t] = out[:-1].reshape(-1, OW)[cbeg + T + (t - T) % T]
    return want


# name -> [(T, limit, chain length, ok)]
REPLICATE_TABLES = {"copies_%d" % n: [(3, 6 + n, 6 + n + 2, 1)] for n in (1, 255, 256, 257, 513)}
REPLICATE_TABLES.update({
    "limit_is_the_length": [(7, 300, 300, 1)],
    "nothing_to_copy": [(5, 10, 40, 1)],
    "not_ok": [(3, 200, 210, 0)],
    "not_ok_and_no_period": [(INT_MAX, 200, 200, 0), (0, 50, 50, 0)],
    "three_regions": [(4, 700, 701, 1), (2, 5, 5, 1), (16, 290, 300, 1)],
    "three_regions_one_refused": [(4, 300, 301, 1), (5, 600, 700, 0), (1, 90, 90, 1)],
    "period_at_the_cap": [(CAP, 2 * CAP + 300, 2 * CAP + 300, 1)],
})


def check_replicate(pk, name, OW, threads=256):
    regions = REPLICATE_TABLES[name]
    B = len(regions)
    reg_off = i32(np.concatenate([[0], np.cumsum([g[2] for g in regions])]))
    n_steps = int(reg_off[-1])
    pb0 = new_pb(B)
    for r, (T, limit, _, ok) in enumerate(regions):
        rows(pb0)[K_T, r], rows(pb0)[K_LIMIT, r], rows(pb0)[K_OK, r] = T, limit, ok
    out0 = i32(np.random.RandomState(OW).randint(-2 ** 31, 2 ** 31 - 1, size=n_steps * OW + 1))   # (every word tells: no two alike)
    want = replicate_reference(reg_off, rows(pb0), OW, out0)
    pb, out = pb0.copy(), out0.copy()
    assert pk.replicate(reg_off, n_steps, OW, pb, out, threads) == 0, (name, OW)
    bad = np.flatnonzero(out != want)
    assert bad.size == 0, (name, OW, threads, bad[:6] // OW)
    assert (pb == pb0).all()
    for r, (T, limit, _, ok) in enumerate(regions):                # (and by hand: a copied step is the step one period back)
        o = out[:-1].reshape(-1, OW)[reg_off[r]:]
        if ok and limit > 2 * T:
            assert (o[limit - 1] == o[limit - 1 - T]).all() and (o[2 * T] == o[T]).all()


def check_entry_refusals(pk):
    """Tables whose indices leave the arrays are refused without a launch: every buffer comes back as it went."""
    (w, out, flags, cnt1, cnt, pb), _ = judge_table("rests")
    _, _, s, n_states, OW = JUDGE_TABLES["rests"]

    def judge_refused(why, w=w, s=s, n_states=n_states, OW=OW, out=out, pb=pb, threads=128):
        o, f, c1, c, p = out.copy(), flags.copy(), cnt1.copy(), cnt.copy(), pb.copy()
        assert pk.judge(w, s, n_states, OW, o, f, c1, c, p, threads) == BAD_ARG, why
        assert (o == out).all() and (c == cnt).all() and (p == pb).all(), why

    judge_refused("the state", s=2)
    judge_refused("the state", s=-1)
    judge_refused("the workgroup", threads=96)
    judge_refused("the record's width", OW=6)
    p = pb.copy(); rows(p)[K_LIMIT, 1] = w.reg_off[2] - w.reg_off[1] + 1
    judge_refused("a limit behind the chain", pb=p)
    o = out.copy(); o[(w.reg_off[2] + 12 + 3) * OW] = 3                       # a counted step with three picks in a record of three words
    judge_refused("a record with more picks than it holds", out=o)

    def other(**kw):
        v = World(w.N, w.NX, w.reg_off, w.reg_lo, w.reg_hi, w.leaf_node, w.alive, w.crec)
        for key, val in kw.items():
            setattr(v, key, i32(val) if key != "N" else val)
        return v

    off = w.reg_off.copy(); off[-1] += 1
    judge_refused("a chain behind the records", w=other(reg_off=off))
    hi = w.reg_hi.copy(); hi[-1] += 1
    judge_refused("leaves behind the table", w=other(reg_hi=hi))
    leaf = w.leaf_node.copy(); leaf[2] = w.NX
    judge_refused("a node behind the counters", w=other(leaf_node=leaf))
    judge_refused("more ids than counters", w=other(N=w.NX + 1))
    # verify, segments: the chains against the records
    pbv = new_pb(w.B)
    assert pk.verify(off, w.crec, pbv) == BAD_ARG and pk.segments(off, w.n_steps, 0, pbv) == BAD_ARG and (pbv == P32).all()
    assert pk.verify(w.reg_off, w.crec, pbv, threads=100) == BAD_ARG and (pbv == P32).all()
    # replicate: an ok region with no period, one period only in front of the limit, a limit behind the chain
    reg_off = i32([0, 50])
    for T, limit in ((0, 20), (-2, 20), (CAP + 1, 50), (6, 11), (6, 51)):
        pr = new_pb(1)
        rows(pr)[K_T, 0], rows(pr)[K_LIMIT, 0], rows(pr)[K_OK, 0] = T, limit, 1
        o = np.full(50 * 2 + 1, POISON, dtype=np.int32)
        assert pk.replicate(reg_off, 50, 2, pr, o) == BAD_ARG and (o == P32).all(), (T, limit)
    assert pk.replicate(reg_off, 50, 6, new_pb(1), np.full(50 * 6 + 1, POISON, dtype=np.int32)) == BAD_ARG


# =============================================================================================================================
# The form as a whole against one sequential walk
# =============================================================================================================================
# The chain kernels are not part of this: a small automaton stands in for them, one that satisfies the form's premise (its
# state is the region's counters, compared inside the region only; its input per step the words 1..23 of the record).  Per step
# it picks the k lowest live leaves outside the exclude class of the step's top leaf (word 6; -1: none), ties to the lowest
# leaf; each pick adds the step's weight (word 1); the picks are the step's `out` record.

def record(top_leaf, weight, cls, step):
    rec = [-1] * KCW
    rec[0], rec[1], rec[2], rec[3], rec[4], rec[5], rec[6], rec[23] = 100000 + 7 * step, weight, 0, 0x3ff80000, top_leaf, 1 << 24, cls, 16
    return rec


def walk(w, s, OW, cnt, out, beg, end):
    """Steps [beg[r], end[r]) of every region, one after the other."""
    rec = w.crec.reshape(-1, KCW)
    o = out[:-1].reshape(-1, OW)
    for r in range(w.B):
        lo, hi = int(w.reg_lo[r]), int(w.reg_hi[r])
        cand = [pos for pos in range(lo, hi) if 0 <= w.leaf_node[pos] < w.N and w.alive[w.leaf_node[pos]]]
        at = s * w.NX + w.leaf_node[cand].astype(np.int64)        # the live leaves' counters, in leaf order
        cls = np.asarray(w.leaf_cls, dtype=np.int64)[cand]
        for t in range(int(beg[r]), int(end[r])):
            weight, excl = int(rec[t, 1]), int(rec[t, 6])
            free = np.flatnonzero(cls != excl) if excl >= 0 else np.arange(len(cand))
            lowest = free[np.argsort(cnt[at[free]], kind="stable")[:w.k]]     # (stable: ties go to the lowest leaf)
            picks = at[lowest] - s * w.NX
            cnt[at[lowest]] += weight
            o[t] = -1
            o[t, 0] = len(picks) | ((1 + r) << 16)
            o[t, 1:1 + len(picks)] = picks


class Chain:
    def __init__(self, leaves, tops, reps, rest=0, tail=(), cls_size=0, weights=None, init="zero"):
        """leaves: as JRegion's; tops: the places among the leaves of one period's top priority nodes; the records repeat them
        reps times, then `rest` steps of another period; tail: places of steps behind the periodic stretch; cls_size: leaves
        per exclude class (0: none); weights: per step of the period; init: the counters the walk starts from."""
        self.leaves, self.tops, self.reps, self.rest, self.tail, self.cls_size = leaves, list(tops), reps, rest, list(tail), cls_size
        self.weights, self.init = weights or [1] * len(self.tops), init


def build_world(chains, k, seed=3):
    rng = np.random.RandomState(seed)
    N = max(1, sum(sum(1 for ch in c.leaves if ch in "ld") for c in chains))
    NX = N + sum(c.leaves.count("o") for c in chains) + 1
    alive = np.zeros(NX, dtype=np.uint8)
    leaf_node, leaf_cls, reg_off, reg_lo, reg_hi, recs = [], [], [0], [], [], []
    init = np.zeros(NX, dtype=np.int64)
    nxt_in, nxt_out = 0, N
    for c in chains:
        reg_lo.append(len(leaf_node))
        for i, ch in enumerate(c.leaves):
            leaf_cls.append(i // c.cls_size if c.cls_size else -1)
            if ch == "-":
                leaf_node.append(-1)
                continue
            n = nxt_out if ch == "o" else nxt_in
            nxt_out, nxt_in = nxt_out + (ch == "o"), nxt_in + (ch != "o")
            leaf_node.append(n)
            alive[n] = ch != "d"
            init[n] = {"zero": 0, "level": 9}.get(c.init, rng.randint(0, 4))
        reg_hi.append(len(leaf_node))
        steps = [(c.tops[j % len(c.tops)], c.weights[j % len(c.tops)]) for j in range(len(c.tops) * c.reps + c.rest)] + [(p, 1) for p in c.tail]
        for top, wt in steps:
            recs.append(record(top, wt, top // c.cls_size if c.cls_size else -1, len(recs)))
        reg_off.append(len(recs))
    w = World(N, NX, reg_off, reg_lo, reg_hi, leaf_node, alive, np.asarray(recs, dtype=np.int64).reshape(-1), leaf_cls, k)
    return w, init


def world_of_find_table(name, k=1):
    """A table of tests/period_case_tables.py as a world: its records name the top leaf (word 4) and its class (word 6: 16 leaves
    a class)."""
    regions, arrays, _ = PT.table(name)
    N, NX, reg_off, reg_lo, reg_hi, leaf_node, alive, crec, _ = arrays
    leaf_cls = [i // 16 for r in regions for i in range(len(r.leaves))]
    return World(N, NX, reg_off, reg_lo, reg_hi, leaf_node, alive, crec, leaf_cls, k), np.zeros(NX, dtype=np.int64)


def find_reference(w):
    """T per region by the definition: the smallest t in [1, min(len - 1, cap)] whose words 1..23 are the first step's."""
    rec = w.crec.reshape(-1, KCW)
    Ts = []
    for r in range(w.B):
        mine = rec[w.reg_off[r]:w.reg_off[r + 1], 1:]
        Ts.append(next((t for t in range(1, min(len(mine) - 1, CAP) + 1) if (mine[t] == mine[0]).all()), INT_MAX))
    return Ts


def expectation(w, init, s, n_states, OW, cut):
    """On the reference alone: one walk of every chain from its first step to its last, and per region (T, limit, must_copy):
    must_copy -- the records are periodic for at least four periods and the walk re-enters its state: the counters after 2T steps
    are those after T steps plus one d >= 0 on every live leaf (no other counter moves in this automaton)."""
    Ts = find_reference(w)
    limits = verify_reference(w.reg_off, w.crec, Ts, [int(w.reg_off[r + 1] - w.reg_off[r]) for r in range(w.B)])
    if cut > 0:
        limits = [min(x, cut) for x in limits]
    cnt = np.full(n_states * w.NX + 1, POISON, dtype=np.int32)
    cnt[s * w.NX:(s + 1) * w.NX] = init
    out = np.full(w.n_steps * OW + 1, POISON, dtype=np.int32)
    kinds = []
    snap = {}
    for r in range(w.B):
        beg, end = w.reg_off.copy(), w.reg_off.copy()                 # (only region r has steps)
        T, limit, cbeg = Ts[r], limits[r], int(w.reg_off[r])
        if not joins(T, limit):
            kinds.append((T, limit, False))
            end[r] = w.reg_off[r + 1]
            walk(w, s, OW, cnt, out, beg, end)
            continue
        end[r] = cbeg + T
        walk(w, s, OW, cnt, out, beg, end)
        snap[r] = cnt.copy()
        beg[r], end[r] = cbeg + T, cbeg + 2 * T
        walk(w, s, OW, cnt, out, beg, end)
        diffs = set(int(cnt[s * w.NX + n]) - int(snap[r][s * w.NX + n]) for n in w.live(r))
        kinds.append((T, limit, len(diffs) == 1 and min(diffs) >= 0))
        beg[r], end[r] = cbeg + 2 * T, w.reg_off[r + 1]
        walk(w, s, OW, cnt, out, beg, end)
    return cnt, out, kinds


def is_round_robin(w):
    """The premise of k_period_find's known mode: every chain is the region's live leaves in leaf order, again and again."""
    rec = w.crec.reshape(-1, KCW)
    for r in range(w.B):
        lo = int(w.reg_lo[r])
        tops = [pos - lo for pos in range(lo, int(w.reg_hi[r])) if 0 <= w.leaf_node[pos] < w.N and w.alive[w.leaf_node[pos]]]
        mine = rec[w.reg_off[r]:w.reg_off[r + 1]]
        if len(mine) and (not tops or tops[0] != mine[0, 4]):
            return False
        for j in range(len(mine)):
            if mine[j, 4] != tops[j % len(tops)] or (mine[j, 1:] != mine[j % len(tops), 1:]).any():
                return False
    return True


def check_pipeline(pk, w, init, cut=0, judge_threads=128, s=1, n_states=2):
    """find, verify, segments, walk, copy, walk, judge, replicate, walk -- the kernels real, the walks the automaton's -- against
    one walk of the whole chain.  Returns per region (T, limit, must_copy, ok)."""
    OW = w.k + 1
    want_cnt, want_out, kinds = expectation(w, init, s, n_states, OW, cut)
    pb = new_pb(w.B)
    assert pk.find(w, pb, 0, 1024) == 0
    assert pk.verify(w.reg_off, w.crec, pb) == 0
    if is_round_robin(w):                                         # the known mode, and no verify: the same words
        known = new_pb(w.B)
        assert pk.find(w, known, 1, 256) == 0
        assert (known == pb).all(), (rows(known)[:4], rows(pb)[:4])
    assert pk.segments(w.reg_off, w.n_steps, cut, pb) == 0
    P = rows(pb)
    cnt = np.full(n_states * w.NX + 1, POISON, dtype=np.int32)
    cnt[s * w.NX:(s + 1) * w.NX] = init
    out = np.full(w.n_steps * OW + 1, POISON, dtype=np.int32)
    flags = np.zeros(CHAIN_FLAGS + 1, dtype=np.int32)
    flags[-1] = POISON
    walk(w, s, OW, cnt, out, P[K_BEG1], P[K_END1])
    cnt1 = cnt.copy()
    walk(w, s, OW, cnt, out, P[K_BEG2], P[K_END2])
    assert pk.judge(w, s, n_states, OW, out, flags, cnt1, cnt, pb, judge_threads) == 0
    assert pk.replicate(w.reg_off, w.n_steps, OW, pb, out) == 0
    walk(w, s, OW, cnt, out, P[K_BEG3], P[K_END3])
    result = []
    for r, (T, limit, must) in enumerate(kinds):
        assert (int(P[K_T, r]), int(P[K_LIMIT, r])) == (T, limit), (r, P[:, r], T, limit)
        # a region of the kind MUST be copied, all of its periodic stretch behind two periods; no other may be
        assert int(P[K_OK, r]) == int(must), (r, P[:, r], T, limit, must)
        assert int(P[K_BEG3, r]) == int(w.reg_off[r]) + (limit if must else 2 * T if joins(T, limit) else int(w.reg_off[r + 1] - w.reg_off[r]))
        result.append((T, limit, must, int(P[K_OK, r])))
    bad = np.flatnonzero(out != want_out)
    assert bad.size == 0, ("out of step", bad[:6] // OW, [int(x) for x in w.reg_off], P)
    bad = np.flatnonzero(cnt != want_cnt)
    assert bad.size == 0, ("counter", bad[:6], cnt[bad[:6]], want_cnt[bad[:6]])
    assert (flags[:-1] == 0).all() and flags[-1] == P32 and pb[-1] == P32
    return result


RING = lambda n, start=0: [(start + i) % n for i in range(n)]   # noqa: E731

# name -> (chains, k, cut)
PIPELINE_WORLDS = {
    "tail_behind_the_stretch": ([Chain("l" * 8, RING(8), 6, rest=3, tail=[5, 5, 1, 0, 7])], 2, 0),
    "tail_of_one_step": ([Chain("l" * 8, RING(8), 4, rest=0, tail=[3])], 1, 0),
    "tail_and_classes": ([Chain("l" * 16, RING(16, 3), 5, rest=9, tail=[0, 0, 2], cls_size=4), Chain("lld-lol", [0, 1, 3, 6], 7, rest=1, tail=[6, 6])], 2, 0),
    "cut_inside_a_period": ([Chain("l" * 8, RING(8), 12, rest=5)], 2, 45),
    "cut_at_four_periods": ([Chain("l" * 8, RING(8), 12, rest=5), Chain("l" * 5, RING(5), 30)], 1, 32),
    "cut_that_keeps_a_region_out": ([Chain("l" * 8, RING(8), 12, rest=5), Chain("l" * 5, RING(5), 30)], 1, 31),
    "cut_above_everything": ([Chain("l" * 8, RING(8), 12, rest=5)], 3, 5000),
    "state_not_re_entered": ([Chain("l" * 6, RING(6), 9, rest=2, init="random"), Chain("l" * 7, [0, 1, 2], 20, rest=1)], 2, 0),
    "too_short_beside_long": ([Chain("l" * 8, RING(8), 3, rest=7), Chain("l" * 8, RING(8), 4), Chain("l" * 3, [], 0)], 1, 0),
    "wide_regions": ([Chain("l" * 192, RING(192), 5, rest=100, cls_size=16), Chain(_mixed(256), [i for i, ch in enumerate(_mixed(256)) if ch == "l"], 4, rest=17)], 3, 0),
    # THE WEIGHT OF THE COUNTED STEPS: as JUDGE_TABLES' case, through the whole form
    "weights_differ_inside_a_period": ([Chain("l" * 64, RING(64) + RING(64), 4, rest=70, weights=[1] * 64 + [2] * 64),
                                        Chain("l" * 64, RING(64) + RING(64), 5, rest=127, weights=[2] * 64 + [1] * 64, tail=[4, 4])], 1, 0),
}
# the tables of k_period_find that have steps
PIPELINE_FIND_TABLES = [n for n, regions in PT.TABLES.items() if any(r.length for r in regions)]


def pipeline_world(name):
    chains, k, cut = PIPELINE_WORLDS[name]
    w, init = build_world(chains, k)
    return w, init, cut


def random_world(seed):
    """At most 3 regions, 64 leaves, k <= 3, T <= 48, 600 steps.  Most regions are rings over their live leaves from level
    counters, which the automaton re-enters; some start from uneven counters, repeat tops inside a period, are too short, or
    have a tail."""
    rng = np.random.RandomState(1000 + seed)
    chains = []
    k = int(rng.randint(1, 4))
    for _ in range(int(rng.randint(1, 4))):
        n = int(rng.randint(2, 65))
        leaves = "".join(rng.choice(list("lllllllld-o")) for _ in range(n))
        live = [i for i, ch in enumerate(leaves) if ch == "l"]
        if not live:
            leaves, live = "l" + leaves[1:], [0]
        live = live[:48]
        odd = rng.randint(0, 16)
        if odd == 0 and len(live) > 2:                            # tops that repeat inside a period (the first only once)
            tops = [live[0]] + [live[i] for i in rng.randint(1, len(live), size=int(rng.randint(2, 20)))]
        else:
            start = int(rng.randint(0, len(live)))
            tops = live[start:] + live[:start]
        T = len(tops)
        reps = int(rng.randint(4, min(12, 192 // T) + 1)) if odd != 1 else int(rng.randint(1, 4))
        rest = int(rng.randint(0, min(T, 192 - T * reps + 1)))
        tail = [int(x) for x in rng.choice(live, size=int(rng.randint(1, 9)))] if odd in (2, 3, 4, 5) else []
        chains.append(Chain(leaves, tops, reps, rest=rest, tail=tail, cls_size=int(rng.choice([0, 0, 2, 4, 16])),
                            weights=[int(rng.choice([1, 1, 2, 3]))] * T, init=str(rng.choice(["zero"] * 5 + ["level"] * 6 + ["random"]))))
    w, init = build_world(chains, k, seed)
    assert w.B <= 3 and max(len(c.leaves) for c in chains) <= 64 and w.n_steps <= 600
    return w, init


RANDOM_SEEDS = list(range(40))


# =============================================================================================================================
# The stand-alone sanitizer program's case file
# =============================================================================================================================

def write_program_input(path, judge_runs, replicate_runs):
    """judge_runs: (table, threads, escaped); replicate_runs: (table, OW).  One case a block: a line of numbers, then a line
    per array.  Returns what the program must print, line by line."""
    want = []
    line = lambda a: " ".join(str(int(x)) for x in a) + "\n"    # noqa: E731
    with open(path, "w") as f:
        for name, threads, escaped in judge_runs:
            (w, out, flags, cnt1, cnt, pb), (want_cnt, want_pb, _) = judge_table(name, escaped)
            _, _, s, n_states, OW = JUDGE_TABLES[name]
            f.write("J %d %d %d %d %d %d %d %d %d\n" % (w.B, threads, s, n_states, w.N, w.NX, OW, w.n_steps, len(w.leaf_node)))
            for a in (w.reg_off, w.reg_lo, w.reg_hi, w.leaf_node, w.alive, w.crec, out, flags, cnt1, cnt, pb):
                f.write(line(a))
            want.append("J 0 " + " ".join(line(a).strip() for a in (want_cnt, want_pb, out, flags, cnt1)))
        for name, OW in replicate_runs:
            regions = REPLICATE_TABLES[name]
            reg_off = i32(np.concatenate([[0], np.cumsum([g[2] for g in regions])]))
            pb = new_pb(len(regions))
            for r, (T, limit, _, ok) in enumerate(regions):
                rows(pb)[K_T, r], rows(pb)[K_LIMIT, r], rows(pb)[K_OK, r] = T, limit, ok
            out = i32(np.random.RandomState(OW).randint(-2 ** 31, 2 ** 31 - 1, size=int(reg_off[-1]) * OW + 1))
            f.write("R %d 256 %d %d\n" % (len(regions), OW, int(reg_off[-1])))
            for a in (reg_off, pb, out):
                f.write(line(a))
            want.append("R 0 " + " ".join(line(a).strip() for a in (pb, replicate_reference(reg_off, rows(pb), OW, out))))
    return want
