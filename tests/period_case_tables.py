"""k_period_find alone (blance_amd/csrc/k_period.h): hand-made region tables and chain records, the reference and the check,
shared by tests/test_period_cases_emulated.py (SIMT emulator) and tests/test_period_cases_gpu.py (device).

A region is a run of leaves, each with a node or none (-1); a node is alive (a candidate: in nodesNext), dead, or outside the
cluster's first N ids.  Its chain is what the pass behind a round robin gathers: the region's alive nodes in leaf order, again
and again, `len` steps, from any place of the cycle; words 1..23 of a record are a function of the step's top priority node,
word 0 is the step's own index.  The searched mode finds the period in the records, the known mode counts the alive leaves:
both must leave T, limit, ok and d as the reference says, and every other word of the buffer as it was."""
import ctypes as C

import numpy as np

KCW = 24
CAP = 4096                       # kPeriodCap
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
POISON = 0x5a5a5a5a
BAD_ARG = -100
K_T, K_LIMIT, K_OK, K_D = 0, 1, 2, 3


class Region:
    def __init__(self, leaves, length, start=0, dead=(), outside=()):
        """leaves: per leaf True (a node) or False (none); dead / outside: places among the leaves whose node is no candidate
        (not alive / an id of N or more)."""
        self.leaves, self.length, self.start, self.dead, self.outside = list(leaves), length, start, set(dead), set(outside)


def full(n, length, **kw):
    return Region([True] * n, length, **kw)


# name -> the regions of one table (B = their number)
TABLES = {
    # ---- B = 1: 1, 16, 120 and 192 alive leaves
    "one_leaf": [full(1, 9)],
    "16_leaves": [full(16, 16 * 31 + 4)],
    "120_of_128_leaves": [Region([i % 16 != 5 for i in range(128)], 120 * 12 + 7)],
    "192_leaves": [full(192, 1500, start=77)],
    # ---- fewer steps than nodes, as many, one more (the first candidate that can be found), no step at all
    "fewer_steps_than_nodes": [full(128, 100)],
    "as_many_steps_as_nodes": [full(128, 128)],
    "one_step_more_than_nodes": [full(128, 129)],
    "no_steps": [full(128, 0)],
    "one_step": [full(16, 1)],
    # ---- the chain's length no multiple of the period; the chain starting inside the cycle
    "len_no_multiple": [full(16, 16 * 7 + 9, start=5)],
    # ---- leaves that are no candidates: a dead node, a node outside the first N ids, no node
    "dead_and_outside_nodes": [Region([i != 3 for i in range(64)], 64 * 6 + 1, dead=(0, 17, 63), outside=(9, 40))],
    "nothing_alive": [Region([True] * 8, 0, dead=range(8))],
    # ---- B = 3: regions of different widths and lengths, an empty chain between two others
    "three_regions": [full(128, 128 * 16), full(122, 122 * 4 + 121, start=3), Region([i % 17 != 5 for i in range(128)], 2000)],
    "three_regions_middle_empty": [full(16, 200), full(16, 0), full(12, 13)],
    "three_regions_short": [full(128, 100), full(1, 2), full(192, 193)],
    # ---- at and beyond kPeriodCap: 4,096 alive leaves with 4,097 steps (the last candidate), with 9,000; 4,100 alive leaves
    "period_at_the_cap": [full(CAP, CAP + 1)],
    "period_at_the_cap_long": [full(CAP, 9000, start=11)],
    "period_past_the_cap": [full(CAP + 4, 5000)],
}


def build(regions):
    """The arrays of one table: (N, NX, reg_off, reg_lo, reg_hi, leaf_node, alive, crec, alive counts)."""
    n_in = sum(sum(1 for i, has in enumerate(r.leaves) if has and i not in r.outside) for r in regions)
    n_out = sum(len(r.outside) for r in regions)
    N, NX = max(n_in, 1), max(n_in, 1) + n_out + 1
    alive = np.zeros(NX, dtype=np.uint8)
    leaf_node, reg_off, reg_lo, reg_hi, recs, counts = [], [0], [], [], [], []
    nxt_in, nxt_out, step = 0, N, 0
    for r in regions:
        lo = len(leaf_node)
        tops = []                                                 # (local leaf) of the alive nodes, in leaf order
        for i, has in enumerate(r.leaves):
            if not has:
                leaf_node.append(-1)
            elif i in r.outside:
                leaf_node.append(nxt_out)
                alive[nxt_out] = 1                                    # (alive, but no id of the cluster: k_period_judge's n < N)
                nxt_out += 1
            else:
                leaf_node.append(nxt_in)
                if i not in r.dead:
                    alive[nxt_in] = 1
                    tops.append(i)
                nxt_in += 1
        reg_lo.append(lo)
        reg_hi.append(len(leaf_node))
        counts.append(len(tops))
        assert r.length == 0 or tops
        for j in range(r.length):
            leaf = tops[(r.start + j) % len(tops)]
            rec = [-1] * KCW
            rec[0] = 100000 + 7 * step                             # (the step's pass index: never equal, never compared)
            rec[1] = 1
            rec[2], rec[3] = 0, 0x3ff80000                          # stick = 1.5
            rec[4] = leaf
            rec[5] = 1 << 24
            rec[6] = leaf // 16
            rec[23] = 16
            recs.append(rec)
            step += 1
        reg_off.append(step)
    i32 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.int32))   # noqa: E731
    crec = i32(recs).reshape(-1) if recs else np.zeros(0, dtype=np.int32)
    return N, NX, i32(reg_off), i32(reg_lo), i32(reg_hi), i32(leaf_node), alive, crec, counts


def reference(regions, counts):
    """[(T, limit, ok, d)] by the definition: the smallest t in [1, min(len - 1, cap)] whose record equals the first step's is
    the number of alive leaves, when that is a candidate at all."""
    out = []
    for r, count in zip(regions, counts):
        last = min(r.length - 1, CAP)
        out.append((count if 1 <= count <= last else INT_MAX, r.length, 0, INT_MIN))
    return out


class PeriodCases:
    def __init__(self, lib_path):
        self.lib = C.CDLL(lib_path)
        self.lib.blance_case_period_words.restype = C.c_int
        self.lib.blance_case_period_find.restype = C.c_int
        self.lib.blance_case_period_find.argtypes = [C.c_int] * 7 + [C.c_void_p] * 7
        self.words = self.lib.blance_case_period_words()

    def find(self, arrays, B, known, threads):
        """(status, pb[kPWords][B]) of one launch over a buffer of POISON."""
        N, NX, reg_off, reg_lo, reg_hi, leaf_node, alive, crec, _ = arrays
        pb = np.full((self.words, B), POISON, dtype=np.int32)
        keep = crec if crec.size else np.zeros(1, dtype=np.int32)
        leaves = leaf_node if leaf_node.size else np.zeros(1, dtype=np.int32)
        st = self.lib.blance_case_period_find(B, int(known), threads, N, NX, len(crec) // KCW, len(leaf_node), reg_off.ctypes.data,
                                              reg_lo.ctypes.data, reg_hi.ctypes.data, leaves.ctypes.data, alive.ctypes.data,
                                              keep.ctypes.data, pb.ctypes.data)
        return st, pb


_built = {}


def table(name):
    if name not in _built:
        regions = TABLES[name]
        arrays = build(regions)
        _built[name] = (regions, arrays, reference(regions, arrays[-1]))
    return _built[name]


def check(pc, name):
    regions, arrays, want = table(name)
    B = len(regions)
    assert pc.words >= 10
    got = {}
    # (the searched mode on the product's 1,024 threads and on one wave: more than one trip over the candidates; the known
    # mode on the product's 256 and on one wave: more than one trip over the leaves)
    for known, threads in ((0, 1024), (0, 64), (1, 256), (1, 64)):
        if not known and threads == 64 and max(r.length for r in regions) > 3000:
            continue                                              # (thousands of trips of one wave: the emulator's minutes)
        st, pb = pc.find(arrays, B, known, threads)
        assert st == 0, (name, known, threads, st)
        for r in range(B):
            assert tuple(int(pb[w][r]) for w in (K_T, K_LIMIT, K_OK, K_D)) == want[r], (name, known, threads, r, pb[:4, r], want[r])
        assert (pb[4:] == np.int32(POISON)).all(), (name, known, threads)
        got[(known, threads)] = pb
    assert (got[(0, 1024)] == got[(1, 256)]).all(), name


def check_refusals(pc):
    regions, arrays, _ = table("three_regions")
    N, NX, reg_off, reg_lo, reg_hi, leaf_node, alive, crec, counts = arrays

    def refused(**change):
        a = dict(N=N, NX=NX, reg_off=reg_off.copy(), reg_lo=reg_lo.copy(), reg_hi=reg_hi.copy(), leaf_node=leaf_node.copy(), crec=crec)
        a.update(change)
        st, pb = pc.find((a["N"], a["NX"], a["reg_off"], a["reg_lo"], a["reg_hi"], a["leaf_node"], alive, a["crec"], counts), 3, 1, 256)
        assert st == BAD_ARG and (pb == np.int32(POISON)).all(), (change.keys(), st)              # (nothing ran)

    off = reg_off.copy(); off[3] += 1
    refused(reg_off=off)                                          # a chain past the records
    off = reg_off.copy(); off[1], off[2] = off[2], off[1]
    refused(reg_off=off)                                          # not monotone
    hi = reg_hi.copy(); hi[2] += 1
    refused(reg_hi=hi)                                            # leaves past the table
    lo = reg_lo.copy(); lo[0] = -1
    refused(reg_lo=lo)
    leaf = leaf_node.copy(); leaf[5] = NX
    refused(leaf_node=leaf)                                       # a node past `alive`
    refused(N=NX + 1)
    assert pc.find(arrays, 3, 1, 100)[0] == BAD_ARG                # (no workgroup size of the driver's)
