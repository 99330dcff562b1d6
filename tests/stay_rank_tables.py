"""k_stay_by_top's rank function alone (stay_round_ranks, blance_amd/csrc/k_stay.h): the cases, a plain reference and the
check, shared by tests/test_stay_ranks_emulated.py (SIMT emulator) and tests/test_stay_ranks_gpu.py (device).

A round is 64 lanes of KM slots; a slot holds a leaf of a region of `size` leaves, or -1 for "no such node".  The rank of
(lane, slot j) is the number of (earlier lane, slot j2) pairs that hold the same leaf: a leaf an earlier lane holds in two
slots counts twice, and -1 matches nothing and has rank 0.  Lanes from `nv` on hold -1 everywhere, as in the kernel."""
import ctypes as C
import random

import numpy as np

KMS = (2, 4)
SIZES = (1, 2, 3, 64, 128, 129, 256, 257, 512)        # bit counts 0 .. 9 of the leaf index
NVS = (1, 2, 63, 64)
BAD_ARG = -100


def reference(round_, km):
    """[64][km] ranks of one round [64][km], by the definition."""
    rk = [[0] * km for _ in range(64)]
    for lane in range(64):
        for j in range(km):
            x = round_[lane][j]
            if x < 0:
                continue
            rk[lane][j] = sum(1 for e in range(lane) for j2 in range(km) if round_[e][j2] == x)
    return rk


def rounds_for(km, size):
    """The rounds of one (KM, size): a list of (name, [64][km])."""
    top = size - 1
    out = []

    def add(name, f, nvs=NVS):
        for nv in nvs:
            r = [[-1] * km for _ in range(64)]
            for lane in range(nv):
                r[lane] = [int(v) for v in f(lane)]
                assert len(r[lane]) == km and all(-1 <= v < size for v in r[lane]), (name, r[lane])
            out.append(("%s nv=%d" % (name, nv), r))

    add("all the same leaf", lambda l: [top] * km)
    add("all the same leaf 0", lambda l: [0] + [-1] * (km - 1))
    add("all distinct", lambda l: [(l * km + j) % size if l * km + j < size else -1 for j in range(km)])
    add("distinct from the top down", lambda l: [top - (l * km + j) if l * km + j < size else -1 for j in range(km)])
    add("one leaf in two slots", lambda l: [(l // 2) % size, (l // 2) % size] + [-1] * (km - 2))
    add("one leaf in the first and the last slot", lambda l: [(3 * l) % size] + [-1] * (km - 2) + [(3 * l) % size])
    add("-1 in slot 0 only", lambda l: [-1] + [(l + j) % size for j in range(1, km)])
    add("-1 in slot 1 only", lambda l: [l % size, -1] + [(l + j) % size for j in range(2, km)])
    for prefix in (1, 5, 40, 64):
        add("-1 in every slot of the first %d lanes" % prefix,
            lambda l, p=prefix: [-1] * km if l < p else [(l + j) % min(size, 7) for j in range(km)], nvs=(63, 64))
    # the highest leaf held by lane 0 and by lane 63, other leaves (and its lower neighbours in bits) between them
    add("the highest leaf in lanes 0 and 63",
        lambda l: [top] * km if l in (0, 63) else [(top ^ (1 << (l % 9))) % size if l % 2 else l % size] + [top if l == 31 else -1] * (km - 1),
        nvs=(64,))
    # a leaf and the leaf one bit of it away, bit by bit: a bit too few merges them
    for b in range(9):
        if (1 << b) < size:
            add("leaves that differ in bit %d" % b,
                lambda l, b=b: [((top ^ (1 << b)) if l % 2 else top) % size, ((l % 3) << b) % size] + [-1] * (km - 2), nvs=(64,))
    rnd = random.Random(1000 * km + size)
    for i in range(16):                                             # (288 in all)
        nv = rnd.choice(NVS + (rnd.randrange(1, 65),))
        span = rnd.choice([1, 2, 3, 8, size])                       # few values: many equals
        base = rnd.randrange(0, size)
        r = [[-1] * km for _ in range(64)]
        for lane in range(nv):
            for j in range(km):
                if rnd.random() >= 0.15:
                    r[lane][j] = (base + rnd.randrange(0, span)) % size
        out.append(("random %d nv=%d" % (i, nv), r))
    return out


class RankCases:
    def __init__(self, lib_path):
        self.lib = C.CDLL(lib_path)
        self.lib.blance_case_stay_ranks.restype = C.c_int
        self.lib.blance_case_stay_ranks.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]

    def ranks(self, km, size, rounds):
        """(status, [rounds][64][km]) of one call."""
        a = np.ascontiguousarray(np.asarray(rounds, dtype=np.int32).reshape(len(rounds), 64, km))
        out = np.full(a.shape, -7, dtype=np.int32)
        st = self.lib.blance_case_stay_ranks(km, size, len(rounds), a.ctypes.data, out.ctypes.data)
        return st, out


_expected = {}


def expected(km, size):
    """The rounds of (km, size) and their reference ranks, computed once."""
    if (km, size) not in _expected:
        rs = rounds_for(km, size)
        _expected[(km, size)] = (rs, [reference(r, km) for _, r in rs])
    return _expected[(km, size)]


def check(rc, km, size):
    rs, want = expected(km, size)
    st, got = rc.ranks(km, size, [r for _, r in rs])
    assert st == 0, st
    for i, (name, r) in enumerate(rs):
        assert got[i].tolist() == want[i], (km, size, name, r, got[i].tolist(), want[i])


def check_refusals(rc):
    for km in KMS:
        r = [[-1] * km for _ in range(64)]
        for size, bad in ((1, 1), (3, 3), (256, 256), (512, 512), (128, -2)):
            r2 = [row[:] for row in r]
            r2[17][km - 1] = bad
            st, got = rc.ranks(km, size, [r, r2])
            assert st == BAD_ARG, (km, size, bad, st)
            assert (got == -7).all()                                   # (nothing ran)
        assert rc.ranks(km, 513, [r])[0] == BAD_ARG
        assert rc.ranks(km, 0, [r])[0] == BAD_ARG
    assert rc.ranks(3, 8, [[[-1] * 3 for _ in range(64)]])[0] == BAD_ARG


def table_has_both_kinds():
    """On the reference alone: (rounds with a rank above 0, rounds with a rank of two or more from one earlier lane's two
    slots, number of rounds)."""
    n = pos = twice = 0
    for km in KMS:
        for size in SIZES:
            rs, want = expected(km, size)
            for (name, r), w in zip(rs, want):
                n += 1
                pos += any(v > 0 for row in w for v in row)
                twice += "two slots" in name and any(v >= 2 for row in w for v in row)
    return pos, twice, n
