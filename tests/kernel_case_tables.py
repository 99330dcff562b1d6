"""The single-kernel cases: binding, case tables, references and checks shared by tests/test_kernel_cases_emulated.py (the
SIMT emulator) and tests/test_kernel_cases_gpu.py (the device).  Both run exactly the same tables through the same entries
(tests/kernels/kernel_cases.inc); only the library differs.

The references are plain numpy / Python written from each operation's definition: a shifted cumsum, a stable argsort, a
bincount, a heap of (score, node), an automaton walked one step at a time, a greedy with the excluded node left out.
Everything is integers or IEEE fp64 with contraction off, so every comparison is exact equality.

Every table is generated from fixed seeds: the two modules see the same bytes."""
import ctypes
import functools
import heapq
import itertools

import numpy as np

INT_MAX = 2 ** 31 - 1
GUARD = 0x5A5A5A5A                                   # what the entries fill outputs and their guard words with
BAD_ARG = -100                                       # kCaseBadArg
SCAN_TILE, PART_CHUNK, SORT_TILE = 8192, 1024, 2048  # kScanTile, kPartChunk, kSortTile
U64 = np.uint64


# ---- binding ----------------------------------------------------------------------------------------------------------------

def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _i32(x):
    return np.ascontiguousarray(x, dtype=np.int32)


def _u8(x):
    return np.ascontiguousarray(x, dtype=np.uint8)


class KernelCases:
    """The entries of kernel_cases.inc in one loaded library.  A non-zero return raises, except where a test asks for the
    code (check=False)."""

    def __init__(self, path):
        self.lib = lib = ctypes.CDLL(path)
        vp, ci, cu64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_ulonglong
        sigs = {
            "kcase_scan_excl": [ci, vp],
            "kcase_group_by_key": [ci, vp, vp, ci, vp, vp, vp],
            "kcase_partition_category": [ci, vp, vp, vp],
            "kcase_category_buckets": [],
            "kcase_radix_sort": [ci, vp, vp, ci, cu64, vp, vp, vp],
            "kcase_sort_varbits": [ci, vp, vp],
            "kcase_flat_scan_min": [ci, vp, ci, ci, ci, vp, vp],
            "kcase_flat_row_count": [ci, ci, vp, vp],
            "kcase_fresh_select": [ci, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, vp, vp, vp],
            "kcase_fresh_excl": [ci, ci, ci, vp, vp, vp, vp],
            "kcase_fresh_excl_shape": [ci, vp, vp],
        }
        for name, args in sigs.items():
            f = getattr(lib, name)
            f.argtypes, f.restype = args, ci
        lib.blance_last_error.restype = ctypes.c_char_p

    def _ok(self, rc, check=True):
        if check and rc != 0:
            raise RuntimeError("kernel case entry returned %d: %s" % (rc, self.lib.blance_last_error().decode()))
        return rc

    def scan_excl(self, data, guard):
        buf = _i32(np.concatenate([data, [guard]]))
        self._ok(self.lib.kcase_scan_excl(len(data), _p(buf)))
        return buf[:-1], int(buf[-1])

    def group_by_key(self, key, src, B, want_oi, check=True):
        n = len(key)
        key = _i32(key)
        src = None if src is None else _i32(src)
        offs, out = np.zeros(B + 2, np.int32), np.zeros(n + 1, np.int32)
        oi = np.zeros(n + 1, np.int32) if want_oi else None
        rc = self._ok(self.lib.kcase_group_by_key(n, _p(key), _p(src), B, _p(offs), _p(out), _p(oi)), check)
        return rc, offs, out, oi

    def partition_category(self, cat, index, check=True):
        n = len(cat)
        cat, index = _u8(cat), _i32(index)
        out = np.zeros(n + 1, np.int32)
        rc = self._ok(self.lib.kcase_partition_category(n, _p(cat), _p(index), _p(out)), check)
        return rc, out

    def category_buckets(self):
        return self.lib.kcase_category_buckets()

    def radix_sort(self, keys, vals, known_varying=None):
        n = len(keys)
        keys, vals = np.ascontiguousarray(keys, dtype=U64), _i32(vals)
        out, in_a, launches = np.zeros(n, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int64)
        self._ok(self.lib.kcase_radix_sort(n, _p(keys), _p(vals), 0 if known_varying is None else 1,
                                           int(known_varying or 0), _p(out), _p(in_a), _p(launches)))
        return out, int(in_a[0]), int(launches[0])

    def sort_varbits(self, keys):
        keys = np.ascontiguousarray(keys, dtype=U64)
        out = np.zeros(1, U64)
        self._ok(self.lib.kcase_sort_varbits(len(keys), _p(keys), _p(out)))
        return int(out[0])

    def flat_scan_min(self, part, with_scan, with_not_whole, end, sentinel=-7):
        part = _i32(part)
        scan, nw = np.full(2, sentinel, np.int32), np.full(1, sentinel, np.int32)
        self._ok(self.lib.kcase_flat_scan_min(part.shape[1], _p(part), int(with_scan), int(with_not_whole), end, _p(scan), _p(nw)))
        return [int(scan[0]), int(scan[1])], int(nw[0])

    def flat_row_count(self, top, N, check=True):
        top = _i32(top)
        rows = np.zeros(N + 1, np.int32)
        rc = self._ok(self.lib.kcase_flat_row_count(len(top), N, _p(top), _p(rows)), check)
        return rc, rows

    def fresh_select(self, c, R, int_keys=0, cycle=0, check=True):
        N = c["N"]
        m, moff, seq = np.zeros(N, np.int32), np.zeros(N + 1, np.int32), np.zeros(R, np.int32)
        rc = self._ok(self.lib.kcase_fresh_select(N, _p(_u8(c["alive"])), _p(_i32(c["cnt"])), _p(_i32(c["tot"])), _p(_i32(c["ntn"])),
                                                  _p(_i32(c["node_w"])), _p(_u8(c["has_w"])), c["NP"], c["booster"], c["w"], R,
                                                  int_keys, cycle, _p(m), _p(moff), _p(seq)), check)
        return rc, m, moff, seq

    def fresh_excl(self, N, k, S, excl, check=True):
        R = len(excl)
        S, excl = _i32(S), _i32(excl)
        assert len(S) == k * R + k
        picks, bad = np.zeros(k * R, np.int32), np.zeros(1, np.int32)
        rc = self._ok(self.lib.kcase_fresh_excl(N, k, R, _p(S), _p(excl), _p(picks), _p(bad)), check)
        return rc, picks, int(bad[0])

    def fresh_excl_shape(self, R):
        G, per = np.zeros(1, np.int32), np.zeros(1, np.int32)
        self._ok(self.lib.kcase_fresh_excl_shape(R, _p(G), _p(per)))
        return int(G[0]), int(per[0])


def _rng(*seed):
    return np.random.default_rng([20260919] + [int(s) for s in seed])


# ---- a. exclusive scan ------------------------------------------------------------------------------------------------------

# 4 * 8192 is the last size of the one-workgroup path; the last three take tile sums -> scan -> apply
SCAN_SIZES = [1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 8191, 8192, 8193, 4 * 8192 - 1, 4 * 8192, 4 * 8192 + 1, 5 * 8192 - 3,
              9 * 8192 + 5]
SCAN_KINDS = ["random", "zeros", "ones", "last_only", "first_of_last_tile", "total_int_max"]


def scan_data(n, kind):
    r = _rng(1, n)
    if kind == "random":
        return r.integers(0, 1001, n)
    if kind == "zeros":
        return np.zeros(n, np.int64)
    if kind == "ones":
        return np.ones(n, np.int64)
    d = np.zeros(n, np.int64)
    if kind == "last_only":
        d[n - 1] = 12345
    elif kind == "first_of_last_tile":
        d[((n - 1) // SCAN_TILE) * SCAN_TILE] = 54321
    elif kind == "total_int_max":                    # the total, which the scan forms as its carry, is exactly 2^31 - 1
        d = r.integers(0, INT_MAX // n + 1, n) if n > 1 else d
        d[r.integers(0, n)] += INT_MAX - int(d.sum())
    return d


def check_scan(kc, n):
    for kind in SCAN_KINDS:
        d = scan_data(n, kind)
        want = np.concatenate([[0], np.cumsum(d.astype(np.int64))])          # want[n]: the total
        assert 0 <= want.min() and want.max() <= INT_MAX, "the case itself leaves int32"
        if kind == "total_int_max":
            assert want[n] == INT_MAX
        got, guard = kc.scan_excl(d, 0x7EADBEEF)
        assert guard == 0x7EADBEEF, (n, kind, "the word behind data[n - 1] was written")
        assert np.array_equal(got, want[:n]), (n, kind, int(np.argmax(got != want[:n])))


# ---- b. stable counting sort ------------------------------------------------------------------------------------------------

PART_SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 3 * 1024 + 17]
PART_BUCKETS = [1, 2, 3, 64, 65, 257, 1000]
PART_KINDS = ["first_bucket", "middle_bucket", "last_bucket", "empty_buckets", "random", "descending"]


def part_keys(n, B, kind):
    r = _rng(2, n, B)
    if kind == "first_bucket":
        return np.zeros(n, np.int64)
    if kind == "middle_bucket":
        return np.full(n, B // 2, np.int64)
    if kind == "last_bucket":
        return np.full(n, B - 1, np.int64)
    if kind == "empty_buckets":                      # every third bucket used, at most four of them
        used = np.arange(0, B, 3)[-4:]
        return used[r.integers(0, len(used), n)]
    if kind == "random":
        return r.integers(0, B, n)
    return ((n - 1 - np.arange(n, dtype=np.int64)) * B) // n       # never ascending; strictly descending where B >= n


def check_group_by_key(kc, n):
    for B in PART_BUCKETS:
        for kind in PART_KINDS:
            key = part_keys(n, B, kind)
            assert key.min() >= 0 and key.max() < B
            order = np.argsort(key, kind="stable")
            offs_want = np.concatenate([[0], np.cumsum(np.bincount(key, minlength=B))])
            src = _rng(3, n, B).integers(-2 ** 31, 2 ** 31, n)
            for use_src, want_oi in ((True, True), (False, False), (False, True)):
                _, offs, out, oi = kc.group_by_key(key, src if use_src else None, B, want_oi)
                tag = (n, B, kind, use_src, want_oi)
                assert np.array_equal(offs[:B + 1], offs_want), tag
                assert offs[B + 1] == GUARD and out[n] == GUARD, tag
                assert np.array_equal(out[:n], src[order].astype(np.int32) if use_src else order), tag
                if want_oi:
                    assert oi[n] == GUARD, tag
                    assert np.array_equal(oi[:n], order), tag
                    for b in np.unique(key):         # stability, said on its own: inside a bucket the positions ascend
                        seg = oi[offs_want[b]:offs_want[b + 1]]
                        assert np.all(np.diff(seg) > 0) and np.all(key[seg] == b), tag


def check_group_by_key_refuses(kc):
    """A key outside [0, B) must come back as an error code without a launch (it would index LDS and the counts)."""
    for bad in (-1, 5, 2 ** 30):
        key = np.array([0, 1, bad, 2])
        rc, offs, out, _ = kc.group_by_key(key, None, 5, False, check=False)
        assert rc == BAD_ARG and not offs.any() and not out.any()


CAT_KINDS = ["random", "all_0", "all_1", "all_2", "descending", "ascending"]


def check_partition_category(kc, n):
    B = kc.category_buckets()
    assert B == 3                                    # partitionSorter's categories (plan.go:542-561)
    for kind in CAT_KINDS:
        r = _rng(4, n, CAT_KINDS.index(kind))
        if kind == "random":
            cat = r.integers(0, B, n)
        elif kind.startswith("all_"):
            cat = np.full(n, int(kind[-1]))
        else:
            cat = (np.arange(n) * B) // n
            if kind == "descending":
                cat = cat[::-1]
        for index in (np.arange(n), r.permutation(n)):
            _, out = kc.partition_category(cat, index)
            want = index[np.argsort(cat[index], kind="stable")]
            assert out[n] == GUARD, (n, kind)
            assert np.array_equal(out[:n], want), (n, kind)
    rc, out = kc.partition_category(np.array([0, 3, 1]), np.arange(3), check=False)
    assert rc == BAD_ARG and not out.any()
    rc, out = kc.partition_category(np.array([0, 2, 1]), np.array([0, 3, 1]), check=False)
    assert rc == BAD_ARG and not out.any()


# ---- c. radix sort of pairs -------------------------------------------------------------------------------------------------

SORT_SIZES = [1, 2, 63, 64, 65, 2047, 2048, 2049, 3 * 2048 + 1]
SORT_BIG = 128 * 2048 + 1                            # the smallest n whose histogram (256 per tile) scans in tiles: 256 * 129 > 4 * 8192
SORT_KINDS = ["all_equal", "top_byte", "low_byte", "bytes_0_7", "bytes_0_3_7", "doubles", "duplicates", "random64"]


def sortable_key(v):
    """The order-preserving image of fp64 in uint64 (k_flat.h: sortable_key), from its definition: -0.0 counts as +0.0, a
    negative number's bits are inverted, a positive one's sign bit is set."""
    v = np.where(v == 0.0, 0.0, np.asarray(v, dtype=np.float64))
    u = v.view(U64)
    return np.where(u >> U64(63) != 0, ~u, u | U64(1 << 63))


def sort_keys(n, kind):
    r = _rng(5, n, SORT_KINDS.index(kind))
    base = U64(0x1234567800ABCD00)
    byte = lambda: r.integers(0, 256, n).astype(U64)
    if kind == "all_equal":
        return np.full(n, base | U64(0x42), U64)
    if kind == "top_byte":
        return (base & U64(0x00FFFFFFFFFFFFFF)) | (byte() << U64(56))
    if kind == "low_byte":
        return base | byte()
    if kind == "bytes_0_7":
        return (base & U64(0x00FFFFFFFFFFFFFF)) | byte() | (byte() << U64(56))
    if kind == "bytes_0_3_7":
        return (base & U64(0x00FFFFFF00FFFFFF)) | byte() | (byte() << U64(24)) | (byte() << U64(56))
    if kind == "doubles":
        special = np.array([-0.0, 0.0, -1.5, 1.5, 5e-324, -5e-324, 2.2250738585072009e-308, np.inf, -1e300, 1e300, 0.0, -0.0])
        v = np.concatenate([special, r.normal(0, 1e3, n)])[:n]
        return sortable_key(r.permutation(v) if n > 2 else v)
    if kind == "duplicates":
        return r.integers(0, 2 ** 63, 5).astype(U64)[r.integers(0, 5, n)]
    return r.integers(0, 2 ** 64, n, dtype=U64)


def varying_bits(keys):
    return int(np.bitwise_or.reduce(keys ^ keys[0]))


def _passes(varying):
    return sum(1 for s in range(0, 64, 8) if (varying >> s) & 0xFF)


def check_radix_one(kc, keys, tag, supersets=True):
    n = len(keys)
    vals = (np.arange(n, dtype=np.int64) * 7 + 3).astype(np.int32)           # distinct: a stable sort has ONE right answer
    want = vals[np.argsort(keys, kind="stable")]
    exact = varying_bits(keys)
    runs = [None, exact]
    if supersets:
        runs += [exact | (0xFF << 16), exact | (1 << 63) | 1, 2 ** 64 - 1]
    for known in runs:
        got, in_a, launches = kc.radix_sort(keys, vals, known)
        npass = _passes(exact if known is None else known)
        assert np.array_equal(got, want), (tag, known)
        assert in_a == (1 if npass % 2 == 0 else 0), (tag, known, "which buffer the values ended in")
        assert launches == 3 * npass + (1 if known is None else 0), (tag, known)
    if exact == 0:                                   # no pass at all: buffer a itself, untouched
        got, in_a, launches = kc.radix_sort(keys, vals, None)
        assert in_a == 1 and launches == 1 and np.array_equal(got, vals), tag


def check_radix(kc, n):
    for kind in SORT_KINDS:
        keys = sort_keys(n, kind)
        check_radix_one(kc, keys, (n, kind))


def check_radix_doubles_order(kc):
    """The sort of sortable_key images orders the doubles themselves: -0.0 and +0.0 tie (and keep their order), negatives,
    subnormals and +inf fall where < puts them."""
    v = np.array([0.0, -0.0, 1.0, -1.0, 5e-324, -5e-324, np.inf, -np.inf, 0.0, -0.0, 2.0 ** -1050, -2.0 ** -1050, 1e308, -1e308])
    keys = sortable_key(v)
    assert keys[0] == keys[1]
    got, _, _ = kc.radix_sort(keys, np.arange(len(v)), None)
    assert np.array_equal(got, np.argsort(v, kind="stable"))                 # (numpy's < on doubles: -0.0 == 0.0)


def check_radix_big(kc):
    keys = sort_keys(SORT_BIG, "bytes_0_7")
    assert 256 * (-(-SORT_BIG // SORT_TILE)) > 4 * SCAN_TILE
    check_radix_one(kc, keys, ("big", "bytes_0_7"), supersets=False)


VARBITS_SIZES = [1, 15, 16, 17, 16 * 64 - 1, 16 * 64, 16 * 64 + 1, 16 * 256 - 1, 16 * 256, 16 * 256 + 1, 3 * 16 * 256 + 5]
VARBITS_DIFFS = [1, 1 << 63, 0x0100000000000080, 0x00000001_80000000]


def check_varbits(kc, n):
    base = 0x0F0F0F0F12345678
    assert kc.sort_varbits(np.full(n, base, U64)) == 0
    for idx in sorted({0, 1, n - 1} & set(range(n))):
        for diff in VARBITS_DIFFS:
            keys = np.full(n, base, U64)
            keys[idx] ^= U64(diff)
            want = varying_bits(keys)
            assert want == (diff if n > 1 else 0)
            assert kc.sort_varbits(keys) == want, (n, idx, hex(diff))
    keys = _rng(6, n).integers(0, 2 ** 64, n, dtype=U64) & U64(0x00FF00FFFF0000FF)
    assert kc.sort_varbits(keys) == varying_bits(keys), n


# ---- d. k_flat_scan_min, k_flat_row_count -----------------------------------------------------------------------------------

SCAN_MIN_WAVES = [1, 15, 16, 17, 1023, 1024, 1025, 5000]


def check_flat_scan_min(kc, n_waves):
    r = _rng(7, n_waves)
    low = 4321

    def row(where):
        v = r.integers(low + 10, 10 ** 6, n_waves)
        if where == "absent":
            return np.full(n_waves, INT_MAX)
        v[0 if where == "first" else n_waves - 1] = low
        return v

    for w0, w1 in (("first", "last"), ("last", "absent"), ("absent", "first"), ("last", "last")):
        part = np.stack([row(w0), row(w1)])
        m0, m1 = int(part[0].min()), int(part[1].min())
        ends = [low - 1, low, low + 1] if w0 != "absent" else [0, INT_MAX]
        for with_scan, with_nw, end in itertools.product((1, 0), (1, 0), ends):
            scan, nw = kc.flat_scan_min(part, with_scan, with_nw, end)
            tag = (n_waves, w0, w1, with_scan, with_nw, end)
            assert scan == ([m0, m1] if with_scan else [-7, -7]), tag
            assert nw == ((1 if m0 < end else 0) if with_nw else -7), tag


ROW_COUNT_P = [1, 63, 64, 65, 300]
ROW_COUNT_HOLES = ["nowhere", "lane_0", "lane_63", "last_wave", "many"]


def check_flat_row_count(kc, P):
    N = 5                                            # few rows: every wave's atomics collide
    for holes in ROW_COUNT_HOLES:
        r = _rng(8, P, ROW_COUNT_HOLES.index(holes))
        top = r.integers(0, N, P)
        if holes == "lane_0":
            top[0::64] = -1
        elif holes == "lane_63":
            top[63::64] = -2
            top[0] = -1 if P == 1 else top[0]
        elif holes == "last_wave":                   # the last wave of the pass: partly filled unless P is a multiple of 64
            top[P - 1] = -1
            top[((P - 1) // 64) * 64] = -2
        elif holes == "many":
            top[r.random(P) < 0.5] = -1
        _, rows = kc.flat_row_count(top, N)
        want = np.concatenate([np.bincount(top[top >= 0], minlength=N), [np.count_nonzero(top < 0)]])
        assert np.array_equal(rows, want), (P, holes)
    rc, rows = kc.flat_row_count(np.array([0, N]), N, check=False)
    assert rc == BAD_ARG and not rows.any()


# ---- e. fresh-run selection -------------------------------------------------------------------------------------------------

CBGT = 1                                             # BLANCE_BOOSTER_CBGT


def node_score(cnt, ntn, tot, hasw, w, NP, cf, booster):
    """nodeSorter.Score (plan.go:634-689) in the reference's operation order, in Python floats (IEEE fp64, no contraction)."""
    lp = ff = 0.0
    if NP > 0:
        lp = float(ntn) / float(NP)
        ff = (0.001 * float(tot)) / float(NP)
    r = float(cnt)
    r = r + lp
    r = r + ff
    if hasw:
        if w > 0:
            r = r / float(w)
        elif w < 0 and booster == CBGT:
            b = float(-w)
            if b < cf:
                b = cf
            r = r + b
    r = r - cf
    return r


def fresh_reference(c, R):
    """The first R picks of the greedy when every step is identical: a heap of (score, node) over the live nodes; pop,
    record, bump the node's counters by w, push.  -> picks per node, exclusive offsets (N + 1), the pick sequence."""
    N, w, NP = c["N"], c["w"], c["NP"]
    picks = [0] * N

    def score(n):
        k = picks[n]
        return node_score(int(c["cnt"][n]) + k * w, int(c["ntn"][n]) + k, int(c["tot"][n]) + k * w, int(c["has_w"][n]),
                          int(c["node_w"][n]), NP, 0.0, c["booster"])

    heap = [(score(n), n) for n in range(N) if c["alive"][n]]
    heapq.heapify(heap)
    seq = np.zeros(R, np.int32)
    for i in range(R):
        _, n = heap[0]
        seq[i] = n
        picks[n] += 1
        heapq.heapreplace(heap, (score(n), n))
    m = np.array(picks, np.int64)
    return m, np.concatenate([[0], np.cumsum(m)]), seq


FRESH_N = [1, 2, 63, 64, 65, 1023, 1024, 1025, 2500, 8192]      # k_fresh_threshold's slices: 1, 1, 1, 1, 1, 1, 1, 2, 3, 8 nodes a thread
FRESH_MASKS = ["all", "holes", "one"]
FRESH_COUNTERS = ["zero", "random", "one_ahead", "one_behind", "two_groups"]
FRESH_WEIGHTS = ["none", "some_1_2_4", "has_weight_0", "negative", "negative_cbgt"]
FRESH_R_BIG = 20000


def fresh_mask(N, kind):
    alive = np.ones(N, np.uint8)
    if kind == "one":
        alive[:] = 0
        alive[N // 2] = 1
    elif kind == "holes" and N > 1:
        # dead nodes at both ends and on both sides of the seams of the tie hand-out's thread slices (`per` nodes each; where
        # a slice is one or two nodes, every fifth seam), of the waves (64 threads) and of the 1024-node register rows
        per = (N + 1023) // 1024
        seams = set(range(per * (1 if per >= 3 else 5), N, per * (1 if per >= 3 else 5)))
        seams |= set(range(64 * per, N, 64 * per)) | set(range(1024, N, 1024))
        dead = {0, N - 1} | {s for s in seams} | {s - 1 for s in seams}
        alive[sorted(d for d in dead if 0 <= d < N)] = 0
        if not alive.any():
            alive[N // 2] = 1
    return alive


def fresh_case(N, mask="all", counters="zero", w=1, weights="none", NP=0, seed=0):
    """One input of the selection.  What validate_tail_b guarantees the kernels holds by construction: every counter is at
    most 10^6 and R w <= 2 * 10^7, so tot0 + R w < 2^31 -- the overflow that check guards against is not under test here
    (and the entry refuses an input that breaks it)."""
    r = _rng(9, N, FRESH_MASKS.index(mask), FRESH_COUNTERS.index(counters), w, FRESH_WEIGHTS.index(weights), NP, seed)
    alive = fresh_mask(N, mask)
    live = np.flatnonzero(alive)
    cnt = np.zeros(N, np.int64)
    if counters == "random":
        cnt = r.integers(0, 51, N)
    elif counters == "one_ahead":                    # it gets nothing
        cnt = r.integers(0, 5, N)
        cnt[live[len(live) // 2]] = 10 ** 6
    elif counters == "one_behind":                   # it gets nearly everything
        cnt = 30000 * w + r.integers(0, 5, N)
        cnt[live[len(live) // 3]] = 0
    elif counters == "two_groups":
        cnt = np.where(np.arange(N) % 2 == 0, 5, 9)
    tot = cnt + (r.integers(0, 21, N) if counters == "random" else 0)
    node_w, has_w = np.zeros(N, np.int64), np.zeros(N, np.uint8)
    if weights == "some_1_2_4":
        has_w = (r.random(N) < 0.5).astype(np.uint8)
        node_w = np.array([1, 2, 4])[r.integers(0, 3, N)] * has_w
    elif weights == "has_weight_0":
        has_w = (r.random(N) < 0.5).astype(np.uint8)
    elif weights in ("negative", "negative_cbgt"):
        has_w = (r.random(N) < 0.5).astype(np.uint8)
        node_w = -np.array([1, 3, 7])[r.integers(0, 3, N)] * has_w
    ntn = r.integers(0, 31, N) if NP > 0 else np.zeros(N, np.int64)          # a non-trivial "" row of the matrix
    return dict(N=N, alive=alive, cnt=cnt, tot=tot, ntn=ntn, node_w=node_w, has_w=has_w, NP=NP, w=w,
                booster=CBGT if weights == "negative_cbgt" else 0, int_keys_legal=(NP == 0 and not has_w.any()),
                tag=(N, mask, counters, w, weights, NP))


def fresh_rs(c, big=True):
    A = int(np.count_nonzero(c["alive"]))
    rs = [1, A - 1, A, A + 1, 3 * A + 7] + ([FRESH_R_BIG] if big else [])
    return sorted({R for R in rs if R > 0})


def fresh_table(N):
    """(case, [R ...]) for one N: all counters zero -- every element of a round ties, the tie hand-out in node order
    crosses every seam -- under every live mask and every R; then the other starting counters, step weights, node weights
    and NumPartitions, each with two R."""
    table = [(fresh_case(N, mask), None) for mask in FRESH_MASKS]
    variety = list(itertools.product(FRESH_COUNTERS[1:], (1, 3, 1000)))
    for i, (counters, w) in enumerate(variety):
        weights = FRESH_WEIGHTS[i % len(FRESH_WEIGHTS)]
        NP = (0, 977)[(i // len(FRESH_WEIGHTS) + i) % 2] if N <= 2048 else 0
        mask = ("all", "holes")[i % 2]
        c = fresh_case(N, mask, counters, w, weights, NP, seed=i)
        rs = fresh_rs(c)
        table.append((c, sorted({rs[i % len(rs)], rs[(i + 3) % len(rs)]})))
    # each node weight kind and NumPartitions > 0 over zero counters too (ties everywhere, fp64 keys)
    for i, weights in enumerate(FRESH_WEIGHTS[1:]):
        c = fresh_case(N, "holes", "zero", (1, 3)[i % 2], weights, 977 if N <= 2048 else 0, seed=100 + i)
        rs = fresh_rs(c, big=False)
        table.append((c, rs[-2:]))
    return table


def check_fresh_one(kc, c, R):
    m_want, moff_want, seq_want = fresh_reference(c, R)
    assert moff_want[-1] == R
    seqs = []
    for int_keys in ((0, 1) if c["int_keys_legal"] else (0,)):
        _, m, moff, seq = kc.fresh_select(c, R, int_keys=int_keys)
        tag = (c["tag"], R, int_keys)
        assert np.array_equal(m, m_want), tag
        assert np.array_equal(moff, moff_want), tag
        assert np.array_equal(seq, seq_want), (tag, int(np.argmax(seq != seq_want)))
        seqs.append(seq)
    if len(seqs) == 2:
        assert np.array_equal(seqs[0], seqs[1])      # both key forms: one sequence
    return seq_want


def check_fresh(kc, N):
    for c, rs in fresh_table(N):
        for R in (fresh_rs(c) if rs is None else rs):
            check_fresh_one(kc, c, R)


def check_fresh_refuses(kc):
    c = fresh_case(8, counters="random")
    c["tot"] = c["tot"].copy()
    c["tot"][3] = INT_MAX - 10                       # tot0 + R w would pass 2^31
    rc, m, _, _ = kc.fresh_select(c, 100, check=False)
    assert rc == BAD_ARG and not m.any()
    rc, m, _, _ = kc.fresh_select(fresh_case(8, weights="some_1_2_4", seed=1), 10, int_keys=1, check=False)
    assert rc == BAD_ARG and not m.any()


# k_fresh_cycle's closed form against the general path: (N, live mask, RS) -- a live mask with holes and RS % A != 0 among them
CYCLE_SHAPES = [(64, "all", None), (1025, "holes", None), (2500, "holes", FRESH_R_BIG)]


def check_fresh_cycle(kc, N, mask, RS):
    c = fresh_case(N, mask)
    A = int(np.count_nonzero(c["alive"]))
    RS = 3 * A + 7 if RS is None else RS
    assert RS % A != 0
    m_want, _, seq_want = fresh_reference(c, RS)
    _, m_gen, _, seq_gen = kc.fresh_select(c, RS, int_keys=1)
    _, m_cyc, _, seq_cyc = kc.fresh_select(c, RS, int_keys=1, cycle=1)
    assert np.array_equal(seq_cyc, seq_gen) and np.array_equal(m_cyc, m_gen)
    assert np.array_equal(seq_cyc, seq_want) and np.array_equal(m_cyc, m_want)


# ---- f. exclusion automaton -------------------------------------------------------------------------------------------------

EXCL_R = [1, 2, 1023, 1024, 1025, 4096, 4097, 8193, 70000]      # G = 1, 1, 1, 1, 1, 1, 2, 3, 18 workgroups; 1 to 4 steps a thread
EXCL_KINDS = ["none", "random_5", "random_50", "seam", "seam_twice", "seam_thrice", "second", "skewed_5", "skewed_seam"]
EXCL_N = 37
NO_BAD = INT_MAX


def excl_shape(R):
    """Workgroups and steps per thread of the composition scan for a run of R steps (run_flat_pass: one workgroup per 4096
    steps, 64 at the most)."""
    G = min(64, max(1, -(-R // 4096)))
    return G, -(-R // (G * 1024))


@functools.lru_cache(maxsize=None)
def excl_sequence(skewed, n):
    """S: the exclusion-free sequence, built as case e builds it (the heap reference, which the selection is checked
    against): level random counters, or two nodes so far behind that they come up again and again at first."""
    c = fresh_case(EXCL_N, "all", "random", seed=77)
    # loads within one pick of each other: consecutive elements of S are different nodes, as a step of two picks needs them
    c["cnt"] = 40 + c["cnt"] % 2
    if skewed:
        c["cnt"][[5, 11]] = 0
    c["tot"] = c["cnt"].copy()
    _, _, seq = fresh_reference(c, n)
    return c, seq


def excl_case(R, k, kind):
    """-> (S[k R + k], excl[R], the counters S was made from)"""
    c, seq = excl_sequence(kind.startswith("skewed"), 2 * max(EXCL_R) + 2)
    S = seq[:k * R + k]
    r = _rng(10, R, k, EXCL_KINDS.index(kind))
    excl = np.full(R, -1, np.int64)
    G, per = excl_shape(R)
    # the last step of a thread's slice (a few threads, wave seams among them) and of every workgroup's slice
    lasts = sorted({t for t in [per * (j + 1) - 1 for j in (0, 1, 62, 63, 64, 500, 1022)] +
                    [per * 1024 * (g + 1) - 1 for g in range(G)] if 0 <= t < R})
    if kind in ("random_5", "skewed_5"):
        hit = r.random(R) < 0.05
        excl[hit] = r.integers(0, EXCL_N, R)[hit]
        if kind == "skewed_5":                       # a node that is behind, excluded while it is due again and again
            excl[r.random(R) < 0.02] = 5
    elif kind == "random_50":
        hit = r.random(R) < 0.5
        excl[hit] = r.integers(0, EXCL_N, R)[hit]
    elif kind in ("seam", "seam_twice", "seam_thrice", "skewed_seam"):
        reps = {"seam": 1, "skewed_seam": 1, "seam_twice": 2, "seam_thrice": 3}[kind]
        for t in lasts:                              # excluded exactly where its turn is: pending across the seam; then
            for j in range(reps):                    # excluded again by the next step(s): the A_t case
                if t + j < R:
                    excl[t + j] = S[k * t]
    elif kind == "second":
        hit = r.random(R) < 0.05
        excl[hit] = S[k * np.flatnonzero(hit) + (k - 1)]
        for t in lasts:
            excl[t] = S[k * t + (k - 1)]
    return S, excl, c


def excl_cases():
    return [(R, k, kind) for R in EXCL_R for k in (1, 2) for kind in EXCL_KINDS if not (kind == "second" and k == 1)]


def excl_automaton(k, S, excl):
    """Reference 1, the rule above fresh_excluded walked one step at a time: one pending bit b (a node can only be pending
    if the previous step excluded it) and three ways to pick -- nothing pending: the next k elements of S, skipping e;
    pending and not excluded again: the pending node, then k - 1 elements of S, skipping e; pending and excluded again:
    k elements of S behind it.  -> picks[k R], the first step that is not exact (NO_BAD: none)."""
    R = len(excl)
    picks = np.zeros(k * R, np.int32)
    first_bad, b, eprev = NO_BAD, False, -1
    for t in range(R):
        e, base = int(excl[t]), k * t
        again = e >= 0 and e == eprev

        def take_from(i, count):                     # `count` elements of S from i on, stepping over e once for each
            out = []
            for _ in range(count):
                if e >= 0 and S[i] == e:
                    i += 1
                out.append(int(S[i]))
                i += 1
            return out

        if not b:
            take = take_from(base, k)
        elif not again:
            take = [eprev] + take_from(base + 1, k - 1)
        else:
            take = [int(S[base + 1])] + ([int(S[base + 2])] if k == 2 else [])
        in_turn = e >= 0 and e in [int(x) for x in S[base:base + k]]         # e among what the step would take from S
        after_x = e >= 0 and k == 2 and int(S[base + 1]) == e                # ... among the k - 1 it would take after x
        nb = (True if again else after_x) if b else in_turn
        picks[base:base + k] = take
        bad = e >= 0 and e in take                   # the skip landed on e again
        bad = bad or (k == 2 and take[0] == take[1])                         # a node taken twice in one step
        bad = bad or (nb and int(S[base + k]) == e)                          # the pending node comes up again while it waits
        if bad and first_bad == NO_BAD:
            first_bad = t
        b, eprev = nb, e
    return picks, first_bad


def excl_greedy(c, k, excl, steps):
    """Reference 2, the true greedy: every step takes the k best of the CURRENT scores among the live nodes without its
    excluded node (no commit between a step's picks, plan.go:171-172), then commits them (counter + w each)."""
    w = c["w"]
    cnt = [int(x) for x in c["cnt"]]
    heap = [(cnt[n], n) for n in range(c["N"]) if c["alive"][n]]
    heapq.heapify(heap)
    out = np.zeros(k * steps, np.int32)
    for t in range(steps):
        e, taken, aside = int(excl[t]), [], []
        while len(taken) < k:
            s, n = heapq.heappop(heap)
            (aside if n == e else taken).append((s, n))
        for j, (s, n) in enumerate(taken):
            out[k * t + j] = n
            heapq.heappush(heap, (s + w, n))
        for it in aside:
            heapq.heappush(heap, it)
    return out


@functools.lru_cache(maxsize=None)
def excl_reference(R, k, kind):
    S, excl, c = excl_case(R, k, kind)
    picks, first_bad = excl_automaton(k, S, excl)
    exact = min(R, first_bad)
    greedy = excl_greedy(c, k, excl, exact)
    return picks, first_bad, greedy


def check_excl(kc, R):
    assert kc.fresh_excl_shape(R) == excl_shape(R)
    for (R_, k, kind) in excl_cases():
        if R_ != R:
            continue
        S, excl, _ = excl_case(R, k, kind)
        picks_want, bad_want, greedy = excl_reference(R, k, kind)
        _, picks, bad = kc.fresh_excl(EXCL_N, k, S, excl)
        tag = (R, k, kind)
        assert bad == bad_want, tag
        assert np.array_equal(picks, picks_want), (tag, int(np.argmax(picks != picks_want)) // k)
        # the exactness claim: before the first bad step the automaton IS the greedy
        exact = min(R, bad)
        assert np.array_equal(picks[:k * exact], greedy), (tag, int(np.argmax(picks[:k * exact] != greedy)) // k)
        if kind == "none":
            assert bad == NO_BAD and np.array_equal(picks, S[:k * R]), tag
    rc, picks, _ = kc.fresh_excl(EXCL_N, 1, np.zeros(5, np.int32), np.array([0, EXCL_N, -1, -1]), check=False)
    assert rc == BAD_ARG and not picks.any()


def excl_reference_counts():
    """Over the whole table, on the references alone: how many cases with exclusions run to the end, how many end early."""
    to_end = early = 0
    for R, k, kind in excl_cases():
        if kind == "none":
            continue
        _, first_bad, _ = excl_reference(R, k, kind)
        if first_bad == NO_BAD:
            to_end += 1
        else:
            early += 1
    return to_end, early
