"""The single-kernel cases: binding, case tables, references and checks shared by tests/test_kernel_cases_emulated.py (the
SIMT emulator) and tests/test_kernel_cases_gpu.py (the device).  Both run exactly the same tables through the same entries
(tests/kernels/kernel_cases.inc); only the library differs.

The references are plain numpy / Python written from each operation's definition: a shifted cumsum, a stable argsort, a
bincount, a heap of (score, node), an automaton walked one step at a time, a greedy with the excluded node left out; for the
flat pass's certain-stay decision (g. to k.) a sorted list of (score, node), the stay rule and the fresh rule one step at a
time, and the full argmin over the live nodes, which does not use the rule's bound at all.
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
            "kcase_flat_prepare": [ci, ci, ci, vp, vp, vp, vp, ci, ci, ci, vp, vp, vp, vp],
            "kcase_flat_scan": [ci, ci, ci, vp, vp, vp, vp, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, vp, vp, ci],
            "kcase_flat_scan_waves": [ci, ci],
            "kcase_flat_stay_live": [ci, ci, ci, vp, vp, vp, vp, ci, ci, ci, ci, ci, vp, vp, vp, vp, ci, vp, vp, vp, vp, ci, ci, ci, vp,
                                     vp],
            "kcase_flat_commit_stay": [ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, vp, vp],
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

    # ---- the flat pass's stay side (g. to k. below).  wd: a world of flat_world(); sa: the steps as steps_arrays() makes them

    @staticmethod
    def _world(wd):
        return (_i32(wd["cnt"]), _u8(wd["alive"]), _i32(wd["node_w"]), _u8(wd["has_w"]))

    def flat_prepare(self, wd, check=True, fill=0):
        NX = wd["NX"]
        cnt, alive, nw, hw = self._world(wd)
        tot, top_n = np.full(NX + 1, fill, np.int32), np.full(TOP_LIST + 1, fill, np.int32)
        g, top_g = np.full(NX + 1, fill, U64), np.full(TOP_LIST + 1, fill, U64)
        rc = self._ok(self.lib.kcase_flat_prepare(wd["N"], NX, wd["M"], _p(cnt), _p(alive), _p(nw), _p(hw), wd["NP"], wd["booster"],
                                                  wd["s"], _p(tot), _p(g), _p(top_g), _p(top_n)), check)
        return rc, tot, g, top_g, top_n

    def flat_scan_waves(self, beg, end):
        return self.lib.kcase_flat_scan_waves(beg, end)

    def flat_scan(self, wd, sa, row_count, k, beg, end, top_state, mask, check=True, fill=0):
        cnt, alive, nw, hw = self._world(wd)
        waves = 4 * (-(-(end - beg) // 256)) if end > beg else 1
        scan, part = np.full(3, fill, np.int32), np.full(2 * waves + 1, fill, np.int32)
        row_count = _i32(row_count)
        assert len(row_count) == wd["NX"] + 1
        rc = self._ok(self.lib.kcase_flat_scan(wd["N"], wd["NX"], wd["M"], _p(cnt), _p(alive), _p(nw), _p(hw), wd["NP"], wd["booster"],
                                               wd["s"], sa["P"], sa["L"], _p(sa["lists"]), _p(sa["len"]), _p(sa["kind"]), _p(sa["w"]),
                                               _p(sa["stick"]), _p(row_count), k, top_state, mask, beg, end, _p(scan), _p(part),
                                               len(part)), check)
        return rc, scan, part, waves

    def flat_stay_live(self, wd, lv, k, top_state, mask, word=0, check=True, fill=0):
        """lv: a pass as live_problem() makes it.  -> rc, the three words (sentinel, verdict, sentinel), row_count[NX + 2]"""
        cnt, alive, nw, hw = self._world(wd)
        words = np.array([SENTINEL_A, word, SENTINEL_B], np.int32)
        rows = np.full(wd["NX"] + 2, fill, np.int32)
        rc = self._ok(self.lib.kcase_flat_stay_live(wd["N"], wd["NX"], wd["M"], _p(cnt), _p(alive), _p(nw), _p(hw), wd["NP"],
                                                    wd["booster"], wd["s"], lv["P"], lv["L"], _p(lv["lists"]), _p(lv["len"]),
                                                    _p(lv["kind"]), _p(lv["order"]), lv["weights_nil"], _p(lv["part_has_w"]),
                                                    _p(lv["part_w"]), _p(lv["state_stick"]), _p(lv["state_has_stick"]), k, top_state,
                                                    mask, _p(words), _p(rows)), check)
        return rc, words, rows

    def flat_commit_stay(self, N, NX, M, sa, s, top_state, NP, beg, end, bump, ntn, check=True):
        ntn = _i32(ntn).copy()
        assert len(ntn) == (NX + 1) * N + 1
        out = np.zeros(2 * sa["P"] + 1, np.int32)
        rc = self._ok(self.lib.kcase_flat_commit_stay(N, NX, M, sa["P"], sa["L"], _p(sa["lists"]), _p(sa["len"]), _p(sa["kind"]),
                                                      _p(sa["w"]), _p(sa["stick"]), s, top_state, NP, beg, end, bump, _p(ntn), _p(out)),
                      check)
        return rc, ntn, out


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


# ---- g. k_flat_prepare: totals, partition-independent scores, the top list -----------------------------------------------------

TOP_LIST = 8                                         # kTopList
LIST_ABSENT, LIST_NIL, LIST_SET = 0, 1, 2            # kListAbsent, kListNil, kListSet
SENTINEL_A, SENTINEL_B = 0x1234ABCD, 0x0BADF00D      # around k_flat_stay_live's verdict word
POS_INF_BITS = 0x7FF0000000000000


def flat_world(cnt_s, N=None, extra=None, alive=None, node_w=None, has_w=None, NP=0, booster=0, M=4, s=2, other=None):
    """The node tables of a flat pass: NX = len(cnt_s) node names of which the first N are nodesNext (the rest: removed),
    cnt[(M + 1) NX] with row s = cnt_s, row M (the extra loads) = `extra`, every other row = `other`."""
    NX = len(cnt_s)
    N = NX if N is None else N
    cnt = np.zeros((M + 1, NX), np.int64)
    if other is not None:
        cnt[:M] = other
    cnt[s] = cnt_s
    if extra is not None:
        cnt[M] = extra
    return dict(N=N, NX=NX, M=M, s=s, cnt=cnt, NP=NP, booster=booster,
                alive=np.ones(N, np.uint8) if alive is None else np.asarray(alive, np.uint8),
                node_w=np.zeros(NX, np.int64) if node_w is None else np.asarray(node_w, np.int64),
                has_w=np.zeros(NX, np.uint8) if has_w is None else np.asarray(has_w, np.uint8))


def f64_bits(v):
    return np.asarray(v, dtype=np.float64).view(U64)


def flat_prepare_reference(wd):
    """-> tot[NX], g[NX] (Python floats), the top list: the first 8 of sorted((g[n], n) for live n < N), padded with
    (+inf, INT_MAX).  Kept with the world: every check of one world shares it."""
    if "_ref" not in wd:
        s, NX = wd["s"], wd["NX"]
        tot = wd["cnt"].sum(axis=0)
        g = [node_score(int(wd["cnt"][s][n]), 0, int(tot[n]), int(wd["has_w"][n]), int(wd["node_w"][n]), wd["NP"], 0.0, wd["booster"])
             for n in range(NX)]
        top = sorted((g[n], n) for n in range(wd["N"]) if wd["alive"][n])[:TOP_LIST]
        top += [(float("inf"), INT_MAX)] * (TOP_LIST - len(top))
        wd["_ref"] = (tot, g, top)
    return wd["_ref"]


PREPARE_N = [1, 2, 7, 8, 9, 1023, 1024, 1025, 2500, 8192]      # one node a thread, the 1024-thread seam, up to 8 nodes a thread
PREPARE_SCORES = ["equal", "last_8", "per_slice", "seam_duplicates"] + FRESH_WEIGHTS + ["removed_loaded"]
PREPARE_LIVE = list(range(10)) + ["all"]


def prepare_world(N, removed, live, scores, NP):
    """One input of k_flat_prepare.  Every live node's counter is at least 1; the dead and the removed ones ([N, N + removed))
    have 0 and no weight, so any of them that got into the top list would lead it.  "removed_loaded": the removed nodes
    have counters of their own in state s, 1 to 5 and weighted, below every live node's 50: g is made from them."""
    r = _rng(11, N, removed, PREPARE_LIVE.index(live), PREPARE_SCORES.index(scores), NP)
    NX = N + removed
    alive = np.ones(N, np.uint8)
    if live != "all":
        alive[:] = 0
        keep = r.choice(N, min(live, N), replace=False)
        if len(keep):
            keep[0] = N - 1                          # the last node, owned by the last busy thread (a repeat only shortens the set)
        alive[keep] = 1
    node_w, has_w = np.zeros(NX, np.int64), np.zeros(NX, np.uint8)
    cnt_s = 50 + r.integers(0, 40, NX)
    if scores == "equal":                            # every reduction ties: the list is the 8 smallest ids
        cnt_s[:] = 3
    elif scores == "last_8":                         # descending: not in id order
        tail = np.arange(max(0, N - 8), N)
        cnt_s[tail] = 1 + (N - 1 - tail)
    elif scores == "per_slice":                      # one per 1024-node slice, the later slices smaller
        ids = sorted({min(N - 1, 1024 * i + 517) for i in range(8)})
        for j, n in enumerate(ids):
            cnt_s[n] = 1 + len(ids) - j
    elif scores == "seam_duplicates":                # the same minimum on both sides of the 1024 seam, the next one at 2048
        for n, v in ((1022, 1), (1023, 1), (1024, 1), (1025, 1), (2047, 2), (2048, 2), (0, 2), (N - 1, 2)):
            if n < N:
                cnt_s[n] = v
    elif scores == "removed_loaded":
        pass                                         # (set below, behind the zeroing)
    else:                                            # the node weight kinds of the fresh-run table
        c = fresh_case(N, "all", "random", 1, scores, 0, seed=3)
        node_w[:N], has_w[:N] = c["node_w"], c["has_w"]
        cnt_s[:N] = 1 + c["cnt"]
    other = r.integers(0, 7, NX) if scores != "equal" else np.full(NX, 2)
    extra = r.integers(0, 900, NX) if scores != "equal" else np.full(NX, 1)
    for arr in (cnt_s, node_w, has_w):
        arr[N:] = 0
        arr[:N][alive == 0] = 0
    if scores == "removed_loaded":
        cnt_s[N:], node_w[N:], has_w[N:] = 1 + np.arange(removed), 2, 1
    return flat_world(cnt_s, N=N, extra=extra, alive=alive, node_w=node_w, has_w=has_w, NP=NP,
                      booster=CBGT if scores == "negative_cbgt" else 0, M=2, s=1, other=other)


def prepare_cases(N):
    """Every score kind once per N with every node alive, the removed nodes and NumPartitions alternating against the kinds
    and from one N to the next; every other live count per N (the even ones at one N, the odd ones at the next)."""
    z = PREPARE_N.index(N)
    cases = []
    for i, scores in enumerate(PREPARE_SCORES):
        removed = 5 if scores == "removed_loaded" else (0, 5)[(i + z) % 2]
        cases.append((N, removed, "all", scores, (0, 977)[((i + z) // 2) % 2]))
    for j, live in enumerate(PREPARE_LIVE[:-1]):
        if (j + z) % 2 == 0:
            cases.append((N, (5, 0)[(j // 2) % 2], live, PREPARE_SCORES[(j + z) % len(PREPARE_SCORES)], (0, 977)[(j // 2 + z) % 2]))
    return cases


def check_flat_prepare_one(kc, wd, tag):
    NX = wd["NX"]
    tot_want, g_want, top = flat_prepare_reference(wd)
    _, tot, g, top_g, top_n = kc.flat_prepare(wd)
    assert tot[NX] == GUARD and top_n[TOP_LIST] == GUARD, tag
    assert int(g[NX]) == (GUARD << 32 | GUARD) and int(top_g[TOP_LIST]) == (GUARD << 32 | GUARD), tag
    assert np.array_equal(tot[:NX], tot_want), tag
    assert np.array_equal(g[:NX], f64_bits(g_want)), (tag, "g differs from the reference's fp64 in some bit")
    assert [int(n) for n in top_n[:TOP_LIST]] == [n for _, n in top], (tag, top_n[:TOP_LIST], top)
    assert np.array_equal(top_g[:TOP_LIST], f64_bits([v for v, _ in top])), tag
    assert all(n == INT_MAX or (n < wd["N"] and wd["alive"][n]) for _, n in top)


def check_flat_prepare(kc, N):
    for case in prepare_cases(N):
        check_flat_prepare_one(kc, prepare_world(*case), case)


# ---- h. the certain-stay and fresh-identical decisions: steps, references, tables ---------------------------------------------

FLAT_M, FLAT_S, FLAT_TOP, FLAT_MASK, FLAT_L = 4, 2, 0, 0b0011, 8      # states 0 (the top state) and 1 outrank s = 2; 3 does not
FLAT_LANES = (0, 1, 31, 62, 63)
BIG_STICK = 10 ** 9                                  # a partition weight no score of a table comes near
FILLER_NODE = 0                                      # live, unweighted and far from the top of every table's list


def st(lists=None, stick=1.5, w=1):
    """One step: lists = {state: [nodes] or "nil"} (a state not named: no list), the partition's stickiness and weight.
    The stickiness is 1.5 or an integer: what a partition's weight or a state's stickiness can give (plan.go:104-115)."""
    assert stick == 1.5 or stick == int(stick)
    return dict(lists=dict(lists or {}), stick=float(stick), w=w)


def step_nodes(step, t):
    l = step["lists"].get(t)
    return l if isinstance(l, list) else []


def step_top(step, top_state=FLAT_TOP):
    l = step_nodes(step, top_state)
    return l[0] if l else -1


def steps_arrays(steps, M=FLAT_M, L=FLAT_L):
    P = len(steps)
    sa = dict(P=P, M=M, L=L, lists=np.zeros((P, M, L), np.int32), len=np.zeros((P, M), np.int32), kind=np.zeros((P, M), np.uint8),
              w=np.zeros(P, np.int32), stick=np.zeros(P, np.float64))
    for i, step in enumerate(steps):
        sa["w"][i], sa["stick"][i] = step["w"], step["stick"]
        for t, l in step["lists"].items():
            if l == "nil":
                sa["kind"][i, t] = LIST_NIL
            else:
                sa["kind"][i, t], sa["len"][i, t] = LIST_SET, len(l)
                sa["lists"][i, t, :len(l)] = l
    return sa


def plain_row_count(wd, steps, top_state=FLAT_TOP):
    """Steps of the pass per top priority node, then the "" row: k_flat_row_count's definition."""
    rows = np.zeros(wd["NX"] + 1, np.int64)
    for step in steps:
        t = step_top(step, top_state)
        rows[wd["NX"] if t < 0 else t] += 1
    return rows


def certain_stay(wd, step, k, row_count, top_state=FLAT_TOP, mask=FLAT_MASK):
    """The rule in the header of k_flat.h, for one step: with k = 1 the partition keeps the ONE live node o it holds in
    state s, and holds in no other list, if the largest score o could have (its nodeToNodeCounts entry bounded by the
    steps of the pass that share its top priority node) beats, as (score, node), the smallest partition-independent
    score among the other candidates -- the first entry of the top list that is neither o nor in a list of a state that
    outranks s.  A list that ends first: no other candidate, a stay; eight entries gone: no bound, no stay."""
    tot, _, top = flat_prepare_reference(wd)
    s, M = wd["s"], wd["M"]
    own = step_nodes(step, s)
    if k != 1 or len(own) != 1:
        return False
    o = own[0]
    if o >= wd["N"] or not wd["alive"][o]:
        return False
    if any(o in step_nodes(step, t) for t in range(M) if t != s):
        return False
    t_ = step_top(step, top_state)
    ub = int(row_count[wd["NX"] if t_ < 0 else t_]) if wd["NP"] > 0 else 0
    s_hi = node_score(int(wd["cnt"][s][o]), ub, int(tot[o]), int(wd["has_w"][o]), int(wd["node_w"][o]), wd["NP"], step["stick"],
                      wd["booster"])
    excluded = {n for t in range(M) if (mask >> t) & 1 for n in step_nodes(step, t)}
    for gv, n in top:
        if n == INT_MAX:
            return True
        if n == o or n in excluded:
            continue
        return (s_hi, o) < (gv, n)
    return False


def fresh_like(wd, step, first, k, top_state=FLAT_TOP, mask=FLAT_MASK):
    """Is the step one of a run of fresh identical steps that begins with `first`?  Its weight is positive and `first`'s;
    with NumPartitions > 0: k = 1 and the partition holds nothing at all; with NumPartitions == 0: k <= 2 and the partition
    holds at most one node, in a state that outranks s."""
    if step["w"] <= 0 or step["w"] != first["w"]:
        return False
    all_len = sum(len(step_nodes(step, t)) for t in range(wd["M"]))
    high_len = sum(len(step_nodes(step, t)) for t in range(wd["M"]) if (mask >> t) & 1)
    if wd["NP"] == 0:
        return k <= 2 and all_len == high_len and high_len <= 1
    return k == 1 and all_len == 0 and step_top(step, top_state) < 0


def scan_reference(wd, steps, k, row_count, beg, end):
    """-> scan[2], part[2][waves], the per-step verdicts (stay[], fresh[]) over [beg, end)"""
    waves = 4 * (-(-(end - beg) // 256))
    stay = {i: certain_stay(wd, steps[i], k, row_count) for i in range(beg, end)}
    fresh = {i: fresh_like(wd, steps[i], steps[beg], k) for i in range(beg, end)}
    part = np.full((2, waves), INT_MAX, np.int64)
    for wv in range(waves):
        rng = range(beg + 64 * wv, min(end, beg + 64 * wv + 64))
        part[0][wv] = min([i for i in rng if not stay[i]], default=INT_MAX)
        part[1][wv] = min([i for i in rng if not fresh[i]], default=INT_MAX)
    return [int(part[0].min()), int(part[1].min())], part, stay, fresh


def stay_filler(top=None):
    """A stay whatever the top list holds: one live unweighted node and a stickiness beyond every score"""
    return st({FLAT_S: [FILLER_NODE], **({FLAT_TOP: [top]} if top is not None else {})}, stick=BIG_STICK)


FRESH_FILLER = st()                                  # nothing held, weight 1
BEFORE_BEG = st(w=0)                                 # neither a stay nor fresh: a scan that started before `beg` would report it


def table_layout(steps, filler, rot, beg, lanes=FLAT_LANES):
    """Every table step in a wave of its own, at one of the lanes 0, 1, 31, 62, 63 (which one rotates with `rot`), the rest
    of the wave filled with steps for which the predicate under test holds.  -> all steps, the table steps' positions"""
    out = [BEFORE_BEG] * beg + [filler] * (64 * len(steps))
    pos = []
    for j, step in enumerate(steps):
        i = beg + 64 * j + lanes[(j + rot) % len(lanes)]
        out[i] = step
        pos.append(i)
    assert len(out) <= 1000
    return out, pos


# Worlds of the stay tables.  Node 0 is the fillers' (counter 20); NumPartitions = 0 and integer counters unless said.
BASE_CNT = [20, 5, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13]             # top list: (4, 2) (5, 1) (5, 3) (6, 4) (7, 5) (8, 6) (9, 7) (10, 8)
S_ = FLAT_S


def _o(o, stick=1.5, **lists):
    """a partition that holds o in state s; t0=..., t1=..., t3=...: its lists in the states 0, 1 and 3"""
    return st({S_: [o], **{int(k[1:]): v for k, v in lists.items()}}, stick=stick)


def stay_group_runs(group):
    """-> [(world, table steps, k), ...] for one group of the stay table"""
    if group == "ties":
        # s_hi == top_g[e]: the node id decides.  Stickiness 1.0: 5 - 1 = 4 = node 2's score.
        a = flat_world(BASE_CNT)
        steps_a = [_o(1, 1), _o(3, 1), _o(1, 2), _o(1, 0), _o(3, 2), _o(3, 0)]
        # Stickiness 1.5: 6 - 1.5 = 4.5 = node 2's 9 / 2
        cnt = list(BASE_CNT)
        cnt[1], cnt[2], cnt[3] = 6, 9, 6
        w, hw = [0] * 12, [0] * 12
        w[2], hw[2] = 2, 1
        b = flat_world(cnt, node_w=w, has_w=hw)
        steps_b = [_o(1), _o(3), _o(1, 2), _o(3, 2), _o(1, 1), _o(3, 1)]
        return [(a, steps_a, 1), (b, steps_b, 1)]
    if group == "row_bound":
        # NumPartitions = 977.  o = 1: 5 + ub / 977 + 0.005 / 977 - 1 against node 2's 4 + 3.504 / 977: a stay while the row's
        # bound is at most 3.  Tops: node 6 once, node 7 twice, node 9 four times, node 13 (removed) once, node 10 as often as
        # the fillers have it, none three times (the "" row, which the fillers without a top share).
        cnt = list(BASE_CNT) + [0, 0]
        extra = [0] * 14
        extra[2] = 3500
        wd = flat_world(cnt, N=12, extra=extra, NP=977)
        steps = [_o(1, 1, t0=[6]), _o(1, 1, t0=[7]), _o(1, 1, t0=[7, 3]), _o(1, 1, t0=[9]), _o(1, 1, t0=[9]), _o(1, 1, t0=[9, 4]),
                 _o(1, 1, t0=[9], t1=[5]), _o(1, 1), _o(1, 1, t0="nil"), _o(1, 1, t0=[], t1=[9]), _o(1, 1, t0=[13]), _o(1, 1, t0=[10])]
        return [(wd, steps, 1)]
    if group == "stickiness":
        wd = flat_world(BASE_CNT)
        steps = [_o(1, 0), _o(1), _o(1, 1000), _o(8, 0), _o(8), _o(8, 5), _o(8, 6), _o(8, 7), _o(8, 1000)]
        return [(wd, steps, 1)]
    if group == "exclusions":
        a = flat_world(BASE_CNT)
        steps_a = [_o(3, 1),                          # node 2 (4) ties with 5 - 1 and 2 < 3: no stay
                   _o(3, 1, t0=[2]),                   # node 2 outranked away: node 1 (5) decides
                   _o(3, 1, t1=[9, 2]),                # ... from the last place of a list of the other higher state
                   _o(3, 1, t3=[2]),                   # a state that does not outrank s excludes nothing
                   _o(3, 1, t0=[2, 1]),                # 2 and 1 gone: node 4 (6) decides
                   _o(2, 0),                           # o itself leads the list: node 1 (5) against 4
                   _o(2, 0, t0=[1], t1=[3]),           # ... node 4 (6)
                   _o(0, 1000, t0=[2, 1, 3, 4, 5, 6, 7, 8]),      # all 8 listed nodes excluded, 12 alive: no bound, no stay
                   _o(0, 1000, t0=[2, 1, 3, 4], t1=[5, 6, 7, 8]),
                   _o(0, 1000, t0=[2, 1, 3, 4, 5, 6, 7]),         # seven: node 8 is left
                   _o(8, 1000, t0=[2, 1, 3, 4, 5, 6, 7]),         # seven and o itself the eighth
                   _o(0, 11, t0=[2, 1, 3, 4, 5, 6, 7]),           # 20 - 11 = 9 < 10
                   _o(0, 10, t0=[2, 1, 3, 4, 5, 6, 7])]           # 20 - 10 = 10 = node 8's, and 0 < 8
        # five nodes alive, fewer than the list is long: (4, 2) (5, 1) (5, 3) (11, 9) (20, 0), then nothing
        alive = [1, 1, 1, 1, 0, 0, 0, 0, 0, 1, 0, 0]
        b = flat_world(BASE_CNT, alive=alive)
        steps_b = [_o(9, 0, t0=[2, 1, 0], t1=[3]),     # every other live node excluded: no candidate, a stay
                   _o(9, 0, t0=[2, 1, 0]),             # node 3 (5) is left: 11 > 5
                   _o(9, 0, t0=[2, 1], t1=[3]),        # node 0 (20) is left: 11 < 20
                   _o(9, 0, t0=[2, 1], t3=[3, 0]),     # 3 and 0 in a state that excludes nothing
                   _o(0, 0, t0=[2, 1, 9], t1=[3]),     # o is the last of the list
                   _o(9, 7, t0=[2]), _o(9, 6, t0=[2])]            # node 1 (5): 11 - 7 < 5 <= 11 - 6
        return [(a, steps_a, 1), (b, steps_b, 1)]
    if group == "held_node":
        alive = [1] * 12
        alive[4] = 0
        wd = flat_world(BASE_CNT + [0, 0], N=12, alive=alive)
        big = 1000
        steps = [_o(3, big),                           # the plain one: a stay
                 _o(4, big),                           # dead
                 _o(12, big), _o(13, big),             # removed
                 _o(3, big, t0=[3]), _o(3, big, t1=[9, 3]), _o(3, big, t3=[3]), _o(3, big, t3=[9, 10, 3]),   # held twice
                 st({S_: []}, big), st({S_: [3, 5]}, big), st({}, big), st({FLAT_TOP: [6]}, big),          # length 0, 2, no list
                 st({S_: "nil"}, big),
                 _o(3, big, t0="nil", t3="nil"),       # nil lists elsewhere hold nobody
                 _o(3, big, t0=[4], t3=[12])]          # a dead and a removed node elsewhere do not matter
        return [(wd, steps, 1)]
    if group == "k_2":
        wd = flat_world(BASE_CNT)
        steps = [_o(1, 1000), _o(3, 2), st({S_: [3, 5]}, 1000), _o(2, 0)]
        return [(wd, steps, 1), (wd, steps, 2)]
    if group == "node_weights":
        # node: 1: 10 / 2 (w 2)  2: 8 / 2 (w 2, the deciding candidate)  3: 10 / 2  5: 5 (has a weight of 0)  6: 5 (w -3)  7: 4 (w -3)
        cnt = [20, 10, 8, 10, 6, 5, 5, 4, 10, 11, 12, 13]
        w = [0, 2, 2, 2, 0, 0, -3, -3, 0, 0, 0, 0]
        hw = [0, 1, 1, 1, 0, 1, 1, 1, 0, 0, 0, 0]
        steps = [_o(1, 1), _o(3, 1), _o(1, 0), _o(3, 2),                   # 10 / 2 - 1 = 4 = node 2's 8 / 2 (and node 7's 4 without the booster)
                 _o(5, 1), _o(5, 2), _o(5, 0),
                 _o(6, 1), _o(6, 2), _o(6, 5), _o(6, 0),                   # with the booster: 5 + max(3, stickiness) - stickiness
                 _o(7, 0), _o(7, 1),
                 _o(1, 1, t0=[2]),                                         # the deciding candidate: node 7 (4), or node 3 (5)
                 _o(0, 13, t0=[2, 1, 3, 5, 4])]                            # ... node 7: 4, or with the booster 4 + 3 = 20 - 13
        return [(flat_world(cnt, node_w=w, has_w=hw, booster=b), steps, 1) for b in (0, CBGT)]
    raise KeyError(group)


STAY_GROUPS = ["ties", "row_bound", "stickiness", "exclusions", "held_node", "k_2", "node_weights"]


def fresh_group_runs(group):
    """-> [(world, table steps, k), ...] for one group of the fresh table"""
    held = [st({FLAT_TOP: [3]}), st({1: [4]}), st({FLAT_TOP: [3], 1: [4]}), st({FLAT_TOP: [3, 4]}), st({3: [3]}), st({S_: [3]}),
            st({FLAT_TOP: [3], 3: [5]}), st({FLAT_TOP: "nil"}), st({FLAT_TOP: []})]
    weights = [st(), st(w=2), st(w=0), st(w=-1)]
    if group == "weights":
        return [(flat_world(BASE_CNT, NP=NP), weights, 1) for NP in (0, 977)]
    if group == "np_0":
        return [(flat_world(BASE_CNT), weights[:2] + held, k) for k in (1, 2, 3)]
    if group == "np_977":
        return [(flat_world(BASE_CNT, NP=977), weights[:2] + held, k) for k in (1, 2)]
    raise KeyError(group)


FRESH_GROUPS = ["weights", "np_0", "np_977"]


def table_runs(kind, group):
    """Every scan of one group: (world, all steps, table positions, k, row_count, beg, which row the filling serves).
    Stay tables: the stay filling at every lane rotation and twice from a `beg` that is no multiple of 64, with the rows
    counted from the pass itself, with the fillers' top set or not, and with all-zero and all-large row bounds; the fresh
    filling once.  Fresh tables: the same with the fillings' roles swapped."""
    runs = []
    for wd, steps, k in (stay_group_runs(group) if kind == "stay" else fresh_group_runs(group)):
        main = [(stay_filler(), 0), (stay_filler(10), 0)] if kind == "stay" else [(FRESH_FILLER, 1)]
        other = (FRESH_FILLER, 1) if kind == "stay" else (stay_filler(), 0)
        # Where no step can pass the predicate (a stay with k = 2, a fresh step with k = 3 or with k = 2 and NumPartitions > 0)
        # no filler passes it either: a table step then shows only as the first of its wave, lane 0.
        holds = k == 1 if kind == "stay" else k <= (2 if wd["NP"] == 0 else 1)
        for filler, row in main:
            for rot in range(len(FLAT_LANES)):
                beg = (0, 40, 0, 1, 0)[rot]
                if (filler["lists"].get(FLAT_TOP) and rot not in (0, 3)) or (not holds and rot not in (0, 1, 3)):
                    continue
                allsteps, pos = table_layout(steps, filler, rot, beg, FLAT_LANES if holds else (0,))
                counts = [plain_row_count(wd, allsteps[beg:])]
                if wd["NP"] > 0 and kind == "stay" and rot == 0:
                    counts += [np.zeros(wd["NX"] + 1, np.int64), np.full(wd["NX"] + 1, 1000)]
                for rc in counts:
                    runs.append((wd, allsteps, pos, k, rc, beg, row))
        allsteps, pos = table_layout(steps, other[0], 2, 0)
        runs.append((wd, allsteps, pos, k, plain_row_count(wd, allsteps), 0, other[1]))
    return runs


def table_outcomes(kind, group):
    """On the references alone: the verdicts of the group's table steps over all its scans under the filling that serves
    them -> (how many hold, how many do not).  Also the condition on the table itself: in such a scan the word of a table
    step's wave names that step exactly when its verdict is "no" -- one wrong verdict for one step changes a compared word."""
    yes = no = 0
    for wd, allsteps, pos, k, rc, beg, row in table_runs(kind, group):
        if row != (0 if kind == "stay" else 1):
            continue
        _, part, stay, fresh = scan_reference(wd, allsteps, k, rc, beg, len(allsteps))
        verdict = stay if kind == "stay" else fresh
        for i in pos:
            assert (part[row][(i - beg) // 64] == i) == (not verdict[i]), (kind, group, k, i, "the step's verdict does not show")
            yes, no = yes + (1 if verdict[i] else 0), no + (0 if verdict[i] else 1)
    return yes, no


# ---- i. k_flat_scan + k_flat_scan_min ---------------------------------------------------------------------------------------

def brute_force_pick(wd, step, ntn_row, mask=FLAT_MASK):
    """The greedy's pick for the step without any bound: the minimum of (score, node) over the live nodes of nodesNext that
    are in no list of a state that outranks s; the node's entry of the nodeToNodeCounts row feeds the score; the
    stickiness is the held node's alone (plan.go:146-172, :634-689)."""
    tot, _, _ = flat_prepare_reference(wd)
    s = wd["s"]
    o = step_nodes(step, s)[0]
    excluded = {n for t in range(wd["M"]) if (mask >> t) & 1 for n in step_nodes(step, t)}
    best = None
    for n in range(wd["N"]):
        if not wd["alive"][n] or n in excluded:
            continue
        sc = node_score(int(wd["cnt"][s][n]), int(ntn_row[n]), int(tot[n]), int(wd["has_w"][n]), int(wd["node_w"][n]), wd["NP"],
                        step["stick"] if n == o else 0.0, wd["booster"])
        if best is None or (sc, n) < best:
            best = (sc, n)
    return best[1]


def check_stays_are_sound(wd, allsteps, reported, row_count, tag):
    """Every step the KERNEL reports as a stay keeps its node under the full argmin, whatever the nodeToNodeCounts row
    holds within the row's bound: all zero, o's entry at the bound and the others zero, three random rows."""
    for i in reported:
        step = allsteps[i]
        own = step_nodes(step, wd["s"])
        assert len(own) == 1, (tag, i, "a stay without ONE held node")
        o = own[0]
        t_ = step_top(step)
        ub = int(row_count[wd["NX"] if t_ < 0 else t_])
        rows = [np.zeros(wd["NX"], np.int64), np.zeros(wd["NX"], np.int64)]
        if o < wd["NX"]:
            rows[1][o] = ub
        r = _rng(12, i, ub)
        rows += [r.integers(0, ub + 1, wd["NX"]) for _ in range(3)]
        for j, row in enumerate(rows):
            assert brute_force_pick(wd, step, row) == o, (tag, i, j, "reported as a certain stay, but the greedy moves it")


def check_flat_scan_table(kc, kind, group):
    for n_run, (wd, allsteps, pos, k, rc, beg, row) in enumerate(table_runs(kind, group)):
        P = len(allsteps)
        tag = (kind, group, n_run, k, beg)
        scan_want, part_want, _, _ = scan_reference(wd, allsteps, k, rc, beg, P)
        _, scan, part, waves = kc.flat_scan(wd, steps_arrays(allsteps), rc, k, beg, P, FLAT_TOP, FLAT_MASK)
        assert waves == kc.flat_scan_waves(beg, P) == part_want.shape[1], tag
        assert scan[2] == GUARD and part[2 * waves] == GUARD, tag
        got = part[:2 * waves].reshape(2, waves)
        assert np.array_equal(got, part_want), (tag, np.argwhere(got != part_want)[:4].tolist())
        assert [int(scan[0]), int(scan[1])] == scan_want, tag
        if row == 0:                                 # the stay filling: what the kernel calls a stay, against the full argmin
            reported = [i for i in pos + [beg + 2] if got[0][(i - beg) // 64] > i]
            check_stays_are_sound(wd, allsteps, reported, rc, tag)


FLAT_SCAN_P = [1, 63, 64, 65, 255, 256, 257, 1000]
FLAT_SCAN_BEG = [0, 1, 64, 200]


def check_flat_scan_geometry(kc, P):
    """Ranges that do not line up with the waves: every beg < P, end = P, the only step that fails at P - 1 or nowhere --
    in the partly filled last wave, whose idle lanes are clamped to step P - 1 and must not speak for it.  And the fresh
    row when `beg`'s own step is not fresh: it holds more than a fresh step may (the steps behind it are fresh and alike:
    it alone fails), or its weight is 0 (no step is fresh then, alike or not)."""
    for beg in [b for b in FLAT_SCAN_BEG if b < P]:
        for NP in ((0, 977)[(FLAT_SCAN_P.index(P) + FLAT_SCAN_BEG.index(beg)) % 2],):       # (alternating over the ranges)
            wd = flat_world(BASE_CNT, NP=NP)
            for first in (st({FLAT_TOP: [3], 1: [4]}) if NP == 0 else st({FLAT_TOP: [3]}), st(w=0)):
                steps = [BEFORE_BEG] * beg + [first] + [FRESH_FILLER] * (P - beg - 1)
                rc = plain_row_count(wd, steps[beg:])
                scan_want, part_want, _, fresh = scan_reference(wd, steps, 1, rc, beg, P)
                assert scan_want[1] == beg and not fresh[beg]
                assert all(fresh[i] == (first["w"] == 1) for i in range(beg + 1, P))
                _, scan, part, waves = kc.flat_scan(wd, steps_arrays(steps), rc, 1, beg, P, FLAT_TOP, FLAT_MASK)
                tag = (P, NP, beg, "beg's own step", first["w"])
                assert scan[2] == GUARD and part[2 * waves] == GUARD, tag
                assert np.array_equal(part[:2 * waves].reshape(2, waves), part_want), tag
                assert [int(scan[0]), int(scan[1])] == scan_want, tag
            for filler, bad in ((stay_filler(), _o(3, 0)), (FRESH_FILLER, st(w=2))):
                for fails in (True, False):
                    if fails and P - 1 == beg and filler is FRESH_FILLER:
                        continue                     # (the range's first step is what the others are compared with)
                    steps = [BEFORE_BEG] * beg + [filler] * (P - beg)
                    if fails:
                        steps[P - 1] = bad
                    rc = plain_row_count(wd, steps[beg:])
                    scan_want, part_want, _, _ = scan_reference(wd, steps, 1, rc, beg, P)
                    row = 0 if filler is not FRESH_FILLER else 1
                    assert scan_want[row] == (P - 1 if fails else INT_MAX)
                    _, scan, part, waves = kc.flat_scan(wd, steps_arrays(steps), rc, 1, beg, P, FLAT_TOP, FLAT_MASK)
                    tag = (P, NP, beg, row, fails)
                    assert scan[2] == GUARD and part[2 * waves] == GUARD, tag
                    assert np.array_equal(part[:2 * waves].reshape(2, waves), part_want), tag
                    assert [int(scan[0]), int(scan[1])] == scan_want, tag


# ---- j. k_flat_prepare(_count_live) + k_flat_stay_live ------------------------------------------------------------------------

def live_problem(steps, order, M=FLAT_M, L=FLAT_L, branch="part", state_stick=None):
    """The pass as partitions: step oi is partition order[oi].  A step's stickiness comes from its partition's weight
    (branch "part"; 1.5: the partition has none) or, where it equals state_stick, from the state's stickiness (branch
    "state"); branch "nil": there are no weights at all and every step's stickiness is 1.5."""
    P = len(steps)
    order = np.asarray(order, np.int32)
    sa = steps_arrays(steps, M, L)
    lv = dict(P=P, M=M, L=L, order=order, weights_nil=1 if branch == "nil" else 0, lists=np.zeros_like(sa["lists"]),
              len=np.zeros_like(sa["len"]), kind=np.zeros_like(sa["kind"]), part_has_w=np.zeros(P, np.uint8), part_w=np.zeros(P, np.int32),
              state_stick=np.full(M, 77, np.int32), state_has_stick=np.zeros(M, np.uint8))
    lv["state_has_stick"][[t for t in range(M) if t != FLAT_S]] = 1       # other states' stickiness is not this pass's
    if branch == "state":
        lv["state_stick"][FLAT_S], lv["state_has_stick"][FLAT_S] = state_stick, 1
    for key in ("lists", "len", "kind"):
        lv[key][order] = sa[key]
    for oi, step in enumerate(steps):
        p = order[oi]
        if branch == "nil":
            assert step["stick"] == 1.5
            lv["part_has_w"][p], lv["part_w"][p] = 1, 0                    # there, and not to be read
        elif branch == "state" and step["stick"] == state_stick:
            pass
        else:
            assert branch == "part" or step["stick"] != 1.5
            if step["stick"] != 1.5:
                lv["part_has_w"][p], lv["part_w"][p] = 1, int(step["stick"])
    return lv


def check_stay_live_pass(kc, wd, steps, k, reverse, tag, branch="part", state_stick=None, word=0):
    P = len(steps)
    order = np.arange(P)[::-1] if reverse else np.arange(P)
    rc = plain_row_count(wd, steps)
    want = 1 if any(not certain_stay(wd, step, k, rc) for step in steps) else word
    _, words, rows = kc.flat_stay_live(wd, live_problem(steps, order, branch=branch, state_stick=state_stick), k, FLAT_TOP, FLAT_MASK,
                                       word=word)
    assert int(words[0]) == SENTINEL_A and int(words[2]) == SENTINEL_B, tag
    assert int(words[1]) == want, (tag, "verdict word", int(words[1]), want)
    assert rows[wd["NX"] + 1] == GUARD, tag
    assert np.array_equal(rows[:wd["NX"] + 1], rc if wd["NP"] > 0 else np.zeros_like(rc)), tag
    return want


def check_flat_stay_live(kc, group):
    """The stay tables of h. through the live lists: no offending step, one at step 0, one at P - 1 (once per group, under
    both pass orders), and every table step in turn as the one step of its pass that is not a filler.  A table step
    gets ONE pass: the order (identity for even steps, reversed for odd ones), the pass length (131, 64, 257) and the lane
    alternate from step to step on purpose -- the kernel treats every position alike, so the table as a whole sees every
    order, length and lane, and a step costs one entry call, not six."""
    for n_run, (wd, steps, k) in enumerate(stay_group_runs(group)):
        filler = stay_filler(10)
        seen = set()
        for i, step in enumerate(steps):
            # the other table steps as fillers that keep their top priority node: the rows count what they do in the table
            P = (131, 64, 257)[i % 3]
            allsteps = [filler] * P
            for j, other in enumerate(steps):
                top = step_top(other)
                allsteps[(13 * j + FLAT_LANES[i % 5]) % P] = step if j == i else stay_filler(top if top >= 0 else None)
            seen.add(check_stay_live_pass(kc, wd, allsteps, k, i % 2 == 1, (group, n_run, i)))
        if k == 1:
            assert seen == {0, 1}, (group, n_run)
        else:
            assert seen == {1}, (group, n_run)
        if k == 1 and n_run == 0:
            for reverse in (False, True):
                for P in (1000, 65):
                    bad = next(step for step in steps if not certain_stay(wd, step, 1, plain_row_count(wd, [filler] * (P - 1) + [step])))
                    assert check_stay_live_pass(kc, wd, [stay_filler()] * P, 1, reverse, (group, n_run, "none", P)) == 0
                    assert check_stay_live_pass(kc, wd, [bad] + [filler] * (P - 1), 1, reverse, (group, n_run, "first", P)) == 1
                    assert check_stay_live_pass(kc, wd, [filler] * (P - 1) + [bad], 1, reverse, (group, n_run, "last", P)) == 1


def check_flat_stay_live_stickiness(kc):
    """The three sources of a step's stickiness (plan.go:104-115), each deciding the verdict: node 1 holds 5 against node
    2's 4 -- a stay with 1.5, none with 0.  The kernel only ever stores a 1: a word that was not zeroed stays."""
    wd = flat_world(BASE_CNT)
    for P in (1, 300):
        for reverse in (False, True):
            tag = ("stickiness", P, reverse)
            # no weights at all: 1.5, although every partition carries a weight of 0 that must not be read
            assert check_stay_live_pass(kc, wd, [_o(1)] * P, 1, reverse, tag, branch="nil") == 0
            # the same partitions with weights: the 0 counts
            assert check_stay_live_pass(kc, wd, [_o(1, 0)] * P, 1, reverse, tag) == 1
            # weights exist, the partition has none, the state has no stickiness (the other states' 77 is not its own): 1.5
            assert check_stay_live_pass(kc, wd, [_o(1)] * P, 1, reverse, tag) == 0
            # ... the state's stickiness of 0 counts, and one of 2 keeps the stay; a partition's own weight goes first
            assert check_stay_live_pass(kc, wd, [_o(1, 0)] * P, 1, reverse, tag, branch="state", state_stick=0) == 1
            assert check_stay_live_pass(kc, wd, [_o(1, 2)] * P, 1, reverse, tag, branch="state", state_stick=2) == 0
            assert check_stay_live_pass(kc, wd, [_o(1, 2)] * (P - 1) + [_o(1, 0)], 1, reverse, tag, branch="state", state_stick=2) == 1
            assert check_stay_live_pass(kc, wd, [_o(1, 2)] * (P - 1) + [_o(1, 3)], 1, reverse, tag, branch="state", state_stick=0) == 0
    assert check_stay_live_pass(kc, wd, [_o(1)] * 70, 1, False, "a word of 7 stays", word=7) == 7
    assert check_stay_live_pass(kc, wd, [_o(1)] * 69 + [_o(3, 0)], 1, False, "a word of 7 becomes 1", word=7) == 1


# ---- k. k_flat_commit_stay ----------------------------------------------------------------------------------------------------

COMMIT_P = [1, 64, 65, 300]
COMMIT_KINDS = ["random", "one_pair", "no_tops", "no_bump", "np_0", "whole"]


def check_flat_commit_stay(kc, P):
    N, NX, M, s, top_state, L = 6, 8, 3, 1, 0, 2
    for kind in COMMIT_KINDS:
        r = _rng(13, P, COMMIT_KINDS.index(kind))
        beg, end = (0, P) if kind == "whole" or P == 1 else (P // 4, P - P // 5)
        steps = []
        for i in range(P):
            if not beg <= i < end:                   # outside the run: nothing held in s, a top that must not be bumped
                steps.append(st({top_state: [1]}))
                continue
            o = 2 if kind == "one_pair" else int(r.integers(0, N))
            top = {"one_pair": [5], "no_tops": [None, "nil", []][i % 3]}.get(kind, [[int(r.integers(0, NX)), 3], None, [int(r.integers(0, NX))], "nil"][int(r.integers(0, 4))])
            steps.append(st({s: [o], 2: [4], **({top_state: top} if top is not None else {})}, stick=int(r.integers(0, 3))))
        NP, bump = (0 if kind == "np_0" else 977), (0 if kind == "no_bump" else 1)
        ntn0 = np.concatenate([r.integers(1, 100, (NX + 1) * N), [0x7EADBEEF]])
        want = ntn0.copy()
        out_want = np.full(2 * P + 1, GUARD, np.int64)
        for i in range(beg, end):
            o, t_ = step_nodes(steps[i], s)[0], step_top(steps[i], top_state)
            out_want[2 * i], out_want[2 * i + 1] = 1, o
            if NP > 0 and bump:
                want[(NX if t_ < 0 else t_) * N + o] += 1
        _, ntn, out = kc.flat_commit_stay(N, NX, M, steps_arrays(steps, M, L), s, top_state, NP, beg, end, bump, ntn0)
        assert np.array_equal(out, out_want), (P, kind, np.flatnonzero(out != out_want)[:4].tolist())
        assert np.array_equal(ntn, want), (P, kind, np.flatnonzero(ntn != want)[:4].tolist())
        if kind == "one_pair":
            assert want[5 * N + 2] - ntn0[5 * N + 2] == end - beg


# ---- refusals ---------------------------------------------------------------------------------------------------------------

def check_flat_refusals(kc):
    """A node id >= NX, a list longer than L, end > P (a pass order outside [0, P)): kCaseBadArg, no launch, outputs as
    they were."""
    wd = flat_world(BASE_CNT)
    steps = [stay_filler()] * 10
    rc0 = plain_row_count(wd, steps)
    FILL = 0x3C

    def broken(how):
        sa = steps_arrays(steps)
        if how == "node":
            sa["lists"][4, FLAT_S, 0] = wd["NX"]
        elif how == "long":
            sa["len"][4, 1] = FLAT_L + 1
        return sa

    pat32 = np.int32(FILL * 0x01010101)
    for how in ("node", "long", "end"):
        end = 11 if how == "end" else 10
        rc, scan, part, _ = kc.flat_scan(wd, broken(how), rc0, 1, 0, end, FLAT_TOP, FLAT_MASK, check=False, fill=pat32)
        assert rc == BAD_ARG and np.all(scan == pat32) and np.all(part == pat32), how
        N, NX = wd["N"], wd["NX"]
        ntn0 = np.arange((NX + 1) * N + 1)
        rc, ntn, out = kc.flat_commit_stay(N, NX, FLAT_M, broken(how), FLAT_S, FLAT_TOP, 977, 0, end, 1, ntn0, check=False)
        assert rc == BAD_ARG and np.array_equal(ntn, ntn0) and not out.any(), how
        lv = live_problem(steps, np.arange(10))
        b = broken(how)
        lv["lists"], lv["len"] = b["lists"], b["len"]
        if how == "end":
            lv["order"][3] = 10
        rc, words, rows = kc.flat_stay_live(wd, lv, 1, FLAT_TOP, FLAT_MASK, word=7, check=False, fill=pat32)
        assert rc == BAD_ARG and [int(x) for x in words] == [SENTINEL_A, 7, SENTINEL_B] and np.all(rows == pat32), how
    sa = steps_arrays([_o(wd["N"] - 1)] * 10)        # commit: the held node of a step of the range is not in nodesNext
    sa["lists"][7, FLAT_S, 0] = 12
    ntn0 = np.arange(13 * 12 + 1)
    rc, ntn, out = kc.flat_commit_stay(12, 12, FLAT_M, sa, FLAT_S, FLAT_TOP, 977, 0, 10, 1, ntn0, check=False)
    assert rc == BAD_ARG and np.array_equal(ntn, ntn0) and not out.any()
    bad = dict(wd, N=wd["NX"] + 1)                   # prepare: more nodes in nodesNext than node names
    rc, tot, g, top_g, top_n = kc.flat_prepare(bad, check=False, fill=FILL)
    assert rc == BAD_ARG and np.all(tot == FILL) and np.all(g == FILL) and np.all(top_g == FILL) and np.all(top_n == FILL)
    rc, tot, _, _, _ = kc.flat_prepare(dict(wd, s=FLAT_M), check=False, fill=FILL)
    assert rc == BAD_ARG and np.all(tot == FILL)
