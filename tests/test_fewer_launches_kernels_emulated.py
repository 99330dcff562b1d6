"""Single kernels of the fewer-launches change under the SIMT emulator, on inputs made by hand, for the branches that no plan
was found to reach (tests/test_fewer_launches_emulated.py has the plans):

* gather_chain_record's `classify` branch: about 5,100 assumed classifications of randgen's plans were searched and none is
  refuted by the device's own words, so k_chain_classify and k_gather_chain(classify = 1) run here over the same hand-made
  lists -- a node of the state in another region, one in no region, lists longer than kChainOwn with such a node behind the
  cut -- and must raise the same two words;
* k_flat_stay_live's verdict store with the one step that is no certain stay at step 0, in the middle, at the last step of
  a wave, at step P - 1 of a last wave that is partly out of range (P no multiple of 64), and nowhere;
* k_period_judge's refusals that need a leaf which is no candidate (a plan with nodesToRemove never walks periodically), a
  negative or missing d, and a raised kFlagEscaped -- beside regions that pass, in one launch, against the counters and
  words worked out here."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from test_simt_emulated import HERE, _deps

SRC = os.path.join(HERE, "simt", "emu_kernel_cases.cpp")
SO = os.path.join(HERE, "simt", "_build", "libblance_emu_kernel_cases.so")

# blance_kernels.h / k_period.h
LIST_ABSENT, LIST_SET = 0, 2
CHAIN_OWN, CW = 4, 24
FLAG_NOT_LOCAL, FLAG_ESCAPED, FLAG_ORPHANS, FLAG_EVENTS, CHAIN_FLAGS = 0, 1, 6, 7, 8
PT, PLIMIT, POK, PD, PBEG1, PEND1, PBEG2, PEND2, PBEG3, PEND3, PWORDS = range(11)
INT_MIN = -2 ** 31


@pytest.fixture(scope="module")
def lib():
    deps = _deps() + [SRC]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.check_call(["g++", "-x", "c++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off",
                               "-Wno-unknown-pragmas", "-o", SO, SRC])
    return ctypes.CDLL(SO)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _i32(x):
    return np.ascontiguousarray(x, dtype=np.int32)


# ---- part 3: k_gather_chain raises k_chain_classify's two words ---------------------------------------------------------

REG = 6                                              # two regions of six leaves: nodes 0-5 and 6-11; node 12 lies in no region
N_NODES, ORPHAN = 13, 12
LOCAL = ([0], [1])                                   # (the top priority node's list, the state's list): all in region 0

# name: (the odd partition's two lists, the words expected: events, orphans, not local)
CLASSIFY_CASES = {
    "all_local": (LOCAL, (0, 0, 0)),
    "node_in_another_region": (([1], [7]), (1, 0, 0)),
    "node_in_no_region": (([2], [ORPHAN]), (1, 1, 0)),
    "both": (([2], [3, ORPHAN, 8]), (1, 1, 0)),
    # lists longer than kChainOwn: the gather cannot represent them (not local) and must still look at every node
    "long_list_all_local": (([5], [0, 1, 2, 3, 4]), (0, 0, 1)),
    "long_list_remote_behind_the_cut": (([5], [0, 1, 2, 3, 4, 7]), (1, 0, 1)),
    "long_list_orphan_behind_the_cut": (([5], [0, 1, 2, 3, 4, ORPHAN]), (1, 1, 1)),
    # a step without a region (no top priority node; its top priority node in no region): neither word, in both kernels
    "no_top_priority_node": ((None, [7, ORPHAN]), (0, 0, 1)),
    "top_priority_node_in_no_region": (([ORPHAN], [7]), (0, 0, 1)),
}


@pytest.mark.parametrize("where", [0, 299])          # (the odd partition in the first / the second workgroup of 256)
@pytest.mark.parametrize("name", list(CLASSIFY_CASES))
def test_gather_raises_the_classification_words(lib, name, where):
    (top, own), (events, orphans, not_local) = CLASSIFY_CASES[name]
    P, M, L = 300, 2, 6
    live = np.full((P, M, L), -1, dtype=np.int32)
    live_len = np.zeros((P, M), dtype=np.int32)
    kind = np.full((P, M), LIST_SET, dtype=np.uint8)
    for p in range(P):
        t, o = (top, own) if p == where else ([p % REG], [(p + 1) % REG])
        for m, lst in ((0, t), (1, o)):
            if lst is None:
                kind[p, m] = LIST_ABSENT
                continue
            live[p, m, :len(lst)] = lst
            live_len[p, m] = len(lst)
    order = _i32(np.arange(P))
    node_region = _i32([0] * REG + [1] * REG + [-1])
    node_leaf_pos = _i32(list(range(2 * REG)) + [-1])
    reg_lo = _i32([0, REG])
    got = {}
    for classify in (1, 0):
        fc, fg = np.zeros(CHAIN_FLAGS, dtype=np.int32), np.zeros(CHAIN_FLAGS, dtype=np.int32)
        lib.emu_case_classify_words(P, M, L, N_NODES, 1, 0, _p(live), _p(live_len), _p(kind), _p(order), _p(node_region),
                                    _p(node_leaf_pos), _p(reg_lo), 2 * REG, classify, _p(fc), _p(fg))
        got[classify] = (fc, fg)
    fc, fg = got[1]
    assert (fc[FLAG_EVENTS], fc[FLAG_ORPHANS]) == (events, orphans), fc             # k_chain_classify, the reference here
    assert (fg[FLAG_EVENTS], fg[FLAG_ORPHANS]) == (events, orphans), fg             # k_gather_chain(classify = 1): the same
    assert fg[FLAG_NOT_LOCAL] == not_local, fg
    fc0, fg0 = got[0]                                                               # a pass that classified: the gather raises neither
    assert (fg0[FLAG_EVENTS], fg0[FLAG_ORPHANS], fg0[FLAG_NOT_LOCAL]) == (0, 0, not_local), fg0
    assert np.array_equal(fc0, fc)


# ---- part 2: k_flat_stay_live's own verdict word ----------------------------------------------------------------------------

STAY_P = 4133                                        # 64 * 64 + 37: the last wave has 37 steps in range; 17 workgroups of 256


@pytest.mark.parametrize("order", ["identity", "reversed"])
@pytest.mark.parametrize("at", [None, (0,), (STAY_P - 1,), (63,), (64,), (2000,), (4095,), (4096,), (0, STAY_P - 1), "all"])
def test_stay_live_stores_the_verdict(lib, at, order):
    """Every partition holds one live node -- a certain stay, no other candidate is listed -- but the steps `at`, which hold
    none.  The word is 1 exactly when there is such a step; its neighbours stay as they were."""
    P, N = STAY_P, 50
    steps = list(range(P)) if at == "all" else list(at or ())
    ordr = _i32(np.arange(P) if order == "identity" else np.arange(P)[::-1])
    live = _i32(np.arange(P) % N)
    live_len = np.ones(P, dtype=np.int32)
    kind = np.full(P, LIST_SET, dtype=np.uint8)
    for oi in steps:
        live_len[ordr[oi]] = 0
    words = _i32([-7, 0, -9])
    lib.emu_case_stay_live(P, N, _p(live), _p(live_len), _p(kind), _p(ordr), _p(words[1:]))
    assert list(words) == [-7, 1 if steps else 0, -9]
    # (a word that an earlier sweep left at 1 stays 1: the kernel never stores a 0, open_sweep's fill does)
    words = _i32([-7, 1, -9])
    lib.emu_case_stay_live(P, N, _p(live), _p(live_len), _p(kind), _p(ordr), _p(words[1:]))
    assert list(words) == [-7, 1, -9]


# ---- part 1: k_period_judge ------------------------------------------------------------------------------------------------------

def _judge_model(rg, s, NX, OW, escaped, cnt1, cnt, pb, out):
    """What k_period_state_max, k_period_state_check, k_period_verdict and k_period_counts did to one joined region."""
    B = pb.shape[1]
    cbeg, cend, T, limit = rg["cbeg"], rg["cend"], rg["T"], rg["limit"]
    live = [n for n, a in rg["leaves"] if n >= 0 and a]
    dead = [n for n, a in rg["leaves"] if n >= 0 and not a]
    diff = lambda n: int(cnt[s * NX + n] - cnt1[s * NX + n])
    d = max([diff(n) for n in live], default=INT_MIN)
    ok = all(diff(n) == 0 for n in dead) and all(diff(n) == d for n in live) and d != INT_MIN and d >= 0 and not escaped
    i = rg["i"]
    pb[PD, i], pb[POK, i], pb[PBEG3, i], pb[PEND3, i] = d, int(ok), cbeg + limit if ok else cbeg + 2 * T, cend
    if ok:
        full, rest = divmod(limit - 2 * T, T)
        for n in live:
            cnt[s * NX + n] += d * full
        for j in range(rest):
            o = out[(cbeg + T + j) * OW:(cbeg + T + j + 1) * OW]
            for c in range(int(o[0]) & 0xffff):
                if 0 <= o[1 + c] < NX:
                    cnt[s * NX + o[1 + c]] += rg["w0"]
    return ok


@pytest.mark.parametrize("threads", [128, 64])
@pytest.mark.parametrize("escaped", [0, 1])
def test_period_judge(lib, threads, escaped):
    rng = np.random.RandomState(11)
    # (leaves, every tenth leaf without a node, periods and a partial period's steps, what goes wrong)
    specs = [
        (5, False, (6, 3), None),                    # passes, d = 2, three steps of a partial last period
        (200, True, (5, 17), None),                  # passes; more leaves than threads, leaves without a node
        (200, False, (4, 0), ("unequal", 150)),      # a live leaf behind the first trip grew by another amount: refused
        (20, False, (7, 1), ("unequal", 0)),
        (20, True, (7, 1), ("dead_moved", 19)),      # a leaf that is no candidate moved: refused
        (20, True, (7, 2), ("dead_still", 19)),      # one that did not: passes
        (12, False, (5, 0), ("negative", None)),     # the counters fell: refused
        (8, False, (4, 0), ("no_live_leaf", None)),  # d stays INT_MIN: refused
        (16, False, (3, 5), ("not_joined", None)),   # fewer than kPeriodMinRounds periods: the kernel leaves the region's words alone
        (16, False, (9, 4), ("d_zero", None)),       # d = 0 is a verdict like any other: passes
    ]
    s, OW, w0 = 1, 3, 1
    B = len(specs)
    N = sum(sp[0] for sp in specs)
    NX = N + 1
    alive = np.ones(N + 1, dtype=np.uint8)
    leaf_node, reg_lo, reg_hi, reg_off, regions = [], [], [], [0], []
    cnt1 = _i32(rng.randint(0, 50, size=2 * NX + 2))
    cnt = cnt1.copy()
    pb = np.full((PWORDS, B), -5, dtype=np.int32)
    node = 0
    for i, (n_leaves, holes, (periods, rest), wrong) in enumerate(specs):
        kind, arg = wrong or (None, None)
        lo = len(leaf_node)
        leaves = []
        for j in range(n_leaves):
            has_node = not (holes and j % 10 == 7)
            a = 1
            if kind in ("dead_moved", "dead_still") and j in (arg, 3):
                a = 0
            if kind == "no_live_leaf":
                a = 0
            leaves.append((node if has_node else -1, a))
            leaf_node.append(node if has_node else -1)
            if has_node:
                alive[node] = a
                node += 1
        T = max(n_leaves // 2, 2)
        limit = periods * T + rest
        cbeg = reg_off[-1]
        reg_off.append(cbeg + limit + 7)             # (a tail behind the periodic stretch)
        reg_lo.append(lo)
        reg_hi.append(len(leaf_node))
        d = {"negative": -1, "d_zero": 0}.get(kind, 2)
        for j, (n, a) in enumerate(leaves):
            if n < 0:
                continue
            g = d if a else 0
            if kind == "unequal" and j == arg:
                g = d + 1 if arg else d - 1
            if kind == "dead_moved" and j == arg:
                g = 1
            cnt[s * NX + n] += g
        pb[PT, i], pb[PLIMIT, i], pb[POK, i], pb[PD, i] = T, limit, 1 if kind != "not_joined" else 0, INT_MIN
        regions.append(dict(i=i, cbeg=cbeg, cend=reg_off[-1], T=T, limit=limit, leaves=leaves, w0=w0, joined=kind != "not_joined"))
    steps = reg_off[-1]
    out = _i32(np.zeros(steps * OW))
    for rg in regions:                               # every step emitted one or two nodes of its region
        nodes = [n for n, _ in rg["leaves"] if n >= 0]
        for t in range(rg["cbeg"], rg["cend"]):
            k = 1 + t % 2
            out[t * OW] = k | (3 << 16)              # (the kernel reads the low half of the word)
            out[t * OW + 1:t * OW + 1 + k] = rng.choice(nodes, size=k)
    crec = _i32(np.full(steps * CW, -1))
    for rg in regions:                               # (every record has its weight: the kernel counts a step with its own)
        crec[rg["cbeg"] * CW + 1:rg["cend"] * CW:CW] = w0
    flags = np.zeros(CHAIN_FLAGS, dtype=np.int32)
    flags[FLAG_ESCAPED] = escaped
    want_cnt, want_pb = cnt.copy(), pb.copy()
    verdicts = [_judge_model(rg, s, NX, OW, escaped, cnt1, want_cnt, want_pb, out) if rg["joined"] else None for rg in regions]
    if not escaped:                                  # (the cases are what their names say)
        assert verdicts == [True, True, False, False, False, True, False, False, None, True]
    else:
        assert not any(verdicts)
    reg_off, reg_lo, reg_hi, leaf_node = _i32(reg_off), _i32(reg_lo), _i32(reg_hi), _i32(leaf_node)
    lib.emu_case_period_judge(B, s, N, NX, OW, _p(reg_off), _p(reg_lo), _p(reg_hi), _p(leaf_node), _p(alive), _p(crec), _p(out),
                              _p(flags), _p(cnt1), _p(cnt), _p(pb), threads)
    assert np.array_equal(pb, want_pb), (pb, want_pb)
    assert np.array_equal(cnt, want_cnt)
