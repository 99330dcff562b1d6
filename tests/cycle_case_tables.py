"""k_cycle_group and k_cycle_top alone (blance_amd/csrc/k_cycle.h): the hand-made worlds, the tables as the upload builds them
(written again here, in plain Python, from the issue's definition) and the check, shared by
tests/test_cycle_cases_emulated.py (SIMT emulator) and tests/test_cycle_cases_gpu.py (device).

A world: regions of consecutive leaves, some leaves with a node, P steps in a scrambled pass order whose step j has
top priority node alive_ids[j % A].  The reference is the parent's own path on the same world -- k_chain_classify, the stable
counting sort by region and k_invert for the grouping; k_gather_chain's keys and the stable counting sort by leaf for the
work list -- and every array is compared word for word: chain_order, chain_oi, chain_inv, reg_off, regid, n_ev, the flags,
top_off, top_order.  Every output starts as a poison pattern, so a word neither path writes compares equal only as poison."""
import ctypes as C

import numpy as np

POISON = -0x35014542
BAD_ARG = -100
FLAG_NOT_LOCAL, FLAG_ORPHANS, FLAG_EVENTS = 0, 6, 7


def world(sizes, has_node, P, seed=1, events=None):
    """sizes: leaves per region; has_node(region, leaf in region) -> bool; events = {step: [nodes the step holds in the pass's
    state]}.  Node ids go by leaf order."""
    reg_lo = np.cumsum([0] + list(sizes))[:-1].astype(np.int32)
    n_leaves = int(sum(sizes))
    node_region, node_leaf = [], []
    for r, sz in enumerate(sizes):
        for lf in range(sz):
            if has_node(r, lf):
                node_region.append(r)
                node_leaf.append(int(reg_lo[r]) + lf)
    NX = len(node_region)
    A = NX
    alive_ids = np.arange(A, dtype=np.int32)
    rng = np.random.RandomState(seed)
    order = rng.permutation(P).astype(np.int32)
    L, M = 2, 2
    live = np.zeros((P, M, L), np.int32)
    live_len = np.zeros((P, M), np.int32)
    live_kind = np.zeros((P, M), np.uint8)
    for oi in range(P):
        p = order[oi]
        live[p, 0, 0] = alive_ids[oi % A]
        live_len[p, 0] = 1
        live_kind[p, 0] = 2
        for x in (events or {}).get(oi, []):
            live[p, 1, live_len[p, 1]] = x
            live_len[p, 1] += 1
            live_kind[p, 1] = 2
    return dict(P=P, L=L, NX=NX, A=A, B=len(sizes), n_leaves=n_leaves, order=order, live=live.reshape(-1), live_len=live_len.reshape(-1),
                live_kind=live_kind.reshape(-1), node_region=np.array(node_region, np.int32), node_leaf_pos=np.array(node_leaf, np.int32),
                reg_lo=reg_lo, alive_ids=alive_ids)


def tables(w, words):
    """The issue's definition: r_a, q_a, c_r; len_r = (P / A) c_r + #{a < P % A : r_a = r}; top_off over the global leaves,
    P / A + (a < P % A) steps at the leaf of alive node a."""
    P, A, B = w["P"], w["A"], w["B"]
    full, part = P // A, P % A
    cyc = np.zeros((A, words), np.int32)
    count = [0] * B
    length = [0] * B
    steps = np.zeros(w["n_leaves"], np.int64)
    for a in range(A):
        n = int(w["alive_ids"][a])
        r = int(w["node_region"][n])
        cyc[a, 0], cyc[a, 1], cyc[a, 2] = r, count[r], w["node_leaf_pos"][n]
        count[r] += 1
        length[r] += full + (1 if a < part else 0)
        steps[w["node_leaf_pos"][n]] = full + (1 if a < part else 0)
    for a in range(A):
        cyc[a, 3] = count[cyc[a, 0]]
    reg_off = np.concatenate([[0], np.cumsum(length)]).astype(np.int32)
    top_off = np.concatenate([[0], np.cumsum(steps)]).astype(np.int32)
    return cyc.reshape(-1), reg_off, top_off


every = lambda r, lf: True
WORLDS = {
    # name -> (sizes, has_node, P)
    "one_alive_node": ([4, 4], lambda r, lf: (r, lf) == (1, 2), 300),
    "region_with_one_node": ([8, 8, 8], lambda r, lf: r != 1 or lf == 5, 1000),
    "region_with_none": ([8, 8, 8], lambda r, lf: r != 1, 1000),
    "fewer_steps_than_nodes": ([16, 16, 16], every, 29),
    "partial_cycle_inside_a_region": ([16, 16, 16], every, 48 * 7 + 21),
    "ragged_last_region": ([16, 16, 5], every, 37 * 11 + 35),
    "leaves_without_a_node": ([16, 16], lambda r, lf: lf % 3 != 1, 700),
    "two_chunks_of_steps": ([128, 128], every, 3000),
    # (a node with 1, 63, 64 and 65 steps: A = 32, P = 32 s + 5 gives s + 1 steps to five nodes and s to the rest)
    "steps_1_and_0": ([16, 16], every, 5),
    "steps_63_and_62": ([16, 16], every, 32 * 62 + 5),
    "steps_64_and_63": ([16, 16], every, 32 * 63 + 5),
    "steps_65_and_64": ([16, 16], every, 32 * 64 + 5),
}


class CycleCases:
    def __init__(self, lib_path):
        self.lib = C.CDLL(lib_path)
        self.lib.blance_case_cycle.restype = C.c_int
        self.words = self.lib.blance_case_cycle_words()
        self.n_flags = self.lib.blance_case_cycle_flags()

    def run(self, which, w, tabs, refute=0, closed=0, with_top=1):
        cyc, reg_off_tab, top_off_tab = tabs
        P, B, nl = w["P"], w["B"], w["n_leaves"]
        out = {k: np.full(n, POISON, np.int32) for k, n in (("chain_order", P), ("chain_oi", P), ("chain_inv", P), ("regid", P), ("n_ev", P + 1),
                                                           ("reg_off", B + 1), ("top_off", nl + 1), ("top_order", P), ("flags", self.n_flags))}
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        st = self.lib.blance_case_cycle(which, P, w["L"], w["NX"], w["A"], B, nl, refute, closed, with_top,
                                        ptr(w["order"]), ptr(w["live"]), ptr(w["live_len"]), ptr(w["live_kind"]), ptr(w["node_region"]),
                                        ptr(w["node_leaf_pos"]), ptr(w["reg_lo"]), ptr(w["alive_ids"]), ptr(cyc), ptr(reg_off_tab), ptr(top_off_tab),
                                        *[ptr(out[k]) for k in ("chain_order", "chain_oi", "chain_inv", "regid", "n_ev", "reg_off", "top_off",
                                                                "top_order", "flags")])
        return st, out


def same(ref, new, skip=()):
    for k in ref:
        if k not in skip:
            assert (ref[k] == new[k]).all(), (k, np.nonzero(ref[k] != new[k])[0][:8], ref[k][:16], new[k][:16])


def check(cc, name):
    sizes, has_node, P = WORLDS[name]
    w = world(sizes, has_node, P)
    tabs = tables(w, cc.words)
    st0, ref = cc.run(0, w, tabs)
    st1, new = cc.run(1, w, tabs)
    assert st0 == 0 and st1 == 0, (st0, st1)
    assert not ref["flags"].any()
    same(ref, new)
    assert (np.sort(new["chain_order"]) == np.arange(P)).all() and (new["top_order"] != POISON).all()


def check_events_and_orphans(cc):
    """Nodes of the pass's state outside the step's region (events: counted per step) and in no region (orphans): the same
    counts and flag words.  (The work list is not compared: the reference's k_gather_chain is not part of these words.)"""
    w = world([8, 8, 8], every, 500, events={3: [20], 77: [1, 17], 400: [2]})
    w["node_region"][17] = -1                      # a node outside every region, never a top priority node here
    w["alive_ids"] = np.array([n for n in range(w["NX"]) if n != 17], np.int32)
    w["A"] = len(w["alive_ids"])
    live = w["live"].reshape(w["P"], 2, 2)
    for oi in range(w["P"]):
        live[w["order"][oi], 0, 0] = w["alive_ids"][oi % w["A"]]
    tabs = tables(w, cc.words)
    st0, ref = cc.run(0, w, tabs, with_top=0)
    st1, new = cc.run(1, w, tabs, with_top=0)
    assert st0 == 0 and st1 == 0
    assert ref["flags"][FLAG_EVENTS] == 1 and ref["flags"][FLAG_ORPHANS] == 1 and ref["flags"][FLAG_NOT_LOCAL] == 0 and ref["n_ev"].sum() == 3
    same(ref, new)


def check_closed_gate(cc):
    """Behind a closed gate neither path writes a word."""
    w = world([16, 16], every, 300)
    tabs = tables(w, cc.words)
    for which in (0, 1):
        st, out = cc.run(which, w, tabs, closed=1)
        assert st == 0
        for k, v in out.items():
            assert (v == POISON).all() if k != "flags" else not v.any(), (which, k)


def check_refute(cc):
    """The knob: step 0 expects the next node.  Only kFlagNotLocal differs from the reference."""
    w = world([16, 16, 5], every, 442)
    tabs = tables(w, cc.words)
    st0, ref = cc.run(0, w, tabs)
    st1, new = cc.run(1, w, tabs, refute=1)
    assert st0 == 0 and st1 == 0
    assert ref["flags"][FLAG_NOT_LOCAL] == 0 and new["flags"][FLAG_NOT_LOCAL] == 1
    new["flags"][FLAG_NOT_LOCAL] = 0
    same(ref, new)


def check_premise(cc):
    """A step whose top priority node is not the round robin's: kFlagNotLocal, and the outputs are still a permutation."""
    w = world([16, 16], every, 300)
    live = w["live"].reshape(300, 2, 2)
    live[w["order"][123], 0, 0] = (live[w["order"][123], 0, 0] + 1) % w["NX"]
    tabs = tables(w, cc.words)
    st, new = cc.run(1, w, tabs)
    assert st == 0 and new["flags"][FLAG_NOT_LOCAL] == 1
    assert (np.sort(new["chain_order"]) == np.arange(300)).all() and (new["chain_inv"][new["chain_order"]] == np.arange(300)).all()


def check_refusals(cc):
    w = world([16, 16], every, 300)
    cyc, ro, to = tables(w, cc.words)
    bad = ro.copy(); bad[1] += 200
    assert cc.run(1, w, (cyc, bad, to))[0] == BAD_ARG
    bad = to.copy(); bad[5] = 299
    assert cc.run(1, w, (cyc, ro, bad))[0] == BAD_ARG
    bad = cyc.copy(); bad[0] = 2
    assert cc.run(1, w, (bad, ro, to))[0] == BAD_ARG
