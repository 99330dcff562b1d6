"""The chain kernel's hand-off: k_pass_chain walks a region only while things move there, stops at the first
stage boundary behind a stage of stay rounds only, and k_stay_by_top checks the rest of that region's chain in parallel, from
the counters the walk left and with the walked steps replayed from what they emitted.

Under the SIMT emulator (its wave fibers are not in lockstep: a helper wave left on a barrier shows as a stuck test), every
plan against the C oracle on digest, iterations and warnings, with a small BLANCE_CHAIN_HANDOFF, on four and on eight waves
(BLANCE_CHAIN_WAVES: stages of 256 and of 512 steps) and with one and two replicas.  Under BLANCE_TRACE the driver says where
each region's walk stopped; the tests read the stops from that line and set them against what the oracle says moved.

The regions are zones of 128 leaves; a step's region is its primary's zone, its place in the region's chain its rank in the
pass order among the steps of that zone.

Events: a pass whose classification finds nodes outside their partition's region (k_chain_classify's word) does not hand off
at all -- k_stay_by_top does not take such passes -- so the kernel's own condition "no event of the region is left" is never
the deciding one in a plan; test_busy_region_beside_a_calm_one checks the driver's side of it (sweep 1 of that rebalance)."""
import re

import numpy as np
import pytest

from blance_amd import hip, synth
from test_simt_emulated import _oracle, emu_lib  # noqa: F401  (the fixture)

WAVES = (4, 8)
KS = (1, 2)
ZONE = 128

HANDED = re.compile(r"region (\d+) at step (\d+) of (\d+);")
WALKED = re.compile(r"region (\d+) walked to its end \((\d+)\);")
MOVED = "a step behind the hand-off moved, the pass runs again without"
NO_HANDOFF = "no hand-off"


def _plan(lib, fp, monkeypatch, capfd, handoff, waves, trace=True, spec="1"):
    """One plan on a fresh planner: (the result, the trace)."""
    monkeypatch.setenv("BLANCE_SPECULATE", spec)
    if handoff is None:
        monkeypatch.delenv("BLANCE_CHAIN_HANDOFF", raising=False)
    else:
        monkeypatch.setenv("BLANCE_CHAIN_HANDOFF", str(handoff))
    monkeypatch.setenv("BLANCE_CHAIN_WAVES", str(waves))
    if trace:
        monkeypatch.setenv("BLANCE_TRACE", "1")
    else:
        monkeypatch.delenv("BLANCE_TRACE", raising=False)
    capfd.readouterr()
    pl = hip.Planner(lib_path=lib, chain_min_parts=64)
    try:
        got = pl.plan(fp)
    finally:
        pl.close()
    return got, capfd.readouterr().err


def _same(got, want, tag):
    assert (got.digest(), got.iterations, got.n_warnings) == (want.digest(), want.iterations, want.n_warnings), tag


def _stops(trace):
    """The hand-off lines of a trace, one dict per pass: region -> (the step its walk stopped at or None, its chain's length)."""
    out = []
    for line in trace.splitlines():
        if "hand-off (" not in line:
            continue
        d = {int(r): (int(at), int(n)) for r, at, n in HANDED.findall(line)}
        d.update({int(r): (None, int(n)) for r, n in WALKED.findall(line)})
        out.append(d)
    return out


def _config3(P, N, k):
    c = synth.config_case(3, P=P, N=N)
    c["model"] = {"primary": {"priority": 0, "constraints": 1}, "replica": {"priority": 1, "constraints": k}}
    return synth.case_to_flat(c)


class Replan:
    """PlanNextMap over the converged plan of config 3's shape (prevMap = partitionsToAssign = that plan): a call in which
    every step stays, until a test changes a list or the pass order."""

    def __init__(self, P, N, k):
        self.P, self.N, self.k = P, N, k
        self.fp0 = _config3(P, N, k)
        self.res0 = _oracle(self.fp0)
        self.M = M = int(self.fp0.n_states)
        self.off = np.asarray(self.res0.out_off[:P * M + 1]).copy()
        self.nodes = np.asarray(self.res0.out_nodes[:self.off[-1]]).copy()
        self.prim = self.nodes[self.off[np.arange(P) * M]]
        self.order = np.asarray(self.fp0.part_order).copy()

    def replicas(self, lists, p):
        return [int(x) for x in lists[self.off[p * self.M + 1]:self.off[p * self.M + 2]]]

    def problem(self, lists=None, order=None, max_iterations=10):
        fp = synth.replan_problem(self.fp0, self.res0)
        if lists is not None:
            fp.set("assign_nodes", lists.copy())
            fp.set("prev_nodes", lists.copy())
        if order is not None:
            fp.set("part_order", order.astype(np.int32))
        fp.scalars.update(max_iterations=max_iterations)
        return fp

    def chain_pos(self, order=None):
        """[P] a partition's place in its region's chain."""
        order = self.order if order is None else order
        pos = np.zeros(self.P, dtype=np.int64)
        seen = {}
        for p in order:
            z = int(self.prim[p]) // ZONE
            pos[p] = seen.get(z, 0)
            seen[z] = pos[p] + 1
        return pos

    def moved_in_sweep_1(self, lists, order=None, replicas=None):
        """The partitions whose lists the oracle's first sweep changes (replicas: a dict that takes their new replicas)."""
        r = _oracle(self.problem(lists, order, max_iterations=1))
        o2 = np.asarray(r.out_off[:self.P * self.M + 1])
        n2 = np.asarray(r.out_nodes[:o2[-1]])
        M = self.M
        moved = [q for q in range(self.P)
                 if list(n2[o2[q * M]:o2[q * M + M]]) != list(lists[self.off[q * M]:self.off[q * M + M]])]
        if replicas is not None:
            replicas.update({q: [int(x) for x in n2[o2[q * M + 1]:o2[q * M + 2]]] for q in moved})
        return moved

    def other_rack(self, lists, p):
        """A node of p's zone in a rack that none of p's nodes is in."""
        z = int(self.prim[p]) // ZONE
        racks = {int(self.prim[p]) // 16} | {x // 16 for x in self.replicas(lists, p)}
        return next(n for n in range(z * ZONE, z * ZONE + ZONE) if n // 16 not in racks)


_replans = {}


def _replan(P, N, k):
    if (P, N, k) not in _replans:
        _replans[(P, N, k)] = Replan(P, N, k)
    return _replans[(P, N, k)]


# ---- config 3's shape: every region calms down after its first stage ------------------------------------------------------

@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("waves", WAVES)
def test_config3_shape_hands_off_after_its_second_stage(emu_lib, monkeypatch, capfd, waves, k):
    """Two zones of 128 leaves, chains of six stages (of eight waves) and more.  Sweep 2's replica pass moves steps in each
    region's first stage only (two replicas; none with one): every region hands off after its second (first) stage, sweep 3
    goes straight to k_stay_by_top, and the plan takes the sweeps and round trips it takes without the hand-off."""
    stage = 64 * waves
    fp = _config3(6144, 256, k)
    want = _oracle(fp)
    got, trace = _plan(emu_lib, fp, monkeypatch, capfd, 64, waves)
    _same(got, want, (waves, k))
    passes = _stops(trace)
    # two replicas: sweep 2 moves steps in each region's first stage, sweep 3 is a pass of stays (k_stay_by_top from step 0);
    # one replica: sweep 2 moves nothing and is the last -- its walk stops after the first stage
    sweeps, calm_after, stay_launches = {2: (3, 2, 2), 1: (2, 1, 1)}[k]
    assert want.iterations == sweeps
    assert len(passes) == 1, trace[-3000:]
    assert passes[0] == {0: (calm_after * stage, 3072), 1: (calm_after * stage, 3072)}, passes
    assert got.struct.stay_pass_launches == stay_launches
    assert MOVED not in trace
    on, _ = _plan(emu_lib, fp, monkeypatch, capfd, 64, waves, trace=False)
    off, _ = _plan(emu_lib, fp, monkeypatch, capfd, 0, waves, trace=False)
    _same(on, want, "on")
    _same(off, want, "off")
    assert (on.struct.host_syncs, on.iterations) == (off.struct.host_syncs, off.iterations)


# ---- a step behind the hand-off moves ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("waves", WAVES)
def test_a_late_move_refutes_the_hand_off(emu_lib, monkeypatch, capfd, waves, k):
    """A replan in which one partition near the end of the pass order has swapped a replica with another late one and now
    holds a node of its primary's rack: found with the oracle, whose first sweep moves that step (beside it only late steps,
    or steps of a region's first stage).  Its region calms down long before
    it, hands off, k_stay_by_top finds the step: the pass runs again with the chain kernel alone and the plan does not try
    a hand-off again."""
    rp = _replan(4096, 256, k)
    pos = rp.chain_pos()
    stage = 64 * waves
    found = None
    for p in range(rp.P - 1, rp.P - 20, -1):
        # p swaps a replica with a partition q a little earlier whose replica lies in p's primary's rack, which the rule
        # excludes for p: every node's load stays what it was (no other step is disturbed), and p cannot keep the node
        rack = int(rp.prim[p]) // 16
        for q in range(p - 1, p - 300, -1):
            for sq, x in enumerate(rp.replicas(rp.nodes, q)):
                if x // 16 != rack or x == rp.prim[p] or x in rp.replicas(rp.nodes, p) or found:
                    continue
                lists = rp.nodes.copy()
                lists[rp.off[q * rp.M + 1] + sq] = lists[rp.off[p * rp.M + 1]]
                lists[rp.off[p * rp.M + 1]] = x
                moved = rp.moved_in_sweep_1(lists)
                late = [m for m in moved if pos[m] >= 2 * stage]
                if p in late and all(pos[m] < stage for m in moved if m not in late):
                    found = (p, lists, late)
        if found:
            break
    assert found, "no such problem among the last partitions"
    p, lists, late = found
    fp = rp.problem(lists)
    want = _oracle(fp)
    got, trace = _plan(emu_lib, fp, monkeypatch, capfd, 64, waves)
    _same(got, want, (waves, k, p))
    passes = _stops(trace)
    assert len(passes) == 1, trace[-3000:]                 # (one attempt in this plan)
    z = int(rp.prim[p]) // ZONE
    at, _ = passes[0][z]
    assert at is not None and at <= pos[p], (passes, late, pos[p])
    assert trace.count(MOVED) == 1, trace[-3000:]
    assert trace.index(MOVED) > trace.index("hand-off (")
    assert NO_HANDOFF in trace[trace.index(MOVED):]        # (the pass that runs again, and every later one)


# ---- a region that never calms beside one that does; events ---------------------------------------------------------------

@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("waves", WAVES)
def test_busy_region_beside_a_calm_one(emu_lib, monkeypatch, capfd, waves, k):
    """The rebalance after every tenth node of zone 0 left.  Sweep 1's replica pass has events (the partitions whose primary
    moved to the other zone hold their replicas outside it): no hand-off.  From sweep 2 on zone 0's chain has moves in every
    stage up to its last 512 steps and is walked to its end; zone 1's hands off after its first stage."""
    rp = _replan(4096, 256, k)
    fp = rp.problem()
    rm = np.zeros(rp.N, dtype=np.uint8)
    rm[np.arange(3, ZONE, 10)] = 1
    fp.set("node_removed", rm)
    want = _oracle(fp)
    got, trace = _plan(emu_lib, fp, monkeypatch, capfd, 512, waves)
    _same(got, want, (waves, k))
    assert re.search(r"chain pass state 1: [1-9]\d* events", trace), trace[:3000]
    head = trace[:trace.index("hand-off (")]
    assert NO_HANDOFF in head, head[-2000:]                # (the pass with the events)
    passes = _stops(trace)
    assert passes, trace[-3000:]
    stage = 64 * waves
    for d in passes:
        assert d[0][0] is None, passes                     # the busy region: its chain's end
        assert d[1][0] == stage, passes                    # the calm one
    assert MOVED not in trace


# ---- boundaries ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("waves", WAVES)
def test_hand_off_at_the_last_stage_boundary(emu_lib, monkeypatch, capfd, waves, k):
    """A replan in which every step stays.  Zone 0's chain is one stage and 40 steps: it hands off at its last stage boundary
    with a remainder shorter than a round of 64.  The top priority nodes 40 .. 127 of the zone have all their steps in the
    walked prefix (their waves leave at once), nodes 0 .. 39 one step behind it.  Zone 1's chain is one stage exactly: nothing
    is left to hand off."""
    stage = 64 * waves
    rp = _replan(2 * stage + 40, 256, k)
    fp = rp.problem()
    want = _oracle(fp)
    got, trace = _plan(emu_lib, fp, monkeypatch, capfd, 16, waves)
    _same(got, want, (waves, k))
    passes = _stops(trace)
    assert passes and passes[0] == {0: (stage, stage + 40), 1: (None, stage)}, (passes, trace[-3000:])
    assert MOVED not in trace


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("waves", WAVES)
def test_round_of_replayed_and_tested_lanes(emu_lib, monkeypatch, capfd, waves, k):
    """A replan whose pass order takes each zone's steps with a top priority node of the zone's lower half first (round
    robin over 64 nodes), then the upper half's.  Partition 10 (step 10 of zone 0, top priority node 10) holds, instead of
    its last replica, a node that the later steps of node 10 hold (with one replica, which is the node they all hold: a
    node of its primary's rack); the oracle's first sweep moves it away from that node (to the node they hold), and
    nothing else.  Zone 0 hands off after its second stage: node 10's 24 steps are one round of k_stay_by_top with
    replayed lanes (the mover among them, replayed from what it emitted) in front of tested ones; the upper half's nodes
    have no step in the prefix; zone 1 hands off after its first stage."""
    rp = _replan(6144, 256, k)
    order = np.lexsort((np.arange(rp.P), (rp.prim % ZONE) // 64))
    pos = rp.chain_pos(order)
    stage = 64 * waves
    p = 10
    mine = [q for q in range(rp.P) if rp.prim[q] == rp.prim[p] and pos[q] >= 2 * stage]
    assert 0 < len(mine) < 24 and pos[p] < stage
    held_later = {x for q in mine for x in rp.replicas(rp.nodes, q)}
    rack = int(rp.prim[p]) // 16 * 16
    found = None
    # (a node the later steps hold in place of p's last replica; or, where p holds what they hold, a node of its primary's
    # rack, which the rule excludes: p then moves TO a node they hold)
    for x in sorted(held_later - set(rp.replicas(rp.nodes, p))) + [n for n in range(rack, rack + 16) if n != rp.prim[p]]:
        lists = rp.nodes.copy()
        lists[rp.off[p * rp.M + 2] - 1] = x
        after = {}
        if rp.moved_in_sweep_1(lists, order, after) == [p] and (set(after[p]) ^ set(rp.replicas(lists, p))) & held_later:
            found = lists
            break
    assert found is not None, "no change of partition 10's replicas makes it alone move, to or from a node the later steps hold"
    fp = rp.problem(found, order)
    want = _oracle(fp)
    got, trace = _plan(emu_lib, fp, monkeypatch, capfd, 64, waves)
    _same(got, want, (waves, k))
    passes = _stops(trace)
    assert passes and passes[0] == {0: (2 * stage, 3072), 1: (stage, 3072)}, (passes, trace[-3000:])
    assert MOVED not in trace


# ---- the way out --------------------------------------------------------------------------------------------------------------

def test_handoff_off_is_todays_driver(emu_lib, monkeypatch, capfd):
    """BLANCE_CHAIN_HANDOFF=0: no line of the trace speaks of a hand-off, and the tallies are those that
    tests/test_driver_decisions_emulated.py pins for the shape -- as they are with the default threshold, which chains of
    2,048 steps do not reach."""
    from test_driver_decisions_emulated import EXPECTED, FIELDS, MODES
    fp = synth.config_flat(3, P=4096, N=256)
    want = _oracle(fp)
    head, syncs, launches, steps, kinds = EXPECTED["c3"]
    row = head + (syncs["1"], launches[MODES.index(("1", "1"))]) + steps + kinds
    for handoff in (0, None):
        monkeypatch.delenv("BLANCE_CHAIN_WAVES", raising=False)
        monkeypatch.setenv("BLANCE_FUSED_TAIL", "1")
        got, _ = _plan_default_waves(emu_lib, fp, monkeypatch, capfd, handoff, trace=False)
        _same(got, want, handoff)
        assert tuple(int(getattr(got.struct, f)) for f in FIELDS) == row, handoff
    got, trace = _plan_default_waves(emu_lib, fp, monkeypatch, capfd, 0, trace=True)
    _same(got, want, "trace")
    assert "hand-off" not in trace, [l for l in trace.splitlines() if "hand-off" in l]
    # (and forced on, the same shape does hand off: the switch is what makes the difference)
    got, trace = _plan_default_waves(emu_lib, fp, monkeypatch, capfd, 64, trace=True)
    _same(got, want, "on")
    assert _stops(trace) and all(at is not None for at, _ in _stops(trace)[0].values()), trace[-3000:]


def _plan_default_waves(lib, fp, monkeypatch, capfd, handoff, trace):
    monkeypatch.setenv("BLANCE_SPECULATE", "1")
    if handoff is None:
        monkeypatch.delenv("BLANCE_CHAIN_HANDOFF", raising=False)
    else:
        monkeypatch.setenv("BLANCE_CHAIN_HANDOFF", str(handoff))
    if trace:
        monkeypatch.setenv("BLANCE_TRACE", "1")
    else:
        monkeypatch.delenv("BLANCE_TRACE", raising=False)
    capfd.readouterr()
    pl = hip.Planner(lib_path=lib, chain_min_parts=64)
    try:
        got = pl.plan(fp)
    finally:
        pl.close()
    return got, capfd.readouterr().err


@pytest.mark.parametrize("spec", ["0", "fail"])
def test_other_speculation_modes(emu_lib, monkeypatch, capfd, spec):
    """BLANCE_SPECULATE=0 (every decision read back first: no hand-off) and fail (every deferred verdict comes back bad: the
    pass behind the hand-off runs again without it)."""
    fp = _config3(6144, 256, 2)
    want = _oracle(fp)
    got, trace = _plan(emu_lib, fp, monkeypatch, capfd, 64, 8, spec=spec)
    _same(got, want, spec)
    if spec == "0":
        assert not _stops(trace)
        return
    # fail: sweep 2's pass hands off, its deferred verdict comes back refuted, the pass runs again without a hand-off
    # (a first attempt of the sweep waits behind the settled top-state pass's word, which `fail` raises: its launches return
    # at their gate, and the trace says so)
    assert [d for d in _stops(trace) if d] == [{0: (1024, 3072), 1: (1024, 3072)}], trace[-3000:]
    at = trace.index("hand-off (64 steps or more) in 2 of 2 regions")
    refuted = trace.index("deferred verdict (chain kernel): assumption refuted", at)
    assert NO_HANDOFF in trace[refuted:], trace[refuted:][:3000]
