"""Whole plans in which k_stay_by_top is tried in every chain pass with NumPartitions > 0 (hip.Planner(stay_top="force")),
and one in which it runs behind the chain kernel's hand-off (BLANCE_CHAIN_HANDOFF set low: walked steps are replayed lanes
of its rounds): the problems, shared by tests/test_stay_plans_emulated.py (SIMT emulator) and tests/test_stay_plans_gpu.py (device).

Config 3's shape (primary + k replicas, k = 1, 2 and 3 -- k_stay_by_top<2> and <4> --, the replicas outside the primary's
rack and inside its zone), with and without node weights, with zones of 16, 32
and 128 leaves and one of 320; the partition counts make some top priority node (a primary) the top of exactly 1, 63, 64, 65
or 129 steps -- rounds of one lane, a round that is one lane short, a full round, a round behind a full one (its ranks come
through the LDS row) and a step behind two full rounds.  Each problem is planned from nothing and then planned again from
its own result (every step stays: the pass k_stay_by_top takes on its own).

A wrong rank does not show in the plan: the kernel raises its flag and the driver redoes the pass with the chain kernel.
So each case also pins the tallies of the result (stay_pass_launches, pass_kernel_launches, host_syncs) to what commit
f11090a gives for it under the SIMT emulator -- the build before the ranks came from ballots, where the forced pass stood
in every case listed here (no chain-kernel pass behind a stay pass)."""
import numpy as np

from blance_amd import hip, synth

# name: (rack, racks per zone, nodes, partitions, replicas, weights, BLANCE_CHAIN_HANDOFF or None, a step count some top
# priority node must have)
CASES = {
    "zone16-k2-65": (4, 4, 64, 4128, 2, False, None, 65),
    "zone16-k1-64": (4, 4, 64, 4128, 1, False, None, 64),
    "zone16-k2-129": (4, 4, 32, 4112, 2, False, None, 129),
    "zone16-k1-129w": (4, 4, 32, 4112, 1, True, None, 129),
    "zone32-k2-63": (8, 4, 128, 8128, 2, False, None, 63),
    "zone32-k1-64w": (8, 4, 128, 8128, 1, True, None, 64),
    "zone32-k2-63w": (8, 4, 128, 8128, 2, True, None, 63),
    "zone128-k2-1": (16, 8, 256, 356, 2, False, None, 1),
    "zone128-k1-1": (16, 8, 256, 356, 1, False, None, 1),
    "zone128-k2-65w": (16, 8, 256, 8300, 2, True, None, 65),
    # (three replicas: the <4> instance, whose fourth slot is -1 in every lane -- a -1 taken for a leaf shows here, in the
    # order a step emits its nodes in)
    "zone32-k3-63w": (8, 4, 128, 8128, 3, True, None, 63),
    "zone128-k3-17": (16, 8, 256, 4196, 3, False, None, 17),
    "zone320-k2": (16, 20, 640, 2600, 2, False, None, 4),
    "zone320-k1w": (16, 20, 640, 2600, 1, True, None, 9),
    "zone128-k2-handoff": (16, 8, 256, 6144, 2, False, 64, 24),
}
FIELDS = ("stay_pass_launches", "pass_kernel_launches", "host_syncs")


def problem(name):
    rack, rpz, N, P, k, weighted, _, _ = CASES[name]
    c = synth.config_case(3, P=P, N=N)
    c["model"] = {"primary": {"priority": 0, "constraints": 1}, "replica": {"priority": 1, "constraints": k}}
    c["nodeHierarchy"] = synth.hierarchy_names(N, rack=rack, racks_per_zone=rpz, zones_per_dc=2)
    if weighted:
        c["nodeWeights"] = {("n%04d" % i): [1, 1, 2, 4][(i * 5) % 4] for i in range(N)}
    return synth.case_to_flat(c)


def steps_per_top(fp, res):
    """How many steps each primary is the top priority node of, in a plan over the result `res` of `fp`."""
    P, M = int(fp.n_parts), int(fp.n_states)
    off = np.asarray(res.out_off[:P * M + 1])
    nodes = np.asarray(res.out_nodes[:off[-1]])
    prim = nodes[off[np.arange(P) * M]]
    return np.bincount(prim)


def run(lib_path, name, oracle, monkeypatch, device=False):
    """Plans the case from nothing and again from its result.  Returns [(digest, iterations) equal to the oracle's?, the
    tallies] for the two plans."""
    handoff = CASES[name][6]
    if handoff is None:
        monkeypatch.delenv("BLANCE_CHAIN_HANDOFF", raising=False)
    else:
        monkeypatch.setenv("BLANCE_CHAIN_HANDOFF", str(handoff))
    fp = problem(name)
    want = oracle(fp)
    assert CASES[name][7] in steps_per_top(fp, want).tolist(), (name, sorted(set(steps_per_top(fp, want).tolist())))
    fp2 = synth.replan_problem(fp, want)
    want2 = oracle(fp2)
    kw = dict(device_id=0) if device else dict(lib_path=lib_path)
    # (a forced pass never waits behind a hand-off: the hand-off case runs as tests/test_chain_handoff_emulated.py's plans do,
    # and the chain kernel hands sweep 2's pass to k_stay_by_top after each region's second stage)
    kw.update(dict(chain_min_parts=8, stay_top="force") if handoff is None else dict(chain_min_parts=64))
    pl = hip.Planner(**kw)
    out = []
    try:
        for f, w in ((fp, want), (fp2, want2)):
            got = pl.plan(f)
            same = (got.digest(), got.iterations, got.n_warnings) == (w.digest(), w.iterations, w.n_warnings)
            out.append((same, tuple(int(getattr(got.struct, x)) for x in FIELDS)))
    finally:
        pl.close()
    return out
