"""The chain pass behind a round robin grouped from tables of the upload, not by two counting sorts (k_cycle.h, DESIGN.md
4.1c "The grouping without the sorts"): the whole-plan cases and their checks, shared by tests/test_cycle_group_emulated.py (SIMT
emulator) and tests/test_cycle_group_gpu.py (device).

A case is a plan from nothing on a rack / zone tree: every case of tests/period_known_cases.py, and the ones below.  It is
planned under BLANCE_SPECULATE = 1, 0 and fail, each with BLANCE_CYCLE_GROUP on and off, and every plan must be the C oracle's
(digest, iterations, warnings).  On and off must make the same number of round trips and count the same launches, and reuse
the grouping by region and k_stay_by_top's work list in the same later sweeps; the driver must name the shortcut exactly
where its conditions hold (`holds`, as in period_known_cases: BLANCE_SPECULATE=0 commits no round robin unread, so there is
no shortcut there in any case).  Under BLANCE_CYCLE_GROUP=refute the kernel's check of the premise fails for step 0: the pass
goes in order, the grouping is dropped and not reused, and the plan is still the oracle's (no tally is compared there: the
pass takes another path on purpose).

Mutations of the sources tried against these cases (emulator, every test of tests/test_cycle_group_emulated.py), and what
caught them:
  q off by one (a node's rank in its region + 1)              29 tests: every plan that takes the shortcut (digest), but
                                                              the ones with BLANCE_SPECULATE=0 only
  len_r without the partial cycle (reg_off from P / A alone)  11 tests: stretch_too_short, one_step_past_a_period, refused_region,
                                                              refused_everywhere, fewer_parts_than_nodes, partial_last_period,
                                                              zones_of_192, zones_of_320, ... (P % A != 0; digest)
  top_off without the partial cycle                           refused_region, ragged_last_zone (a later sweep's k_stay_by_top reads
                                                              the list; the other cases with P % A != 0 do not come to use it)
  the premise check dropped, with the knob on                 test_refuted_premise, all three (no "dropped" line)
  the cache not dropped after a refutation                    test_refuted_premise, all three (the next sweep reuses the grouping)
The lean gather of the issue (its bound at T instead of 2T) is not built, so there is nothing to mutate.
"""
from blance_amd import hip, synth

import period_known_cases as K

SPECS = K.SPECS
GROUP = "the steps grouped by region from the round robin's tables, no sort"
TOP = "the steps grouped by top priority node from the round robin's tables, no sort"
DROPPED = "the round robin's tables do not describe this pass, the grouping is dropped"
REGION_STANDS = "the grouping by region of the last sweep stands"
TOP_STANDS = "the steps' grouping by top priority node stands"


def shared_leaf():
    """Two nodes on one leaf of the hierarchy (node 1 moved onto node 0's, in the flat problem: problem.build_problem gives
    every childless vertex a leaf of its own, as the reference does)."""
    fp = K.tree_case(4096, 256, 16, 8)
    leaf, lo, hi = fp.node_leaf_pos.copy(), fp.vertex_leaf_lo.copy(), fp.vertex_leaf_hi.copy()
    leaf[1], lo[1], hi[1] = leaf[0], lo[0], hi[0]
    fp.set("node_leaf_pos", leaf)
    fp.set("vertex_leaf_lo", lo)
    fp.set("vertex_leaf_hi", hi)
    return fp


def node_outside_regions():
    """A node of nodesNext that the hierarchy does not name: it lies in no region of the replica's rule."""
    c = synth.config_case(3, P=3000, N=256)
    c["nodeHierarchy"] = synth.hierarchy_names(256, rack=16, racks_per_zone=8, zones_per_dc=8)
    del c["nodeHierarchy"][c["nodesAll"][77]]
    c["model"] = {"primary": {"priority": 0, "constraints": 1}, "replica": {"priority": 1, "constraints": 2}}
    return synth.case_to_flat(c)


# name -> (the problem, the shortcut's conditions hold, environment of the case)
CASES = dict(K.CASES)
CASES.update({
    "node_outside_regions": (node_outside_regions, False, {}),
    "zones_of_320": (lambda: K.tree_case(3000, 640, 16, 20), True, {}),
    # (four zones of one rack of one node: every region's count is 1)
    "one_node_per_region": (lambda: K.tree_case(300, 4, 1, 1), True, {}),
    # (zones of 16 leaves, the third with one node)
    "region_with_one_node": (lambda: K.tree_case(2000, 33, 4, 4), True, {}),
})
REFUTE = ("zones_of_128", "partial_last_period", "ragged_last_zone")


def plan(lib, fp, spec, group, monkeypatch, capfd, planner=None, **kw):
    """One plan with the trace on: (the result, the trace).  group: "1", "0" or "refute"."""
    monkeypatch.setenv("BLANCE_CYCLE_GROUP", group)
    monkeypatch.delenv("BLANCE_PERIOD_KNOWN", raising=False)
    if planner is not None:
        monkeypatch.setenv("BLANCE_SPECULATE", spec)
        monkeypatch.setenv("BLANCE_TRACE", "1")
        capfd.readouterr()
        got = planner.plan(fp)
        return got, capfd.readouterr().err
    got, err = K.plan(lib, fp, spec, True, monkeypatch, capfd, **kw)
    return got, err


def tallies(got):
    s = got.struct
    return (s.host_syncs, s.kernel_launches, s.pass_kernel_launches, s.blank_pass_launches, s.stay_pass_launches)


def check(lib, name, monkeypatch, capfd):
    make, holds, env = CASES[name]
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    fp = make()
    want = K.oracle(fp)
    want_key = (want.digest(), want.iterations, want.n_warnings)
    for spec in SPECS:
        seen = {}
        for group in ("1", "0"):
            got, err = plan(lib, fp, spec, group, monkeypatch, capfd)
            assert (got.digest(), got.iterations, got.n_warnings) == want_key, (name, spec, group)
            seen[group] = (tallies(got), err.count(REGION_STANDS), err.count(TOP_STANDS))
            n = err.count(GROUP)
            assert err.count(DROPPED) == 0, (name, spec, group)
            if group == "0" or spec == "0" or holds is False:
                assert n == 0 and err.count(TOP) == 0, (name, spec, group, n)
            elif holds:
                assert n == 1, (name, spec, group, err[-3000:])
            # (holds is None: a case that must be exact, whichever pass takes the shortcut)
        assert seen["1"] == seen["0"], (name, spec, seen)


def check_shared_leaf(lib, monkeypatch, capfd):
    """Two nodes share a leaf: no tables, no shortcut, and the switch changes nothing -- the same plan, tallies and trace lines
    on and off.  The plan is NOT compared with the oracle: such a problem lies outside what the reference can express, and the
    region chains of the parent commit already plan it differently from the oracle (digest differs with the switch off as
    with it on, 3 iterations in both; the in-order pass alone agrees)."""
    fp = shared_leaf()
    seen = {}
    for group in ("1", "0"):
        got, err = plan(lib, fp, "1", group, monkeypatch, capfd)
        assert err.count(GROUP) == 0 and err.count(TOP) == 0 and err.count(DROPPED) == 0 and err.count(K.KNOWN) == 0, group
        seen[group] = (got.digest(), got.iterations, got.n_warnings, tallies(got), err.count(REGION_STANDS), err.count(TOP_STANDS))
    assert seen["1"] == seen["0"], seen


def check_refuted(lib, name, monkeypatch, capfd):
    """BLANCE_CYCLE_GROUP=refute: the check of the premise fires for step 0.  The pass goes in order, nothing made from the
    tables is reused -- the next sweep's chain pass groups its steps again, one "stands" line less than without the knob --
    and the plan is the oracle's."""
    make, holds, env = CASES[name]
    assert holds
    fp = make()
    want = K.oracle(fp)
    got_on, err_on = plan(lib, fp, "1", "1", monkeypatch, capfd)
    got, err = plan(lib, fp, "1", "refute", monkeypatch, capfd)
    assert (got.digest(), got.iterations, got.n_warnings) == (want.digest(), want.iterations, want.n_warnings), name
    assert err.count(GROUP) == 1 and err.count(DROPPED) == 1 and err.count(TOP) == 0, (name, err[-3000:])
    assert err_on.count(DROPPED) == 0 and err_on.count(REGION_STANDS) >= 1, (name, err_on[-3000:])
    assert err.count(REGION_STANDS) == err_on.count(REGION_STANDS) - 1, (name, err[-3000:])
    # (the sweep behind the refuted pass: its chain pass reads its classification back, the grouping does not stand)
    behind = err[err.index(DROPPED):]
    first_chain = [ln for ln in behind.splitlines() if "chain pass state" in ln and ("events, not-local 0" in ln or REGION_STANDS in ln)]
    assert first_chain and REGION_STANDS not in first_chain[0], (name, first_chain[:2])


def check_second_plan_and_upload(lib, monkeypatch, capfd):
    """One context: a plan, the same plan again, then a problem of another shape, then the first again.  Every upload
    builds its own tables; every plan takes the shortcut and is the oracle's."""
    kw = {"lib_path": lib} if lib is not None else {"device_id": 0}
    monkeypatch.setenv("BLANCE_TRACE", "1")
    pl = hip.Planner(periodic=True, chain_min_parts=8, **kw)
    try:
        a, b = K.tree_case(2000, 64, 4, 4), K.tree_case(3000, 250, 16, 8)
        for fp in (a, a, b, a):
            want = K.oracle(fp)
            got, err = plan(lib, fp, "1", "1", monkeypatch, capfd, planner=pl)
            assert (got.digest(), got.iterations, got.n_warnings) == (want.digest(), want.iterations, want.n_warnings)
            assert err.count(GROUP) == 1 and err.count(DROPPED) == 0, err[-3000:]
    finally:
        pl.close()


def check_switches(lib, monkeypatch, capfd):
    """hip.Planner(cycle_group=False) is BLANCE_CYCLE_GROUP=0; the variable, when set, decides."""
    fp = K.tree_case(2000, 64, 4, 4)
    want = K.oracle(fp)
    kw0 = {"lib_path": lib} if lib is not None else {"device_id": 0}
    monkeypatch.setenv("BLANCE_TRACE", "1")
    monkeypatch.delenv("BLANCE_SPECULATE", raising=False)
    for kw, env, n in (({}, None, 1), ({"cycle_group": False}, None, 0), ({"cycle_group": False}, "1", 1), ({}, "0", 0)):
        if env is None:
            monkeypatch.delenv("BLANCE_CYCLE_GROUP", raising=False)
        else:
            monkeypatch.setenv("BLANCE_CYCLE_GROUP", env)
        capfd.readouterr()
        pl = hip.Planner(chain_min_parts=8, **kw0, **kw)
        try:
            got = pl.plan(fp)
        finally:
            pl.close()
        err = capfd.readouterr().err
        assert got.digest() == want.digest() and err.count(GROUP) == n, (kw, env, err.count(GROUP))
