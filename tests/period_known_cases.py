"""The periodic first pass that takes its period from the round robin of the pass before (k_period_find's known mode,
DESIGN.md 4.1c): the whole-plan cases and their check, shared by tests/test_period_known_emulated.py (SIMT emulator) and
tests/test_period_known_gpu.py (device).

A case is a plan from nothing on a rack / zone tree.  It is planned under BLANCE_SPECULATE = 1, 0 and fail, each with
BLANCE_PERIOD_KNOWN on and off, and every plan must be the C oracle's (digest, iterations, warnings).  The two modes must say
the same about the regions ("periodic records in ..."), make the same number of round trips and count the same launches; and
the driver must name the shortcut exactly where its conditions hold: `known` below says whether they do when the opening
pass was committed as a round robin (BLANCE_SPECULATE=0 commits nothing unread: no known cycle there in any case).

Mutations of the sources tried against these cases and tests/period_case_tables.py (emulator), and what caught them:
  T = count + 1 in the known mode            12 tables of test_period_cases (every one with a candidate period) and 20 plans here
  limit = len - T in the known mode          the same 12 tables and 13 plans (the "periodic records in" line differs)
  the `present` bit's test dropped           replica_lists_mixed, replica_lists_one_present (the shortcut's line where it must not be)
  the pass order's test dropped              nodes_outside_nodes_to_add, sorted_by_two_categories"""
from blance_amd import hip, synth

SPECS = ("1", "0", "fail")
KNOWN = "the period taken from the round robin of the pass before, no search and no k_period_verify"
PERIODIC = "the regions set up by k_period_find and judged by k_period_judge"


def tree_case(P, N, rack, rpz, k=2, gone=None, present=None, part_weights=False, not_added=None, add_nil=False, third=None):
    """Config 3's shape on another tree (tests/test_fewer_launches_emulated.py: _tree_case): zones of rack * rpz leaves are
    the replica rule's regions.
    gone = (first, step): nodes missing from the cluster, leaves without a node.
    present = f(i): partition i comes with an empty replica list instead of none (the record's `present` bit).
    not_added = f(i): node i is outside nodesToAdd; add_nil: nodesToAdd is nil.
    third = (name, priority, constraints, the replica's priority): a third state under the replica's rule (the reference
    wants the states' priorities and names in one order)."""
    c = synth.config_case(3, P=P, N=N)
    c["nodeHierarchy"] = synth.hierarchy_names(N, rack=rack, racks_per_zone=rpz, zones_per_dc=8)
    c["model"] = {"primary": {"priority": 0, "constraints": 1}, "replica": {"priority": 1, "constraints": k}}
    if third:
        c["model"][third[0]] = {"priority": third[1], "constraints": third[2]}
        c["model"]["replica"]["priority"] = third[3]
        c["hierarchyRules"][third[0]] = list(c["hierarchyRules"]["replica"])
    if gone:
        g = set(c["nodesAll"][gone[0]::gone[1]])
        c["nodesAll"] = [n for n in c["nodesAll"] if n not in g]
        c["nodesToAdd"] = list(c["nodesAll"])
    if not_added:
        c["nodesToAdd"] = [n for i, n in enumerate(c["nodesAll"]) if not not_added(i)]
    if add_nil:
        c["nodesToAdd"] = None
    if present:
        for i, (name, part) in enumerate(c["partitionsToAssign"].items()):
            if present(i):
                part["nodesByState"] = {"replica": []}
    if part_weights:
        c["partitionWeights"] = {p: 1 + int(p) % 3 for p in c["partitionsToAssign"]}
    return synth.case_to_flat(c)


# name -> (the problem, the known cycle's conditions hold, environment of the case)
CASES = {
    # ---- the trees of test_fewer_launches_emulated.PERIODIC_CASES
    "zones_of_128": (lambda: tree_case(4096, 256, 16, 8), True, {}),
    "partial_last_period": (lambda: tree_case(2000, 64, 4, 4), True, {}),
    "stretch_too_short": (lambda: tree_case(600, 256, 16, 8), True, {}),
    "zones_of_192": (lambda: tree_case(3000, 384, 16, 12), True, {}),
    "ragged_last_zone": (lambda: tree_case(3000, 250, 16, 8), True, {}),
    "escapes_k3": (lambda: tree_case(3000, 200, 12, 8, k=3), True, {}),
    "refused_region": (lambda: tree_case(3000, 256, 16, 8, gone=(5, 17)), True, {}),
    "refused_region_short_rack": (lambda: tree_case(1830, 61, 8, 4), True, {}),
    "refused_everywhere": (lambda: tree_case(1931, 64, 8, 4, gone=(1, 5)), True, {}),
    # ---- fewer partitions than nodes: a region with fewer steps than nodes (no period), a region with one step more than
    # nodes (the period is a candidate, the stretch too short), an empty region
    "fewer_parts_than_nodes": (lambda: tree_case(100, 256, 16, 8), True, {}),
    "one_step_past_a_period": (lambda: tree_case(129 + 60, 256, 16, 8), True, {}),
    # ---- the record's `present` bit: every replica list absent (above), every one present, mixed
    "replica_lists_all_present": (lambda: tree_case(4096, 256, 16, 8, present=lambda i: True), True, {}),
    "replica_lists_mixed": (lambda: tree_case(4096, 256, 16, 8, present=lambda i: i % 3 == 0), False, {}),
    # (one present list among 4,095 absent ones, in the last partition of the pass)
    "replica_lists_one_present": (lambda: tree_case(4096, 256, 16, 8, present=lambda i: i == 4095), False, {}),
    # ---- partition weights: the opening pass is no round robin
    "partition_weights": (lambda: tree_case(4096, 256, 16, 8, part_weights=True), False, {}),
    # ---- a third state with constraints: its pass is the sweep's third, never a known cycle; the replica's still is
    "third_state_behind": (lambda: tree_case(4096, 256, 16, 8, third=("spare", 2, 1, 1)), True, {}),
    # (... and one whose pass comes second: of higher priority than the replica.  Its pass is the known cycle, the replica's
    # is the third)
    "third_state_between": (lambda: tree_case(4096, 256, 16, 8, third=("quorum", 1, 1, 2)), None, {}),
    # ---- the pass order.  Some nodes outside nodesToAdd: the second pass sorts the partitions by whether their primary is
    # in nodesToAdd, so its order is not the opening pass's and its chains do not repeat a region's nodes in turn
    "nodes_outside_nodes_to_add": (lambda: tree_case(4096, 256, 16, 8, not_added=lambda i: i % 5 == 0), False, {}),
    "no_node_in_nodes_to_add": (lambda: tree_case(4096, 256, 16, 8, not_added=lambda i: True), True, {}),
    "nodes_to_add_nil": (lambda: tree_case(4096, 256, 16, 8, add_nil=True), True, {}),
    # (the partition kernels run although every partition has one category: the order they leave is the static order)
    "sorted_by_one_category": (lambda: tree_case(4096, 256, 16, 8), True, {"BLANCE_NO_UNIFORM_CATEGORY": "1"}),
    "sorted_by_two_categories": (lambda: tree_case(4096, 256, 16, 8, not_added=lambda i: i % 5 == 0), False, {"BLANCE_NO_UNIFORM_CATEGORY": "1"}),
    "sorted_ragged": (lambda: tree_case(3000, 250, 16, 8), True, {"BLANCE_NO_UNIFORM_CATEGORY": "1"}),
    # ---- the stretch cut below, at and above a period boundary, and below kPeriodMinRounds periods
    "cut_300": (lambda: tree_case(4096, 256, 16, 8), True, {"BLANCE_PERIODIC_CUT": "300"}),
    "cut_1000": (lambda: tree_case(4096, 256, 16, 8), True, {"BLANCE_PERIODIC_CUT": "1000"}),
    "cut_1024": (lambda: tree_case(4096, 256, 16, 8), True, {"BLANCE_PERIODIC_CUT": "1024"}),
    "cut_1030": (lambda: tree_case(4096, 256, 16, 8), True, {"BLANCE_PERIODIC_CUT": "1030"}),
}


def oracle(fp):
    from oracle import loader
    return loader.plan(fp)


def plan(lib, fp, spec, known, monkeypatch, capfd, **kw):
    """One plan on a fresh planner with the trace on: (the result, the trace).  lib: the emulator's library, None: the device."""
    monkeypatch.setenv("BLANCE_SPECULATE", spec)
    monkeypatch.setenv("BLANCE_TRACE", "1")
    monkeypatch.setenv("BLANCE_PERIOD_KNOWN", "1" if known else "0")
    kw.setdefault("chain_min_parts", 8)
    if lib is not None:
        kw["lib_path"] = lib
    else:
        kw.setdefault("device_id", 0)
    capfd.readouterr()
    pl = hip.Planner(periodic=True, **kw)
    try:
        got = pl.plan(fp)
    finally:
        pl.close()
    return got, capfd.readouterr().err


def check(lib, name, monkeypatch, capfd):
    make, holds, env = CASES[name]
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    fp = make()
    want = oracle(fp)
    want_key = (want.digest(), want.iterations, want.n_warnings)
    for spec in SPECS:
        seen = {}
        for known in (True, False):
            got, err = plan(lib, fp, spec, known, monkeypatch, capfd)
            assert (got.digest(), got.iterations, got.n_warnings) == want_key, (name, spec, known)
            lines = [ln for ln in err.splitlines() if "periodic records in" in ln]
            s = got.struct
            seen[known] = (lines, s.host_syncs, s.kernel_launches, s.blank_pass_launches, err.count(PERIODIC))
            n = err.count(KNOWN)
            if not known or spec == "0" or holds is False:
                assert n == 0, (name, spec, known, n)
            elif holds:
                assert n >= 1 and lines, (name, spec, known, err[-3000:])
            # (holds is None: a case that must be exact, whichever pass takes the shortcut)
        assert seen[True] == seen[False], (name, spec, seen)
