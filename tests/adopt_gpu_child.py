"""blance_plan_adopt on the MI355X, in a process of its own: every family of tests/adopt_cases.py through libblance_hip.so, and
the two kernels alone through libblance_adopt_cases.so.  tests/test_adopt_gpu.py starts this program once and reads its
answers, so nothing of these tests -- contexts, streams, the second code-object library, communicator callbacks -- is ever
in the process that runs the rest of the suite.

    python tests/adopt_gpu_child.py OUT.json

OUT.json: {family: "ok" or the traceback}.  A device error ends the run: nothing more is started on the GPU behind it."""
import json
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import adopt_cases as A  # noqa: E402
from blance_amd import abi, hip, synth  # noqa: E402


def golden_cases():
    with open(os.path.join(HERE, "golden", "planner_cases.json")) as f:
        return [c for c in json.load(f)["cases"] if not c.get("ignored")]


def golden(pl, pl2, keep):
    A.honest(A.run_golden(pl, pl2, golden_cases(), keep), ("golden", keep))


def mixed(pl, pl2):
    rounds = A.run_mixed(pl, pl2, 0)
    assert len(rounds) >= 40
    A.honest(rounds, "mixed")


def config5(pl, pl2, hierarchy):
    P, N = 4096, 128
    fp = synth.config5_initial(P, N, hierarchy=hierarchy)
    A.honest(A.run_chain(pl, pl2, fp, A.config5_changes(fp, P, N, hierarchy), ("config 5", hierarchy)), ("config 5", hierarchy))


def config5_three_rounds(pl, pl2):
    fp, changes = A.config5_all_nodes(1024, 64, True)
    A.honest(A.run_chain(pl, pl2, fp, changes, "config 5, all nodes", around=True), "config 5, all nodes")


def config3_three_rounds(pl, pl2):
    fp, changes = A.config3_chain()
    A.honest(A.run_chain(pl, pl2, fp, changes, "config 3"), "config 3")


def rack(pl, pl2):
    fp, changes = A.rack_chain()
    rounds = A.run_chain(pl, pl2, fp, changes, "rack", around=True)
    A.honest(rounds, "rack")
    assert rounds[0].moves["n_moves"] > 0 and rounds[1].moves["n_moves"] > 0


def seam(pl, pl2, P, M):
    fp = A.seam_problem(P, M)
    rounds = A.run_chain(pl, pl2, fp, [A.Change(removed=A.flags(fp, [1])), A.Change(added=A.flags(fp, [1]))], ("seam", P, M),
                         around=True)
    assert len(rounds) == 2 and rounds[0].moves["n_by_kind"]["del"] > 0


def scan_split(pl, pl2):
    """P * M + 1 = 65,537 list lengths: launch_scan_excl goes from one launch to three."""
    from test_plan_moves_emulated import scan_split_problem
    fp = scan_split_problem()
    rounds = A.run_chain(pl, pl2, fp, [A.Change(removed=A.flags(fp, [3]))], "scan split")
    assert rounds[0].moves["n_by_kind"]["add"] > 0


def warnings(pl, pl2):
    fp = A.warnings_case()
    rounds = A.run_chain(pl, pl2, fp, [A.Change(), A.Change(removed=A.flags(fp, [2]))], "warnings", around=True)
    assert all(r.res.n_warnings > 0 for r in rounds)


def refusals(pl, pl2):
    A.run_refusals(lambda: hip.Planner(device_id=0))


def kernels_alone(pl, pl2):
    import __graft_entry__ as entry
    assert A.run_kernel_cases(A.AdoptKernels(entry.build_adopt_cases())) >= 30


FAMILIES = [("golden-keep0", lambda a, b: golden(a, b, False)), ("golden-keep1", lambda a, b: golden(a, b, True)),
            ("loads", lambda a, b: A.honest(A.run_loads(a, b), "loads")), ("mixed", mixed),
            ("config5-flat", lambda a, b: config5(a, b, False)), ("config5-hierarchy", lambda a, b: config5(a, b, True)),
            ("config5-three-rounds", config5_three_rounds), ("config3-three-rounds", config3_three_rounds), ("rack", rack)] + \
           [("seam-P%d-M%d" % (P, M), (lambda P, M: lambda a, b: seam(a, b, P, M))(P, M)) for M in (2, 3) for P in (1, 255, 256, 257)] + \
           [("scan-split", scan_split), ("warnings", warnings), ("refusals", refusals), ("kernels-alone", kernels_alone)]
NAMES = [name for name, _ in FAMILIES]


def main(out_path):
    results = {}

    def save():
        with open(out_path + ".tmp", "w") as f:
            json.dump(results, f)
        os.replace(out_path + ".tmp", out_path)

    pl, pl2 = hip.Planner(device_id=0), hip.Planner(device_id=0)
    for name, fn in FAMILIES:
        try:
            fn(pl, pl2)
            results[name] = "ok"
        except BaseException as e:
            results[name] = traceback.format_exc()
            save()
            if isinstance(e, hip.BlanceError) and e.status == abi.ERR_DEVICE:
                return 1                                   # a device error: the run ends here
            if not isinstance(e, Exception):
                raise
        save()
    pl.close()
    pl2.close()
    return 0 if all(v == "ok" for v in results.values()) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
