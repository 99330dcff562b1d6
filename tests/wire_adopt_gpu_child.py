"""blance_wire_adopt on the MI355X, in a process of its own: every family of tests/wire_adopt_cases.py through
libblance_hip.so, and the two kernels alone through libblance_wire_adopt_cases.so.  tests/test_wire_adopt_gpu.py starts this
program once and reads its answers, so nothing of these tests -- contexts, streams, the second code-object library,
communicator callbacks -- is ever in the process that runs the rest of the suite (DESIGN.md 4.14 has the reason).

    python tests/wire_adopt_gpu_child.py OUT.json

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

import wire_adopt_cases as W  # noqa: E402
from blance_amd import abi, hip  # noqa: E402


def golden_cases():
    with open(os.path.join(HERE, "golden", "planner_cases.json")) as f:
        return [c for c in json.load(f)["cases"] if not c.get("ignored")]


def golden(pls, keep):
    n, sweeps2 = W.run_equal_golden(pls, golden_cases(), keep)
    assert sweeps2 * 3 >= n, (n, sweeps2)


def random_problems(pls):
    assert W.run_equal_random(pls, 0) >= 40


def mutants(pls):
    assert W.run_mutants(pls[0], pls[1]) == 22


def refusals(pls):
    W.run_refusals(lambda: hip.Planner(device_id=0))


def kernels_alone(pls):
    import __graft_entry__ as entry
    assert W.run_kernel_cases(W.WireAdoptKernels(entry.build_wire_adopt_cases())) >= 80


def switch(pls):
    assert W.run_switch(pls[0], pls[1]) == 11


FAMILIES = [("golden-keep0", lambda pls: golden(pls, False)), ("golden-keep1", lambda pls: golden(pls, True)),
            ("random", random_problems), ("mutants", mutants)] + \
           [("seam-P%d-M%d" % (P, M), (lambda P, M: lambda pls: W.run_seam(pls, P, M))(P, M)) for M in (2, 3) for P in (1, 255, 256, 257)] + \
           [("scan-split", W.run_scan_split), ("row-stride", lambda pls: W.run_row_stride(pls[0], pls[1])), ("refusals", refusals),
            ("kernels-alone", kernels_alone), ("switch", switch)]
NAMES = [name for name, _ in FAMILIES]


def main(out_path):
    results = {}

    def save():
        with open(out_path + ".tmp", "w") as f:
            json.dump(results, f)
        os.replace(out_path + ".tmp", out_path)

    pls = [hip.Planner(device_id=0) for _ in range(3)]
    for name, fn in FAMILIES:
        try:
            fn(pls)
            results[name] = "ok"
        except BaseException as e:
            results[name] = traceback.format_exc()
            save()
            if isinstance(e, hip.BlanceError) and e.status == abi.ERR_DEVICE:
                return 1                                   # a device error: the run ends here
            if not isinstance(e, Exception):
                raise
        save()
    for pl in pls:
        pl.close()
    return 0 if all(v == "ok" for v in results.values()) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
