"""The hand-over from one planning round to the next, two ways, alternating in one process after a warm-up:

    (a) the route blance_plan_adopt replaces: blance_download into page-locked arrays, assign_* / prev_* of the next problem
        pointed at them (as synth.replan_problem does, without its copies), blance_upload, blance_plan_wire_names -- the four
        parts timed separately
    (b) blance_plan_adopt (Planner.adopt): the lists stay on the device, the names stay valid

    python tools/adopt_gpu.py [P] [N] [--reps 6]          (default 1048576 4096)

The workload is config 3's plan (synth.config_flat(3, P, N)) and config3_rebalance_flat's change: every tenth node leaves.
Before every repetition of either way the context is put back to "holds config 3's plan" (upload + plan_resident, not
timed).  The plan that follows is timed for both ways and the two digests must be equal.  Times are the host's clock around
calls that end in a device synchronise.  --only adopt runs (b) alone, --reps times: for a kernel trace of its own
(rocprofv3 --kernel-trace --stats -- python tools/adopt_gpu.py P N --only adopt)."""
import argparse
import copy
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from blance_amd import abi, hip, synth  # noqa: E402


def stats(v, unit=1e3):
    return "median %9.3f ms   range %9.3f .. %9.3f ms" % (statistics.median(v) * unit, min(v) * unit, max(v) * unit)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("P", nargs="?", type=int, default=1048576)
    ap.add_argument("N", nargs="?", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--only", choices=["adopt"], help="run this way alone (no comparison)")
    a = ap.parse_args()
    P, N = a.P, a.N
    pl = hip.Planner(device_id=0)
    arena = hip.HostArena()
    fp = synth.config_flat(3, P=P, N=N).pin(arena)
    part_names = [str(p) for p in range(P)]
    node_names = ["n%04d" % i for i in range(fp.n_nodes_ext)]
    state_names = ["primary", "replica", "spare", "dead"][:fp.n_states]
    gone = np.zeros(fp.n_nodes_ext, dtype=np.uint8)
    gone[np.arange(N) % 10 == 3] = 1
    PM = P * fp.n_states

    def restore():
        pl.upload(fp)
        return pl.plan_resident()

    r0 = restore()
    print("P %d  N %d  config 3's plan: %d sweeps, device %.3f ms" % (P, N, r0.iterations, r0.device_ms), flush=True)
    res = abi.FlatResult(fp, arena)
    fp2 = copy.copy(fp)                                        # the next problem: fp's arrays but for the lists and the node change
    fp2.scalars = dict(fp.scalars)
    fp2.arrays = dict(fp.arrays)
    fp2._struct, fp2._keep = None, []
    fp2.set("part_in_prev", arena.copy_of(np.ones(P, dtype=np.uint8)))
    fp2.set("part_prev_never_equal", arena.copy_of(np.zeros(P, dtype=np.uint8)))
    fp2.set("node_removed", arena.copy_of(gone))
    fp2.scalars.update(n_prev=P, nodes_to_add_nil=1)
    out = abi.FlatResult(fp, arena)

    def way_a(t):
        t0 = time.perf_counter()
        pl.download(into=res)
        t1 = time.perf_counter()
        total = int(res.out_off[PM])
        for pre in ("assign", "prev"):
            fp2.set(pre + "_off", res.out_off)
            fp2.set(pre + "_nodes", res.out_nodes[:total])
            fp2.set(pre + "_kind", res.out_kind)
        fp2.as_struct()
        t2 = time.perf_counter()
        pl.upload(fp2)
        t3 = time.perf_counter()
        pl.set_wire_names(part_names, node_names, state_names)
        t4 = time.perf_counter()
        for key, v in zip(("download", "point", "upload", "names"), (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
            t.setdefault(key, []).append(v)
        t.setdefault("whole", []).append(t4 - t0)

    def way_b(t):
        t0 = time.perf_counter()
        pl.adopt(node_removed=gone)
        t.setdefault("whole", []).append(time.perf_counter() - t0)

    def plan_after(t):
        t0 = time.perf_counter()
        r = pl.plan_resident()
        t.setdefault("plan wall", []).append(time.perf_counter() - t0)
        t.setdefault("plan device", []).append(r.device_ms / 1e3)
        t.setdefault("sweeps", []).append(r.iterations)
        return pl.download(into=out).digest()

    if a.only:
        t = {}
        restore()
        way_b({})
        for _ in range(a.reps):
            restore()
            way_b(t)
        print("only adopt: whole call " + stats(t["whole"]))
        pl.close()
        return
    ways = {"a": way_a, "b": way_b}
    for k in "ab":                                             # warm-up: buffers sized, staging grown
        restore()
        ways[k]({})
        plan_after({})
    times, digests = {"a": {}, "b": {}}, {"a": set(), "b": set()}
    for rep in range(a.reps):
        for k in ("ab" if rep % 2 == 0 else "ba"):             # the order alternates
            restore()
            ways[k](times[k])
            digests[k].add(plan_after(times[k]))
    equal = len(digests["a"]) == 1 and digests["a"] == digests["b"]
    print("digests of the following plan equal: %s   sweeps a %s  b %s" % (equal, sorted(set(times["a"]["sweeps"])),
                                                                            sorted(set(times["b"]["sweeps"]))), flush=True)
    if not equal:
        sys.exit(1)
    for key, what in (("download", "blance_download into page-locked arrays"), ("point", "assign_* / prev_* pointed at them"),
                      ("upload", "blance_upload"), ("names", "blance_plan_wire_names (through Python)"), ("whole", "all four")):
        print("(a) %-42s %s" % (what + ":", stats(times["a"][key])))
    print("(a) download + upload:                         median %9.3f ms" %
          ((statistics.median(times["a"]["download"]) + statistics.median(times["a"]["upload"])) * 1e3))
    print("(b) %-42s %s" % ("blance_plan_adopt:", stats(times["b"]["whole"])))
    for k in "ab":
        print("(%s) the following plan, wall:                  %s" % (k, stats(times[k]["plan wall"])))
        print("(%s) the following plan, device_ms:             %s" % (k, stats(times[k]["plan device"])))
    pl.close()


if __name__ == "__main__":
    main()
