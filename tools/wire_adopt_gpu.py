"""A PartitionMap document as the next round's prevMap and partitionsToAssign, two routes, alternating in one process after a
warm-up:

    (a) the route blance_wire_adopt replaces: blance_wire_decode_device from a page-locked document into page-locked arrays
        of a known capacity, prev_* / assign_* / part_in_prev of the next problem pointed at them, blance_upload -- the three
        parts timed separately
    (b) blance_wire_adopt (Planner.adopt_wire) from the same page-locked document: the lists stay on the device

    python tools/wire_adopt_gpu.py [P] [N] [--reps 6]          (default 1048576 4096)

The workload is config 3's plan (synth.config_flat(3, P, N)): its document, as blance_plan_wire_get returns it, is the map the
cluster has; the next call's change is config3_rebalance_flat's -- every tenth node leaves.  Before every repetition of either
route the context is put back to "holds config 3's problem" (blance_upload, not timed).  The plan that follows is timed for both
routes and the two digests must be equal.  Times are the host's clock around calls that end in a device synchronise;
device_ms is what the calls report (first kernel to last, the host's round trips between them included).  --only adopt runs
(b) alone, --reps times: for a kernel trace of its own
(rocprofv3 --kernel-trace --stats -- python tools/wire_adopt_gpu.py P N --only adopt)."""
import argparse
import copy
import ctypes as C
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
    ap.add_argument("--only", choices=["adopt"], help="run this route alone (no comparison)")
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
    M = fp.n_states
    PM = P * M

    pl.upload(fp)
    r0 = pl.plan_resident()
    pl.set_wire_names(part_names, node_names, state_names)
    doc, _ = pl.plan_wire()
    n_refs = int(pl.download().out_off[PM])
    wdict = pl.wire_dict(part_names, node_names, state_names)
    pinned_doc = arena.copy_of(np.frombuffer(doc, np.uint8))
    print("P %d  N %d  config 3's plan: %d sweeps, device %.3f ms; document %d bytes, %d node references" %
          (P, N, r0.iterations, r0.device_ms, len(doc), n_refs), flush=True)

    # route (a)'s arrays, page-locked, and the next problem that points at them
    lists = [arena.empty(max(P, 1), np.uint8), arena.empty(PM + 1, np.int32), arena.empty(max(PM, 1), np.uint8),
             arena.empty(max(n_refs, 1), np.int32)]
    in_prev, never = arena.empty(max(P, 1), np.uint8), arena.empty(max(P, 1), np.uint8)
    fp2 = copy.copy(fp)
    fp2.scalars = dict(fp.scalars)
    fp2.arrays = dict(fp.arrays)
    fp2._struct, fp2._keep = None, []
    fp2.set("node_removed", arena.copy_of(gone))
    fp2.scalars.update(nodes_to_add_nil=1)
    out = abi.FlatResult(fp, arena)
    dev = {"a decode": [], "b adopt_wire": []}

    def way_a(t):
        t0 = time.perf_counter()
        wl = abi.WireLists()
        wl.part_kind, wl.off, wl.kind, wl.nodes = [x.ctypes.data for x in lists]
        wl.capacity = n_refs
        pl._check(pl.lib.blance_wire_decode_device(pl._h, wdict._h, pinned_doc.ctypes.data, pinned_doc.size, C.byref(wl)))
        t1 = time.perf_counter()
        total = int(wl.n_node_refs)
        for pre in ("assign", "prev"):
            fp2.set(pre + "_off", lists[1])
            fp2.set(pre + "_nodes", lists[3][:total])
            fp2.set(pre + "_kind", lists[2][:PM])
        np.not_equal(lists[0][:P], abi.LIST_ABSENT, out=in_prev[:P].view(np.bool_))
        np.equal(lists[0][:P], abi.LIST_NIL, out=never[:P].view(np.bool_))
        fp2.set("part_in_prev", in_prev[:P])
        fp2.set("part_prev_never_equal", never[:P])
        fp2.scalars.update(n_prev=int(wl.n_parts_seen))
        fp2.as_struct()
        t2 = time.perf_counter()
        pl.upload(fp2)
        t3 = time.perf_counter()
        for key, v in zip(("decode", "point", "upload"), (t1 - t0, t2 - t1, t3 - t2)):
            t.setdefault(key, []).append(v)
        t.setdefault("whole", []).append(t3 - t0)
        dev["a decode"].append(float(wl.device_ms) / 1e3)

    def way_b(t):
        t0 = time.perf_counter()
        info = pl.adopt_wire(wdict, pinned_doc, node_removed=gone)
        t.setdefault("whole", []).append(time.perf_counter() - t0)
        if not info["adopted"]:
            print("adopt_wire refused: %s" % info)
            sys.exit(1)
        t.setdefault("inside", []).append(info["total_ms"] / 1e3)
        dev["b adopt_wire"].append(info["device_ms"] / 1e3)

    def plan_after(t):
        t0 = time.perf_counter()
        r = pl.plan_resident()
        t.setdefault("plan wall", []).append(time.perf_counter() - t0)
        t.setdefault("plan device", []).append(r.device_ms / 1e3)
        t.setdefault("sweeps", []).append(r.iterations)
        return pl.download(into=out).digest()

    def restore():
        pl.upload(fp)

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
    dev = {"a decode": [], "b adopt_wire": []}
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
    for key, what in (("decode", "blance_wire_decode_device, page-locked"), ("point", "the problem's arrays pointed at the lists"),
                      ("upload", "blance_upload"), ("whole", "all three")):
        print("(a) %-44s %s" % (what + ":", stats(times["a"][key])))
    print("(b) %-44s %s" % ("blance_wire_adopt (through Python):", stats(times["b"]["whole"])))
    print("(b) %-44s %s" % ("blance_wire_adopt (total_ms of the call):", stats(times["b"]["inside"])))
    print("(a) device_ms of the decode (split + both parses):        %s" % stats(dev["a decode"]))
    print("(b) device_ms of adopt_wire (the same + summary + write): %s" % stats(dev["b adopt_wire"]))
    print("(b) - (a) device_ms = k_wire_adopt_sum, its round trip, the node arrays' copies, k_wire_adopt_write: median %.3f ms" %
          ((statistics.median(dev["b adopt_wire"]) - statistics.median(dev["a decode"])) * 1e3))
    ma, mb = statistics.median(times["a"]["whole"]), statistics.median(times["b"]["whole"])
    print("(a) - (b) medians: %.3f ms   a / b = %.2f   not slower: %s" % ((ma - mb) * 1e3, ma / mb, mb <= ma))
    for k in "ab":
        print("(%s) the following plan, wall:                  %s" % (k, stats(times[k]["plan wall"])))
        print("(%s) the following plan, device_ms:             %s" % (k, stats(times[k]["plan device"])))
    pl.close()


if __name__ == "__main__":
    main()
