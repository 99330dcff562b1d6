"""A PartitionMap document into the planner's list arrays, two routes, alternating in one process after a warm-up:

    (a) the host route: wire.decode (blance_wire_decode, one core), then planner.lists_of_wire_map (the decoder's first-seen
        ids carried over to the problem's ids, numpy) -- timed as one and apart
    (b) blance_wire_decode_device from a pageable document
    (c) blance_wire_decode_device from a page-locked document (hip.HostArena), the arrays page-locked too

    python tools/wire_decode_gpu.py [P] [N] [--reps 5]          (default 1048576 4096)

The workload is config 3's shape (synth.config_flat(3, P, N)), uploaded and planned once; the document is the one
blance_plan_wire_get returns for the plan.  Every route's arrays must equal the downloaded plan (out_off / out_nodes /
out_kind) before a time is printed: the timed run is a correctness run.  Printed: blance_wire_dict_create on a line of its own
(once per set of names), every route's median and range (host clock), the device's time for the kernels of a call, and a
host-to-device copy of the document's bytes made in this process with torch for scale -- the one cost no design avoids.
--only b|c runs that route alone, --reps times: for a kernel trace of its own."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from blance_amd import abi, hip, planner, synth, wire  # noqa: E402


def stats(v, unit=1e3):
    return "median %9.3f ms   range %9.3f .. %9.3f ms" % (statistics.median(v) * unit, min(v) * unit, max(v) * unit)


def h2d_copy_ms(nbytes, reps):
    import torch
    src = torch.zeros(nbytes, dtype=torch.uint8).pin_memory()
    dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dst.copy_(src, non_blocking=True)
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(src, non_blocking=True)
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("P", nargs="?", type=int, default=1048576)
    ap.add_argument("N", nargs="?", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=["b", "c"], help="run this route alone (no comparison)")
    a = ap.parse_args()
    P, N = a.P, a.N
    pl = hip.Planner(device_id=0)
    fp = synth.config_flat(3, P=P, N=N)
    part_names = fp.part_names or [str(p) for p in range(fp.n_parts)]
    node_names = fp.node_names or ["n%04d" % i for i in range(fp.n_nodes_ext)]
    state_names = fp.state_names or ["primary", "replica", "spare", "dead"][:fp.n_states]
    pl.upload(fp)
    r = pl.plan_resident()
    pl.set_wire_names(part_names, node_names, state_names)
    doc, _ = pl.plan_wire()
    res = pl.download()
    PM = fp.n_parts * fp.n_states
    n_refs = int(res.out_off[PM])
    print("P %d  N %d  plan: %d sweeps, device %.3f ms; document %d bytes, %d node references" %
          (P, N, r.iterations, r.device_ms, len(doc), n_refs), flush=True)
    t_dict = []
    for _ in range(max(a.reps, 5)):
        t0 = time.perf_counter()
        wdict = pl.wire_dict(part_names, node_names, state_names)
        t_dict.append(time.perf_counter() - t0)
        wdict.close()
    print("wire_dict (once per set of names; through Python: blobs built, three hash tables, the upload): " + stats(t_dict), flush=True)
    wdict = pl.wire_dict(part_names, node_names, state_names)
    arena = hip.HostArena()
    pageable_doc = np.frombuffer(doc, np.uint8).copy()
    pinned_doc = arena.copy_of(pageable_doc)

    def arrays(new):
        return [new(max(fp.n_parts, 1), np.uint8), new(PM + 1, np.int32), new(max(PM, 1), np.uint8), new(max(n_refs, 1), np.int32)]

    pageable_out = arrays(lambda n, dt: np.empty(n, dtype=dt))
    pinned_out = arrays(arena.empty)

    def device(src, out):
        wl = abi.WireLists()
        wl.part_kind, wl.off, wl.kind, wl.nodes = [x.ctypes.data for x in out]
        wl.capacity = n_refs
        pl._check(pl.lib.blance_wire_decode_device(pl._h, wdict._h, src.ctypes.data, src.size, C.byref(wl)))
        return {"part_kind": out[0], "off": out[1], "kind": out[2], "nodes": out[3][:int(wl.n_node_refs)]}, float(wl.device_ms)

    split = {"decode": [], "carry": []}

    def way_a():
        t0 = time.perf_counter()
        wm = wire.decode(doc)
        t1 = time.perf_counter()
        out = planner.lists_of_wire_map(wm, wdict)
        t2 = time.perf_counter()
        wm.close()
        split["decode"].append(t1 - t0)
        split["carry"].append(t2 - t1)
        return out, None

    ways = {"a host decoder + ids carried over": way_a, "b decode_wire, pageable": lambda: device(pageable_doc, pageable_out),
            "c decode_wire, page-locked": lambda: device(pinned_doc, pinned_out)}

    def is_the_plan(got):
        return (np.array_equal(got["off"], res.out_off[:PM + 1]) and np.array_equal(got["nodes"], res.out_nodes[:n_refs]) and
                np.array_equal(got["kind"], res.out_kind[:PM]) and (got["part_kind"] == abi.LIST_SET).all())

    if a.only:
        fn = ways["b decode_wire, pageable"] if a.only == "b" else ways["c decode_wire, page-locked"]
        fn()
        t, dev = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            got, ms = fn()
            t.append(time.perf_counter() - t0)
            dev.append(ms / 1e3)
        print("only %s: equals the downloaded plan: %s" % (a.only, is_the_plan(got)))
        print("only %s: wall %s" % (a.only, stats(t)))
        print("only %s: device_ms %s" % (a.only, stats(dev)))
        pl.close()
        return
    names = list(ways)
    for k in names:
        ways[k]()                                              # warm-up: buffers sized, staging grown
    split = {"decode": [], "carry": []}
    times, dev, ok = {k: [] for k in names}, {k: [] for k in names}, {}
    for rep in range(a.reps):
        for k in names[rep % 3:] + names[:rep % 3]:            # the order rotates every repetition
            t0 = time.perf_counter()
            got, ms = ways[k]()
            times[k].append(time.perf_counter() - t0)
            if ms is not None:
                dev[k].append(ms / 1e3)
            ok[k] = is_the_plan(got)
    print("every route's arrays equal the downloaded plan: %s" % ok, flush=True)
    if not all(ok.values()):
        sys.exit(1)
    for k in names:
        print("(%s) whole call: %s" % (k, stats(times[k])))
    print("(a) of which wire.decode: %s" % stats(split["decode"]))
    print("(a) of which lists_of_wire_map: %s" % stats(split["carry"]))
    med = {k: statistics.median(times[k]) for k in names}
    print("a / b = %.1f   a / c = %.1f   wire.decode alone / c = %.1f" %
          (med[names[0]] / med[names[1]], med[names[0]] / med[names[2]], statistics.median(split["decode"]) / med[names[2]]))
    for k in names[1:]:
        print("(%s) device_ms, the record split + both parsing passes + scans: %s" % (k, stats(dev[k])))
    c = names[2]
    print("(c) whole call minus device_ms = H2D copy of the document + host round trips + D2H copy of the arrays: median %.3f ms"
          % ((med[c] - statistics.median(dev[c])) * 1e3))
    # a count-only call from the page-locked document moves the document in and two words out: its whole call minus its
    # device_ms is the H2D copy of the document (and two host round trips) as this library makes it
    t_count, dev_count = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        info = pl.decode_wire(wdict, pinned_doc, count_only=True)
        t_count.append(time.perf_counter() - t0)
        dev_count.append(info["device_ms"] / 1e3)
    print("count-only call, page-locked document: whole call %s" % stats(t_count))
    print("count-only call, page-locked document: device_ms, the record split + the first parsing pass + scans: %s" % stats(dev_count))
    print("count-only call: whole call minus device_ms = H2D copy of the document + host round trips: median %.3f ms"
          % ((statistics.median(t_count) - statistics.median(dev_count)) * 1e3))
    try:
        h2d = h2d_copy_ms(len(doc), a.reps)
        print("host-to-device copy of %d bytes from page-locked memory (torch, same process): %s" % (len(doc), stats([x / 1e3 for x in h2d])))
    except Exception as e:                                     # (torch without a device: the figure is for scale only)
        print("host-to-device copy: not measured (%s)" % e)
    pl.close()


if __name__ == "__main__":
    main()
