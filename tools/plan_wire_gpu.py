"""A resident plan as PartitionMap JSON bytes, three ways, alternating in one process after a warm-up:

    (a) the route blance_plan_wire_get replaces: blance_download, then the host encoder on the downloaded arrays
        (wire.ResultEncoder: numpy builds the encoder's view, blance_wire_encode writes the document)
    (b) blance_plan_wire_get into a pageable buffer
    (c) blance_plan_wire_get into a page-locked buffer (hip.HostArena)

    python tools/plan_wire_gpu.py [P] [N] [--reps 7]          (default 1048576 4096)

The workload is config 3's shape (synth.config_flat(3, P, N)), uploaded and planned once (upload + plan_resident), with the
partition names "0" .. "P-1", which are not in byte order.  The three documents must be equal before a time is printed.
Printed: the one-time cost of set_wire_names on a line of its own, every way's median and range (host clock around calls
that end in a device synchronise), device_ms of the whole call and of the size-only call (sizing pass + scan), and a
device-to-device copy of the document's bytes made in this process with torch for scale.
--only b|c|size runs that way alone, --reps times: for a kernel trace of its own."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from blance_amd import hip, synth, wire  # noqa: E402


def stats(v, unit=1e3):
    return "median %9.3f ms   range %9.3f .. %9.3f ms" % (statistics.median(v) * unit, min(v) * unit, max(v) * unit)


def d2d_copy_ms(nbytes, reps):
    import torch
    src = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    dst.copy_(src)
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(src)
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("P", nargs="?", type=int, default=1048576)
    ap.add_argument("N", nargs="?", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", choices=["b", "c", "size"], help="run this way alone (no comparison)")
    a = ap.parse_args()
    P, N = a.P, a.N
    pl = hip.Planner(device_id=0)
    fp = synth.config_flat(3, P=P, N=N)
    part_names = fp.part_names or [str(p) for p in range(fp.n_parts)]
    node_names = fp.node_names or ["n%04d" % i for i in range(fp.n_nodes_ext)]
    state_names = fp.state_names or ["primary", "replica", "spare", "dead"][:fp.n_states]
    pl.upload(fp)
    r = pl.plan_resident()
    print("P %d  N %d  plan: %d sweeps, device %.3f ms" % (P, N, r.iterations, r.device_ms), flush=True)
    t_names = []
    for _ in range(3):
        t0 = time.perf_counter()
        pl.set_wire_names(part_names, node_names, state_names)
        t_names.append(time.perf_counter() - t0)
    print("set_wire_names (once per uploaded problem; through Python: blobs built, every string escaped, the key sort, "
          "the upload): " + stats(t_names), flush=True)
    arena = hip.HostArena()
    need = pl.plan_wire(size_only=True)[1]["need"]
    enc = wire.ResultEncoder(part_names, node_names, state_names)
    res = pl.download()
    pinned = arena.empty(need, np.uint8)
    pageable = np.empty(need, np.uint8)

    def raw(buf):
        import ctypes as C
        n, ms = C.c_size_t(0), C.c_double(0.0)
        pl._check(pl.lib.blance_plan_wire_get(pl._h, buf.ctypes.data, need, C.byref(n), C.byref(ms)))
        return buf, float(ms.value)

    def way_a():
        pl.download(into=res)
        return enc.encode(res), None

    ways = {"a download + host encoder": way_a, "b plan_wire, pageable": lambda: raw(pageable),
            "c plan_wire, page-locked": lambda: raw(pinned)}
    if a.only:
        fn = {"b": ways["b plan_wire, pageable"], "c": ways["c plan_wire, page-locked"],
              "size": lambda: (None, pl.plan_wire(size_only=True)[1]["device_ms"])}[a.only]
        fn()
        t, dev = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            _, ms = fn()
            t.append(time.perf_counter() - t0)
            dev.append(ms / 1e3)
        print("only %s: wall %s" % (a.only, stats(t)))
        print("only %s: device_ms %s" % (a.only, stats(dev)))
        pl.close()
        return
    names = list(ways)
    for k in names:
        ways[k]()                                              # warm-up: buffers sized, staging grown
    times, dev, last = {k: [] for k in names}, {k: [] for k in names}, {}
    for rep in range(a.reps):
        for k in names[rep % 3:] + names[:rep % 3]:            # the order rotates every repetition
            t0 = time.perf_counter()
            out, ms = ways[k]()
            times[k].append(time.perf_counter() - t0)
            if ms is not None:
                dev[k].append(ms / 1e3)
            last[k] = out if isinstance(out, bytes) else out.tobytes()
    docs = [last[k] for k in names]
    equal = docs[0] == docs[1] == docs[2]
    print("documents equal: %s   bytes: %d" % (equal, len(docs[0])), flush=True)
    if not equal:
        sys.exit(1)
    for k in names:
        print("(%s) whole call: %s" % (k, stats(times[k])))
    med = {k: statistics.median(times[k]) for k in names}
    print("a / b = %.1f   a / c = %.1f" % (med[names[0]] / med[names[1]], med[names[0]] / med[names[2]]))
    for k in names[1:]:
        print("(%s) device_ms, sizing pass + scan + writing pass: %s" % (k, stats(dev[k])))
    size_ms = []
    for _ in range(a.reps):
        size_ms.append(pl.plan_wire(size_only=True)[1]["device_ms"] / 1e3)
    print("size-only call, device_ms, sizing pass + scan: " + stats(size_ms))
    c = names[2]
    print("(c) whole call minus device_ms = host round trip + D2H copy of the document: median %.3f ms"
          % ((med[c] - statistics.median(dev[c])) * 1e3))
    try:
        d2d = d2d_copy_ms(len(docs[0]), a.reps)
        print("device-to-device copy of %d bytes (torch, same process): %s" % (len(docs[0]), stats([x / 1e3 for x in d2d])))
    except Exception as e:                                     # (torch without a device: the figure is for scale only)
        print("device-to-device copy: not measured (%s)" % e)
    pl.close()


if __name__ == "__main__":
    main()
