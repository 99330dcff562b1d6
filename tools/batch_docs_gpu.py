"""A batch of rebalances planned from the stored PartitionMap documents, three routes alternating in one process after a
warm-up.  The documents are those of a previous blance_plan_batch_wire; every tenth node leaves.

    (a) per index the host decoder (wire.decode), the carry-over into ids (planner.lists_of_wire_map) and
        problem.wire_adopted_problem, then ONE blance_plan_batch_wire
    (b) per index blance_upload + blance_wire_adopt + blance_plan_resident + the readers (download, plan_wire)
    (c) ONE blance_plan_batch_docs with blance_batch_dict objects made beforehand (their creation timed apart)

    python tools/batch_docs_gpu.py --B 512 --reps 7
    python tools/batch_docs_gpu.py --B 512 --only c --reps 3          (for a kernel trace of (c) alone)

One JSON line per B: every route's wall times (host clock around calls that end in a device synchronise), their median and
min..max, the launches and bytes, and the checks, all made before a time is reported: every result digest and every
document of (c) equal to (a)'s and to (b)'s."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from blance_amd import abi, hip, planner, problem, synth, wire  # noqa: E402

SHAPES = {"cbgt": dict(P_range=(64, 2048), N_range=(8, 256)), "small": dict(P_range=(16, 256), N_range=(8, 64))}


def leaving(fp):
    """fp with every tenth node of nodesAll leaving."""
    fp2 = abi.FlatProblem()
    fp2.scalars = dict(fp.scalars)
    for name, a in fp.arrays.items():
        fp2.set(name, a.copy())
    fp2.node_names, fp2.state_names, fp2.part_names = fp.node_names, fp.state_names, fp.part_names
    gone = np.zeros(fp.n_nodes_ext, dtype=np.uint8)
    gone[[n for n in range(fp.n_nodes) if n % 10 == 3]] = 1
    fp2.set("node_removed", gone)
    fp2.set("node_added", np.zeros(fp.n_nodes_ext, dtype=np.uint8))
    fp2.scalars["nodes_to_add_nil"] = 1
    return fp2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[512])
    ap.add_argument("--shape", choices=sorted(SHAPES), default="cbgt")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", choices=["a", "b", "c"], default=None, help="time one route alone (nothing is compared)")
    a = ap.parse_args()
    pl = hip.Planner(device_id=0)

    def way_a(sk, docs, names, dicts, wdict_names):
        fps = []
        for fp, doc, d in zip(sk, docs, dicts):
            wm = wire.decode(doc)
            try:
                lists = planner.lists_of_wire_map(wm, d)
            finally:
                wm.close()
            fps.append(problem.wire_adopted_problem(fp, lists, fp.node_removed, fp.node_added, True, True, False, row_stride=8))
        results, _, _, out, info = pl.plan_batch_wire(fps, names)
        return results, out, info

    def way_b(sk, docs, names, dicts, wdict_names):
        results, out = [], []
        for fp, doc in zip(sk, docs):
            pl.upload(fp)
            wd = pl.wire_dict(fp)
            pl.set_wire_names(fp)
            got = pl.adopt_wire(wd, doc, fp.node_removed, fp.node_added, True, True, False)
            assert got["adopted"], got
            pl.plan_resident()
            results.append(pl.download())
            out.append(pl.plan_wire()[0])
            wd.close()
        return results, out, None

    def way_c(sk, docs, names, dicts, wdict_names):
        results, _, _, out, oc, info = pl.plan_batch_docs(sk, docs, dicts, names=names)
        assert all(o["status"] == 0 for o in oc), [o for o in oc if o["status"]][:3]
        return results, out, info

    all_ways = {"a": way_a, "b": way_b, "c": way_c}
    ways = all_ways if a.only is None else {a.only: all_ways[a.only]}

    def prepared(B, seed):
        fps = [fp for fp in synth.cbgt_batch(B, seed=seed, **SHAPES[a.shape]) if fp.max_iterations > 0]
        names = [pl.batch_names(fp) for fp in fps]
        _, _, _, docs, _ = pl.plan_batch_wire(fps, names)
        t0 = time.perf_counter()
        dicts = [pl.batch_dict(fp) for fp in fps]
        return [leaving(fp) for fp in fps], docs, names, dicts, time.perf_counter() - t0

    w = prepared(8, a.seed + 99)
    for fn in ways.values():
        fn(*w[:4], None)
    ok_all = True
    for B in a.B:
        sk, docs, names, dicts, dicts_s = prepared(B, a.seed)
        for fn in ways.values():                          # this B's shapes warmed up too
            fn(sk, docs, names, dicts, None)
        times = {k: [] for k in ways}
        last = {}
        order = list(ways)
        for r in range(a.reps):
            s = r % len(order)
            for k in order[s:] + order[:s]:               # the order rotates every repetition
                t0 = time.perf_counter()
                out = ways[k](sk, docs, names, dicts, None)
                times[k].append(time.perf_counter() - t0)
                last[k] = out
        summary = {k: {"median_s": round(statistics.median(v), 5), "min_s": round(min(v), 5), "max_s": round(max(v), 5),
                       "runs_s": [round(x, 5) for x in v]} for k, v in times.items()}
        line = {"B": len(sk), "shape": a.shape, "reps": a.reps, "partitions": int(sum(fp.n_parts for fp in sk)),
                "document_bytes_in": int(sum(len(d) for d in docs)), "times": summary, "dicts_create_s": round(dicts_s, 5)}
        if a.only is None:
            (ra, da, ia), (rb, db, _), (rc, dc, ic) = last["a"], last["b"], last["c"]
            docs_equal = dc == da and dc == db
            digests = all(x.digest() == y.digest() == z.digest() and x.iterations == y.iterations == z.iterations
                          for x, y, z in zip(rc, ra, rb))
            ok = docs_equal and digests
            ok_all = ok_all and ok
            if not ok:
                print(json.dumps({"B": B, "error": "check failed: no time reported", "documents_equal": docs_equal,
                                  "digests_equal": digests}), flush=True)
                continue
            sa, sb, sc = (summary[k] for k in ("a", "b", "c"))
            line.update({
                "document_bytes_out": int(sum(len(d) for d in dc)),
                "a_over_c_median": round(sa["median_s"] / sc["median_s"], 3), "b_over_c_median": round(sb["median_s"] / sc["median_s"], 3),
                "a_minus_c_median_s": round(sa["median_s"] - sc["median_s"], 5), "b_minus_c_median_s": round(sb["median_s"] - sc["median_s"], 5),
                "spread_s": {k: round(summary[k]["max_s"] - summary[k]["min_s"], 5) for k in ("a", "b", "c")},
                "launches": {"a": int(ia["kernel_launches"]), "c": int(ic["kernel_launches"])},
                "device_ms": {"a": round(ia["device_ms"], 3), "c": round(ic["device_ms"], 3)},
                "n_batched": ic["n_batched"], "n_fallback": ic["n_fallback"],
                "documents_equal_a_and_b": docs_equal, "digests_equal_a_and_b": digests})
        print(json.dumps(line), flush=True)
        for x in names + dicts:
            x.close()
    pl.close()
    if not ok_all:
        sys.exit(1)


if __name__ == "__main__":
    main()
