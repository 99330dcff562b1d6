"""A batch of plans and each plan as PartitionMap JSON bytes, three routes alternating in one process after a warm-up:

    (a) blance_plan_batch, then per plan problem.decode_result + wire.encode on the host (the route
        blance_plan_batch_wire replaces); (a2) the same with wire.ResultEncoder objects made beforehand, the fastest host
        route the package has (numpy view + blance_wire_encode, no Python loop over partitions)
    (b) blance_plan_batch_wire with blance_batch_names objects made beforehand (their creation timed apart)
    (c) blance_plan_batch alone

    python tools/batch_wire_gpu.py --B 64 512 4096 --reps 5
    python tools/batch_wire_gpu.py --B 512 --only b --reps 3          (for a kernel trace of (b) alone)

One JSON line per B: every route's wall times (host clock around calls that end in a device synchronise), their median and
minimum, (a)/(b), (b)/(c) beside (c)'s own min-max spread, launches, bytes, and the checks, all made before a time is
reported: every document of (b) equal to (a)'s and to (a2)'s, every digest of (b) equal to (c)'s."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from blance_amd import hip, problem, synth, wire  # noqa: E402

SHAPES = {"cbgt": dict(P_range=(64, 2048), N_range=(8, 256)), "small": dict(P_range=(16, 256), N_range=(8, 64))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[64, 512, 4096])
    ap.add_argument("--shape", choices=sorted(SHAPES), default="cbgt")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=["a", "a2", "b", "c"], default=None, help="time one route alone (nothing is compared)")
    a = ap.parse_args()
    pl = hip.Planner(device_id=0)

    def way_a(fps, names, encs):
        results, info = pl.plan_batch(fps)
        return results, [wire.encode(problem.decode_result(fp, r)[0]) for fp, r in zip(fps, results)], info

    def way_a2(fps, names, encs):
        results, info = pl.plan_batch(fps)
        return results, [e.encode(r) for e, r in zip(encs, results)], info

    def way_b(fps, names, encs):
        results, _, _, docs, info = pl.plan_batch_wire(fps, names)
        return results, docs, info

    def way_c(fps, names, encs):
        results, info = pl.plan_batch(fps)
        return results, None, info

    all_ways = {"a": way_a, "a2": way_a2, "b": way_b, "c": way_c}
    ways = all_ways if a.only is None else {a.only: all_ways[a.only]}

    def prepared(fps):
        t0 = time.perf_counter()
        names = [pl.batch_names(fp) for fp in fps]
        t1 = time.perf_counter()
        encs = [wire.ResultEncoder(fp.part_names, fp.node_names, fp.state_names) for fp in fps]
        return names, encs, t1 - t0, time.perf_counter() - t1

    warm = synth.cbgt_batch(8, seed=a.seed + 99, **SHAPES[a.shape])
    wn, we, _, _ = prepared(warm)
    for fn in ways.values():
        fn(warm, wn, we)
    ok_all = True
    for B in a.B:
        fps = synth.cbgt_batch(B, seed=a.seed, **SHAPES[a.shape])
        names, encs, names_s, encs_s = prepared(fps)
        for fn in ways.values():                          # this B's shapes warmed up too
            fn(fps, names, encs)
        times = {k: [] for k in ways}
        last = {}
        order = list(ways)
        for r in range(a.reps):
            s = r % len(order)
            for k in order[s:] + order[:s]:               # the order rotates every repetition
                t0 = time.perf_counter()
                out = ways[k](fps, names, encs)
                times[k].append(time.perf_counter() - t0)
                last[k] = out
        summary = {k: {"median_s": round(statistics.median(v), 5), "min_s": round(min(v), 5), "max_s": round(max(v), 5),
                       "runs_s": [round(x, 5) for x in v]} for k, v in times.items()}
        line = {"B": B, "shape": a.shape, "reps": a.reps, "partitions": int(sum(fp.n_parts for fp in fps)), "times": summary,
                "names_create_s": round(names_s, 5), "result_encoders_create_s": round(encs_s, 5)}
        if a.only is None:
            (ra, da, _), (_, da2, _), (rb, db, ib), (rc, _, ic) = last["a"], last["a2"], last["b"], last["c"]
            docs_equal = db == da and db == da2
            digests = all(x.digest() == y.digest() and x.iterations == y.iterations for x, y in zip(rb, rc)) and \
                all(x.digest() == y.digest() for x, y in zip(ra, rc))
            ok = docs_equal and digests
            ok_all = ok_all and ok
            if not ok:
                print(json.dumps({"B": B, "error": "check failed: no time reported", "documents_equal": docs_equal,
                                  "digests_equal": digests}), flush=True)
                continue
            sa, sa2, sb, sc = (summary[k] for k in ("a", "a2", "b", "c"))
            line.update({
                "document_bytes": int(sum(len(d) for d in db)),
                "a_over_b_median": round(sa["median_s"] / sb["median_s"], 3), "a_over_b_min": round(sa["min_s"] / sb["min_s"], 3),
                "a2_over_b_median": round(sa2["median_s"] / sb["median_s"], 3), "a2_over_b_min": round(sa2["min_s"] / sb["min_s"], 3),
                "b_over_c_median": round(sb["median_s"] / sc["median_s"], 4), "b_over_c_min": round(sb["min_s"] / sc["min_s"], 4),
                "c_spread_s": round(sc["max_s"] - sc["min_s"], 5),
                "b_minus_c_median_s": round(sb["median_s"] - sc["median_s"], 5),
                "a_minus_c_median_s": round(sa["median_s"] - sc["median_s"], 5),
                "a2_minus_c_median_s": round(sa2["median_s"] - sc["median_s"], 5),
                "launches": {"b": int(ib["kernel_launches"]), "c": int(ic["kernel_launches"])},
                "device_ms": {"b": round(ib["device_ms"], 3), "c": round(ic["device_ms"], 3)},
                "n_batched": ib["n_batched"], "n_fallback": ib["n_fallback"],
                "documents_equal_a_and_a2": docs_equal, "digests_equal_c": digests})
        print(json.dumps(line), flush=True)
        for nm in names:
            nm.close()
    pl.close()
    if not ok_all:
        sys.exit(1)


if __name__ == "__main__":
    main()
