"""A batch of plans and their plan statistics, three ways, alternating in one process after a warm-up:

    (a) blance_plan_batch, then per problem blance_plan + blance_plan_stats_get (the path before blance_plan_batch_stats;
        only for B <= --single-max: it plans every problem a second time, one at a time)
    (b) blance_plan_batch_stats: plans and statistics in one call, no moves
    (c) blance_plan_batch alone

    python tools/batch_stats_gpu.py --B 64 512 4096 --reps 5

One JSON line per B: every way's wall times (host clock around calls that end in a device synchronise), their median
and minimum, (c)'s min-max spread and whether (b) lands inside it, launches, and the checks, all made before a time is
reported: every digest of (a), (b) equal to (c)'s; every statistics block of (b) equal to oracle.stats_ref on (c)'s plan
(--ref-max of them; all by default) and, where (a) ran, to (a)'s."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from blance_amd import abi, hip, synth  # noqa: E402
from oracle import stats_ref  # noqa: E402

SHAPES = {"cbgt": dict(P_range=(64, 2048), N_range=(8, 256)), "small": dict(P_range=(16, 256), N_range=(8, 64))}
KEYS = abi.PLAN_STATS_ARRAYS


def way_a(pl, fps):
    results, info = pl.plan_batch(fps)
    stats = []
    for fp in fps:
        pl.plan(fp)
        stats.append(pl.plan_stats(int(fp.n_states)))
    return results, stats, info


def way_b(pl, fps):
    results, _, stats, info = pl.plan_batch_stats(fps)
    return results, stats, info


def way_c(pl, fps):
    results, info = pl.plan_batch(fps)
    return results, None, info


def same_stats(x, y):
    return int(x["n_nodes_next"]) == int(y["n_nodes_next"]) and \
        all(np.array_equal(np.asarray(x[k], dtype=np.int64), np.asarray(y[k], dtype=np.int64)) for k in KEYS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[64, 512, 4096])
    ap.add_argument("--shape", choices=sorted(SHAPES), default="cbgt")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--single-max", type=int, default=64, help="way (a) runs only for B up to this")
    ap.add_argument("--ref-max", type=int, default=1 << 30, help="statistics checked against oracle.stats_ref for this many")
    a = ap.parse_args()
    pl = hip.Planner(device_id=0)
    all_ways = {"a_plan_batch_then_plan_and_stats_get": way_a, "b_plan_batch_stats": way_b, "c_plan_batch": way_c}
    warm = synth.cbgt_batch(8, seed=a.seed + 99, **SHAPES[a.shape])
    for fn in all_ways.values():
        fn(pl, warm)
    ok_all = True
    for B in a.B:
        ways = {k: v for k, v in all_ways.items() if not k.startswith("a_") or B <= a.single_max}
        fps = synth.cbgt_batch(B, seed=a.seed, **SHAPES[a.shape])
        for fn in ways.values():                          # this B's shapes warmed up too
            fn(pl, fps)
        times = {k: [] for k in ways}
        last = {}
        names = list(ways)
        for r in range(a.reps):
            s = r % len(names)
            for k in names[s:] + names[:s]:               # the order rotates every repetition
                t0 = time.perf_counter()
                out = ways[k](pl, fps)
                times[k].append(time.perf_counter() - t0)
                last[k] = out
        rb, sb, ib = last["b_plan_batch_stats"]
        rc, _, ic = last["c_plan_batch"]
        digests = all(x.digest() == y.digest() and x.iterations == y.iterations for x, y in zip(rb, rc))
        stats_equal_a = None
        if "a_plan_batch_then_plan_and_stats_get" in last:
            ra, sa, _ = last["a_plan_batch_then_plan_and_stats_get"]
            digests = digests and all(x.digest() == y.digest() for x, y in zip(ra, rc))
            stats_equal_a = all(same_stats(x, y) for x, y in zip(sa, sb))
        n_ref = min(B, a.ref_max)
        ref_equal = all(same_stats(s, stats_ref.plan_stats(fp, r)) for fp, r, s in zip(fps[:n_ref], rc[:n_ref], sb[:n_ref]))
        ok = digests and ref_equal and stats_equal_a is not False
        ok_all = ok_all and ok
        if not ok:
            print(json.dumps({"B": B, "error": "check failed: no time reported", "digests_equal": digests,
                              "stats_ref_equal": ref_equal, "stats_b_equal_a": stats_equal_a}), flush=True)
            continue
        summary = {k: {"median_s": round(statistics.median(v), 5), "min_s": round(min(v), 5), "max_s": round(max(v), 5),
                       "runs_s": [round(x, 5) for x in v]} for k, v in times.items()}
        b, c = summary["b_plan_batch_stats"], summary["c_plan_batch"]
        spread = c["max_s"] - c["min_s"]
        line = {"B": B, "shape": a.shape, "reps": a.reps, "times": summary,
                "b_over_c_median": round(b["median_s"] / c["median_s"], 4), "b_over_c_min": round(b["min_s"] / c["min_s"], 4),
                "c_spread_s": round(spread, 5), "b_minus_c_median_s": round(b["median_s"] - c["median_s"], 5),
                "b_minus_c_min_s": round(b["min_s"] - c["min_s"], 5),
                "b_median_within_c_spread": bool(b["median_s"] - c["median_s"] <= spread),
                "b_min_within_c_spread": bool(b["min_s"] - c["min_s"] <= spread),
                "launches": {"b": int(ib["kernel_launches"]), "c": int(ic["kernel_launches"])},
                "device_ms": {"b": round(ib["device_ms"], 3), "c": round(ic["device_ms"], 3)},
                "plans_per_s": {"b": round(B / b["median_s"], 1), "c": round(B / c["median_s"], 1)},
                "n_batched": ib["n_batched"], "n_fallback": ib["n_fallback"], "digests_equal_c": digests,
                "stats_ref_checked": n_ref, "stats_ref_equal": ref_equal, "stats_b_equal_a": stats_equal_a}
        if "a_plan_batch_then_plan_and_stats_get" in summary:
            am = summary["a_plan_batch_then_plan_and_stats_get"]["median_s"]
            line["a_over_b_median"] = round(am / b["median_s"], 2)
            line["plans_per_s"]["a"] = round(B / am, 1)
        print(json.dumps(line), flush=True)
    pl.close()
    if not ok_all:
        sys.exit(1)


if __name__ == "__main__":
    main()
