"""The partition moves of a resident plan, three ways, alternating in one process after a warm-up:

    (a) download, both maps rebuilt on the host as (M + 1)-state CSRs, blance_calc_moves (the route before
        blance_plan_moves_get)
    (b) blance_plan_moves_get: the moves from the maps on the device
    (c) blance_plan_moves_get, count only

    python tools/plan_moves_gpu.py --sizes 1048576x4096 65536x1024 --reps 5

The workload is config 3's rebalance (synth.config3_rebalance_flat: the plan of config 3, every tenth node removed),
uploaded and planned once per size (upload + plan_resident); the three ways then answer for that resident plan.  One JSON
line per size: every way's wall times (host clock around calls that end in a device synchronise), their median and
minimum, device_ms of (b) and (c), the counters, and the checks: the plan's digest equal to the C oracle's (--oracle), every
moves array of (b) equal to (a)'s before a time is printed, (c)'s counters equal to (b)'s.
--only b (or c) runs that way alone, --reps times: for a kernel trace of its own."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from blance_amd import hip, synth  # noqa: E402


def way_a(pl, fp, favor, arena):
    res = pl.download()
    op_off, op_node, op_state, op_kind, _ = pl.calc_moves(int(fp.n_states), favor, *hip.moves_problem_of(fp, res))
    t = int(op_off[-1])
    return (op_off, op_node[:t], op_state[:t], op_kind[:t]), None


def way_b(pl, fp, favor, arena):
    return pl.plan_moves(favor, arena=arena)


def way_c(pl, fp, favor, arena):
    return pl.plan_moves(favor, count_only=True)


WAYS = {"a_download_csr_calc_moves": way_a, "b_plan_moves": way_b, "c_plan_moves_count_only": way_c}
COUNTERS = ("n_moves", "n_by_kind", "n_parts_moved")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["1048576x4096", "65536x1024"], help="PxN")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--favor-min-nodes", action="store_true")
    ap.add_argument("--pinned", action="store_true", help="(b)'s output arrays in page-locked memory (hip.HostArena)")
    ap.add_argument("--oracle", action="store_true", help="also compare the plan's digest with the C oracle's (slow at full size)")
    ap.add_argument("--only", choices=["b", "c"], help="run this way alone (no comparison)")
    a = ap.parse_args()
    pl = hip.Planner(device_id=0)
    favor = a.favor_min_nodes
    ok_all = True
    for size in a.sizes:
        P, N = [int(x) for x in size.lower().split("x")]
        fp1 = synth.config_flat(3, P=P, N=N)
        fp = synth.config3_rebalance_flat(fp1, pl.plan(fp1))
        pl.upload(fp)
        r = pl.plan_resident()
        arena = hip.HostArena() if a.pinned else None
        if a.only:
            fn = way_b if a.only == "b" else way_c
            fn(pl, fp, favor, arena)
            t = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                _, info = fn(pl, fp, favor, arena)
                t.append(time.perf_counter() - t0)
            print(json.dumps({"P": P, "N": N, "only": a.only, "reps": a.reps, "median_s": round(statistics.median(t), 6),
                              "min_s": round(min(t), 6), "device_ms": round(info["device_ms"], 4), "n_moves": info["n_moves"]}),
                  flush=True)
            continue
        for fn in WAYS.values():                              # warm-up: buffers sized, staging grown
            fn(pl, fp, favor, arena)
        names = list(WAYS)
        times = {k: [] for k in names}
        dev = {k: [] for k in names}
        last = {}
        for rep in range(a.reps):
            for k in names[rep % 3:] + names[:rep % 3]:       # the order rotates every repetition
                t0 = time.perf_counter()
                out = WAYS[k](pl, fp, favor, arena)
                times[k].append(time.perf_counter() - t0)
                if out[1] is not None:
                    dev[k].append(out[1]["device_ms"])
                last[k] = out
        mv_a, mv_b = last["a_download_csr_calc_moves"][0], last["b_plan_moves"][0]
        info_b, info_c = last["b_plan_moves"][1], last["c_plan_moves_count_only"][1]
        moves_equal = all(np.array_equal(x, y) for x, y in zip(mv_a, mv_b))
        counters_equal = all(info_b[k] == info_c[k] for k in COUNTERS) and info_b["n_moves"] == int(mv_a[0][-1])
        digest_ok = None
        if a.oracle:
            from oracle import loader
            digest_ok = pl.download().digest() == loader.plan(fp).digest()
        ok = moves_equal and counters_equal and digest_ok is not False
        ok_all = ok_all and ok
        if not ok:
            print(json.dumps({"P": P, "N": N, "moves_b_equal_a": moves_equal, "counters_c_equal_b": counters_equal,
                              "digest_equal_oracle": digest_ok}), flush=True)
            continue
        summary = {k: {"median_s": round(statistics.median(v), 6), "min_s": round(min(v), 6),
                       "runs_s": [round(x, 6) for x in v]} for k, v in times.items()}
        med = {k: summary[k]["median_s"] for k in names}
        print(json.dumps({
            "P": P, "N": N, "favor_min_nodes": favor, "pinned": a.pinned, "reps": a.reps, "plan_device_ms": round(r.device_ms, 3),
            "plan_iterations": int(r.iterations), "times": summary,
            "a_over_b": round(med["a_download_csr_calc_moves"] / med["b_plan_moves"], 2),
            "device_ms": {k: round(statistics.median(v), 4) for k, v in dev.items() if v},
            "counters": {k: info_b[k] for k in COUNTERS},
            "moves_b_equal_a": moves_equal, "counters_c_equal_b": counters_equal, "digest_equal_oracle": digest_ok}), flush=True)
    pl.close()
    if not ok_all:
        sys.exit(1)


if __name__ == "__main__":
    main()
