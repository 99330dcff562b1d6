"""Many small plans: blance_plan one after another vs one blance_plan_batch vs the C oracle on one host core.

    python tools/batch_gpu.py --B 1 64 512 4096 --shape cbgt

One JSON line per B: plans/s and assignments/s of each way, launches per plan, the batch's device_ms, every digest
checked against the oracle.  Shapes: cbgt (64-2,048 partitions, 8-256 nodes) and small (16-256 partitions, 8-64 nodes)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from blance_amd import hip, synth  # noqa: E402
from oracle import loader  # noqa: E402

SHAPES = {"cbgt": dict(P_range=(64, 2048), N_range=(8, 256)), "small": dict(P_range=(16, 256), N_range=(8, 64))}


def assignments(fps):
    return sum(int(fp.n_parts) * int(sum(max(int(k), 0) for k in fp.arrays["state_constraints"])) for fp in fps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[1, 64, 512])
    ap.add_argument("--shape", choices=sorted(SHAPES), default="cbgt")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--oracle-max", type=int, default=512, help="oracle timing on at most this many problems (all are checked)")
    a = ap.parse_args()
    pl = hip.Planner(device_id=0)
    warm = synth.cbgt_batch(8, seed=a.seed + 99, **SHAPES[a.shape])
    pl.plan_batch(warm)
    for fp in warm:
        pl.plan(fp)
    for B in a.B:
        fps = synth.cbgt_batch(B, seed=a.seed, **SHAPES[a.shape])
        n_asg = assignments(fps)
        t0 = time.perf_counter()
        seq = [pl.plan(fp) for fp in fps]
        t_seq = time.perf_counter() - t0
        launches_seq = sum(int(r.struct.kernel_launches) for r in seq)
        t0 = time.perf_counter()
        got, info = pl.plan_batch(fps)
        t_batch = time.perf_counter() - t0
        n_or = min(B, a.oracle_max)
        t0 = time.perf_counter()
        want = [loader.plan(fp) for fp in fps[:n_or]]
        t_or = time.perf_counter() - t0
        want += [loader.plan(fp) for fp in fps[n_or:]]
        ok = all(g.digest() == w.digest() and s.digest() == w.digest() and g.iterations == w.iterations
                 for g, s, w in zip(got, seq, want))
        print(json.dumps({
            "B": B, "shape": a.shape, "digests_equal": ok, "assignments": n_asg,
            "sequential": {"s": round(t_seq, 4), "plans_per_s": round(B / t_seq, 1), "assignments_per_s": round(n_asg / t_seq),
                           "launches_per_plan": round(launches_seq / B, 1)},
            "batch": {"s": round(t_batch, 4), "plans_per_s": round(B / t_batch, 1), "assignments_per_s": round(n_asg / t_batch),
                      "launches_per_plan": round(info["kernel_launches"] / B, 4), "device_ms": round(info["device_ms"], 3),
                      "total_ms": round(info["total_ms"], 3), "n_batched": info["n_batched"], "n_fallback": info["n_fallback"]},
            "oracle_one_core": {"problems_timed": n_or, "plans_per_s": round(n_or / t_or, 1),
                                "assignments_per_s": round(assignments(fps[:n_or]) / t_or)},
            "host_cores": os.cpu_count()}), flush=True)
        if not ok:
            sys.exit(1)
    pl.close()


if __name__ == "__main__":
    main()
