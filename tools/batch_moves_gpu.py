"""A batch of plans and their partition moves, three ways, alternating in one process after a warm-up:

    (a) blance_plan_batch, then one blance_calc_moves per problem (the path before blance_plan_batch_moves)
    (b) blance_plan_batch_moves: plans and moves in one call
    (c) blance_plan_batch alone

    python tools/batch_moves_gpu.py --B 64 512 4096 --reps 5

One JSON line per B: every way's wall times (host clock around calls that end in a device synchronise), their median
and minimum, launches, and the checks: every digest of (a), (b), (c) equal and equal to the C oracle's; every moves list
of (b) equal to (a)'s, and to oracle.moves_ref for the first --ref-max problems."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from blance_amd import hip, synth  # noqa: E402
from oracle import loader  # noqa: E402
from oracle.moves_ref import calc_partition_moves  # noqa: E402

SHAPES = {"cbgt": dict(P_range=(64, 2048), N_range=(8, 256)), "small": dict(P_range=(16, 256), N_range=(8, 64))}


def with_pseudo_state(off, nodes, P, M):
    """A CSR over p * M + state -> blance_calc_moves's CSR over p * (M + 1) + state (pseudo state M empty)."""
    lens = np.zeros((P, M + 1), dtype=np.int64)
    lens[:, :M] = np.diff(off[:P * M + 1].astype(np.int64)).reshape(P, M)
    out = np.zeros(P * (M + 1) + 1, dtype=np.int32)
    out[1:] = np.cumsum(lens)
    return out, nodes[:int(off[P * M])]


def way_a(pl, fps, begs, favor):
    results, info = pl.plan_batch(fps)
    moves = []
    for fp, r, (boff, bnod) in zip(fps, results, begs):
        P, M = int(fp.n_parts), int(fp.n_states)
        eoff, enod = with_pseudo_state(r.out_off, r.out_nodes, P, M)
        op_off, op_node, op_state, op_kind, _ = pl.calc_moves(M, favor, boff, bnod, eoff, enod)
        t = int(op_off[P])
        moves.append((op_off, op_node[:t], op_state[:t], op_kind[:t]))
    return results, moves, info


def way_b(pl, fps, begs, favor):
    return pl.plan_batch_moves(fps, favor)


def way_c(pl, fps, begs, favor):
    results, info = pl.plan_batch(fps)
    return results, None, info


def same_moves(x, y):
    return all(np.array_equal(a, b) for a, b in zip(x, y))


def ref_ok(fp, res, mv, favor):
    P, M = int(fp.n_parts), int(fp.n_states)
    off, nodes = fp.prev_off, fp.prev_nodes
    op_off, op_node, op_state, op_kind = mv
    for p, lists in enumerate(res.lists()):
        beg = {m: nodes[off[p * M + m]:off[p * M + m + 1]].tolist() for m in range(M)}
        end = {m: ids.tolist() for m, (_, ids) in enumerate(lists)}
        want = calc_partition_moves(list(range(M)), beg, end, favor)
        got = [(int(op_node[j]), "" if op_state[j] < 0 else int(op_state[j]), ["add", "del", "promote", "demote"][op_kind[j]])
               for j in range(op_off[p], op_off[p + 1])]
        if got != want:
            return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[64, 512, 4096])
    ap.add_argument("--shape", choices=sorted(SHAPES), default="cbgt")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--favor-min-nodes", action="store_true")
    ap.add_argument("--ref-max", type=int, default=64, help="moves also checked against oracle.moves_ref for this many")
    a = ap.parse_args()
    pl = hip.Planner(device_id=0)
    ways = {"a_plan_batch_then_calc_moves": way_a, "b_plan_batch_moves": way_b, "c_plan_batch": way_c}
    warm = synth.cbgt_batch(8, seed=a.seed + 99, **SHAPES[a.shape])
    warm_begs = [with_pseudo_state(fp.prev_off, fp.prev_nodes, int(fp.n_parts), int(fp.n_states)) for fp in warm]
    for fn in ways.values():
        fn(pl, warm, warm_begs, a.favor_min_nodes)
    ok_all = True
    for B in a.B:
        fps = synth.cbgt_batch(B, seed=a.seed, **SHAPES[a.shape])
        begs = [with_pseudo_state(fp.prev_off, fp.prev_nodes, int(fp.n_parts), int(fp.n_states)) for fp in fps]
        for fn in ways.values():                          # this B's shapes warmed up too
            fn(pl, fps, begs, a.favor_min_nodes)
        times = {k: [] for k in ways}
        last = {}
        names = list(ways)
        for r in range(a.reps):
            for k in names[r % 3:] + names[:r % 3]:       # the order rotates every repetition
                t0 = time.perf_counter()
                out = ways[k](pl, fps, begs, a.favor_min_nodes)
                times[k].append(time.perf_counter() - t0)
                last[k] = out
        ra, ma, ia = last["a_plan_batch_then_calc_moves"]
        rb, mb, ib = last["b_plan_batch_moves"]
        rc, _, ic = last["c_plan_batch"]
        want = [loader.plan(fp) for fp in fps]
        digests = all(x.digest() == y.digest() == z.digest() == w.digest() and x.iterations == w.iterations
                      for x, y, z, w in zip(ra, rb, rc, want))
        moves_equal = all(same_moves(x, y) for x, y in zip(ma, mb))
        n_ref = min(B, a.ref_max)
        moves_ref = all(ref_ok(fp, r, m, a.favor_min_nodes) for fp, r, m in zip(fps[:n_ref], rb[:n_ref], mb[:n_ref]))
        ok = digests and moves_equal and moves_ref
        ok_all = ok_all and ok
        summary = {k: {"median_s": round(statistics.median(v), 5), "min_s": round(min(v), 5),
                       "runs_s": [round(x, 5) for x in v]} for k, v in times.items()}
        med_b, med_c = summary["b_plan_batch_moves"]["median_s"], summary["c_plan_batch"]["median_s"]
        print(json.dumps({
            "B": B, "shape": a.shape, "favor_min_nodes": a.favor_min_nodes, "reps": a.reps, "times": summary,
            "b_over_c": round(med_b / med_c, 4), "a_over_b": round(summary["a_plan_batch_then_calc_moves"]["median_s"] / med_b, 2),
            "moves": int(sum(int(m[0][-1]) for m in mb)),
            "launches": {"a": int(ia["kernel_launches"]) + 3 * B, "b": int(ib["kernel_launches"]), "c": int(ic["kernel_launches"])},
            "device_ms": {"b": round(ib["device_ms"], 3), "c": round(ic["device_ms"], 3)},
            "n_batched": ib["n_batched"], "n_fallback": ib["n_fallback"],
            "digests_equal_oracle": digests, "moves_b_equal_a": moves_equal, "moves_ref_checked": n_ref,
            "moves_ref_equal": moves_ref}), flush=True)
    pl.close()
    if not ok_all:
        sys.exit(1)


if __name__ == "__main__":
    main()
