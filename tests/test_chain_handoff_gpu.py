"""The chain kernel's hand-off on an MI355X: the first three cases of tests/test_chain_handoff_emulated.py at
8,192 to 65,536 partitions, against the C oracle, and config 3 at its full size against tests/golden/config_digests.json with
the hand-off on and off."""
import json
import os

import numpy as np
import pytest

from blance_amd import hip, synth
from test_chain_handoff_emulated import MOVED, NO_HANDOFF, ZONE, Replan, _same, _stops

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module", autouse=True)
def torch_runtime_first():
    """This file sorts in front of tests/test_dist.py, whose GPU test was the suite's first and looks at the devices through
    torch.  torch brings its own copies of the HIP and HSA runtimes: loaded after libblance_hip.so has initialised the
    system's, they leave a later dlopen of librccl.so (tests/test_hip_parity.py: blance_comm_init_rccl) with an HSA
    that was never initialised -- 'no ROCm-capable device is detected'.  So torch looks first here, as it did there."""
    import torch
    if torch.cuda.is_available():
        torch.cuda.device_count()


def _oracle(fp):
    from oracle import loader
    return loader.plan(fp)


def plan_on_device(fp, monkeypatch, capfd, handoff, trace=True, **kw):
    """One plan on a fresh planner: (the result, the trace).  handoff = None: the default threshold."""
    monkeypatch.setenv("BLANCE_SPECULATE", "1")
    monkeypatch.delenv("BLANCE_CHAIN_WAVES", raising=False)
    if handoff is None:
        monkeypatch.delenv("BLANCE_CHAIN_HANDOFF", raising=False)
    else:
        monkeypatch.setenv("BLANCE_CHAIN_HANDOFF", str(handoff))
    if trace:
        monkeypatch.setenv("BLANCE_TRACE", "1")
    else:
        monkeypatch.delenv("BLANCE_TRACE", raising=False)
    capfd.readouterr()
    kw.setdefault("device_id", 0)
    pl = hip.Planner(chain_min_parts=64, **kw)
    try:
        got = pl.plan(fp)
    finally:
        pl.close()
    return got, capfd.readouterr().err


def check_config3_shape(plan):
    """65,536 x 512: four zones, chains of 16,384 steps -- the default threshold hands off.  Sweep 2's replica pass (stages of
    512 steps) moves steps in each region's first stage only; every region hands off after its second stage."""
    fp = synth.config_flat(3, P=65536, N=512)
    want = _oracle(fp)
    got, trace = plan(fp, None)
    _same(got, want, "default")
    passes = _stops(trace)
    assert len(passes) == 1, trace[-3000:]
    assert passes[0] == {r: (1024, 16384) for r in range(4)}, passes
    assert MOVED not in trace
    assert got.struct.stay_pass_launches == 2
    on, _ = plan(fp, None, trace=False)
    off, _ = plan(fp, 0, trace=False)
    _same(on, want, "on")
    _same(off, want, "off")
    assert (on.struct.host_syncs, on.iterations) == (off.struct.host_syncs, off.iterations) == (4, 3)


def check_late_move(plan):
    """16,384 x 256, a replan: a partition near the end of the pass order has swapped a replica with another late one and
    holds a node of its primary's rack.  The oracle's first sweep moves it; its region has handed off long before."""
    rp = Replan(16384, 256, 2)
    pos = rp.chain_pos()
    stage = 256                                            # (a plan's first sweep walks on four waves)
    found = None
    for p in range(rp.P - 1, rp.P - 20, -1):
        rack = int(rp.prim[p]) // 16
        for q in range(p - 1, p - 300, -1):
            for sq, x in enumerate(rp.replicas(rp.nodes, q)):
                if x // 16 != rack or x == rp.prim[p] or x in rp.replicas(rp.nodes, p) or found:
                    continue
                lists = rp.nodes.copy()
                lists[rp.off[q * rp.M + 1] + sq] = lists[rp.off[p * rp.M + 1]]
                lists[rp.off[p * rp.M + 1]] = x
                moved = rp.moved_in_sweep_1(lists)
                late = [m for m in moved if pos[m] >= 2 * stage]
                if p in late and all(pos[m] < stage for m in moved if m not in late):
                    found = (p, lists)
        if found:
            break
    assert found, "no such problem among the last partitions"
    p, lists = found
    fp = rp.problem(lists)
    want = _oracle(fp)
    got, trace = plan(fp, 64)
    _same(got, want, p)
    passes = _stops(trace)
    assert len(passes) == 1, trace[-3000:]
    at, _ = passes[0][int(rp.prim[p]) // ZONE]
    assert at is not None and at <= pos[p], (passes, pos[p])
    assert trace.count(MOVED) == 1, trace[-3000:]
    assert NO_HANDOFF in trace[trace.index(MOVED):]


def check_busy_beside_calm(plan):
    """8,192 x 256, the rebalance after every tenth node of zone 0 left: sweep 1's pass has events (no hand-off); from sweep
    2 on zone 0's chain (3,910 steps) keeps moving through its first half and, with 2,048 steps as the least to hand off, is
    walked to its end; zone 1's hands off after its first stage."""
    rp = Replan(8192, 256, 2)
    fp = rp.problem()
    rm = np.zeros(rp.N, dtype=np.uint8)
    rm[np.arange(3, ZONE, 10)] = 1
    fp.set("node_removed", rm)
    want = _oracle(fp)
    got, trace = plan(fp, 2048)
    _same(got, want, "rebalance")
    assert NO_HANDOFF in trace[:trace.index("hand-off (")], trace[:3000]
    passes = _stops(trace)
    assert passes, trace[-3000:]
    for d in passes:
        assert d[0][0] is None and d[1][0] == 512, passes
    assert MOVED not in trace


@pytest.mark.parametrize("check", [check_config3_shape, check_late_move, check_busy_beside_calm])
def test_against_the_oracle(monkeypatch, capfd, check):
    check(lambda fp, handoff, trace=True: plan_on_device(fp, monkeypatch, capfd, handoff, trace))


@pytest.mark.parametrize("handoff", [None, 0])
def test_config3_full_size(monkeypatch, capfd, handoff):
    with open(os.path.join(HERE, "golden", "config_digests.json")) as f:
        want = json.load(f)["config3"]
    fp = synth.config_flat(3)
    got, _ = plan_on_device(fp, monkeypatch, capfd, handoff, trace=False)
    assert (got.iterations, got.n_warnings, got.digest()) == (want["iterations"], want["warnings"], want["digest"]), handoff
    assert got.struct.host_syncs == 4
    assert got.struct.stay_pass_launches == (2 if handoff is None else 1)
