"""blance_plan_wire_names / blance_plan_wire_get on the MI355X: k_wire_size and k_wire_write against the host encoder on
the downloaded result (the route the call replaces) and against json.loads of the document; the checks of
test_plan_wire_emulated at the smallest shapes at which the kernels can go wrong, and three larger plans."""
import json

import numpy as np
import pytest

from blance_amd import abi, hip, synth, wire
from test_plan_batch_moves_emulated import _mixed
from test_plan_wire_emulated import (check_document, named, plan_and_check, renamed, run_context_undisturbed, run_escapes,
                                     run_golden, run_long_name, run_size_only_and_capacity, run_small_stage, top_keys,
                                     unordered_names)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def planner():
    pl = hip.Planner(device_id=0)
    yield pl
    pl.close()


def test_golden_cases(planner, golden_cases):
    n, missing, empty, full, null = run_golden(planner, golden_cases)
    assert n >= 60
    assert missing > 0 and empty > 0 and full > 0


def test_random_cases(planner):
    pairs = [(fp, prev) for fp, prev in _mixed(0) if planner.validate(fp) == abi.OK]
    sweeps = []
    for i, (fp, _) in enumerate(pairs):
        res, _, _ = plan_and_check(planner, fp, ("mixed", 0, i))
        sweeps.append(res.iterations if fp.n_prev > 0 else 0)
    assert max(sweeps) >= 2


@pytest.mark.parametrize("P", [1, 255, 257, 4099])
def test_order(planner, P):
    fp = renamed(synth.config_flat(2, P=P, N=16), unordered_names(P))
    res, doc, _ = plan_and_check(planner, fp, ("order", P))
    keys = top_keys(doc)
    assert len(keys) == P and keys == sorted(n.encode() for n in fp.part_names)


def test_escapes(planner):
    run_escapes(planner)


def test_small_stage(monkeypatch):
    """BLANCE_WIRE_STAGE is read when a context is made: a planner of its own."""
    run_small_stage(lambda: hip.Planner(device_id=0), monkeypatch)


def test_long_name(planner):
    run_long_name(planner)


def test_size_only_and_capacity(planner):
    run_size_only_and_capacity(planner)


def test_host_memory(planner):
    """The document in page-locked memory (written by DMA where it lies) and in an ordinary numpy array."""
    fp = named(synth.config_flat(3, P=3000, N=64))
    res = planner.plan(fp)
    planner.set_wire_names(fp)
    pageable, info_a = planner.plan_wire()
    arena = hip.HostArena()
    pinned, info_b = planner.plan_wire(arena=arena)
    assert arena.n_blocks == 1
    assert pageable == pinned and info_a["need"] == info_b["need"] == len(pinned)
    check_document(fp, res, pinned, "pinned")


def test_context_undisturbed(planner):
    run_context_undisturbed(planner, 3000, 64)


def against_host_encoder(planner, fp, tag):
    res = planner.plan(fp)
    planner.set_wire_names(fp)
    doc, info = planner.plan_wire()
    want = wire.ResultEncoder(fp.part_names, fp.node_names, fp.state_names).encode(res)
    assert info["need"] == len(doc) == len(want), tag
    assert doc == want, tag
    return res, doc


@pytest.mark.parametrize("hierarchy", [True, False])
def test_mid_size_rebalance(planner, hierarchy):
    P, N = 4096, 128
    fp1 = synth.config5_initial(P, N, hierarchy=hierarchy)
    fp = named(synth.config5_rebalance(fp1, planner.plan(fp1), P, N, hierarchy=hierarchy))
    res, doc = against_host_encoder(planner, fp, ("mid size", hierarchy))
    check_document(fp, res, doc, ("mid size", hierarchy))


def test_config3_65536(planner):
    """Many workgroups, a few megabytes of document, numeric names: the order of the document is far from id order."""
    P, N = 65536, 1024
    fp = named(synth.config_flat(3, P=P, N=N))
    assert fp.part_names[:3] == ["0", "1", "2"]
    res, doc = against_host_encoder(planner, fp, "config 3")
    assert len(doc) > 4 << 20
    keys = top_keys(doc)
    assert len(keys) == P and keys == sorted(keys) and keys[:3] == [b"0", b"1", b"10"]
    first = json.loads(doc)["10"]
    lists = res.lists()[10]
    assert first == {"name": "10", "nodesByState": {s: [fp.node_names[i] for i in lists[m][1].tolist()]
                                                    for m, s in enumerate(fp.state_names) if lists[m][0] != abi.LIST_ABSENT}}
