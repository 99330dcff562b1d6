"""The sweep's tail in one kernel (DESIGN.md 4.5 "The sweep's tail") on an MI355X: config 3 at reduced and full size, and
later sweeps whose top-state pass is refuted behind an enqueued tail, with BLANCE_FUSED_TAIL=1 and 0 under every
BLANCE_SPECULATE mode, against the C oracle and tests/golden/config_digests.json."""
import json
import os

import pytest

from blance_amd import hip, synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MODES = [(fused, spec) for fused in ("1", "0") for spec in ("1", "0", "fail")]


def _oracle(fp):
    from oracle import loader
    return loader.plan(fp)


def _planner(monkeypatch, fused, spec, **kw):
    monkeypatch.setenv("BLANCE_FUSED_TAIL", fused)
    monkeypatch.setenv("BLANCE_SPECULATE", spec)
    return hip.Planner(device_id=0, **kw)


def _same(got, want, tag):
    assert (got.digest(), got.iterations, got.n_warnings) == (want.digest(), want.iterations, want.n_warnings), tag


@pytest.mark.parametrize("which", ["config3", "rebalance", "named_weighted"])
def test_reduced_shapes_every_mode(monkeypatch, which):
    if which == "config3":
        fp = synth.config_flat(3, P=131072, N=1024)
    else:
        fp = synth.config3_named_weighted_flat(16384, 512)
        if which == "rebalance":
            fp = synth.config3_rebalance_flat(fp, _oracle(fp))
    want = _oracle(fp)
    for fused, spec in MODES:
        pl = _planner(monkeypatch, fused, spec, chain_min_parts=64)
        try:
            for rep in range(2):                               # (a second plan on the same context: the buffers swapped back)
                _same(pl.plan(fp), want, (which, fused, spec, rep))
        finally:
            pl.close()


def test_config3_full_size(monkeypatch):
    with open(os.path.join(HERE, "golden", "config_digests.json")) as f:
        want = json.load(f)["config3"]
    fp = synth.config_flat(3)
    launches = {}
    for fused in ("1", "0"):
        pl = _planner(monkeypatch, fused, "1")
        try:
            for rep in range(2):
                got = pl.plan(fp)
                assert (got.iterations, got.n_warnings, got.digest()) == (want["iterations"], want["warnings"], want["digest"]), (fused, rep)
        finally:
            pl.close()
        assert got.struct.host_syncs == 4, fused
        launches[fused] = got.struct.kernel_launches
    assert launches["1"] < launches["0"], launches
