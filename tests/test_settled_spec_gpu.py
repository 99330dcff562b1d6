"""The settled top-state pass left on the device (DESIGN.md 4.5 "The host's shortcuts") on an MI355X: the cases of
tests/test_settled_spec_emulated.py, and config 3 at its full size with BLANCE_SPECULATE=1, 0 and fail against
tests/golden/config_digests.json."""
import json
import os

import pytest

from blance_amd import hip, synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _oracle(fp):
    from oracle import loader
    return loader.plan(fp)


def _plan(fp, spec, monkeypatch, **kw):
    monkeypatch.setenv("BLANCE_SPECULATE", spec)
    pl = hip.Planner(device_id=0, **kw)
    try:
        return pl.plan(fp)
    finally:
        pl.close()


def _same(got, want, tag):
    assert (got.digest(), got.iterations, got.n_warnings) == (want.digest(), want.iterations, want.n_warnings), tag


def test_config3_shapes(monkeypatch):
    """Config 3's shape at reduced sizes: the same map in every mode; 4 round trips with the shortcuts on, 13 off."""
    for P, N in ((16384, 256), (131072, 1024)):
        fp = synth.config_flat(3, P=P, N=N)
        want = _oracle(fp)
        syncs = {}
        for spec in ("1", "0", "fail"):
            got = _plan(fp, spec, monkeypatch, chain_min_parts=64)
            _same(got, want, (P, N, spec))
            syncs[spec] = got.struct.host_syncs
        assert syncs["1"] == 4 and syncs["0"] == 13, (P, N, syncs)


def test_config2_shape(monkeypatch):
    fp = synth.config_flat(2, P=65536, N=256)
    want = _oracle(fp)
    for spec in ("1", "0", "fail"):
        _same(_plan(fp, spec, monkeypatch), want, spec)


@pytest.mark.parametrize("which", ["rebalance", "named_weighted"])
def test_refuted_for_real(monkeypatch, which):
    """Later sweeps whose top-state pass moves steps: refuted by the device's word, run again, the oracle's map."""
    fp = synth.config3_named_weighted_flat(16384, 512)
    if which == "rebalance":
        fp = synth.config3_rebalance_flat(fp, _oracle(fp))
    want = _oracle(fp)
    for spec in ("1", "0", "fail"):
        _same(_plan(fp, spec, monkeypatch, chain_min_parts=64), want, (which, spec))


def test_config3_full_size_every_mode(monkeypatch):
    with open(os.path.join(HERE, "golden", "config_digests.json")) as f:
        want = json.load(f)["config3"]
    fp = synth.config_flat(3)
    syncs = {}
    for spec in ("1", "0", "fail"):
        monkeypatch.setenv("BLANCE_SPECULATE", spec)
        pl = hip.Planner(device_id=0)
        try:
            for rep in range(2 if spec == "1" else 1):
                got = pl.plan(fp)
                assert (got.iterations, got.n_warnings, got.digest()) == (want["iterations"], want["warnings"], want["digest"]), (spec, rep)
        finally:
            pl.close()
        syncs[spec] = got.struct.host_syncs
    assert syncs["1"] == 4 and syncs["0"] == 13, syncs
