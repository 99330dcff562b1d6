"""The settled top-state pass left on the device (DESIGN.md 4.5 "The host's shortcuts"): from the second sweep on, the first
pass of a sweep -- the top state's flat pass -- is taken to be one run of stays without reading its stay test back; every
launch behind it waits for the test's word, and the word comes back with the sweep's convergence word.  Under the SIMT
emulator, against the oracle, with BLANCE_SPECULATE=1, 0 and fail."""
import pytest

from blance_amd import hip, synth
from test_simt_emulated import _oracle, emu_lib  # noqa: F401  (the fixture)


def _plan(lib, fp, spec, monkeypatch, trace=False):
    monkeypatch.setenv("BLANCE_SPECULATE", spec)
    if trace:
        monkeypatch.setenv("BLANCE_TRACE", "1")
    else:
        monkeypatch.delenv("BLANCE_TRACE", raising=False)
    pl = hip.Planner(lib_path=lib, chain_min_parts=64)
    try:
        return pl.plan(fp)
    finally:
        pl.close()


def _same(got, want, tag):
    assert (got.digest(), got.iterations, got.n_warnings) == (want.digest(), want.iterations, want.n_warnings), tag


REFUTED = "was not one run of stays: the sweep runs again"
STANDS = "the first pass was one run of stays"


def test_config3_settled_sweeps(emu_lib, monkeypatch, capfd):
    """Config 3's shape: sweeps 2 and 3 open with a settled primary pass, the replica's chain pass and (sweep 3) its
    k_stay_by_top verdict share the sweep's one readback with it: four round trips instead of six; 13 with the shortcuts off."""
    fp = synth.config_flat(3, P=16384, N=256)
    want = _oracle(fp)
    syncs = {}
    for spec in ("1", "0", "fail"):
        got = _plan(emu_lib, fp, spec, monkeypatch, trace=True)
        err = capfd.readouterr().err
        _same(got, want, spec)
        if spec != "fail":                                            # (counted without the trace: it reads back more)
            syncs[spec] = _plan(emu_lib, fp, spec, monkeypatch).struct.host_syncs
        if spec == "1":
            assert err.count(STANDS) == 2 and REFUTED not in err, err[-2000:]
            assert got.struct.stay_pass_launches >= 1
        elif spec == "fail":
            assert err.count(REFUTED) == 1, err[-2000:]              # (once: the plan reads the pass back from then on)
        else:
            assert STANDS not in err and REFUTED not in err
    assert syncs["1"] == 4 and syncs["0"] == 13, syncs


def test_config2_shape(emu_lib, monkeypatch):
    """Config 2's shape (both states flat): its later passes read back, so the first pass is read back as before."""
    fp = synth.config_flat(2, P=8192, N=64)
    want = _oracle(fp)
    syncs = {}
    for spec in ("1", "0", "fail"):
        got = _plan(emu_lib, fp, spec, monkeypatch)
        _same(got, want, spec)
        syncs[spec] = got.struct.host_syncs
    assert syncs["1"] < syncs["0"], syncs


@pytest.mark.parametrize("which", ["rebalance", "named_weighted"])
def test_refuted_for_real(emu_lib, monkeypatch, capfd, which):
    """Shapes in which a later sweep's top-state pass does move steps: the assumption is refuted by the device's own word
    (not by BLANCE_SPECULATE=fail), the sweep runs again from its first pass, and the plan is the oracle's."""
    fp = synth.config3_named_weighted_flat(4096, 256)
    if which == "rebalance":
        fp = synth.config3_rebalance_flat(fp, _oracle(fp))
    want = _oracle(fp)
    for spec in ("1", "0", "fail"):
        got = _plan(emu_lib, fp, spec, monkeypatch, trace=True)
        err = capfd.readouterr().err
        _same(got, want, (which, spec))
        if spec == "1":
            assert err.count(REFUTED) == 1, err[-2000:]          # (once: the plan reads the pass back from then on)


def test_config3_rebalance_reduced(emu_lib, monkeypatch):
    """Config 3's rebalance after every tenth node left, at reduced size: later sweeps open with settled passes again."""
    fp = synth.config_flat(3, P=16384, N=256)
    fp2 = synth.config3_rebalance_flat(fp, _oracle(fp))
    want = _oracle(fp2)
    syncs = {}
    for spec in ("1", "0", "fail"):
        got = _plan(emu_lib, fp2, spec, monkeypatch)
        _same(got, want, spec)
        syncs[spec] = got.struct.host_syncs
    assert syncs["1"] < syncs["0"], syncs
