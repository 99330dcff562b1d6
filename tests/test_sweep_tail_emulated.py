"""The sweep's tail in one kernel (DESIGN.md 4.5 "The sweep's tail"): k_sweep_tail applies the last pass's list edits, tests
for convergence, writes prevMap back, and counts the next sweep's stateNodeCounts and kinds ahead.  Under the SIMT emulator,
against the C oracle, with BLANCE_FUSED_TAIL=1 (default) and 0 (the unfused k_scatter / k_converge / k_live_refresh /
k_count_prev sequence), each under BLANCE_SPECULATE=1, 0 and fail."""
import pytest

from blance_amd import hip, problem, synth
from helpers import build_from_case
from randgen import random_case, random_regular_case
from test_simt_emulated import _oracle, emu_lib  # noqa: F401  (the fixture)

MODES = [(fused, spec) for fused in ("1", "0") for spec in ("1", "0", "fail")]


def _planner(lib, monkeypatch, fused, spec, **kw):
    monkeypatch.setenv("BLANCE_FUSED_TAIL", fused)
    monkeypatch.setenv("BLANCE_SPECULATE", spec)
    monkeypatch.delenv("BLANCE_TRACE", raising=False)
    return hip.Planner(lib_path=lib, **kw)


def _same(got, want, tag):
    assert (got.digest(), got.iterations, got.n_warnings) == (want.digest(), want.iterations, want.n_warnings), tag


def test_golden_cases_every_mode(emu_lib, golden_cases, monkeypatch):
    wants = [_oracle(build_from_case(c)) for c in golden_cases]
    for fused, spec in MODES:
        pl = _planner(emu_lib, monkeypatch, fused, spec)
        try:
            for c, want in zip(golden_cases, wants):
                _same(pl.plan(build_from_case(c)), want, (c["source"], fused, spec))
        finally:
            pl.close()


def test_random_cases_every_mode(emu_lib, monkeypatch):
    """Small random cases: nil lists and absent keys in prevMap (the result's kinds come from prevMap as written back),
    partition weights, nodesToRemove / nodesToAdd, and plans cut short by MaxIterationsPerPlan (1 and 2 sweeps)."""
    cases = [random_case(s) for s in range(40)] + [random_regular_case(s) for s in range(20)]
    fps = []
    for c in cases:
        for mi in (10, 2, 1):
            try:
                fps.append(build_from_case(c, max_iterations=mi))
            except problem.Unsupported:                     # (inputs the reference panics on)
                break
    assert len(fps) > 100
    wants = [_oracle(fp) for fp in fps]
    for fused, spec in MODES:
        pl = _planner(emu_lib, monkeypatch, fused, spec)
        try:
            for i, (fp, want) in enumerate(zip(fps, wants)):
                _same(pl.plan(fp), want, (i, fused, spec))
        finally:
            pl.close()


def test_config3_shape_fewer_launches(emu_lib, monkeypatch):
    """Config 3's shape: the same map in every mode; with the fused tail, no k_live_refresh / k_count_prev in sweeps 2 and
    3 and one launch for the tail's three: fewer launches, the same four round trips."""
    fp = synth.config_flat(3, P=16384, N=256)
    want = _oracle(fp)
    launches, syncs = {}, {}
    for fused, spec in MODES:
        pl = _planner(emu_lib, monkeypatch, fused, spec, chain_min_parts=64)
        try:
            got = pl.plan(fp)
        finally:
            pl.close()
        _same(got, want, (fused, spec))
        launches[fused, spec] = got.struct.kernel_launches
        syncs[fused, spec] = got.struct.host_syncs
    assert syncs["1", "1"] == syncs["0", "1"] == 4, syncs
    assert launches["1", "1"] < launches["0", "1"], launches


@pytest.mark.parametrize("which", ["rebalance", "named_weighted"])
def test_refuted_after_the_tail_was_enqueued(emu_lib, monkeypatch, which):
    """Later sweeps whose top-state pass moves steps: the tail was enqueued behind the refuted word and wrote nothing (not
    the second counter buffer either); the sweep runs again and its tail then counts.  Weighted partitions: counter parity."""
    fp = synth.config3_named_weighted_flat(4096, 256)
    if which == "rebalance":
        fp = synth.config3_rebalance_flat(fp, _oracle(fp))
    want = _oracle(fp)
    for fused, spec in MODES:
        pl = _planner(emu_lib, monkeypatch, fused, spec, chain_min_parts=64)
        try:
            _same(pl.plan(fp), want, (which, fused, spec))
        finally:
            pl.close()

