"""The host driver's decisions, pinned (DESIGN.md 4.5 "The host's shortcuts"): for four shapes, under BLANCE_SPECULATE=1, 0
and fail and BLANCE_FUSED_TAIL=1 and 0, the sweeps, round trips, launches and the kind of every pass the sweep driver of
blance_hip.hip chose -- the numbers a restructuring of that driver must leave alone.  Under the SIMT emulator, each planner
fresh, chain_min_parts=64 and no BLANCE_TRACE (the trace reads back more).

Run as a program it prints the same rows for the product library (the device's values need not equal the emulator's: a
change is checked by comparing the output before and after it)."""
import os

import pytest

from blance_amd import hip, synth

FIELDS = ("iterations", "converged", "n_warnings", "host_syncs", "kernel_launches", "steps_total", "steps_batched",
          "pass_kernel_launches", "flat_passes", "blank_pass_launches", "stay_pass_launches")
MODES = [(spec, fused) for spec in ("1", "0", "fail") for fused in ("1", "0")]


def _oracle(fp):
    from oracle import loader
    return loader.plan(fp)


def _c3():
    return synth.config_flat(3, P=4096, N=256)


def _c3_rebalance():
    fp = _c3()
    return synth.config3_rebalance_flat(fp, _oracle(fp))


SHAPES = {
    "c3": _c3,
    "c3_rebalance": _c3_rebalance,
    "c5_initial": lambda: synth.config5_initial(3000, 128),
    "c2": lambda: synth.config_flat(2, P=8192, N=64),
}

# shape -> (iterations, converged, n_warnings), host_syncs by BLANCE_SPECULATE, kernel_launches in the order of MODES,
# (steps_total, steps_batched), (pass_kernel_launches, flat_passes, blank_pass_launches, stay_pass_launches)
EXPECTED = {
    "c3": ((3, 1, 0), {"1": 4, "0": 13, "fail": 17}, (95, 102, 98, 105, 178, 189), (24576, 24576), (3, 3, 1, 1)),
    "c3_rebalance": ((4, 1, 0), {"1": 14, "0": 22, "fail": 31}, (126, 136, 120, 130, 225, 240), (32768, 32000), (4, 4, 0, 0)),
    "c5_initial": ((3, 1, 0), {"1": 30, "0": 30, "fail": 30}, (147, 148, 149, 150, 147, 148), (18000, 17488), (2, 4, 0, 0)),
    "c2": ((2, 1, 0), {"1": 5, "0": 9, "fail": 5}, (50, 50, 61, 61, 50, 50), (32768, 32768), (0, 4, 0, 0)),
}

_problems = {}


def _problem(shape):
    if shape not in _problems:
        fp = SHAPES[shape]()
        _problems[shape] = (fp, _oracle(fp))
    return _problems[shape]


def _row(lib, fp, spec, fused, trace=False):
    """One plan on a fresh planner in the given mode: (the result, its FIELDS)."""
    saved = {k: os.environ.get(k) for k in ("BLANCE_SPECULATE", "BLANCE_FUSED_TAIL", "BLANCE_TRACE")}
    os.environ["BLANCE_SPECULATE"] = spec
    os.environ["BLANCE_FUSED_TAIL"] = fused
    os.environ.pop("BLANCE_TRACE", None)
    if trace:
        os.environ["BLANCE_TRACE"] = "1"
    try:
        pl = hip.Planner(lib_path=lib, chain_min_parts=64) if lib else hip.Planner(chain_min_parts=64)
        try:
            got = pl.plan(fp)
        finally:
            pl.close()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return got, tuple(int(getattr(got.struct, f)) for f in FIELDS)


@pytest.fixture(scope="module")
def emu_lib():
    from test_simt_emulated import build_emu
    return build_emu()


@pytest.mark.parametrize("spec,fused", MODES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_decisions(emu_lib, shape, spec, fused):
    fp, want = _problem(shape)
    head, syncs, launches, steps, kinds = EXPECTED[shape]
    got, row = _row(emu_lib, fp, spec, fused)
    assert got.digest() == want.digest(), (shape, spec, fused)
    assert row == head + (syncs[spec], launches[MODES.index((spec, fused))]) + steps + kinds, (shape, spec, fused, row)


def test_flat_pass_leaves_the_chain_flags_alone(emu_lib, capfd):
    """Config 3's shape with two primaries: the top state's flat bulk pass (k = 2) runs a fresh run with exclusions, whose
    scan words and `bad` word (INT_MAX when nothing is bad) once lay on the chain flags; the replica's chain pass of the
    same sweep then skipped its memset (the flags counted as clean) and read an orphan count of INT_MAX."""
    c = synth.config_case(3, P=4096, N=256)
    c["modelStateConstraints"] = {"primary": 2, "replica": 2}
    fp = synth.case_to_flat(c)
    want = _oracle(fp)
    capfd.readouterr()
    got, _ = _row(emu_lib, fp, "1", "1", trace=True)
    err = capfd.readouterr().err
    assert (got.digest(), got.iterations, got.n_warnings) == (want.digest(), want.iterations, want.n_warnings)
    passes = [l for l in err.splitlines() if l.startswith("[blance] chain pass state") and "orphans" in l]
    assert passes, err[-2000:]
    assert "orphans 2147483647" not in err, passes
    assert passes[0].endswith("orphans 0"), passes[0]


if __name__ == "__main__":
    for name in SHAPES:
        problem_, _ = _problem(name)
        for spec_, fused_ in MODES:
            print(name, "spec=" + spec_, "fused=" + fused_, *_row(None, problem_, spec_, fused_)[1], flush=True)
