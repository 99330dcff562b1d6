"""The periodic first pass with its period taken from the round robin of the pass before (k_period_find's known mode, DESIGN.md
4.1c), whole plans under the SIMT emulator: every case of tests/period_known_cases.py against the C oracle, under
BLANCE_SPECULATE = 1, 0 and fail, with BLANCE_PERIOD_KNOWN on and off.  tests/test_period_known_gpu.py runs the same on the
device; tests/test_period_cases_emulated.py has the kernel alone."""
import pytest

import period_known_cases as K
from test_simt_emulated import emu_lib  # noqa: F401  (the fixture)


@pytest.mark.parametrize("name", list(K.CASES))
def test_period_known_plans(emu_lib, monkeypatch, capfd, name):
    K.check(emu_lib, name, monkeypatch, capfd)


def test_planner_keyword_switches_it_off(emu_lib, monkeypatch, capfd):
    """hip.Planner(period_known=False) is BLANCE_PERIOD_KNOWN=0; the variable, when set, decides."""
    fp = K.tree_case(4096, 256, 16, 8)
    want = K.oracle(fp)
    monkeypatch.setenv("BLANCE_TRACE", "1")
    monkeypatch.delenv("BLANCE_PERIOD_KNOWN", raising=False)
    monkeypatch.delenv("BLANCE_SPECULATE", raising=False)
    from blance_amd import hip
    for kw, env, n in (({}, None, 1), ({"period_known": False}, None, 0), ({"period_known": False}, "1", 1), ({}, "0", 0)):
        if env is None:
            monkeypatch.delenv("BLANCE_PERIOD_KNOWN", raising=False)
        else:
            monkeypatch.setenv("BLANCE_PERIOD_KNOWN", env)
        capfd.readouterr()
        pl = hip.Planner(lib_path=emu_lib, chain_min_parts=8, **kw)
        try:
            got = pl.plan(fp)
        finally:
            pl.close()
        err = capfd.readouterr().err
        assert got.digest() == want.digest() and err.count(K.KNOWN) == n, (kw, env, err.count(K.KNOWN))
