"""Whole plans with k_stay_by_top forced into every chain pass with NumPartitions > 0 ON THE DEVICE, against the C oracle:
the cases, the checks and the pinned tallies of tests/test_stay_plans_emulated.py (tests/stay_plan_cases.py).  The driver's
decisions do not depend on where the kernels run, so the tallies of commit f11090a under the emulator hold here too: a
forced pass that is redone adds a pass-kernel launch and a round trip."""
import pytest

import stay_plan_cases as S
from test_stay_plans_emulated import EXPECTED

pytestmark = pytest.mark.gpu


def _oracle(fp):
    from oracle import loader
    return loader.plan(fp)


@pytest.mark.parametrize("name", sorted(S.CASES))
def test_forced_stay_pass_stands(monkeypatch, name):
    got = S.run(None, name, _oracle, monkeypatch, device=True)
    assert [same for same, _ in got] == [True, True], (name, got)
    assert tuple(t for _, t in got) == EXPECTED[name], (name, got)
