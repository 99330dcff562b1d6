"""Whole plans with k_stay_by_top forced into every chain pass with NumPartitions > 0, under the SIMT emulator, against the C
oracle: the problems of tests/stay_plan_cases.py (zones of 16, 32, 128 and 320 leaves; top priority nodes of 1, 63, 64, 65
and 129 steps; one, two and three replicas (both instances of the kernel); with and without node weights; one case behind a hand-off, where replayed lanes run).
Each is planned from nothing and again from its own result.

The plan alone does not tell whether the kernel's ranks are right: a wrong rank makes a stay look like a move, the kernel
raises its flag and the chain kernel quietly redoes the pass.  EXPECTED pins stay_pass_launches, pass_kernel_launches and
host_syncs of both plans to the values of commit f11090a under the emulator (the rank loop over the round's lanes), where
the forced pass stood in every case; a pass that is redone adds a pass-kernel launch and a round trip.
tests/test_stay_plans_gpu.py runs the same on the device."""
import pytest

import stay_plan_cases as S
from test_simt_emulated import _oracle, emu_lib  # noqa: F401  (the fixture)

# name: the tallies (S.FIELDS) of the plan from nothing and of the plan from its result, commit f11090a, SIMT emulator
EXPECTED = {
    "zone16-k2-65": ((2, 4, 7), (1, 1, 3)),
    "zone16-k1-64": ((1, 2, 3), (1, 1, 3)),
    "zone16-k2-129": ((2, 4, 7), (1, 1, 3)),
    "zone16-k1-129w": ((1, 2, 4), (1, 1, 3)),
    "zone32-k2-63": ((2, 4, 7), (1, 1, 3)),
    "zone32-k1-64w": ((1, 2, 4), (1, 1, 3)),
    "zone32-k2-63w": ((2, 3, 5), (1, 1, 3)),
    "zone128-k2-1": ((1, 3, 6), (1, 1, 3)),
    "zone128-k1-1": ((1, 2, 3), (1, 1, 3)),
    "zone128-k2-65w": ((2, 3, 5), (1, 1, 3)),
    "zone32-k3-63w": ((2, 3, 5), (1, 1, 3)),
    "zone128-k3-17": ((1, 3, 6), (1, 1, 3)),
    "zone320-k2": ((1, 3, 6), (1, 1, 3)),
    "zone320-k1w": ((1, 2, 4), (1, 1, 3)),
    "zone128-k2-handoff": ((2, 4, 4), (1, 2, 3)),        # (both plans hand off: a k_stay_by_top launch behind the walk)
}


def test_every_case_is_pinned():
    assert sorted(EXPECTED) == sorted(S.CASES)


@pytest.mark.parametrize("name", sorted(S.CASES))
def test_forced_stay_pass_stands(emu_lib, monkeypatch, name):
    got = S.run(emu_lib, name, _oracle, monkeypatch)
    assert [same for same, _ in got] == [True, True], (name, got)
    assert tuple(t for _, t in got) == EXPECTED[name], (name, got)
