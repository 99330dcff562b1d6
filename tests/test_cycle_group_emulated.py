"""The chain pass behind a round robin grouped from the upload's tables (k_cycle.h), whole plans under the
SIMT emulator: every case of tests/cycle_group_cases.py against the C oracle, under BLANCE_SPECULATE = 1, 0 and fail, with
BLANCE_CYCLE_GROUP on and off; the refuted premise; a second plan and a second upload on one context; the switches.
tests/test_cycle_group_gpu.py runs the same on the device."""
import pytest

import cycle_group_cases as G
from test_simt_emulated import emu_lib  # noqa: F401  (the fixture)


@pytest.mark.parametrize("name", list(G.CASES))
def test_cycle_group_plans(emu_lib, monkeypatch, capfd, name):
    G.check(emu_lib, name, monkeypatch, capfd)


@pytest.mark.parametrize("name", G.REFUTE)
def test_refuted_premise(emu_lib, monkeypatch, capfd, name):
    G.check_refuted(emu_lib, name, monkeypatch, capfd)


def test_second_plan_and_second_upload(emu_lib, monkeypatch, capfd):
    G.check_second_plan_and_upload(emu_lib, monkeypatch, capfd)


def test_planner_keyword_switches_it_off(emu_lib, monkeypatch, capfd):
    G.check_switches(emu_lib, monkeypatch, capfd)


def test_two_nodes_share_a_leaf(emu_lib, monkeypatch, capfd):
    G.check_shared_leaf(emu_lib, monkeypatch, capfd)
