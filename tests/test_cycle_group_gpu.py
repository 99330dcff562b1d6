"""The whole plans of tests/test_cycle_group_emulated.py on an MI355X (tests/cycle_group_cases.py): the chain pass behind a
round robin grouped from the upload's tables, against the C oracle, with the shortcut on, off and refuted."""
import pytest

import cycle_group_cases as G

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(G.CASES))
def test_cycle_group_plans(monkeypatch, capfd, name):
    G.check(None, name, monkeypatch, capfd)


@pytest.mark.parametrize("name", G.REFUTE)
def test_refuted_premise(monkeypatch, capfd, name):
    G.check_refuted(None, name, monkeypatch, capfd)


def test_second_plan_and_second_upload(monkeypatch, capfd):
    G.check_second_plan_and_upload(None, monkeypatch, capfd)


def test_planner_keyword_switches_it_off(monkeypatch, capfd):
    G.check_switches(None, monkeypatch, capfd)


def test_two_nodes_share_a_leaf(monkeypatch, capfd):
    G.check_shared_leaf(None, monkeypatch, capfd)
