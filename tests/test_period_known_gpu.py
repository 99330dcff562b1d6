"""The whole plans of tests/test_period_known_emulated.py on an MI355X (tests/period_known_cases.py): the period of the
periodic first pass taken from the round robin of the pass before, against the C oracle, with the shortcut on and off."""
import pytest

import period_known_cases as K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(K.CASES))
def test_period_known_plans(monkeypatch, capfd, name):
    K.check(None, name, monkeypatch, capfd)
