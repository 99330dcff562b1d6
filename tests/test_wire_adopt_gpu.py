"""blance_wire_adopt on the MI355X: the cases and checks of tests/test_wire_adopt_emulated.py (tests/wire_adopt_cases.py)
through libblance_hip.so, and the two kernels alone through the entry compiled by hipcc for gfx950
(tests/kernels/wire_adopt_cases.hip -> libblance_wire_adopt_cases.so, made by __graft_entry__.build_wire_adopt_cases).

They run in ONE child process (tests/wire_adopt_gpu_child.py), started once per module and under a timeout; every test here
reads its family's answer.  Why a child: as tests/test_adopt_gpu.py says -- three contexts, more for the
refusals, communicator callbacks and a second code-object library stay out of the process that runs the rest of the suite."""
import json
import os
import subprocess
import sys

import pytest

import wire_adopt_gpu_child as child

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("wire_adopt_gpu") / "answers.json")
    p = subprocess.run([sys.executable, os.path.join(HERE, "wire_adopt_gpu_child.py"), out], capture_output=True, text=True, timeout=900)
    got = {}
    if os.path.exists(out):
        with open(out) as f:
            got = json.load(f)
    return p, got


@pytest.mark.parametrize("family", child.NAMES)
def test_family(answers, family):
    p, got = answers
    assert family in got, "the child ended (status %d) before this family:\n%s" % (p.returncode, p.stderr[-3000:])
    assert got[family] == "ok", got[family]


def test_child_ran_every_family(answers):
    p, got = answers
    assert p.returncode == 0 and sorted(got) == sorted(child.NAMES), p.stderr[-3000:]
