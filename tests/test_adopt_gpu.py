"""blance_plan_adopt on the MI355X: the cases and checks of tests/test_adopt_emulated.py (tests/adopt_cases.py) through
libblance_hip.so, and the two kernels alone through the entry compiled by hipcc for gfx950 (tests/kernels/adopt_cases.hip ->
libblance_adopt_cases.so, made by __graft_entry__.build_adopt_cases).

They run in ONE child process (tests/adopt_gpu_child.py), started once per module; every test here reads its family's answer.
Why a child: these tests put two contexts, a third for the refusals, communicator callbacks and a second code-object library
into whatever process runs them, and a one-process run of the whole GPU suite that had them in front of
test_hip_parity.py's RCCL tests saw ncclCommInitRank fail there.  What in that process RCCL trips over was not found; the
adoption tests followed by test_hip_parity.py alone pass.  In a process of their own they leave nothing behind, whatever
file order pytest takes."""
import json
import os
import subprocess
import sys

import pytest

import adopt_gpu_child as child

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("adopt_gpu") / "answers.json")
    p = subprocess.run([sys.executable, os.path.join(HERE, "adopt_gpu_child.py"), out], capture_output=True, text=True, timeout=900)
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
