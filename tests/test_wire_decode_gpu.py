"""blance_wire_dict_create / blance_wire_decode_device on the MI355X: the kernels of blance_amd/csrc/k_wire_decode.h against
the host decoder carried over to the dictionary's ids, json.loads, the arrays problem.build_problem makes of the same map and
the downloaded plan -- the checks of tests/test_wire_decode_emulated.py (documents and references: tests/wire_decode_cases.py),
every map of at most a few thousand partitions.  The mutants run here because they are green on the emulator and under the
stand-alone sanitizer program (test_wire_decode_emulated.py::test_sanitized_program): they are ordinary API input."""
import json
import os

import pytest

from blance_amd import hip
from test_wire_decode_emulated import (ROOT, run_capacity_and_memory, run_context_undisturbed, run_dictionary, run_fallback,
                                       run_mutants, run_problem_arrays, run_refusals, run_round_trip, run_seams, run_subset)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def planner():
    pl = hip.Planner(device_id=0)
    yield pl
    pl.close()


@pytest.fixture(scope="module")
def wire_cases():
    with open(os.path.join(ROOT, "tests", "golden", "wire_cases.json")) as f:
        return json.load(f)


def test_problem_arrays(planner, golden_cases):
    accepted, reasons = run_problem_arrays(planner, golden_cases)
    assert accepted >= 40, (accepted, reasons)
    assert reasons, "no case exercises a refusal"


def test_round_trip(planner, golden_cases):
    assert run_round_trip(planner, golden_cases) >= 60


def test_subset(planner):
    assert run_subset(planner) > 60


@pytest.mark.parametrize("tile", [64, None])
def test_seams(monkeypatch, tile):
    """BLANCE_WIRE_IN_TILE is read when a context is made: a planner of its own."""
    assert run_seams(lambda: hip.Planner(device_id=0), monkeypatch, tile) > 30


@pytest.mark.parametrize("tile", [64, None])
def test_refusals(monkeypatch, tile, wire_cases):
    run_refusals(lambda: hip.Planner(device_id=0), monkeypatch, tile, wire_cases)


def test_small_stage(monkeypatch):
    """Most workgroups read global memory: a stage of 256 bytes holds two or three records."""
    monkeypatch.setenv("BLANCE_WIRE_IN_STAGE", "256")
    assert run_seams(lambda: hip.Planner(device_id=0), monkeypatch, 64) > 30


def test_capacity_and_memory(planner):
    run_capacity_and_memory(planner, hip.HostArena())


def test_dictionary(planner):
    other = hip.Planner(device_id=0)
    try:
        run_dictionary(planner, other)
    finally:
        other.close()


def test_context_undisturbed(planner):
    run_context_undisturbed(planner, 3000, 64)


def test_fallback(planner):
    run_fallback(planner)


def test_mutants(planner):
    assert run_mutants(planner) >= 400
