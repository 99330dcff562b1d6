"""k_cycle_group and k_cycle_top alone under the SIMT emulator (blance_amd/csrc/k_cycle.h) against the launches they stand for,
on the hand-made worlds of tests/cycle_case_tables.py: one alive node; a region with one alive node, with none; fewer steps
than nodes; a last cycle that ends inside a region; a ragged last region; leaves without a node; nodes with 1, 63, 64 and 65
steps; events and orphans; a closed gate; the `refute` knob; a step off the round robin.  tests/test_cycle_cases_gpu.py runs
the same on the device."""
import os
import subprocess

import pytest

import cycle_case_tables as T
from test_simt_emulated import HERE, _deps

SRC = os.path.join(HERE, "simt", "emu_cycle_cases.cpp")
INC = os.path.join(HERE, "kernels", "cycle_cases.inc")
SO = os.path.join(HERE, "simt", "_build", "libblance_emu_cycle_cases.so")


def build_emu_cycle_cases():
    """The emulator library with the entry.  Workers of one run take turns at a lock: one compiles, under a name of its own
    that is moved into place whole, the others find it made."""
    import fcntl
    deps = _deps() + [SRC, INC]
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    with open(SO + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
            tmp = "%s.%d.tmp" % (SO, os.getpid())
            subprocess.check_call(["g++", "-x", "c++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off",
                                   "-Wno-unknown-pragmas", "-o", tmp, SRC])
            os.replace(tmp, SO)
    return SO


@pytest.fixture(scope="module")
def cc():
    return T.CycleCases(build_emu_cycle_cases())


@pytest.mark.parametrize("name", list(T.WORLDS))
def test_tables_give_the_sorts(cc, name):
    T.check(cc, name)


def test_events_and_orphans(cc):
    T.check_events_and_orphans(cc)


def test_closed_gate_writes_nothing(cc):
    T.check_closed_gate(cc)


def test_refute_knob_raises_not_local_only(cc):
    T.check_refute(cc)


def test_step_off_the_round_robin(cc):
    T.check_premise(cc)


def test_entry_refuses_tables_out_of_bounds(cc):
    T.check_refusals(cc)
