"""k_stay_by_top's rank function alone (stay_round_ranks, blance_amd/csrc/k_stay.h) under the SIMT emulator: the ranks of a
round of 64 lanes from wave ballots over the bits of the leaf indices, against the definition in plain Python
(tests/stay_rank_tables.py has the cases, the reference and the check; tests/test_stay_ranks_gpu.py runs the same on the
device).  KM = 2 and 4; regions of 1 .. 512 leaves (0 .. 9 bits); rounds of 1, 2, 63 and 64 steps; equal leaves, distinct
leaves, a leaf in two slots of one lane, -1 in single slots and in every slot of a prefix of lanes, the highest leaf in
the first and the last lane, leaves one bit apart, and 288 seeded random rounds."""
import os
import subprocess

import pytest

import stay_rank_tables as T
from test_simt_emulated import HERE, _deps

SRC = os.path.join(HERE, "simt", "emu_stay_rank_cases.cpp")
INC = os.path.join(HERE, "kernels", "stay_rank_cases.inc")
SO = os.path.join(HERE, "simt", "_build", "libblance_emu_stay_rank_cases.so")


def build_emu_rank_cases():
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
def rc():
    return T.RankCases(build_emu_rank_cases())


@pytest.mark.parametrize("size", T.SIZES)
@pytest.mark.parametrize("km", T.KMS)
def test_round_ranks(rc, km, size):
    T.check(rc, km, size)


def test_entry_refuses_leaves_outside_the_region(rc):
    T.check_refusals(rc)


def test_table_exercises_ranks():
    """On the reference alone: most rounds have a rank above 0, and the rounds with one leaf in two slots of a lane have
    ranks of two and more."""
    pos, twice, n = T.table_has_both_kinds()
    assert n > 1000 and 2 * pos > n and twice >= 40, (pos, twice, n)
