"""k_period_find alone under the SIMT emulator (blance_amd/csrc/k_period.h): its known mode -- the period counted from the
region's alive leaves, no record read -- against its searched mode and against the definition, on hand-made region tables and
records (tests/period_case_tables.py has the cases, the reference and the check; tests/test_period_cases_gpu.py runs the same
on the device).  Regions of 1, 16, 120, 192 and 4,096 alive leaves; leaves without a node, with a dead node, with a node
outside the cluster's ids; fewer steps than nodes, as many, one more, none; lengths that are no multiple of the period; chains
that start inside the cycle; one region and three."""
import os
import subprocess

import pytest

import period_case_tables as T
from test_simt_emulated import HERE, _deps

SRC = os.path.join(HERE, "simt", "emu_period_cases.cpp")
INC = os.path.join(HERE, "kernels", "period_cases.inc")
SO = os.path.join(HERE, "simt", "_build", "libblance_emu_period_cases.so")


def build_emu_period_cases():
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
def pc():
    return T.PeriodCases(build_emu_period_cases())


@pytest.mark.parametrize("name", list(T.TABLES))
def test_known_mode_is_the_search(pc, name):
    T.check(pc, name)


def test_entry_refuses_tables_out_of_bounds(pc):
    T.check_refusals(pc)


def test_reference_is_the_search_in_plain_python():
    """On the tables alone: the reference's T is the smallest t whose record equals the first step's in words 1..23."""
    for name in T.TABLES:
        regions, arrays, want = T.table(name)
        reg_off, crec = arrays[2], arrays[7].reshape(-1, T.KCW)
        for r, region in enumerate(regions):
            rec = crec[reg_off[r]:reg_off[r + 1], 1:]
            found = next((t for t in range(1, min(region.length - 1, T.CAP) + 1) if (rec[t] == rec[0]).all()), T.INT_MAX)
            assert found == want[r][0], (name, r, found, want[r])
