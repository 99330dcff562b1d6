"""Stage 1 of the device decoder alone under the SIMT emulator (blance_amd/csrc/k_wire_decode.h: k_wd_tail, k_wd_quotes,
k_wd_walk -- where the records of a PartitionMap document begin): the kernels' unescaped-quote bits, per-tile quote counts and
depth changes and the record offsets against a definition in plain Python, one sequential walk over the bytes
(tests/wire_decode_cases.py: split_reference), on the seam documents of test_wire_decode_emulated and on 200 random byte strings
over the alphabet `"\\{}[],: a`.  tests/test_wire_decode_kernels_gpu.py runs the same on the device."""
import os
import subprocess

import pytest

import wire_decode_cases as W
from test_simt_emulated import HERE, _deps

SRC = os.path.join(HERE, "simt", "emu_wire_decode_cases.cpp")
INC = os.path.join(HERE, "kernels", "wire_decode_cases.inc")
SO = os.path.join(HERE, "simt", "_build", "libblance_emu_wire_decode_cases.so")


def build_emu_wire_decode_cases():
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
def sc():
    return W.SplitCases(build_emu_wire_decode_cases())


def test_split_is_the_definition(sc):
    assert W.run_split_cases(sc) > 60


def test_entry_refuses_bad_tiles(sc):
    W.check_split_refusals(sc)


def test_definition_on_a_document_by_hand():
    """The definition itself, where the answer is plain: an escaped quote, a brace inside a string, two records.
    (This checks the reference the kernels are compared with: it runs no new kernel and passes without the decoder.)"""
    doc = b'{"a\\"{":{"name":"x"}, "b":null}'
    bits, quotes, depth, starts = W.split_reference(doc, 64)
    assert starts == [1, doc.index(b'"b"')] and quotes == [8] and depth == [0]
    assert bits[3] == 0 and bits[4] == 0 and bits[1] == 1 and sum(bits) == 8
