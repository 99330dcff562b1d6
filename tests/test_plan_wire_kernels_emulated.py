"""k_wire_size and k_wire_write under the SIMT emulator on lists made by hand, for the one branch no plan reaches: a nil
list, written as `null`.  removeNodesFromNodesByState (plan.go:408-421) always returns slices, and neither the golden cases
(0 nil lists among 68 plans) nor hand-made problems with nil lists in prevMap and partitionsToAssign gave a result with one
(tests/test_plan_wire_emulated.py has the plans).  The kernels must still agree with the host encoder on such a map."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from blance_amd import wire
from test_simt_emulated import HERE, _deps

SRC = os.path.join(HERE, "simt", "emu_wire_cases.cpp")
SO = os.path.join(HERE, "simt", "_build", "libblance_emu_wire_cases.so")
ABSENT, NIL, SET = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    deps = _deps() + [SRC]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.check_call(["g++", "-x", "c++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off",
                               "-Wno-unknown-pragmas", "-o", SO, SRC])
    so = ctypes.CDLL(SO)
    so.emu_case_wire.restype = ctypes.c_longlong
    return so


def _escaped(strs, tail=b""):
    """What blance_plan_wire_names keeps of names that need no escape: the quoted strings and their offsets."""
    parts = [b'"' + s.encode() + b'"' + tail for s in strs]
    off = np.zeros(len(parts) + 1, np.int32)
    off[1:] = np.cumsum([len(x) for x in parts])
    return ctypes.create_string_buffer(b"".join(parts) + b"\0"), off


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.mark.parametrize("P,stage", [(1, 32768), (7, 32768), (300, 32768), (300, 128)])
def test_nil_lists(lib, P, stage):
    M, L, NX = 3, 2, 5
    parts = ["p%04d" % p for p in range(P)]                     # in byte order already
    states, nodes = ["a", "b", "c"], ["n%d" % i * (1 + i % 2) for i in range(NX)]
    rng = np.random.RandomState(P)
    kind = rng.choice([ABSENT, NIL, SET], size=P * M).astype(np.uint8)
    kind[:3] = [NIL, NIL, NIL]                                  # a partition of nil lists only, in front
    kind[-1] = NIL                                              # ... and `null` as the document's last value
    length = rng.randint(0, L + 1, size=P * M).astype(np.int32)
    lists = rng.randint(0, NX, size=P * M * L).astype(np.int32)
    pmap = {}
    for p, name in enumerate(parts):
        nbs = {}
        for m, s in enumerate(states):
            i = p * M + m
            if kind[i] != ABSENT:
                nbs[s] = None if kind[i] == NIL else [nodes[x] for x in lists[i * L:i * L + length[i]]]
        pmap[name] = {"name": name, "nodesByState": nbs}
    want = wire.encode(pmap)
    assert want.count(b"null") >= 3
    pbuf, poff = _escaped(parts)
    nbuf, noff = _escaped(nodes)
    sbuf, soff = _escaped(states, b":")
    raw = np.full(len(want) + 64 + 16, 0xAB, np.uint8)
    skip = (-raw.ctypes.data) % 16                              # the document buffer is 16-byte aligned on the device
    doc = raw[skip:skip + len(want) + 32]
    n = lib.emu_case_wire(P, M, L, NX, pbuf, _p(poff), nbuf, _p(noff), sbuf, _p(soff), _p(lists), _p(length), _p(kind),
                          stage, _p(doc), ctypes.c_longlong(len(want)))
    assert n == len(want)
    assert doc[:n].tobytes() == want
    assert (doc[n:] == 0xAB).all()
