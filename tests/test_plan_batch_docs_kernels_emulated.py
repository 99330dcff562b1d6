"""k_batch_decode alone under the SIMT emulator (blance_amd/csrc/k_batch_decode.h), on documents, dictionary blocks and packed
input slices made by hand (tests/batch_decode_cases.py has the cases, the definition and the check;
tests/test_plan_batch_docs_kernels_gpu.py runs the same on the device).  The record split is compared with the sequential
definition of tests/wire_decode_cases.py for every document; parse, place and sum with numpy on what json.loads makes of the
document; every word the kernel does not own must come back as the poison it went in with.  Below them the same cases in a
stand-alone program under AddressSanitizer and UBSan."""
import os
import subprocess

import pytest

import batch_decode_cases as K
from test_simt_emulated import HERE, _deps

SRC = os.path.join(HERE, "simt", "emu_batch_decode_cases.cpp")
INC = os.path.join(HERE, "kernels", "batch_decode_cases.inc")
SO = os.path.join(HERE, "simt", "_build", "libblance_emu_batch_decode_cases.so")
WORLDS = K.worlds()


def build_emu_batch_decode_cases():
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
def lib():
    import ctypes
    return ctypes.CDLL(build_emu_batch_decode_cases())


@pytest.mark.parametrize("name", sorted(WORLDS))
def test_kernel_against_the_definition(lib, name):
    K.check(lib, WORLDS[name])


def test_entry_refuses_blocks_out_of_bounds(lib):
    """The entry checks every offset before it launches: nothing out of bounds reaches the kernel."""
    w = WORLDS["empty_documents"]
    for field, j, at, value in (("shape", 0, 4, 1 << 28), ("ddesc", 1, 9, 1 << 28), ("ddesc", 0, 0, 99), ("shape", 1, 2, 257),
                                ("ddesc", 0, 10, 0), ("ddesc", 1, 2, 8), ("ddesc", 0, 3, 1 << 28)):
        keep = getattr(w, field)[j][at]
        getattr(w, field)[j][at] = value
        try:
            with pytest.raises(AssertionError):
                w.run(lib)
        finally:
            getattr(w, field)[j][at] = keep
    K.check(lib, w)


def test_cases_are_not_vacuous():
    w = WORLDS["long_lists_and_duplicates"]
    sums = w.expected()[4].reshape(-1, K.SUM)
    assert (sums[:, 8] != K.INT_MAX).sum() >= 2 and (sums[:, 7] != K.INT_MAX).sum() >= 1 and (sums[:, 6] != K.INT_MAX).sum() >= 2
    assert len(WORLDS["chunks"].problems[0].doc) > 3 * 256 * 64
    assert {len(pb.doc) % 16 for pb in WORLDS["residues"].problems} == set(range(16))
    assert len({pb.refusal[0] for pb in WORLDS["refused"].problems}) >= 8


ASAN_SRC = os.path.join(HERE, "simt", "batch_decode_asan_main.cpp")
ASAN_EXE = os.path.join(HERE, "simt", "_build", "batch_decode_asan")
SANITIZE = ["-fsanitize=address,undefined", "-static-libasan", "-static-libubsan"]     # the runtimes inside the program


def build_asan_program():
    """The program, or None with the linker's or the runtime's words when a sanitized program does not link or start here."""
    import fcntl
    deps = _deps() + [ASAN_SRC, INC]
    os.makedirs(os.path.dirname(ASAN_EXE), exist_ok=True)
    with open(ASAN_EXE + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not os.path.exists(ASAN_EXE) or any(os.path.getmtime(d) > os.path.getmtime(ASAN_EXE) for d in deps):
            probe = subprocess.run(["g++"] + SANITIZE + ["-x", "c++", "-", "-o", ASAN_EXE + ".probe"],
                                   input="int main(){return 0;}\n", capture_output=True, text=True)
            if probe.returncode != 0:
                return None, probe.stderr[-400:]
            started = subprocess.run([ASAN_EXE + ".probe"], capture_output=True, text=True)      # (in the environment as it is)
            os.remove(ASAN_EXE + ".probe")
            if started.returncode != 0:
                return None, "the program does not start: " + started.stderr[-400:]
            tmp = "%s.%d.tmp" % (ASAN_EXE, os.getpid())
            subprocess.check_call(["g++", "-x", "c++", "-std=c++17", "-O1", "-g1"] + SANITIZE + ["-fno-sanitize-recover=undefined",
                                   "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wno-unknown-pragmas", "-o", tmp, ASAN_SRC])
            os.replace(tmp, ASAN_EXE)
    return ASAN_EXE, ""


def test_sanitized_program(tmp_path):
    """Every world through a stand-alone program under AddressSanitizer and UBSan, every block of exactly its size on the
    heap: a read or a write one byte outside is reported; every block afterwards is the definition's."""
    exe, why = build_asan_program()
    if exe is None:
        pytest.skip("-fsanitize=address does not link or start on this machine: " + why)
    path = tmp_path / "cases.txt"
    K.write_program_input(str(path), WORLDS)
    env = dict(os.environ)                                                           # as it is, plus the two sanitizers' options
    env["ASAN_OPTIONS"] = "detect_leaks=0:detect_stack_use_after_return=0:abort_on_error=1"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    got = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600, env=env)
    assert got.returncode == 0, got.stdout[-300:] + got.stderr[-4000:]
    assert "AddressSanitizer" not in got.stderr and "runtime error" not in got.stderr, got.stderr[-4000:]
    assert got.stdout.strip().split("\n")[-1] == "ran %d cases, 0 wrong" % len(WORLDS)
