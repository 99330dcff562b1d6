"""k_batch_wire_size and k_batch_wire_write alone under the SIMT emulator (blance_amd/csrc/k_batch_wire.h), on result CSRs and
names blocks made by hand (tests/batch_wire_cases.py has the cases, the definition and the check;
tests/test_plan_batch_wire_kernels_gpu.py runs the same on the device): the two kernels in a row, and each alone on what the other
leaves.  Every word and byte a kernel does not own must come back as the poison it went in with -- the scratch and the output
slices around the offsets and the length word, the 0 to 15 bytes between two documents, everything behind the last.  Below
them the same cases in a stand-alone program under AddressSanitizer and UBSan."""
import os
import subprocess

import pytest

import batch_wire_cases as K
from test_simt_emulated import HERE, _deps

SRC = os.path.join(HERE, "simt", "emu_batch_wire_cases.cpp")
INC = os.path.join(HERE, "kernels", "batch_wire_cases.inc")
SO = os.path.join(HERE, "simt", "_build", "libblance_emu_batch_wire_cases.so")
WORLDS = K.worlds()


def build_emu_batch_wire_cases():
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
    return ctypes.CDLL(build_emu_batch_wire_cases())


@pytest.mark.parametrize("which", [3, 1, 2])
@pytest.mark.parametrize("name", sorted(WORLDS))
def test_kernels_against_the_definition(lib, name, which):
    K.check(lib, WORLDS[name], which)


def test_cases_are_not_vacuous():
    assert K.gaps_seen(WORLDS["every_gap"]) == set(range(16))
    mixed = WORLDS["mixed"]
    assert sum(d is None for d in mixed.docs) == 3 and sum(not pb.ask for pb in mixed.problems) == 1
    both = b"".join(d for d in mixed.docs if d is not None)
    assert b"null" in both and b"[]" in both and b'"nodesByState":{}' in both
    for stage in (64, 128, 256):
        w = WORLDS["stage_%d" % stage]
        offs = [pb.piece_offsets() for pb in w.problems]
        lens = [o[1:] - o[:-1] for o in offs]
        assert max(l.max() for l in lens) > stage - 16 >= min(l.min() for l in lens)     # the first-wave path and the stage


def test_entry_refuses_blocks_out_of_bounds(lib):
    w = WORLDS["skipped_first_and_last"]
    for field, at, value in (("shape", 5, 1 << 28), ("wdesc", 2, 1 << 28), ("wdesc", 0, 99), ("shape", 2, 257)):
        keep = getattr(w, field)[at]
        getattr(w, field)[at] = value
        try:
            st, _ = K.run(lib, w)
        finally:
            getattr(w, field)[at] = keep
        assert st == -100, (field, at)
    K.check(lib, w)


# ---- the stand-alone sanitizer program ------------------------------------------------------------------------------------------

ASAN_SRC = os.path.join(HERE, "simt", "batch_wire_asan_main.cpp")
ASAN_EXE = os.path.join(HERE, "simt", "_build", "batch_wire_asan")
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
    """Every world, the two kernels in a row and each alone, through a stand-alone program under AddressSanitizer and UBSan,
    every block of exactly its size on the heap; every block afterwards is the definition's."""
    exe, why = build_asan_program()
    if exe is None:
        pytest.skip("-fsanitize=address does not link or start on this machine: " + why)
    runs = [(WORLDS[name], which) for name in sorted(WORLDS) for which in (3, 1, 2)]
    path = tmp_path / "cases.txt"
    K.write_program_input(str(path), runs)
    env = dict(os.environ)                                                           # as it is, plus the two sanitizers' options
    env["ASAN_OPTIONS"] = "detect_leaks=0:detect_stack_use_after_return=0:abort_on_error=1"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    got = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600, env=env)
    assert got.returncode == 0, got.stdout[-300:] + got.stderr[-4000:]
    assert "AddressSanitizer" not in got.stderr and "runtime error" not in got.stderr, got.stderr[-4000:]
    assert got.stdout.strip().split("\n")[-1] == "ran %d cases, 0 wrong" % len(runs)
