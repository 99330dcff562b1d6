"""blance_wire_adopt without a GPU: k_wire_adopt.h's kernels and the host side compiled against the SIMT emulator
(tests/simt).  The cases and their checks are tests/wire_adopt_cases.py's; tests/test_wire_adopt_gpu.py runs the same on
the device.  Every test here fails on a library without blance_wire_adopt (Planner.adopt_wire refuses; abi.WireAdopt and the
kernels' header do not exist)."""
import os
import subprocess

import pytest

import adopt_cases as A
import wire_adopt_cases as W
from blance_amd import hip
from test_simt_emulated import HERE, _deps, build_emu

SRC = os.path.join(HERE, "simt", "emu_wire_adopt_cases.cpp")
INC = os.path.join(HERE, "kernels", "wire_adopt_cases.inc")
SO = os.path.join(HERE, "simt", "_build", "libblance_emu_wire_adopt_cases.so")


def build_emu_wire_adopt_cases():
    """The emulator library with the kernels' entry.  Workers of one run take turns at a lock: one compiles, under a name of
    its own that is moved into place whole, the others find it made."""
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
def planners():
    pls = [hip.Planner(lib_path=build_emu()) for _ in range(3)]
    yield pls
    for pl in pls:
        pl.close()


# ---- 1: equal to blance_plan_adopt

@pytest.mark.parametrize("keep", [False, True])
def test_golden_cases_equal_plan_adopt(planners, golden_cases, keep):
    n, sweeps2 = W.run_equal_golden(planners, golden_cases, keep)
    assert sweeps2 * 3 >= n, (n, sweeps2)


def test_random_problems_equal_plan_adopt(planners):
    assert W.run_equal_random(planners, 0) >= 40


# ---- 2: documents that are not the plan

def test_documents_that_are_not_the_plan(planners):
    assert W.run_mutants(planners[0], planners[1]) == 22


# ---- 3: seams

@pytest.mark.parametrize("M", [2, 3])
@pytest.mark.parametrize("P", [1, 255, 256, 257])
def test_seams(planners, P, M):
    W.run_seam(planners, P, M)


def test_scan_split(planners):
    W.run_scan_split(planners)


def test_row_stride_and_smallest_offender(planners):
    W.run_row_stride(planners[0], planners[1])


# ---- 4: refusals

def test_every_refusal_leaves_the_context_as_found():
    W.run_refusals(lambda: hip.Planner(lib_path=build_emu()))


def test_struct_layout_matches_the_header(tmp_path):
    import ctypes as C
    from blance_amd import abi
    header = os.path.join(HERE, "..", "include", "blance_hip.h")
    fields = [name for name, _ in abi.WireAdopt._fields_]
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu", sizeof(struct blance_wire_adopt));\n%s\n'
                    'printf("\\n");return 0;}\n' % (os.path.abspath(header), "\n".join(
                        'printf(" %%zu", offsetof(struct blance_wire_adopt, %s));' % f for f in fields)))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-o", str(exe), str(prog)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(abi.WireAdopt)] + [getattr(abi.WireAdopt, f).offset for f in fields]
    assert fields[:9] == ["dict", "json", "len", "node_removed", "node_added", "nodes_to_add_nil", "assign_too", "keep_prev_only", "reserved"]


# ---- 5: the kernels alone

def test_kernels_alone():
    assert W.run_kernel_cases(W.WireAdoptKernels(build_emu_wire_adopt_cases())) >= 80


# ---- 6: the switch

def test_adopt_partition_map_routes(planners):
    assert W.run_switch(planners[0], planners[1]) == 11


# ---- the stand-alone sanitizer program

ASAN_SRC = os.path.join(HERE, "simt", "wire_adopt_asan_main.cpp")
ASAN_EXE = os.path.join(HERE, "simt", "_build", "wire_adopt_asan")
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
    """The kernels' cases through the stand-alone program under AddressSanitizer and UBSan, every buffer of exactly its
    documented size; the program compares with the definition's numbers itself."""
    exe, why = build_asan_program()
    if exe is None:
        pytest.skip("-fsanitize=address does not link or start on this machine: " + why)
    path = tmp_path / "input.txt"
    n = W.write_program_input(str(path))
    env = dict(os.environ)                                                           # as it is, plus the two sanitizers' options
    env["ASAN_OPTIONS"] = "detect_leaks=0:detect_stack_use_after_return=0:abort_on_error=1"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stdout[-1000:] + out.stderr[-4000:]
    assert "AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
    assert n >= 28 and out.stdout.strip().split("\n")[-1] == "ran %d cases, 0 wrong" % n
