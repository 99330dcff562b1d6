"""blance_plan_adopt without a GPU: k_adopt.h's kernels and the host side of the adoption compiled against the SIMT emulator
(tests/simt).  The cases and their checks are tests/adopt_cases.py's; tests/test_adopt_gpu.py runs the same on the device.
Every test that adopts fails on a library without blance_plan_adopt (Planner.adopt refuses)."""
import os
import subprocess

import pytest

import adopt_cases as A
from blance_amd import hip
from test_simt_emulated import HERE, _deps, build_emu

SRC = os.path.join(HERE, "simt", "emu_adopt_cases.cpp")
INC = os.path.join(HERE, "kernels", "adopt_cases.inc")
SO = os.path.join(HERE, "simt", "_build", "libblance_emu_adopt_cases.so")


def build_emu_adopt_cases():
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
    pl, pl2 = hip.Planner(lib_path=build_emu()), hip.Planner(lib_path=build_emu())
    yield pl, pl2
    pl.close()
    pl2.close()


@pytest.mark.parametrize("keep", [False, True])
def test_golden_cases(planners, golden_cases, keep):
    rounds = A.run_golden(*planners, golden_cases, keep)
    A.honest(rounds, ("golden", keep))


def test_loads_survive_and_go(planners):
    """keep_prev_only with surviving and dropped load entries at once, in chains that switch it on and off."""
    rounds = A.run_loads(*planners)
    A.honest(rounds, "loads")


def test_mixed_random_problems(planners):
    rounds = A.run_mixed(*planners, 0)
    assert len(rounds) >= 40
    A.honest(rounds, "mixed")


@pytest.mark.parametrize("hierarchy", [False, True])
def test_config5_removal_and_addition(planners, hierarchy):
    from blance_amd import synth
    P, N = 4096, 128
    fp = synth.config5_initial(P, N, hierarchy=hierarchy)
    rounds = A.run_chain(*planners, fp, A.config5_changes(fp, P, N, hierarchy), ("config 5", hierarchy))
    A.honest(rounds, ("config 5", hierarchy))


def test_config5_three_rounds(planners):
    fp, changes = A.config5_all_nodes(1024, 64, True)
    rounds = A.run_chain(*planners, fp, changes, "config 5, all nodes", around=True)
    A.honest(rounds, "config 5, all nodes")


def test_config3_three_rounds(planners):
    fp, changes = A.config3_chain()
    rounds = A.run_chain(*planners, fp, changes, "config 3")
    A.honest(rounds, "config 3")


def test_rack_leaves_and_returns(planners):
    fp, changes = A.rack_chain()
    rounds = A.run_chain(*planners, fp, changes, "rack", around=True)
    A.honest(rounds, "rack")
    assert rounds[0].moves["n_moves"] > 0 and rounds[1].moves["n_moves"] > 0


@pytest.mark.parametrize("M", [2, 3])
@pytest.mark.parametrize("P", [1, 255, 256, 257])
def test_seams(planners, P, M):
    fp = A.seam_problem(P, M)
    rounds = A.run_chain(*planners, fp, [A.Change(removed=A.flags(fp, [1])), A.Change(added=A.flags(fp, [1]))], ("seam", P, M),
                         around=True)
    assert len(rounds) == 2 and rounds[0].moves["n_by_kind"]["del"] > 0


def test_scan_split(planners):
    """P * M + 1 = 65,537 list lengths: launch_scan_excl goes from one launch to three."""
    from test_plan_moves_emulated import scan_split_problem
    fp = scan_split_problem()
    rounds = A.run_chain(*planners, fp, [A.Change(removed=A.flags(fp, [3]))], "scan split")
    assert rounds[0].moves["n_by_kind"]["add"] > 0


def test_adopted_plan_with_warnings(planners):
    fp = A.warnings_case()
    rounds = A.run_chain(*planners, fp, [A.Change(), A.Change(removed=A.flags(fp, [2]))], "warnings", around=True)
    assert all(r.res.n_warnings > 0 for r in rounds)


def test_refusals():
    A.run_refusals(lambda: hip.Planner(lib_path=build_emu()))


def test_struct_layout_matches_the_header(tmp_path):
    import ctypes as C
    from blance_amd import abi
    header = os.path.join(HERE, "..", "include", "blance_hip.h")
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\n'
                    'int main(){printf("%%zu %%zu %%zu\\n", sizeof(blance_adopt), offsetof(blance_adopt, keep_prev_only),'
                    ' offsetof(blance_adopt, reserved));return 0;}\n' % os.path.abspath(header))
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-o", str(exe), str(prog)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(abi.Adopt), abi.Adopt.keep_prev_only.offset, abi.Adopt.reserved.offset]


def test_kernels_alone():
    assert A.run_kernel_cases(A.AdoptKernels(build_emu_adopt_cases())) >= 30


# ---- the stand-alone sanitizer program -----------------------------------------------------------------------------------

ASAN_SRC = os.path.join(HERE, "simt", "adopt_asan_main.cpp")
ASAN_EXE = os.path.join(HERE, "simt", "_build", "adopt_asan")
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
    A.write_program_input(str(path))
    env = dict(os.environ)                                                           # as it is, plus the two sanitizers' options
    env["ASAN_OPTIONS"] = "detect_leaks=0:detect_stack_use_after_return=0:abort_on_error=1"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stdout[-1000:] + out.stderr[-4000:]
    assert "AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
    n = sum(1 for P, M, L in A.KERNEL_SHAPES if P * M <= 4000)
    assert out.stdout.strip().split("\n")[-1] == "ran %d cases, 0 wrong" % n
