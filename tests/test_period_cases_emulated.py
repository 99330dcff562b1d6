"""k_period_find alone under the SIMT emulator (blance_amd/csrc/k_period.h): its known mode -- the period counted from the
region's alive leaves, no record read -- against its searched mode and against the definition, on hand-made region tables and
records (tests/period_case_tables.py has the cases, the reference and the check; tests/test_period_cases_gpu.py runs the same
on the device).  Regions of 1, 16, 120, 192 and 4,096 alive leaves; leaves without a node, with a dead node, with a node
outside the cluster's ids; fewer steps than nodes, as many, one more, none; lengths that are no multiple of the period; chains
that start inside the cycle; one region and three.

Below them the form's other four kernels -- k_period_verify, k_period_segments, k_period_judge, k_period_replicate -- one launch
at a time against references written from the definitions, the five kernels with a small automaton's walks between them
against one sequential walk, and a stand-alone sanitizer program over the judge's and replicate's cases
(tests/period_kernel_cases.py has the cases, the references and the checks)."""
import os
import subprocess

import pytest

import period_case_tables as T
import period_kernel_cases as K
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


# ---- the other four kernels alone, and the form as a whole (tests/period_kernel_cases.py) ---------------------------------------
# k_period_verify, k_period_segments, k_period_judge and k_period_replicate each in one launch through the same library, against
# references written from the definitions; then find, verify, segments, judge and replicate with a small automaton's walks
# between them against one walk of the whole chain.


@pytest.fixture(scope="module")
def pk():
    return K.PeriodKernels(build_emu_period_cases())


@pytest.mark.parametrize("name", list(K.VERIFY_CASES))
def test_verify_alone(pk, name):
    K.check_verify(pk, name)


@pytest.mark.parametrize("cut", K.SEGMENT_CUTS)
def test_segments_alone(pk, cut):
    want = K.check_segments(pk, len(K.SEGMENT_REGIONS), cut, 64)
    if cut == 17:
        assert want[K.K_OK][13] == 1 and want[K.K_OK][14] == 0    # (cut to 17: four periods of 4 still join, four of 5 no longer)
    K.check_segments(pk, 65, cut, 64)                             # the second workgroup's rg >= B
    K.check_segments(pk, 65, cut, 256)


@pytest.mark.parametrize("threads", [128, 64, 256])
@pytest.mark.parametrize("name", list(K.JUDGE_TABLES))
def test_judge_alone(pk, name, threads):
    K.check_judge(pk, name, threads)


@pytest.mark.parametrize("threads", [128, 64])
@pytest.mark.parametrize("name", ["rests", "refusals", "picks_to_skip", "wide"])
def test_judge_refuses_behind_an_escape(pk, name, threads):
    """flags[kFlagEscaped]: every region that joins is refused, no counter changes."""
    assert not any(K.check_judge(pk, name, threads, escaped=1))
    assert not any(K.check_judge(pk, name, threads, escaped=-5))


@pytest.mark.parametrize("OW", [2, 3, 4, 5])
@pytest.mark.parametrize("name", list(K.REPLICATE_TABLES))
def test_replicate_alone(pk, name, OW):
    K.check_replicate(pk, name, OW)
    if name == "three_regions":
        K.check_replicate(pk, name, OW, threads=64)


def test_entries_refuse_tables_out_of_bounds(pk):
    K.check_entry_refusals(pk)


@pytest.mark.parametrize("name", K.PIPELINE_FIND_TABLES)
def test_form_on_the_find_tables(pk, name):
    w, init = K.world_of_find_table(name, k=2)
    K.check_pipeline(pk, w, init)


@pytest.mark.parametrize("threads", [128, 64])
@pytest.mark.parametrize("name", list(K.PIPELINE_WORLDS))
def test_form_against_one_walk(pk, name, threads):
    w, init, cut = K.pipeline_world(name)
    got = K.check_pipeline(pk, w, init, cut, judge_threads=threads)
    if name.startswith("tail") or name in ("cut_inside_a_period", "cut_at_four_periods", "cut_above_everything", "wide_regions",
                                           "weights_differ_inside_a_period"):
        assert all(ok for _, _, _, ok in got), got                # (these cases are about regions that are copied)
    if name == "state_not_re_entered":
        assert got[1][3] == 0 and K.joins(got[1][0], got[1][1])


def test_random_family_is_mostly_of_the_kind():
    """On the CPU alone: at least three quarters of the random family's regions have records periodic for four periods and a
    walk that re-enters its state -- the regions check_pipeline demands to be copied."""
    kinds = []
    for seed in K.RANDOM_SEEDS:
        w, init = K.random_world(seed)
        kinds += [must for _, _, must in K.expectation(w, init, 1, 2, w.k + 1, 0)[2]]
    assert len(kinds) >= 60 and sum(kinds) >= 0.75 * len(kinds), (sum(kinds), len(kinds))
    assert sum(kinds) < len(kinds)                                # (and some are not)


@pytest.mark.parametrize("seed", K.RANDOM_SEEDS)
def test_form_on_random_worlds(pk, seed):
    w, init = K.random_world(seed)
    K.check_pipeline(pk, w, init)


# ---- the stand-alone sanitizer program ------------------------------------------------------------------------------------------

ASAN_SRC = os.path.join(HERE, "simt", "period_cases_asan_main.cpp")
ASAN_EXE = os.path.join(HERE, "simt", "_build", "period_cases_asan")
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
    """The judge's and replicate's cases -- the picks out of range and the escaped flag among them -- through a stand-alone
    program under AddressSanitizer and UBSan, every buffer of exactly its size on the heap; its answers are the references'."""
    exe, why = build_asan_program()
    if exe is None:
        pytest.skip("-fsanitize=address does not link or start on this machine: " + why)
    judge_runs = [(name, threads, 0) for name in K.JUDGE_TABLES for threads in (128, 64)]
    judge_runs += [(name, 128, 1) for name in ("rests", "refusals", "picks_to_skip", "wide")]
    replicate_runs = [(name, OW) for name in K.REPLICATE_TABLES for OW in (2, 3, 4, 5)]
    path = tmp_path / "cases.txt"
    want = K.write_program_input(str(path), judge_runs, replicate_runs)
    env = dict(os.environ)                                                           # as it is, plus the two sanitizers' options
    env["ASAN_OPTIONS"] = "detect_leaks=0:detect_stack_use_after_return=0:abort_on_error=1"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    got = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600, env=env)
    assert got.returncode == 0, got.stdout[-300:] + got.stderr[-4000:]
    assert "AddressSanitizer" not in got.stderr and "runtime error" not in got.stderr, got.stderr[-4000:]
    lines = got.stdout.strip().split("\n")
    assert lines[-1] == "ran %d cases" % len(want)
    for i, (line, expected) in enumerate(zip(lines, want)):
        assert line == expected, (i, (judge_runs + replicate_runs)[i])
