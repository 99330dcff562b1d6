// TEST INFRASTRUCTURE ONLY: the entry of cycle_cases.inc behind the product's headers, compiled by hipcc for gfx950 into
// libblance_cycle_cases.so (__graft_entry__.build_cycle_cases; tests/test_cycle_cases_gpu.py).  The library is k_sweep.h's and
// k_cycle.h's kernels and the entry; it links no product object.  tests/simt/emu_cycle_cases.cpp is the same for the SIMT
// emulator.
#include "../../blance_amd/csrc/dev_prelude.h"
#include "../../blance_amd/csrc/k_sweep.h"
#include "../../blance_amd/csrc/k_cycle.h"
#include "cycle_cases.inc"
