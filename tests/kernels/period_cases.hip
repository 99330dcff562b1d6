// TEST INFRASTRUCTURE ONLY: the entries of period_cases.inc behind the product's headers, compiled by hipcc for gfx950 into
// libblance_period_cases.so (__graft_entry__.build_period_cases; tests/test_period_cases_gpu.py).  The library is k_period.h's
// kernels and the entry; it links no product object.  tests/simt/emu_period_cases.cpp is the same for the SIMT emulator.
#include "../../blance_amd/csrc/dev_prelude.h"
#include "../../blance_amd/csrc/k_period.h"
#include "period_cases.inc"
