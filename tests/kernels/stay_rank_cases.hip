// TEST INFRASTRUCTURE ONLY: the entry of stay_rank_cases.inc behind the product's headers, compiled by hipcc for gfx950 into
// libblance_stay_rank_cases.so (__graft_entry__.build_stay_rank_cases; tests/test_stay_ranks_gpu.py).  No product kernel is
// instantiated here: the library is the rank function and its one-wave test kernel.
// tests/simt/emu_stay_rank_cases.cpp is the same for the SIMT emulator.
#include "../../blance_amd/csrc/dev_prelude.h"
#include "../../blance_amd/csrc/k_pass_chain.h"
#include "../../blance_amd/csrc/k_stay.h"
#include "stay_rank_cases.inc"
