// TEST INFRASTRUCTURE ONLY: k_stay_by_top's rank function alone under the SIMT emulator (tests/test_stay_ranks_emulated.py):
// the library is emu_lib.cpp's plus the entry the device build runs (tests/kernels/stay_rank_cases.hip).
#include "emu_lib.cpp"
#include "../kernels/stay_rank_cases.inc"
