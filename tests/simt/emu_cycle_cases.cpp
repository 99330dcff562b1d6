// TEST INFRASTRUCTURE ONLY: k_cycle_group and k_cycle_top alone under the SIMT emulator (tests/test_cycle_cases_emulated.py):
// the library is emu_lib.cpp's plus the entry the device build runs (tests/kernels/cycle_cases.hip).
#include "emu_lib.cpp"
#include "../kernels/cycle_cases.inc"
