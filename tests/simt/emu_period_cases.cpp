// TEST INFRASTRUCTURE ONLY: k_period_find alone under the SIMT emulator (tests/test_period_cases_emulated.py): the library
// is emu_lib.cpp's plus the entry the device build runs (tests/kernels/period_cases.hip).
#include "emu_lib.cpp"
#include "../kernels/period_cases.inc"
