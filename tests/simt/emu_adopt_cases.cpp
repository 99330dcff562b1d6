// TEST INFRASTRUCTURE ONLY: the two kernels of blance_plan_adopt alone under the SIMT emulator (tests/test_adopt_emulated.py):
// the library is emu_lib.cpp's plus the entry the device build runs (tests/kernels/adopt_cases.hip).
#include "emu_lib.cpp"
#include "../kernels/adopt_cases.inc"
