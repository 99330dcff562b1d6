// TEST INFRASTRUCTURE ONLY: the two kernels of blance_plan_batch_wire alone under the SIMT emulator
// (tests/test_plan_batch_wire_kernels_emulated.py): the library is emu_lib.cpp's plus the entry the device build runs
// (tests/kernels/batch_wire_cases.hip).
#include "emu_lib.cpp"
#include "../kernels/batch_wire_cases.inc"
