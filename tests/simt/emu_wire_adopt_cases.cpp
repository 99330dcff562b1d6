// TEST INFRASTRUCTURE ONLY: the two kernels of blance_wire_adopt alone under the SIMT emulator
// (tests/test_wire_adopt_emulated.py): the library is emu_lib.cpp's plus the entry the device build runs
// (tests/kernels/wire_adopt_cases.hip).
#include "emu_lib.cpp"
#include "../kernels/wire_adopt_cases.inc"
