// TEST INFRASTRUCTURE ONLY: stage 1 of the device decoder alone under the SIMT emulator
// (tests/test_wire_decode_kernels_emulated.py): the library is emu_lib.cpp's plus the entry the device build runs
// (tests/kernels/wire_decode_cases.hip).
#include "emu_lib.cpp"
#include "../kernels/wire_decode_cases.inc"
