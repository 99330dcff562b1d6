// TEST INFRASTRUCTURE ONLY: the kernel of blance_plan_batch_docs alone under the SIMT emulator
// (tests/test_plan_batch_docs_kernels_emulated.py): the library is emu_lib.cpp's plus the entry the device build runs
// (tests/kernels/batch_decode_cases.hip).
#include "emu_lib.cpp"
#include "../kernels/batch_decode_cases.inc"
