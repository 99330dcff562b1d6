// TEST INFRASTRUCTURE ONLY: the host driver's translation unit with the single-kernel entries of kernel_cases.inc and sweep_cases.inc behind it,
// compiled by hipcc for gfx950 and linked with the product's pass-kernel objects into libblance_kernel_cases.so
// (__graft_entry__.build_kernel_cases; tests/test_kernel_cases_gpu.py).  tests/simt/emu_kernel_cases.cpp is the same for
// the SIMT emulator.
#include "../../blance_amd/csrc/blance_hip.hip"
#include "kernel_cases.inc"
#include "sweep_cases.inc"
