// TEST INFRASTRUCTURE ONLY: the entry of wire_adopt_cases.inc behind the product's headers, compiled by hipcc for gfx950 into
// libblance_wire_adopt_cases.so (__graft_entry__.build_wire_adopt_cases; tests/test_wire_adopt_gpu.py).  The library is
// k_wire_adopt.h's kernels and the entry; it links no product object.  tests/simt/emu_wire_adopt_cases.cpp is the same for
// the SIMT emulator.
#include "../../blance_amd/csrc/dev_prelude.h"
#include <vector>
#include "../../blance_amd/csrc/k_wire_adopt.h"
#include "wire_adopt_cases.inc"
