// TEST INFRASTRUCTURE ONLY: the entry of batch_wire_cases.inc behind the product's headers, compiled by hipcc for gfx950 into
// libblance_batch_wire_cases.so (__graft_entry__.build_batch_wire_cases; tests/test_plan_batch_wire_kernels_gpu.py).  The library is
// k_batch_wire.h's kernels and the entry; it links no product object.  tests/simt/emu_batch_wire_cases.cpp is the same for
// the SIMT emulator.
#include "../../blance_amd/csrc/dev_prelude.h"
#include <vector>
#include "../../blance_amd/csrc/k_batch_wire.h"
#include "batch_wire_cases.inc"
