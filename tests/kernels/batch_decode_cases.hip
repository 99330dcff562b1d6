// TEST INFRASTRUCTURE ONLY: the entry of batch_decode_cases.inc behind the product's headers, compiled by hipcc for gfx950 into
// libblance_batch_decode_cases.so (__graft_entry__.build_batch_decode_cases; tests/test_plan_batch_docs_kernels_gpu.py).  The
// library is k_batch_decode.h's kernel (with k_wire_decode.h's parser) and the entry; it links no product object.
// tests/simt/emu_batch_decode_cases.cpp is the same for the SIMT emulator.
#include "../../blance_amd/csrc/dev_prelude.h"
#include <vector>
#include "../../blance_amd/csrc/k_batch_decode.h"
#include "batch_decode_cases.inc"
