// Translation unit of k_plan_batch, k_batch_moves, k_batch_stats, k_batch_wire_* and k_batch_decode: many small problems in
// one launch, and their launch wrappers.
#include "dev_prelude.h"
#include "k_plan_batch.h"
#include "k_batch_moves.h"
#include "k_batch_stats.h"
#include "k_batch_wire.h"
#include "k_batch_decode.h"

namespace blance {

size_t plan_batch_lds(int threads, int M, int NX) {
    const size_t words = (size_t)(M + 1) * NX > (size_t)threads ? (size_t)(M + 1) * NX : (size_t)threads;
    return sizeof(RedSlot) * 2 * (threads / 64) + sizeof(int) * (32 + kMaxStates * kBatchMaxL + kMaxStates) + sizeof(int) * words;
}

void launch_plan_batch(hipStream_t stream, const BatchParams& q, int threads, int n, size_t lds) {
    if (n <= 0) return;
    if (threads == 64) BLANCE_LAUNCH(k_plan_batch<64>, n, 64, lds, stream, q);
    else BLANCE_LAUNCH(k_plan_batch<256>, n, 256, lds, stream, q);
}

void launch_batch_moves(hipStream_t stream, const BatchMovesParams& q, int n) {
    if (n <= 0) return;
    BLANCE_LAUNCH(k_batch_moves, n, kBatchMovesThreads, sizeof(int) * kBatchMovesThreads, stream, q);
}

size_t batch_stats_lds(int M, int NX) {
    return sizeof(long long) * (size_t)M * (2 + 5 * (kBatchStatsThreads / 64)) + sizeof(int) * (size_t)M * NX;
}

void launch_batch_stats(hipStream_t stream, const BatchStatsParams& q, int n, size_t lds) {
    if (n <= 0) return;
    BLANCE_LAUNCH(k_batch_stats, n, kBatchStatsThreads, lds, stream, q);
}

void launch_batch_wire(hipStream_t stream, const BatchWireParams& q0, int n) {
    if (n <= 0) return;
    BatchWireParams q = q0;                               // (the stage and the reduction words share 64 KB of LDS)
    if ((size_t)q.stage > 64 * 1024 - kBatchWireRedLds) q.stage = (int32_t)(64 * 1024 - kBatchWireRedLds);
    BLANCE_LAUNCH(k_batch_wire_size, n, kBatchWireThreads, kBatchWireSizeLds, stream, q);
    BLANCE_LAUNCH(k_batch_wire_write, n, kBatchWireThreads, kBatchWireRedLds + (size_t)q.stage, stream, q);
}

void launch_batch_decode(hipStream_t stream, const BatchDecodeParams& q0, int n) {
    if (n <= 0) return;
    BatchDecodeParams q = q0;                             // (the stage and the scan words share 64 KB of LDS)
    if ((size_t)q.stage > 64 * 1024 - (size_t)kBatchDecodeLdsHead) q.stage = (int32_t)(64 * 1024 - kBatchDecodeLdsHead);
    BLANCE_LAUNCH(k_batch_decode, n, kBatchDecodeThreads, (size_t)kBatchDecodeLdsHead + (size_t)q.stage, stream, q);
}

}  // namespace blance
