/*
 * blance_batch.h -- many independent PlanNextMapEx problems in one call.
 *
 * An extension of the C ABI of blance_hip.h, exported by the same library and additive to ABI 6: the
 * version stays 6, and a caller that may meet a library without it looks the symbol up before use.
 */
#ifndef BLANCE_BATCH_H
#define BLANCE_BATCH_H

#include "blance_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- many independent problems in one call ------------------------------------------------
 * One PlanNextMapEx per index of a cluster: tens to a few thousand partitions each.  For every i,
 * res[i] receives exactly what blance_plan(ctx, pbs[i], res[i]) would write.  Problems inside the
 * batched envelope (n_nodes_ext <= 256, n_parts <= 16384, longest state list incl.
 * constraints <= 8) are packed into one upload, planned by one kernel launch per size class (one
 * workgroup per problem) and come back in one download; any other valid problem is planned in the
 * same call by the single-problem path, one after another.  Engine fields of a batched problem:
 * steps_total is its own, device_ms / total_ms are the batch's, the other counters 0.
 * Every problem is validated and every result's capacities checked (out_capacity >=
 * blance_result_capacity(), warn_capacity >= n_parts * (states with constraints > 0)) before
 * anything runs: a refusal returns that status, names the problem's index in blance_last_error()
 * and writes no result.  n == 0 is valid and launches nothing.  A context with a communicator
 * (blance_comm_*) answers BLANCE_ERR_UNSUPPORTED.  Afterwards the context holds no problem:
 * blance_plan_resident / blance_download / blance_plan_stats_get answer BLANCE_ERR_BAD_ARG until
 * the next upload or plan.  */
typedef struct blance_batch_info {
    int32_t n_batched;        /* out: problems planned by k_plan_batch            */
    int32_t n_fallback;       /* out: problems planned by the single-problem path */
    int64_t kernel_launches;  /* out: all launches of the call                    */
    int64_t steps_total;      /* out: findBestNodes calls over all problems       */
    double  device_ms, total_ms;
} blance_batch_info;

int blance_plan_batch(blance_ctx* ctx, int32_t n, const blance_problem* const* pbs,
                      blance_result* const* res, blance_batch_info* info /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* BLANCE_BATCH_H */
