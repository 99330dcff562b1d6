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

/* ---- the same batch, and the partition moves of each plan --------------------
 * For every problem i with mvs[i] != NULL, mvs[i]->out receives what blance_calc_moves would return for
 * CalcPartitionMoves(sortStateNames(model), prevMap[name].NodesByState, nextMap[name].NodesByState,
 * favor_min_nodes) over the partitions of partitionsToAssign in partition id order (orchestrate.go:273-287):
 * prevMap as the call passes it (before the write-back of plan.go:49-52), nextMap the plan's result, node ids in
 * the problem's own id space.  Batched problems get theirs from k_batch_moves in the same call (one launch after
 * the plan launches, moves in the same download); every other problem from the path of blance_calc_moves.
 * Every request is checked with its problem before anything runs (null arrays, CSR offsets that do not start at 0
 * or are not monotone, other-node ids outside [0, n_nodes_ext), a capacity below blance_batch_moves_capacity(),
 * max_iterations <= 0: PlanNextMapEx returns no map there): a refusal names the problem's index and writes no
 * result and no moves.  mvs == NULL is exactly blance_plan_batch.  out.device_ms is the batch's. */
typedef struct blance_batch_moves {
    int32_t favor_min_nodes;          /* in */
    /* in, may both be NULL: prevMap[name]'s nodes under state keys that are not in the model, CSR over partitions
     * ([P + 1], ids < n_nodes_ext).  They only feed flattenNodesByState (moves.go:60-64), like blance_moves_problem's
     * pseudo state M; partitionsToAssign never has such keys, so the result never has them. */
    const int32_t* beg_other_off;
    const int32_t* beg_other_nodes;
    blance_moves_result out;          /* op_off [P + 1], op_node / op_state / op_kind [capacity]; device_ms = the batch's */
} blance_batch_moves;

/* prev_off[P*M] + beg_other_off[P] + blance_result_capacity(pb): enough for every partition's moves */
int64_t blance_batch_moves_capacity(const blance_problem* pb, const blance_batch_moves* mv);

int blance_plan_batch_moves(blance_ctx* ctx, int32_t n, const blance_problem* const* pbs, blance_result* const* res,
                            blance_batch_moves* const* mvs /* mvs[i] may be NULL: no moves for problem i */,
                            blance_batch_info* info /* may be NULL */);

/* ---- the same batch, and the plan statistics of each plan -------------------
 * For every problem i with sts[i] != NULL, sts[i] receives exactly what blance_plan(ctx, pbs[i], res[i]) followed
 * by blance_plan_stats_get(ctx, sts[i]) would write: n_nodes_next, per state load_min / load_max / load_sum /
 * load_sumsq / nodes_used / unmet_slots, and rule_violations when that pointer is not NULL; all zeros with
 * n_nodes_next = 0 for a plan with iterations == 0.  The caller owns the arrays; n_states is their capacity.
 * Batched problems get theirs from k_batch_stats in the same call (one launch after the plan launches whenever at
 * least one batched problem asks, the numbers in the same download: with moves and statistics a fully batched
 * call is at most 4 launches); every other problem from the path of blance_plan_stats_get right after its plan.
 * Every request is checked with its problem before anything runs (n_states below the problem's, one of the six
 * mandatory arrays NULL): a refusal returns BLANCE_ERR_BAD_ARG, names the problem's index and writes no result, no
 * moves and no statistics.  mvs follows blance_plan_batch_moves.  sts == NULL is exactly blance_plan_batch_moves;
 * sts == NULL and mvs == NULL is exactly blance_plan_batch.  Afterwards the context holds no problem, as after every
 * batch: blance_plan_stats_get answers BLANCE_ERR_BAD_ARG. */
int blance_plan_batch_stats(blance_ctx* ctx, int32_t n, const blance_problem* const* pbs, blance_result* const* res,
                            blance_batch_moves* const* mvs /* may be NULL; mvs[i] may be NULL */,
                            blance_plan_stats* const* sts /* may be NULL; sts[i] may be NULL: no statistics for problem i */,
                            blance_batch_info* info /* may be NULL */);

/* ---- the same batch, and each plan as PartitionMap JSON bytes ----------------
 * The names of an index do not change between rebalances, so what depends on them alone is prepared once, on the
 * host: the order of the partitions in the document (byte order of their names), every name in its escaped form, the
 * states in the order of their names -- what blance_plan_wire_names prepares for the problem a context holds.  A
 * blance_batch_names is host memory only, tied to no context and immutable: any number of calls, contexts and threads
 * may use one at the same time, and two problems of one batch may share one.  names follows blance_plan_wire_names
 * (strings of any bytes; n_parts / n_nodes_ext / n_states strings).  Refusals: BLANCE_ERR_BAD_ARG for a NULL, a negative
 * size, offsets that do not start at 0 or are not monotone, two states with one name; BLANCE_ERR_UNSUPPORTED for two
 * partitions with one name and for 2^31 escaped bytes or more. */
typedef struct blance_batch_names blance_batch_names;
int  blance_batch_names_create(const blance_wire_names* names, int32_t n_parts, int32_t n_nodes_ext, int32_t n_states,
                               blance_batch_names** out);
void blance_batch_names_destroy(blance_batch_names* nm);   /* NULL is fine */

/* For every problem i with wrs[i] != NULL, wrs[i]->buf receives json.Marshal(PartitionMap) of the plan in res[i]: the
 * bytes blance_wire_encode makes of that result, and the bytes blance_plan(ctx, pbs[i], res[i]) followed by
 * blance_plan_wire_names and blance_plan_wire_get would return; need is the document's length, buf[need ..) is left
 * untouched.  Batched problems get theirs from k_batch_wire_size and k_batch_wire_write in the same call (two launches
 * after the plan launches whenever at least one batched problem asks: with moves, statistics and documents a fully
 * batched call is at most 6 launches; the lengths come in the same download, the documents in one more copy of exactly
 * their bytes); every other problem from the path of blance_plan_wire_get right after its plan.  An empty map
 * (n_parts == 0) is "{}".  Every request is checked with its problem before anything runs (names or buf NULL, sizes of
 * names that differ from the problem's, cap below blance_batch_wire_capacity(), max_iterations <= 0: PlanNextMapEx
 * returns no map there): a refusal names the problem's index and writes no result, no moves, no statistics and no
 * document.  mvs and sts follow blance_plan_batch_stats; wrs == NULL is exactly blance_plan_batch_stats.  Afterwards the
 * context holds no problem and no names, as after every batch: blance_plan_wire_get answers BLANCE_ERR_BAD_ARG. */
typedef struct blance_batch_wire {
    const blance_batch_names* names;  /* in: sizes must equal the problem's n_parts / n_nodes_ext / n_states */
    char*  buf;                       /* in: caller-owned, cap bytes */
    size_t cap;                       /* in: >= blance_batch_wire_capacity(pb, names) */
    size_t need;                      /* out: the document's length; buf[need ..) is left untouched */
} blance_batch_wire;

/* An upper bound on the document, known before the plan, from the sums a blance_batch_names keeps:
 *   2 + 29 * P + 2 * (escaped partition bytes) + P * ((escaped "state": bytes) + 5 * M)
 *     + blance_result_capacity(pb) * ((longest escaped node name) + 1)
 * 29 = a partition's punctuation ( , or {   :{"name":   ,"nodesByState":{   }} ), 5 per (partition, state) = the comma
 * and `null` (or the two brackets), + 1 per list entry = its comma, 2 = "{}" and the document's last brace.
 * 0 when an argument is NULL. */
size_t blance_batch_wire_capacity(const blance_problem* pb, const blance_batch_names* names);

int blance_plan_batch_wire(blance_ctx* ctx, int32_t n, const blance_problem* const* pbs, blance_result* const* res,
                           blance_batch_moves* const* mvs /* may be NULL; mvs[i] may be NULL */,
                           blance_plan_stats* const* sts /* may be NULL; sts[i] may be NULL */,
                           blance_batch_wire* const* wrs /* may be NULL; wrs[i] may be NULL: no document for problem i */,
                           blance_batch_info* info /* may be NULL */);

/* ---- the same batch, planned from PartitionMap documents decoded on the device ----
 * What a caller holds of an index is its stored document, not interned arrays.  A blance_batch_dict is what
 * blance_wire_dict_create builds for the device -- per kind of name (partitions, nodes, states) an open-addressing table at
 * load <= 1/2 over the raw names, the raw bytes and their int32 offsets -- as one block of int32 words in host memory: tied
 * to no context and immutable, like a blance_batch_names; calls, contexts and threads may share one.  Refusals are exactly
 * those of blance_wire_dict_create (BLANCE_ERR_BAD_ARG / BLANCE_ERR_UNSUPPORTED, same conditions). */
typedef struct blance_batch_dict blance_batch_dict;
int  blance_batch_dict_create(const blance_wire_names* names, int32_t n_parts, int32_t n_nodes_ext, int32_t n_states,
                              blance_batch_dict** out);
void blance_batch_dict_destroy(blance_batch_dict* d);      /* NULL is fine */

/* For dcs[i] != NULL, pbs[i] is a valid skeleton and the problem planned is P'_i: the problem blance_wire_adopt defines
 * (blance_hip.h) for the document decoded against dict, with node_removed / node_added / nodes_to_add_nil read from pbs[i]
 * and assign_too / keep_prev_only as given.  res[i], mvs[i], sts[i] and wrs[i] receive what blance_plan_batch_wire would
 * write for P'_i; the moves start from the document's map.
 *
 * The outcome is per document, not per call: what the document decides lands in dcs[i] and the call returns BLANCE_OK.
 * status BLANCE_ERR_UNSUPPORTED: not planned -- refusal / refusal_at exactly what blance_wire_decode_device reports for
 * these bytes (BLANCE_WIRE_REFUSED_DOCUMENT_TOO_LONG at 0 for len >= 2^31), or why / why_at exactly what blance_wire_adopt
 * reports (BLANCE_WIRE_ADOPT_*, the smallest offender); res[i], mvs[i], sts[i] and wrs[i] (buffer included) are then not
 * written and the caller takes the host route for that index.  info->n_batched + info->n_fallback
 * counts the planned problems only.
 *
 * Argument errors refuse the whole call before anything runs (BLANCE_ERR_BAD_ARG, the problem's index in
 * blance_last_error(), nothing written): dict NULL, json NULL with len > 0, dict sizes that differ from the problem's,
 * non-zero reserved, mvs[i]->beg_other_off together with a document (P' has no prevMap keys outside the model), a document
 * on a problem with max_iterations <= 0.  The capacity checks of a document problem use blance_batch_doc_bounds.
 *
 * Batched document problems are decoded by k_batch_decode, one workgroup per document, straight into the packed input
 * slices (row stride 8): against the same call without documents a fully batched call adds ONE launch, whatever n, and one
 * host round trip (the documents' summary words).  A document problem goes the single path inside the same call, from
 * the original bytes (blance_upload(pbs[i]), a temporary context dictionary, blance_wire_adopt, blance_plan_resident and
 * the readers), when pbs[i] is outside the batched envelope by its own sizes, when the document has a list longer than 8,
 * when the document is longer than 2^28 bytes or would take the documents decoded in this call past 2^31 bytes (in call
 * order), or when k_plan_batch marks the problem not done; refusals and why codes of that path pass into dcs[i] unchanged
 * (a list longer than pbs[i]'s own row stride is BLANCE_WIRE_ADOPT_LIST_TOO_LONG there).
 * dcs[i] == NULL: problem i exactly as by blance_plan_batch_wire; dcs == NULL is exactly blance_plan_batch_wire. */
typedef struct blance_batch_doc {
    /* in */
    const blance_batch_dict* dict;     /* sizes must equal the problem's; its ids are the problem's ids (caller's contract) */
    const char* json; size_t len;
    int32_t assign_too, keep_prev_only;
    int32_t reserved[2];               /* zero */
    /* out */
    int32_t status;                    /* BLANCE_OK: planned; BLANCE_ERR_UNSUPPORTED: not planned, see refusal / why */
    int32_t refusal; int64_t refusal_at;          /* exactly what blance_wire_decode_device reports for this document */
    int32_t why;     int64_t why_at;              /* BLANCE_WIRE_ADOPT_*, exactly what blance_wire_adopt reports */
    int64_t n_node_refs, n_parts_seen;
} blance_batch_doc;

/* Upper bounds known before the plan.  A list of r node references takes at least 3 r + 1 bytes, so a document of len
 * bytes holds at most len / 3 references:
 *   result_cap = n_parts * sum_m max(k_m, 0) + len / 3 with assign_too, else blance_result_capacity(pb);
 *   moves_cap  = len / 3 + result_cap;
 *   wire_cap   = blance_batch_wire_capacity's formula with result_cap in place of blance_result_capacity(pb) (0 when
 *                names is NULL).
 * Any of the three pointers may be NULL.  BLANCE_ERR_BAD_ARG when pb or dc is NULL. */
int blance_batch_doc_bounds(const blance_problem* pb, const blance_batch_doc* dc, const blance_batch_names* names /* may be NULL */,
                            int64_t* result_cap, int64_t* moves_cap, size_t* wire_cap);

int blance_plan_batch_docs(blance_ctx* ctx, int32_t n, const blance_problem* const* pbs, blance_result* const* res,
                           blance_batch_moves* const* mvs /* may be NULL; mvs[i] may be NULL */,
                           blance_plan_stats* const* sts /* may be NULL; sts[i] may be NULL */,
                           blance_batch_wire* const* wrs /* may be NULL; wrs[i] may be NULL */,
                           blance_batch_doc* const* dcs /* may be NULL; dcs[i] may be NULL: no document for problem i */,
                           blance_batch_info* info /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* BLANCE_BATCH_H */
