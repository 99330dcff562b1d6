/*
 * blance_hip.h -- C ABI of the MI355X-native PlanNextMap planner.
 *
 * This is the drop-in boundary for couchbase/blance's planner path.  The
 * reference has no FFI; the seam this ABI replaces is the call
 *
 *     PlanNextMapEx(...) -> planNextMapEx(...)        api.go:147-157, plan.go:23-58
 *
 * i.e. the whole convergence loop (plan.go:32-56) with every greedy sweep
 * (planNextMapInnerEx, plan.go:60-331) runs behind ONE call of blance_plan().
 * The host side (Go over cgo, or the C++/Python mirrors in this repo) interns
 * strings to dense ids, flattens the maps to the int32 SoA arrays below, calls
 * blance_plan(), un-interns the result and replays the caller-visible
 * mutations of plan.go:49-55.  See INTEGRATION.md for the cgo stub.
 *
 * ABI rules: plain C, caller owns every buffer, nothing is retained after a
 * call returns (cgo pointer rule), no exceptions cross the boundary, every
 * entry point returns an int status (0 = ok, <0 = error).  The planning entry
 * points take no callbacks; the one function-pointer table of this header is
 * the struct blance_comm: an embedder's own collectives for a plan sharded over several
 * ranks; a production multi-GPU caller uses blance_comm_init_rccl instead
 * and passes none.
 *
 * Id spaces
 *   node id      0..n_nodes-1 = position in nodesAll (plan.go:72-75; names must
 *                be unique).  n_nodes..n_nodes_ext-1 = names that occur only in
 *                partition lists / nodesToRemove / nodesToAdd / NodeWeights:
 *                they are counted and filtered but are never candidates
 *                (candidates come from nodesAll, plan.go:77,:142).
 *   state id     0..n_states-1 = the model's states in sortStateNames() order
 *                (plan.go:437-474), which is the pass order of plan.go:307.
 *                Pseudo state id n_states ("other") carries loads of state
 *                names that are not in the model; they only feed
 *                nodePartitionCounts (plan.go:118-124).
 *   partition id 0..n_parts-1 = the partitions of partitionsToAssign, any order.
 *   vertex id    hierarchy vertices: 0..n_nodes_ext-1 are the nodes, the rest
 *                are interior names of NodeHierarchy plus the "" vertex that
 *                findAncestor() yields past a root (plan.go:755-762).
 */
#ifndef BLANCE_HIP_H
#define BLANCE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BLANCE_ABI_VERSION 6

/* status codes */
#define BLANCE_OK                0
#define BLANCE_ERR_BAD_ARG      -1  /* NULL / inconsistent sizes / id out of range      */
#define BLANCE_ERR_UNSUPPORTED  -2  /* input outside the supported envelope             */
#define BLANCE_ERR_CAPACITY     -3  /* caller's output buffers too small                */
#define BLANCE_ERR_DEVICE       -4  /* HIP runtime failure (see blance_last_error)      */
#define BLANCE_ERR_NO_DEVICE    -5  /* no gfx950 device visible                         */
#define BLANCE_ERR_COMM         -6  /* RCCL / caller collective failure                 */

/* list kinds: Go distinguishes a missing map key, a nil slice and an empty
 * non-nil slice under reflect.DeepEqual (plan.go:38). */
#define BLANCE_LIST_ABSENT 0
#define BLANCE_LIST_NIL    1
#define BLANCE_LIST_SET    2

/* NodeScoreBooster (plan.go:691-697) cannot be an arbitrary Go callback on the
 * device; the one booster known in the wild (couchbase/cbgt, restated in
 * control_test.go:19-26: max(float64(-w), stickiness)) is a built-in. */
#define BLANCE_BOOSTER_NONE 0
#define BLANCE_BOOSTER_CBGT 1

/* engines (blance_options.engine) */
#define BLANCE_ENGINE_AUTO        0 /* fastest exact schedule available                 */
#define BLANCE_ENGINE_SEQUENTIAL  1 /* one in-order step at a time (always exact)       */

typedef struct blance_problem {
    /* ---- sizes -------------------------------------------------------- */
    int32_t n_nodes;          /* N  = len(nodesAll)                                      */
    int32_t n_nodes_ext;      /* NX >= N                                                 */
    int32_t n_states;         /* M  = len(model)                                         */
    int32_t n_parts;          /* P  = len(partitionsToAssign)                            */
    int32_t n_prev;           /* len(prevMap): NumPartitions of sweep 1 (plan.go:161)    */
    int32_t n_loads;          /* entries in load_*                                       */
    int32_t n_rules;          /* entries in rule_inc/rule_exc                            */
    int32_t n_vertices;       /* VX (0 when hierarchy_rules_nil)                         */
    int32_t max_iterations;   /* MaxIterationsPerPlan (plan.go:21)                       */

    /* ---- flags -------------------------------------------------------- */
    int32_t partition_weights_nil;  /* opts.PartitionWeights == nil (plan.go:105,:270)   */
    int32_t nodes_to_add_nil;       /* nodesToAdd == nil (plan.go:554)                   */
    int32_t hierarchy_rules_nil;    /* opts.HierarchyRules == nil (plan.go:174)          */
    int32_t booster_kind;           /* BLANCE_BOOSTER_*                                  */
    int32_t top_state;              /* state id of minimum Priority (plan.go:126-132)    */

    /* ---- model, by state id ------------------------------------------ */
    const int32_t* state_priority;        /* [M] PartitionModelState.Priority            */
    const int32_t* state_constraints;     /* [M] effective k: ModelStateConstraints
                                                 override applied (plan.go:308-319)      */
    const int32_t* state_stickiness;      /* [M] opts.StateStickiness[state]             */
    const uint8_t* state_has_stickiness;  /* [M] key present (0 everywhere if map nil)   */

    /* ---- nodes, by node id ------------------------------------------- */
    const uint8_t* node_removed;      /* [NX] in nodesToRemove                           */
    const uint8_t* node_added;        /* [NX] in nodesToAdd                              */
    const int32_t* node_weight;       /* [NX] opts.NodeWeights[node]                     */
    const uint8_t* node_has_weight;   /* [NX] key present (0 everywhere if map nil)      */

    /* ---- partitions of partitionsToAssign, by partition id ------------ */
    const int32_t* part_order;        /* [P] partition ids ordered by the static part of
                                             partitionSorter's key (weight desc, numeric
                                             name, name), plan.go:519-540; the per-pass
                                             category "0/1/2" (plan.go:542-561) is
                                             applied on the device as a stable 3-way
                                             partition of this order                     */
    const int32_t* part_weight;       /* [P] opts.PartitionWeights[name]                 */
    const uint8_t* part_has_weight;   /* [P]                                             */
    const uint8_t* part_in_prev;      /* [P] name is a key of prevMap                    */
    const uint8_t* part_prev_never_equal; /* [P] prevMap[name] can never DeepEqual a
                                             result (nil NodesByState map, non-model
                                             state keys, Name != key)                    */
    /* partitionsToAssign[p].NodesByState[state], CSR over (p * M + state) */
    const int32_t* assign_off;        /* [P*M + 1]                                       */
    const int32_t* assign_nodes;      /* [assign_off[P*M]] node ids, list order kept     */
    const uint8_t* assign_kind;       /* [P*M] BLANCE_LIST_*                             */
    /* prevMap[name].NodesByState[state] for the same partitions (empty when
     * !part_in_prev) */
    const int32_t* prev_off;          /* [P*M + 1]                                       */
    const int32_t* prev_nodes;
    const uint8_t* prev_kind;         /* [P*M]                                           */

    /* ---- extra prevMap loads (countStateNodes, plan.go:374-399) -------- */
    /* One entry per (partition, state, node) occurrence that the CSR above does
     * not carry: partitions that are only in prevMap, and non-model states. */
    const int32_t* load_state;        /* [n_loads] 0..M (M = "other")                    */
    const int32_t* load_node;         /* [n_loads] node id                               */
    const int32_t* load_weight;       /* [n_loads] the partition's weight                */
    const uint8_t* load_first_sweep_only; /* [n_loads] entry belongs to a partition that
                                             is also in partitionsToAssign, so sweep 1's
                                             write-back (plan.go:49-52) replaces it      */

    /* ---- hierarchy (plan.go:703-774) ---------------------------------- */
    const int32_t* rule_off;          /* [M + 1] rules of state s: rule_off[s]..[s+1]    */
    const int32_t* rule_inc;          /* [n_rules] HierarchyRule.IncludeLevel            */
    const int32_t* rule_exc;          /* [n_rules] HierarchyRule.ExcludeLevel            */
    int32_t        vertex_empty;      /* vertex id of ""                                 */
    const int32_t* vertex_parent;     /* [VX] NodeHierarchy[v], vertex_empty if missing  */
    const int32_t* vertex_leaf_lo;    /* [VX] leaves(v) = leaf positions [lo, hi) in a   */
    const int32_t* vertex_leaf_hi;    /* [VX] DFS over children sorted by name           */
    const int32_t* node_leaf_pos;     /* [NX] leaf position of the node, -1 if the node
                                             has children (it is then never a leaf)      */
} blance_problem;

typedef struct blance_result {
    /* nextMap[p].NodesByState[state], CSR over (p * M + state); caller allocates */
    int32_t* out_off;         /* [P*M + 1]                                               */
    int32_t* out_nodes;       /* [out_capacity]                                          */
    uint8_t* out_kind;        /* [P*M]                                                   */
    int64_t  out_capacity;    /* in: capacity of out_nodes (blance_result_capacity())    */
    /* warnings of the last sweep (plan.go:70,:231-235): one (partition, state)
     * pair per message, grouped by pass, in processing order */
    int32_t* warn_part;       /* [warn_capacity]                                         */
    int32_t* warn_state;      /* [warn_capacity]                                         */
    int64_t  warn_capacity;   /* in: P*M always suffices                                 */
    int64_t  n_warnings;      /* out                                                     */
    int32_t  iterations;      /* out: sweeps run (1..max_iterations)                     */
    int32_t  converged;       /* out: loop left through plan.go:43-45                    */
    /* out: timings of this call */
    double   device_ms;       /* first kernel -> last kernel, hipEvents                  */
    double   total_ms;        /* incl. H2D / D2H of problem and result                   */
    /* out: engine statistics (steps = findBestNodes calls) */
    int64_t  steps_total;
    int64_t  steps_sequential;    /* steps resolved one at a time                        */
    int64_t  steps_batched;       /* steps resolved by an exact parallel schedule        */
    int64_t  kernel_launches;
    /* out: the dominant kernel -- the state-pass kernel (k_pass_chain, or
     * k_pass_seq over a whole pass), one launch per hierarchy-rule state pass --
     * timed with hipEvents on the planner's stream: sum of its launch durations
     * and launch count; and the same for passes run by the flat bulk driver
     * (several small kernels + host round trips per pass) */
    double   pass_kernel_ms;
    int64_t  pass_kernel_launches;
    double   flat_pass_ms;
    int64_t  flat_passes;
    /* out: of pass_kernel_ms / pass_kernel_launches, the part of the all-blank chain kernel
     * (k_pass_chain_planes / k_pass_chain_blank: the first hierarchy pass of a fresh plan) */
    double   blank_pass_ms;
    int64_t  blank_pass_launches;
    /* out (ABI 5): of pass_kernel_ms / pass_kernel_launches, the part of chain passes that k_stay_by_top verified as stays
     * (one thread per top priority node, incl. the grouping by top node in front of it) -- what is left after this and the
     * all-blank part is k_pass_chain (hierarchy-rule states) or k_pass_queue / k_pass_tree / k_pass_seq (flat states) */
    double   stay_pass_ms;
    int64_t  stay_pass_launches;
    /* out (ABI 6): stream synchronisations the host made inside this plan (each one reads a few flag words that decide what
     * is launched next; the device idles for the round trip) */
    int64_t  host_syncs;
} blance_result;

typedef struct blance_options {
    int32_t engine;           /* BLANCE_ENGINE_*                                         */
    int32_t device_id;        /* HIP device ordinal                                      */
    int32_t reserved[6];      /* zero in production.  Test knobs: [0] workgroup size of k_pass_seq (64 / 256 / 512 /
                               * 1024), [1] smallest pass handed to the bulk engines, [2] & 1 = k_pass_seq without
                               * verified-stay speculation (further bits of [2]: blance_amd/hip.py).
                               * & 256 = the all-blank chain pass WITHOUT its periodic form (csrc/k_period.h, on by
                               * default since round 4; the environment's BLANCE_PERIODIC=0 does the same);
                               * & 16384 = a communicator of ONE rank takes the sharded branch of every chain pass:
                               * both collectives of "one plan on several GPUs" below execute (how ncclAllReduce /
                               * ncclAllGather are exercised and timed on a one-GPU machine)                      */
} blance_options;

typedef struct blance_ctx blance_ctx;   /* opaque: device buffers, stream, events */

/* Upper bound on out_nodes entries for a problem: sum over (p, state) of
 * max(constraints, len(assign list)). */
int64_t blance_result_capacity(const blance_problem* pb);

/* Create / destroy a planner context bound to one gfx950 device. */
int blance_ctx_create(const blance_options* opt, blance_ctx** out);
void blance_ctx_destroy(blance_ctx* ctx);

/* Run planNextMapEx (plan.go:23-58) for one problem.  Host buffers in, host
 * buffers out.  Re-entrant per context (calls on one ctx are serialised). */
int blance_plan(blance_ctx* ctx, const blance_problem* pb, blance_result* res);

/* Device-resident variant used by the benchmark: upload once, plan many times,
 * download once.  blance_plan() == upload + plan_resident + download. */
int blance_upload(blance_ctx* ctx, const blance_problem* pb);
int blance_plan_resident(blance_ctx* ctx, blance_result* res /* timings+stats only */);
int blance_download(blance_ctx* ctx, blance_result* res);

/* ---- host buffers the device reaches at link speed (ABI 5) ------------------------------------
 * the caller owns every buffer.  blance_host_alloc() hands out page-locked host
 * memory that stays the caller's (free it with blance_host_free(); freed blocks are kept for the
 * next allocation, pinning costs milliseconds).  The arrays of a blance_problem / blance_result
 * that lie in such memory -- or in memory the caller registered with the HIP runtime itself -- are
 * copied by DMA where they lie; every other (pageable) array passes through a page-locked buffer
 * of the context, moved by a few host threads.  Either way nothing of the caller's is touched
 * after the call returns.  NULL when the runtime cannot provide the memory (use malloc then). */
void* blance_host_alloc(size_t bytes);
void blance_host_free(void* p);
/* (ABI 6) Freed blocks are cached for the next blance_host_alloc -- up to 2 GiB of page-locked, unswappable memory per
 * process.  blance_host_trim() returns every cached block to the system now; the destruction of a process's last context
 * does the same.  Blocks the caller still holds are not touched. */
void blance_host_trim(void);

/* ---- CalcPartitionMoves for every partition at once (moves.go:41-136) ---------
 * The planner's consumer (orchestrate.go:273-287 calls it per partition): the
 * ordered node-by-node state transitions from begMap[p] to endMap[p].  Per
 * partition independent.  State ids 0..n_states-1 follow the `states` argument
 * (superior first); pseudo state n_states collects the nodes of map keys that
 * are not in `states` (they only feed flattenNodesByState, plan.go:425-431). */
#define BLANCE_OP_ADD      0
#define BLANCE_OP_DEL      1
#define BLANCE_OP_PROMOTE  2
#define BLANCE_OP_DEMOTE   3

typedef struct blance_moves_problem {
    int32_t n_parts;
    int32_t n_states;             /* M = len(states)                                      */
    int32_t favor_min_nodes;      /* favorMinNodes                                        */
    const int32_t* beg_off;       /* [P*(M+1) + 1] CSR of begNodesByState over p*(M+1)+s  */
    const int32_t* beg_nodes;     /* node ids (any non-negative numbering)                */
    const int32_t* end_off;       /* [P*(M+1) + 1] the same for endNodesByState           */
    const int32_t* end_nodes;
} blance_moves_problem;

typedef struct blance_moves_result {
    int32_t* op_off;              /* [P + 1] moves of partition p: op_off[p]..op_off[p+1] */
    int32_t* op_node;             /* [capacity] NodeStateOp.Node                          */
    int32_t* op_state;            /* [capacity] NodeStateOp.State as a state id, -1 = ""  */
    int32_t* op_kind;             /* [capacity] BLANCE_OP_*                               */
    int64_t  capacity;            /* in: >= beg_off[last] + end_off[last] always suffices */
    double   device_ms;           /* out                                                  */
} blance_moves_result;

int blance_calc_moves(blance_ctx* ctx, const blance_moves_problem* pb, blance_moves_result* res);

/* ---- plan quality: what a caller would otherwise get by re-walking the
 * result map -- countStateNodes (plan.go:374-399) applied to the map the last blance_plan /
 * blance_plan_resident produced, reduced per state over the nodes of nodesNext (plan.go:77).
 * Arrays are the caller's, n_states entries each (state id order). */
typedef struct blance_plan_stats {
    int32_t n_states;        /* in: capacity of the arrays below (>= the problem's n_states) */
    int32_t n_nodes_next;    /* out: nodes counted (nodesAll minus nodesToRemove) */
    int64_t* load_min;       /* out: smallest weighted load of a node in this state */
    int64_t* load_max;
    int64_t* load_sum;       /* out: sum of the loads = sum over partitions of weight * len(list) on live nodes */
    int64_t* load_sumsq;     /* out: sum of squares (variance = sumsq / n - (sum / n)^2) */
    int32_t* nodes_used;     /* out: nodes with load > 0 */
    int64_t* unmet_slots;    /* out: sum over partitions of max(0, constraints - len(list)); warnings of plan.go:231-234 */
    int64_t* rule_violations; /* out (ABI 4; may be NULL): (partition, slot) pairs of this state whose node breaks one of the
                              * state's hierarchy rules against the partition's top priority node or an EARLIER node of the
                              * same list -- outside leaves(findAncestor(a, IncludeLevel)) or inside
                              * leaves(findAncestor(a, ExcludeLevel)) of such an anchor a (plan.go:723-753); what the
                              * fallback of plan.go:216-218 produces when racks disappear.  0 for states without rules */
} blance_plan_stats;

int blance_plan_stats_get(blance_ctx* ctx, blance_plan_stats* stats);

/* ---- the partition moves of the plan the context holds (additive to ABI 6: look the symbols up before use) --------
 * What the orchestrator needs next (orchestrate.go:273-287), from the maps where they lie on the device: for the map
 * the last blance_plan / blance_plan_resident of this context produced (the precondition of blance_plan_stats_get),
 * out receives exactly what blance_calc_moves would return for
 *   CalcPartitionMoves(sortStateNames(model), prevMap[name].NodesByState, nextMap[name].NodesByState, favor_min_nodes)
 * over every partition of partitionsToAssign in partition id order: prevMap as it was uploaded (before the write-back
 * of plan.go:49-52, however many plans ran since), node ids in the problem's own id space, an absent list counts as
 * empty on either side, a partition with !part_in_prev has an empty begin map.  beg_other: prevMap[name]'s nodes under
 * state keys that are not in the model, with the meaning blance_batch.h documents for blance_batch_moves; they only
 * feed flattenNodesByState (moves.go:60-64).
 * Count only: op_node, op_state and op_kind all NULL and capacity 0 -- the three counters are written and nothing else
 * is downloaded (op_off may then be NULL too; it is filled when given).  The counters are written on every successful
 * call.  Capacity: blance_plan_moves_capacity() always suffices; a smaller one is accepted when the plan's moves fit.
 * When they do not, the call returns BLANCE_ERR_CAPACITY with the counters written (size a retry by n_moves) and no
 * array touched.
 * BLANCE_ERR_BAD_ARG, nothing launched and nothing written: a NULL argument; nothing planned yet, or the context holds
 * no problem (as after any blance_plan_batch*); a plan with iterations == 0 (PlanNextMapEx returned no map); op_off
 * NULL while the move arrays are given, or only some of the three given; beg_other with one pointer NULL, offsets that
 * do not start at 0 or are not monotone, an id outside [0, n_nodes_ext).
 * The call does not disturb the context: blance_download, blance_plan_stats_get and blance_plan_resident behave after
 * it as without it.  On a context with a communicator it makes no collective (every rank holds the whole map). */
typedef struct blance_plan_moves {
    int32_t favor_min_nodes;          /* in */
    const int32_t* beg_other_off;     /* in, may both be NULL: CSR over partitions, [P + 1], ids < n_nodes_ext */
    const int32_t* beg_other_nodes;
    blance_moves_result out;          /* op_off [P + 1]; op_node / op_state / op_kind [capacity]; device_ms */
    int64_t n_moves;                  /* out: all moves */
    int64_t n_by_kind[4];             /* out: moves per BLANCE_OP_* */
    int64_t n_parts_moved;            /* out: partitions with at least one move */
} blance_plan_moves;

/* prev_off[P*M] + beg_other_off[P] + blance_result_capacity(pb): the bound of blance_batch_moves_capacity */
int64_t blance_plan_moves_capacity(const blance_problem* pb, const blance_plan_moves* mv);
int blance_plan_moves_get(blance_ctx* ctx, blance_plan_moves* mv);

/* ---- the map a context holds as PartitionMap JSON bytes (additive to ABI 6: look the symbols up before use) ----
 * json.Marshal(PartitionMap) (api.go:24-36) of the map the last blance_plan / blance_plan_resident of this context
 * produced, composed on the device from the planned lists where they lie: the bytes are exactly what
 * the host encoder of blance_wire.h returns for the view a caller would build from blance_download -- key = name = the
 * partition's name, every partition with a nodesByState map, one entry per (partition, state) whose out_kind is not
 * BLANCE_LIST_ABSENT, `null` for BLANCE_LIST_NIL, the node names in list order for BLANCE_LIST_SET.
 *
 * blance_plan_wire_names gives the context the names of the problem it holds (after blance_upload or blance_plan; P, NX
 * and M are that problem's n_parts, n_nodes_ext and n_states): byte blobs with n + 1 offsets, as blance_wire_view's.
 * Everything that depends on the names alone is done here, once: every string escaped, the partitions sorted by name
 * bytewise, the states sorted by name.  The call copies what it needs and retains nothing of the caller's.  The names stay
 * with the context across blance_plan_resident; whatever replaces the context's problem drops them (blance_upload,
 * blance_plan, any blance_plan_batch*).  Errors, with nothing uploaded and earlier names left as they were:
 * BLANCE_ERR_BAD_ARG for a NULL argument, no problem on the context, offsets that do not start at 0 or are not monotone,
 * two states with one name; BLANCE_ERR_UNSUPPORTED for two partitions with one name (the reference's rv[partition.Name],
 * plan.go:326-329, would keep one of them) and for an escaped blob of 2^31 bytes or more. */
typedef struct blance_wire_names {
    const char* part_bytes;  const int64_t* part_off;   /* [P + 1]  partition names by partition id */
    const char* node_bytes;  const int64_t* node_off;   /* [NX + 1] node names by node id */
    const char* state_bytes; const int64_t* state_off;  /* [M + 1]  state names by state id */
} blance_wire_names;
int blance_plan_wire_names(blance_ctx* ctx, const blance_wire_names* names);
/* *need = the document's length; buf receives the document when cap >= *need, else the call returns BLANCE_ERR_CAPACITY
 * with *need written and buf untouched.  Size only: buf == NULL and cap == 0 -- the sizing pass alone runs, *need is
 * written and nothing else is downloaded.  buf in blance_host_alloc memory is written by DMA where it lies, any other
 * buffer through the context's staging buffer.  device_ms (may be NULL): the device's time for the kernels of the call.
 * BLANCE_ERR_BAD_ARG, nothing launched: a NULL ctx or need, buf NULL with cap > 0, nothing planned yet or no problem on
 * the context, a plan with iterations == 0, no names set for the problem the context holds.  BLANCE_ERR_UNSUPPORTED: a
 * document of 2^31 bytes or more.  The call does not disturb the context (blance_download, blance_plan_stats_get,
 * blance_plan_moves_get and blance_plan_resident behave after it as without it) and makes no collective. */
int blance_plan_wire_get(blance_ctx* ctx, char* buf, size_t cap, size_t* need, double* device_ms);

/* ---- a PartitionMap document decoded on the device (additive to ABI 6: look the symbols up before use) ----
 * The way in that mirrors blance_plan_wire_get: json.Unmarshal(document, &PartitionMap{}) against a DICTIONARY of names
 * given beforehand, straight into the id space and the layout blance_problem uses for prev_* and assign_* -- a caller points
 * prev_off / prev_nodes / prev_kind at the output (part_in_prev[p] = part_kind[p] != BLANCE_LIST_ABSENT) and calls
 * blance_upload.
 *
 * Exact or refused, never guessed.  BLANCE_OK only when the document is valid JSON of the shape in blance_wire.h AND lies
 * inside the subset below; the result then equals what blance_wire_decode gives after mapping its names to the dictionary's
 * ids.  Everything else is a REFUSAL: BLANCE_ERR_UNSUPPORTED, a reason code in `refusal`, the byte offset of the record or
 * token that caused it in `refusal_at` (the smallest (offset, reason) of all there are), nothing written to the caller's
 * arrays.  The caller then takes the host decoder, which reports syntax and type errors as before.  The device never
 * accepts a document the host decoder rejects or decodes differently.
 * Inside the subset: JSON whitespace anywhere between tokens; partitions, the two fields of a partition and the state keys
 * in any order; strings with any valid escape (\" \\ \/ \b \f \n \r \t, \uXXXX incl. valid surrogate pairs), compared
 * UNESCAPED with the raw names of the dictionary; bytes >= 0x80 that are well-formed UTF-8; nodesByState null or missing
 * (both: BLANCE_LIST_NIL in part_kind); a state's list null, [] or a list of known node names, duplicates kept; partitions
 * of the dictionary missing from the document; `{}`.  One limit of SIZE belongs to the subset, because one device thread
 * parses one record: every record (a key, its value and the whitespace up to the next key) is shorter than 1 MiB, and so
 * are the bytes in front of the first record and the whitespace behind the closing brace.  What is longer is refused
 * (BLANCE_WIRE_REFUSED_RECORD_TOO_LONG, at the record's offset; at 0 for the bytes in front of the first record, at the
 * last record's offset for the whitespace behind the document), and the whole document is shorter than 2^31 bytes.
 * Refused (BLANCE_WIRE_REFUSED_*): see the codes.  The host decoder accepts some of these with Go's semantics (a repeated
 * key replaces, a field matches case-insensitively, an unknown field is skipped, U+FFFD for bad UTF-8).
 *
 * The dictionary (device hash tables over the names and the raw names) is independent of whatever problem the context
 * holds -- the call is made to BUILD the problem -- and survives blance_upload / blance_plan; it is owned by the context and
 * goes with it at the latest.  n_parts / n_nodes_ext / n_states: the names' counts (names->*_off hold one more).  Errors:
 * BLANCE_ERR_BAD_ARG for a NULL argument, a negative count, offsets that do not start at 0 or are not monotone, two states
 * or two nodes with one name, n_parts * n_states of 2^31 - 1 or more; BLANCE_ERR_UNSUPPORTED for two partitions with one
 * name and for a blob of 2^31 bytes or more.
 *
 * blance_wire_decode_device: `json` in blance_host_alloc memory is read by DMA where it lies, any other buffer through the
 * context's staging buffer.  Count only: nodes == NULL and capacity == 0 -- n_node_refs and n_parts_seen are written and no
 * array is (part_kind, off and kind may then be NULL too).  A capacity below n_node_refs: BLANCE_ERR_CAPACITY with
 * n_node_refs and n_parts_seen written and no array touched.  BLANCE_ERR_BAD_ARG, nothing launched: a NULL ctx, dictionary,
 * out or (with len > 0) json; a dictionary of another context; nodes NULL with capacity > 0 or capacity < 0; part_kind, off
 * or kind NULL while nodes is given.  The call holds the context's lock and leaves the context as it found it:
 * blance_plan_resident, blance_download, blance_plan_stats_get, blance_plan_moves_get and blance_plan_wire_get answer after
 * it as without it.  It makes no collective. */
#define BLANCE_WIRE_REFUSED_GRAMMAR             1  /* not JSON (also: a document that ends early)                       */
#define BLANCE_WIRE_REFUSED_TYPE                2  /* a JSON value of another type than the shape has there             */
#define BLANCE_WIRE_REFUSED_NULL_DOCUMENT       3  /* the document is `null` (a nil PartitionMap)                       */
#define BLANCE_WIRE_REFUSED_UNKNOWN_PARTITION   4  /* a key that is not a partition name of the dictionary              */
#define BLANCE_WIRE_REFUSED_UNKNOWN_STATE       5
#define BLANCE_WIRE_REFUSED_UNKNOWN_NODE        6
#define BLANCE_WIRE_REFUSED_REPEATED_PARTITION  7  /* offset: the second record with that key                           */
#define BLANCE_WIRE_REFUSED_REPEATED_STATE      8
#define BLANCE_WIRE_REFUSED_REPEATED_FIELD      9
#define BLANCE_WIRE_REFUSED_UNKNOWN_FIELD      10  /* a field name that is not exactly name or nodesByState             */
#define BLANCE_WIRE_REFUSED_NULL_PARTITION     11
#define BLANCE_WIRE_REFUSED_NAME_MISSING       12  /* offset: the record                                                */
#define BLANCE_WIRE_REFUSED_NAME_DIFFERS       13  /* name is not the key (or null)                                     */
#define BLANCE_WIRE_REFUSED_NULL_ELEMENT       14  /* null inside a state's list                                        */
#define BLANCE_WIRE_REFUSED_INVALID_UTF8       15
#define BLANCE_WIRE_REFUSED_UNPAIRED_SURROGATE 16
#define BLANCE_WIRE_REFUSED_CONTROL_CHARACTER  17  /* a raw byte below 0x20 inside a string                             */
#define BLANCE_WIRE_REFUSED_RECORD_TOO_LONG    18  /* one partition's record (or the space around it) of 1 MiB or more  */
#define BLANCE_WIRE_REFUSED_DOCUMENT_TOO_LONG  19  /* 2^31 bytes or more: refused before anything is launched           */

typedef struct blance_wire_dict blance_wire_dict;   /* opaque; owned by the context it was made on */
int  blance_wire_dict_create(blance_ctx* ctx, const blance_wire_names* names, int32_t n_parts, int32_t n_nodes_ext,
                             int32_t n_states, blance_wire_dict** out);
void blance_wire_dict_destroy(blance_ctx* ctx, blance_wire_dict* dict);

typedef struct blance_wire_lists {
    uint8_t* part_kind;   /* [P]  BLANCE_LIST_ABSENT: key not in the document; NIL: nil nodesByState; SET: a map */
    int32_t* off;         /* [P*M + 1]  CSR over (p * M + state), as prev_off */
    uint8_t* kind;        /* [P*M]      BLANCE_LIST_*, as prev_kind */
    int32_t* nodes;       /* [capacity] node ids in list order, as prev_nodes */
    int64_t  capacity;    /* in */
    int64_t  n_node_refs, n_parts_seen;       /* out, also with BLANCE_ERR_CAPACITY */
    int32_t  refusal;     /* out: BLANCE_WIRE_REFUSED_*, 0 when accepted */
    int64_t  refusal_at;  /* out: byte offset, -1 when accepted */
    double   device_ms, total_ms;             /* out: the kernels of the call (of a count, a refusal or a capacity error:
                                                 the record split and the first parse; 0 when the call ends before that);
                                                 the whole call incl. the copies, whatever the status */
} blance_wire_lists;
int blance_wire_decode_device(blance_ctx* ctx, const blance_wire_dict* dict, const char* json, size_t len,
                              blance_wire_lists* out);

/* ---- the planned map as the next call's prevMap (additive to ABI 6: look the symbol up before use) ----
 * A planner used in a loop plans, a node leaves or joins, and it plans again with prevMap = partitionsToAssign = the
 * map it just made.  blance_plan_adopt makes that hand-over where the map lies: no list is downloaded
 * or uploaded.  Precondition: the context holds the map of its last blance_plan / blance_plan_resident
 * (blance_plan_moves_get's precondition).  After a successful call the context holds, as if uploaded, the problem P':
 *   - everything of the uploaded problem (sizes, model, stickiness, node and partition weights, part_order, hierarchy,
 *     rules, booster, max_iterations), except:
 *   - assign_* = prev_* = the planned map (out_off / out_nodes / out_kind of its download); part_in_prev = 1 and
 *     part_prev_never_equal = 0 for every partition;
 *   - node_removed, node_added, nodes_to_add_nil as given here;
 *   - keep_prev_only == 0: n_prev = n_parts, n_loads = 0 (prevMap' is the planned map);
 *     keep_prev_only == 1: prevMap' also keeps the old prevMap's partitions outside partitionsToAssign -- the load
 *     entries with load_first_sweep_only == 0 stay, the others go (the stored map replaces them), n_prev = the old
 *     n_prev + the partitions that had part_in_prev == 0.
 * Nothing is planned yet then: blance_plan_resident plans P'; until it has, blance_download, blance_plan_stats_get,
 * blance_plan_moves_get and blance_plan_wire_get refuse.  The names of blance_plan_wire_names and every blance_wire_dict
 * stay valid (same partitions, nodes, states).  After the next plan blance_plan_moves_get gives the moves from the
 * adopted map to the new one; its beg_other must be NULL (P' has no prevMap keys outside the model).  Result buffers
 * sized for the uploaded problem still suffice: blance_result_capacity of P' is not above the uploaded problem's, and
 * P' has at most that many prevMap entries (blance_plan_moves_capacity: twice that).
 * Refused before anything is touched (the context stays as it was, blance_download still answers): BLANCE_ERR_BAD_ARG
 * for nothing planned (also: after any blance_plan_batch*), a plan with iterations == 0, a NULL array (all that
 * blance_validate refuses about node_removed / node_added: they are byte flags, any value is read as zero or not), a
 * non-zero `reserved`; BLANCE_ERR_UNSUPPORTED while a communicator is set (blance_comm_set / blance_comm_init_rccl) -- adopting
 * a plan sharded over ranks is deliberately not offered: every rank would have to adopt in step --, and for a P'
 * blance_validate would refuse (partition weights overflowing the load tables).  A device failure part-way leaves
 * the context without a problem, as a failed blance_upload does. */
typedef struct blance_adopt {
    const uint8_t* node_removed;    /* [n_nodes_ext] nodesToRemove of the NEXT call                 */
    const uint8_t* node_added;      /* [n_nodes_ext] nodesToAdd of the next call                    */
    int32_t        nodes_to_add_nil;
    int32_t        keep_prev_only;  /* 0: prevMap' = nextMap.  1: prevMap' = nextMap plus the
                                       partitions of the old prevMap outside partitionsToAssign   */
    int32_t        reserved[4];     /* zero */
} blance_adopt;
int blance_plan_adopt(blance_ctx* ctx, const blance_adopt* ad);

/* ---- a PartitionMap document as the next call's prevMap (additive to ABI 6: look the symbol up before use) ----
 * blance_plan_adopt hands over the map this context planned.  A caller that reads the map the cluster really has -- a
 * json.Marshal(PartitionMap) document, the planned one only when every move of the last round completed -- plans with
 * prevMap = partitionsToAssign = that document.  blance_wire_adopt decodes it on the device as blance_wire_decode_device does
 * and makes the decoded lists the lists of the problem the context holds, where they lie: per round only
 * the document's bytes cross the bus.
 * Precondition: the context holds an uploaded problem (a plan is not required: upload a skeleton once, then adopt
 * documents) and has no communicator.  dict, json, len: as for blance_wire_decode_device; the dictionary's n_parts /
 * n_nodes_ext / n_states equal the held problem's, and it is the caller's contract that its ids are the problem's ids.
 * After a successful call the context holds, as if uploaded, the problem P': everything of the held problem, except
 *   - prev_off / prev_nodes / prev_kind = the decoded lists; part_in_prev[p] = (part_kind[p] != BLANCE_LIST_ABSENT);
 *     part_prev_never_equal[p] = (part_kind[p] == BLANCE_LIST_NIL) (a nil NodesByState never DeepEquals a result);
 *   - assign_too == 1: assign_* = the same lists (prevMap' = partitionsToAssign' = the document);
 *     assign_too == 0: assign_* stay as they are on the context, uploaded or adopted last;
 *   - node_removed, node_added, nodes_to_add_nil as given here;
 *   - n_prev = n_parts_seen, plus with keep_prev_only == 1 the old prevMap's keys outside partitionsToAssign;
 *   - keep_prev_only == 1: the load entries with load_first_sweep_only == 0 stay, the others go; 0: n_loads = 0.
 * Nothing is planned then: blance_plan_resident plans P'; until it has, the readers refuse as after blance_plan_adopt.
 * Wire names and every blance_wire_dict stay valid.  After the next plan blance_plan_moves_get gives the moves from the
 * document's map (beg_other NULL).  result_capacity is blance_result_capacity of P' (the sum of max(k, length) over its lists
 * to assign): with assign_too it can exceed the uploaded problem's, size blance_result by it.
 * Every refusal is decided before the problem is touched; after one blance_download, the three readers and
 * blance_plan_resident answer as before the call.
 *   1. the document's own: BLANCE_ERR_UNSUPPORTED, refusal / refusal_at exactly as blance_wire_decode_device gives them,
 *      why == 0;
 *   2. the document decoded but P' is no problem this context can take: BLANCE_ERR_UNSUPPORTED, refusal == 0, `why` one of
 *      BLANCE_WIRE_ADOPT_* (the first of them in the order below), why_at the smallest offending p * n_states + state, or p;
 *   3. BLANCE_ERR_BAD_ARG: a NULL argument, a dictionary of another context, no problem on the context, dictionary sizes
 *      that differ from the problem's, a non-zero `reserved`; BLANCE_ERR_UNSUPPORTED with refusal == why == 0: a communicator.
 * A device failure behind the refusals leaves the context without a problem, as a failed blance_upload does. */
#define BLANCE_WIRE_ADOPT_LIST_TOO_LONG        1  /* a list longer than the row stride the upload fixed (the longest list or
                                                     constraint of the uploaded problem): upload again.  why_at: p * M + state */
#define BLANCE_WIRE_ADOPT_PARTITION_MISSING    2  /* assign_too and a partition of the dictionary is not in the document (the
                                                     partitions to assign would change).  why_at: p                           */
#define BLANCE_WIRE_ADOPT_DUPLICATE_NODE       3  /* assign_too and a node twice in one list (duplicates in a document that
                                                     becomes prevMap only are kept).  why_at: p * M + state                   */
#define BLANCE_WIRE_ADOPT_REMOVED_WITHOUT_PREV 4  /* a partition is not in the document, node_removed names a node and some
                                                     state has constraints > 0: the reference panics (plan.go:545).  why_at: p */
#define BLANCE_WIRE_ADOPT_LOAD_OVERFLOW        5  /* blance_validate's bound on the int32 load tables, for P'.  why_at: -1      */
/* (no typedef: in C the function below would collide with it; write `struct blance_wire_adopt`) */
struct blance_wire_adopt {
    /* in */
    const blance_wire_dict* dict;
    const char*    json;
    size_t         len;
    const uint8_t* node_removed;    /* [n_nodes_ext] nodesToRemove of the next call */
    const uint8_t* node_added;      /* [n_nodes_ext] nodesToAdd of the next call    */
    int32_t        nodes_to_add_nil;
    int32_t        assign_too;
    int32_t        keep_prev_only;
    int32_t        reserved[4];     /* zero */
    /* out */
    int32_t        refusal;         /* BLANCE_WIRE_REFUSED_*, 0 when the document decoded */
    int64_t        refusal_at;      /* byte offset, -1 when it decoded */
    int64_t        n_node_refs, n_parts_seen;
    int64_t        result_capacity; /* of P' (written on success) */
    int32_t        why;             /* BLANCE_WIRE_ADOPT_*, 0 when P' was taken */
    int64_t        why_at;          /* -1 when why == 0 */
    double         device_ms, total_ms;   /* the call's kernels (the decoder's, the summary, the write); the whole call */
};
int blance_wire_adopt(blance_ctx* ctx, struct blance_wire_adopt* wa);

/* ---- one plan on several GPUs (BASELINE.json config 4) ------------------------------------
 * The steps of a state pass that runs as region chains (one chain per hierarchy region)
 * shard over the ranks by region: every rank holds the whole problem (upload the same problem on
 * every rank) and runs the chains of its contiguous slice of the regions.  Per such pass the ranks
 * make exactly TWO collectives -- pass boundaries are the only exact exchange points of
 * plan.go:253-303:
 *   A. one int32 sum all-reduce of [8 pass flags | change of the per-node load vector
 *      (stateNodeCounts, plan.go:94)]: (n_states + 1) * n_nodes_ext + 8 words;
 *   B. one all-gather of the pass outputs: a rank's steps are contiguous in chain order, every
 *      rank contributes its slice (padded to the longest slice).
 * Everything else (flat passes, ordering, convergence test) is computed by every rank identically,
 * so all ranks return the same result, bit-identical to a single-rank plan.
 * Collectives: the library's own RCCL communicator (blance_comm_init_rccl; one process per GPU,
 * the 128-byte id of blance_comm_unique_id() made on rank 0 and handed to the others by the host),
 * or an embedder's (blance_comm_set; used by the tests: gloo ranks over the SIMT emulator, and G
 * contexts on ONE MI355X whose buffers the hook sums / gathers).
 * Every rank must make the same sequence of plan calls.  A rank that fails before collective A
 * still takes part in it with a poison flag, so that all ranks return BLANCE_ERR_COMM together;
 * after any failed sharded call the communicator is invalid (destroy the contexts). */
typedef struct blance_comm {
    int32_t rank, n_ranks;
    /* in-place sum over the ranks of `count` int32 values at `device_buf` (device memory of this
     * context); called between kernels with the stream idle; 0 = ok */
    int (*allreduce_sum_i32)(void* user, int32_t* device_buf, int64_t count);
    void* user;
    /* in-place all-gather: `device_buf` holds n_ranks blocks of `count_per_rank` int32 values, this
     * rank's block (at rank * count_per_rank) is filled in; on return every block is.  May be NULL:
     * the outputs are then summed with allreduce_sum_i32 (every rank's foreign slices zeroed). */
    int (*allgather_i32)(void* user, int32_t* device_buf, int64_t count_per_rank);
} blance_comm;

int blance_comm_unique_id(void* id_out_128 /* 128 bytes */);
int blance_comm_init_rccl(blance_ctx* ctx, int32_t n_ranks, int32_t rank, const void* id_128);
int blance_comm_set(blance_ctx* ctx, const blance_comm* comm /* NULL: back to a single rank */);
/* collectives made / int32 words moved by this context's sharded plans so far */
int blance_comm_stats(blance_ctx* ctx, int64_t* calls, int64_t* words);
/* (ABI 5) device time, in ms, this context's plans have spent inside RCCL collectives so far: an event on either side of
 * every ncclAllReduce / ncclAllGather on the planner's stream (0 for an embedder's own collectives, which run on the host) */
int blance_comm_time_ms(blance_ctx* ctx, double* ms);

/* 1 if this library is the GPU-less SIMT emulator build of the tests (its "device" memory is host
 * memory), 0 for the gfx950 product. */
int blance_is_emulated(void);

/* Validate a problem without touching a device (sizes, id ranges, supported
 * envelope).  Same status codes as blance_plan. */
int blance_validate(const blance_problem* pb);

/* Text of the last error on this thread ("" if none). */
const char* blance_last_error(void);

int blance_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* BLANCE_HIP_H */
