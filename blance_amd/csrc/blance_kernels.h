// Device-side data layout and kernel parameter blocks of the MI355X planner.
// Everything here is plain int32/uint8 SoA in HBM; see DESIGN.md "Data layout".
#pragma once
#include <stdint.h>

namespace blance {

constexpr int kListAbsent = 0, kListNil = 1, kListSet = 2;   // include/blance_hip.h BLANCE_LIST_*

constexpr int kMaxK = 8;         // largest supported Constraints per state
constexpr int kMaxAnchors = 9;   // hierarchy anchors per fold: 1 + (#rules of a state) * k <= 9
constexpr int kMaxStates = 16;
constexpr int kRecHead = 4;      // step-record header words: partition, weight, stickiness (fp64)
constexpr int kLpTab = 512;      // chain kernel LDS tables: c / NP for c < kLpTab ...
constexpr int kFfTab = 2048;     // ... and (0.001 * t) / NP for t < kFfTab

// One rule's include/exclude leaf intervals for one anchor (plan.go:723-734):
// leaves(findAncestor(a, IncludeLevel)) = [alo, ahi), leaves(findAncestor(a, ExcludeLevel)) = [blo, bhi).
struct AnchorSet { int32_t alo, ahi, blo, bhi; };

// Parameters of one state pass (assignStateToPartitions, plan.go:253-303).
struct PassParams {
    int32_t N, NX, M, L, P;
    int32_t beg, end;       // steps [beg, end) of the pass order run by this launch
    int32_t s;              // state id of this pass
    int32_t k;              // constraints
    int32_t top_state;
    int32_t NP;             // len(prevMap) of this sweep (plan.go:161)
    int32_t RW, OW;         // words per step record / per step output
    int32_t higher_mask;    // bit t: state t has Priority < Priority of s (plan.go:148)
    int32_t hier;           // HierarchyRules != nil
    int32_t rule_begin, rule_end;
    int32_t booster_kind;
    int32_t n_alive;
    int32_t vertex_empty_anchor;   // anchor index of "" (= NX)
    const uint8_t* alive;          // [NX] node is in nodesNext (plan.go:77)
    const int32_t* node_weight;    // [NX]
    const uint8_t* node_has_weight;
    const int32_t* node_leaf_pos;  // [NX]
    const AnchorSet* anchors;      // [n_rules][NX + 1]
    int32_t* cnt;                  // [(M + 1) * NX] stateNodeCounts
    int32_t* ntn;                  // [(NX + 1) * N] nodeToNodeCounts, zeroed per pass
    const int32_t* rec;            // [P * RW] step records in pass order
    int32_t* out;                  // [P * OW] chosen nodes per step
    int32_t* warn_part;
    int32_t* warn_state;
    int32_t* warn_count;
    int32_t* err;                  // device error word (interval overflow ...)
    int32_t spec;                  // try verified-stay speculation (flat passes; LDS mirrors sized by the host)
    long long* spec_count;         // steps committed as verified stays (statistics, may be null)
    // k_pass_queue (k_pass_queue.h) only:
    uint32_t* ntn_bits;            // [(NX + 1) * BW] one bit per nodeToNodeCounts entry: "is not zero" (BW = words per row, 16-byte rows)
    int32_t* stop;                 // out: [0] first step of [beg, end) NOT done (end: all done), [1] why (kQStop*)
    long long* qstats;             // out, may be null: [0] moving steps, [1] with matrix reads, [2] window rebuilds, [3] dense steps
};

// Parameters of a state pass run as independent per-region chains (DESIGN.md
// "Region chains"): one wave64 per hierarchy region walks that region's steps.
//
// Compact chain step record (k_gather_chain), kCW words, everything already
// translated to leaf indices local to the region:
//   1 weight   2,3 stickiness (fp64)   4 top priority node's leaf
//   0 index of the step in pass order
//   5 counts: own (inside the region) | higher << 8 | lower << 16 | (state list present) << 24
//     | (holds nodes of this state outside the region) << 25
//   6 exclude class of the top priority node
//   7..10  leaves of the nodes the partition holds in this state (-1 padded)
//   11..14 leaves of its higher priority nodes inside the region (never candidates)
//   15..18 leaves of its lower priority nodes inside the region, 19..22 their states
//   23 leaves covered by the top priority node's exclude class
constexpr int kChainOwn = 4, kChainHigh = 4, kChainLow = 4;
constexpr int kChainStage = 256;                 // steps whose records / outputs one staging round of k_pass_chain holds in LDS
constexpr int kChainMaxLeaves = 512;             // leaves of one region (one wave64, 8 leaves per lane)
// k_cycle.h's table of the upload: per alive index a, four words -- its region r_a, its rank q_a among the region's nodes of
// nodesNext, the global leaf of alive_ids[a], the region's count c_r of such nodes.
constexpr int kCycWords = 4;
constexpr int kCycRegion = 0, kCycRank = 1, kCycLeaf = 2, kCycCount = 3;
constexpr int kCW = 24;
constexpr int kCOwn = 7, kCHigh = 11, kCLow = 15, kCLowState = 19;

// A launch the host enqueues BEFORE it has read the words that decide whether it should run (one round trip less per
// decision): the kernel looks at the words itself.  closed = some word flags[b], b a set bit of mask, is non-zero.
struct Gate {
    const int32_t* flags;
    uint32_t mask;
};
constexpr Gate kNoGate = {nullptr, 0u};

// The int32 words of the context's `scalars` buffer (DESIGN.md 4.5 has the table).  The host hands the kernels pointers
// into it; a Gate's flags is always scalars + kScalFlags.
enum ScalarWord : int {
    kScalWarnCount = 0,       // warnings so far
    kScalNotMatch = 1,        // the sweep's convergence word: some partition's lists changed
    kScalErr = 2,             // device error word (interval overflow ...)
    kScalFlags = 4,           // the eight chain flags (ChainFlag), zeroed per sweep and per chain pass
    kScalSpecCount = 12,      // int64: steps the sequential passes committed as verified stays
    kScalSortVarying = 14,    // uint64: the key bits that vary (k_sort_varbits)
    kScalQueueStop = 16,      // k_pass_queue's two stop words
    kScalQueueStats = 18,     // k_pass_queue's four int64 statistics
    kScalReadback = 32,       // the host copies words [0, kScalReadback) back once per sweep
    kScalFlatScan = 36,       // the flat bulk driver's own: k_flat_scan_min's two results ...
    kScalFlatBad = 38,        // ... and k_fresh_excl_apply's first bad step
    kScalWords = 64,
};
// Words of a Gate's flags, i.e. relative to kScalFlags.  [0, kChainFlags): what the chain passes' kernels report --
// k_chain_classify, k_gather_chain, k_pass_chain*, k_period_judge.  Behind them, outside what a chain pass resets:
// k_stay_by_top's "not all stays"; BLANCE_SPECULATE=fail; k_flat_stay_live's "the sweep's first pass is NOT one run of stays".
enum ChainFlag : int {
    kFlagNotLocal = 0,        // a step is not region-local / does not fit the compact record
    kFlagEscaped = 1,         // a chain had to escape (flat mode: it stopped)
    kFlagStaySteps = 2,       // steps committed as verified stays
    kFlagStayBatches = 3,     // ... in this many batches
    kFlagStopAt = 4,          // flat mode: first step not done
    kFlagStopRange = 5,       // flat mode: stopped by the key range
    kFlagOrphans = 6,         // nodes of the state that lie in no region
    kFlagEvents = 7,          // nodes outside their partition's region
    kChainFlags = 8,
    kFlagStayMoved = 22, kFlagForced = 23, kFlagTopMoved = 24,
    kFlagHandedOff = 25,      // steps k_pass_chain handed off: stays, if k_stay_by_top's verdict stands (a count, never in a Gate's mask)
};
constexpr int kGateWords = 32;                   // a Gate's mask has one bit per word
static_assert(kScalErr < kScalFlags && kScalFlags + kChainFlags <= kScalSpecCount && kScalSpecCount + 2 <= kScalSortVarying &&
              kScalSortVarying + 2 <= kScalQueueStop && kScalQueueStop + 2 <= kScalQueueStats &&
              kScalQueueStats + 8 <= kScalFlags + kFlagStayMoved && kFlagStayMoved < kFlagForced && kFlagForced < kFlagTopMoved,
              "the scalar words overlap");
static_assert(kScalSpecCount % 2 == 0 && kScalSortVarying % 2 == 0 && kScalQueueStats % 2 == 0, "a 64-bit scalar word is not 8-byte aligned");
static_assert(kFlagTopMoved < kGateWords && kChainFlags <= kGateWords, "a Gate's mask cannot name the word");
static_assert(kScalFlags + kFlagHandedOff < kScalReadback && kFlagTopMoved < kFlagHandedOff && kScalQueueStats + 8 <= kScalReadback,
              "the per-sweep readback misses a word the host decides on");
static_assert(kScalFlatScan >= kScalFlags + kGateWords && kScalFlatScan >= kScalReadback && kScalFlatScan + 2 <= kScalFlatBad &&
              kScalFlatBad < kScalWords, "the flat driver's words must lie outside what a Gate can address");

struct ChainParams {
    int32_t N, NX, M, L;
    int32_t s, k, NP, OW;
    int32_t booster_kind;
    int32_t n_regions, ntn_in_lds;
    int32_t region_base, n_launch; // regions [region_base, region_base + n_launch) run in this launch (a rank of a
                                   // sharded plan runs a slice of the regions)
    int32_t cls_run;               // k_pass_chain_planes: S if every exclude class of the rule is an aligned run of S = 2^e <= 64
                                   // leaves that all carry nodes (racks of equal size), else 0
    int32_t flat;                  // the whole cluster is ONE region and every node its own exclude class:
                                   // a state pass without hierarchy rules (leaf index = node id); a chain that
                                   // cannot go on stops, keeps what it did and reports the step in flags[kFlagStopAt]
    const int32_t* reg_lo;         // [n_regions] leaf interval of the region
    const int32_t* reg_hi;
    const int32_t* reg_off;        // [n_regions + 1] step range of the region in chain order
    const int32_t* seg_beg;        // k_pass_chain_planes / k_pass_chain_blank, optional (k_period.h): [n_regions] the launch walks steps
    const int32_t* seg_end;        // [seg_beg[r], seg_end[r]) of region r's chain instead of all of it
    const int32_t* leaf_node;      // [n_leaves] node id at a leaf position, -1 if none
    const int32_t* leaf_cls;       // [n_leaves] exclude class of the leaf's node inside its region, -1 if none
    const int32_t* cls_size;       // [n_leaves] leaves covered by class c of the region at reg_lo + c
    const uint8_t* alive;
    const int32_t* node_weight;
    const uint8_t* node_has_weight;
    int32_t* cnt;
    int32_t* cnt_out;              // k_pass_chain_blank: where the new counters go (committed by the host)
    int32_t* ntn;
    // A node the partition holds in this state OUTSIDE its region leaves it (plan.go:290-293)
    // whatever the step decides: a static event for the chain that owns the node, applied
    // before that chain's first step that comes later in pass order.
    const int32_t* ev_off;         // [n_regions + 1] events of the region: ev_perm[ev_off[r] .. ev_off[r + 1])
    const int32_t* ev_perm;        // event ids grouped by region, pass order inside a region
    const int32_t* ev_oi;          // [E] pass index of the step that causes the event
    const int32_t* ev_leaf;        // [E] leaf (local to the owning region) whose counters drop
    const int32_t* ev_w;           // [E] by this much
    const int32_t* crec;           // [P * kCW] compact step records in chain order
    int32_t* out;                  // [P * OW]
    int32_t waves;                 // waves of a region's workgroup: 0 = the launcher decides (8 when the LDS is there), 4, 8
    int32_t* flags;                // the chain flags (ChainFlag, below Gate)
    uint32_t gate;                 // k_pass_chain: words of flags[] (a Gate's mask) that, any of them set, make the launch return
};

// k_pass_chain's second parameter block (its HANDOFF instance reads it; beside ChainParams, not inside: the plain instance's
// scalar loads of ChainParams, and with them its register use, stay what they were)
struct ChainHandoff {
    // The hand-off (k_pass_chain): a region whose last stage was all stay rounds, with no event left and at
    // least handoff_min steps to go, stops at that stage boundary and stores the chain index of its first step not done;
    // k_stay_by_top checks the rest in parallel.  A region that never stops stores its chain's end.  Null / 0: no hand-off.
    // The steps handed off are added to flags[kFlagHandedOff] (one atomic per region; the statistics words kFlagStaySteps and
    // kFlagStayBatches count only what the kernel itself committed).
    int32_t* at;                   // [n_regions]
    int32_t min;
};

// k_stay_by_top (k_stay.h): a chain pass of stays verified by one thread per top priority node
constexpr int kStayMaxLeaves = 512;
struct StayParams {
    int32_t N, NX, M, s, k, NP, OW, booster_kind;
    const int32_t* wg_region;      // [grid] region of workgroup b ...
    const int32_t* wg_chunk;       // ... and which 64 leaves of it: leaf = reg_lo + 64 * chunk + lane
    const int32_t* reg_lo;
    const int32_t* reg_hi;
    const int32_t* leaf_node;
    const int32_t* leaf_cls;
    const int32_t* cls_size;
    const uint8_t* alive;
    const int32_t* node_weight;
    const uint8_t* node_has_weight;
    const int32_t* cnt;
    const int32_t* top_off;        // [n_leaves + 1]
    const int32_t* crec;           // compact step records, chain order
    const int32_t* top_order;      // chain indices grouped by top leaf
    int32_t* out;
    int32_t* flag;                 // set to 1 by any step that is not a certain stay
    Gate gate;                     // closed: the launch returns at once
    // Behind a chain kernel that handed off (ChainHandoff::at): region r's steps with a chain index below from[r] are
    // done -- they are replayed from `out` (the nodes they emitted bump the row), not tested and not written.  Null: every
    // step is tested, from an empty row.
    const int32_t* from;           // [n_regions]
    const int32_t* node_leaf_pos;  // [NX] global leaf of a node (with `from`: what a replayed step emitted, as leaves)
};


// Flat (no hierarchy rule) passes resolved in bulk: DESIGN.md "Flat bulk engine".
constexpr int kTopList = 8;      // smallest partition-independent scores kept for the stay test

struct FlatParams {
    int32_t N, NX, M, L, P;
    int32_t s, k, top_state, NP, RW, OW;
    int32_t higher_mask, booster_kind;
    const uint8_t* alive;
    const int32_t* node_weight;
    const uint8_t* node_has_weight;
    const int32_t* cnt;            // [(M + 1) * NX]
    const int32_t* tot;            // [NX] sum over states, refreshed by k_flat_prepare
    const double* g;               // [NX] partition-independent score of every node
    const double* top_g;           // [kTopList] smallest (g, node) among nodesNext
    const int32_t* top_n;
    const int32_t* row_count;      // [NX + 1] steps of this pass per top priority node
    int32_t* ntn;
    const int32_t* rec;
    int32_t* out;
    int32_t* scan;                 // [0] first step that is not a certain stay, [1] first not fresh-identical
    int32_t* scan_part;            // [2][scan_waves] per wave of k_flat_scan: its first such step, reduced by k_flat_scan_min
    int32_t scan_waves;
    int32_t int_keys;              // a fresh run's sort keys as the integers they are (NumPartitions == 0, no node has a weight: a
                                   // score is count + picks * weight exactly) instead of their fp64 images: fewer varying bytes,
                                   // one radix pass less; any order-preserving injection gives the same sorted values
};

// Many small problems in one launch, one workgroup each: DESIGN.md §4.8 "k_plan_batch".
constexpr int kBatchMaxNX = 256;       // node names of a batched problem (one thread per node, 64 or 256 threads)
constexpr int kBatchMaxP = 16384;      // partitions
constexpr int kBatchMaxL = 8;          // longest state list (constraints included)
constexpr int kBatchHdr = 8;           // output header words, kBo* below
// the header of a problem's output slice: sweeps made, converged, warnings, list entries, the kernel's error word, 1 once
// k_plan_batch is done with the problem, findBestNodes calls (low 31 bits)
enum { kBoIterations = 0, kBoConverged, kBoWarnings, kBoEntries, kBoError, kBoDone, kBoSteps };

#ifdef __HIPCC__
#define BLANCE_HOST_DEVICE __host__ __device__
#else
#define BLANCE_HOST_DEVICE
#endif
// k_plan_batch planned the problem exactly: what the kernels behind it and the host unpack.  Anything else goes the single path
BLANCE_HOST_DEVICE inline bool batch_planned(const int32_t* hdr) { return hdr[kBoDone] == 1 && hdr[kBoError] == 0; }

// One problem of a batch.  Its arrays are int32 words at fixed offsets inside three slices: input (packed by the host),
// scratch (the kernel's working state) and output (what the host unpacks into the caller's blance_result).
struct BatchDesc {
    int64_t in_base, sc_base, out_base;   // first word of the problem's slice in each block
    int32_t N, NX, M, P, L;
    int32_t n_loads, n_rules, max_iterations, n_prev, fresh, n_alive, any_removed;
    int32_t weights_nil, add_nil, hier_nil, booster_kind, top_state;
    int32_t cap, wcap;                    // list entries / warnings the output slice holds
    // input slice: state words [M][4] (priority, constraints, stickiness, has stickiness); rule_off [M + 1];
    // node words [NX][4] (weight, removed | added << 1 | has weight << 2, leaf position, 0); part_order [P];
    // partition words [P][2] (weight, has weight | in prevMap << 1 | never equal << 2); assign lists [P*M][L] and
    // headers [P*M] (length | kind << 16); the same for prevMap; loads [n_loads][4] (state, node, weight, first sweep
    // only); AnchorSet [n_rules][NX + 1]
    int32_t i_state, i_rule_off, i_node, i_order, i_part, i_alist, i_ahdr, i_plist, i_phdr, i_loads, i_anch;
    // scratch slice: live lists [P*M][L] + headers, prevMap lists [P*M][L] + headers, partition flags [P] (in prevMap |
    // never equal << 1), pass order [P], category by position [P], nodeToNodeCounts [NX + 1][max(N, 1)]
    int32_t s_live, s_lhdr, s_prv, s_phdr, s_pflag, s_order, s_cat, s_ntn;
    // output slice: header [kBatchHdr], out_off [P*M + 1], out_kind [P*M], out_nodes [cap], warn_part [wcap], warn_state [wcap]
    int32_t o_off, o_kind, o_nodes, o_wp, o_ws;
    // blance_plan_batch_docs: the problem's document was refused or goes the single path -- k_plan_batch marks it not done
    int32_t skip;
};

struct BatchParams {
    const BatchDesc* desc;
    const int32_t* in;
    int32_t* sc;
    int32_t* out;
    int32_t first;                        // desc index of workgroup 0 of this launch
};

// The moves of one batched problem (DESIGN.md §4.9 "k_batch_moves"): offsets relative to its BatchDesc's slices.
constexpr int kBatchMovesThreads = 256;
struct BatchMovesDesc {
    int32_t desc;                         // index of the problem's BatchDesc
    int32_t favor_min_nodes;
    int32_t i_ooff, i_onodes;             // input slice: beg_other CSR, offsets [P + 1] and node ids
    int32_t s_cnt, s_mv, stride;          // scratch slice: move counts [P], each partition's moves [P][stride]
    int32_t o_moff, o_mops, cap;          // output slice: op_off [P + 1], moves [cap] as node | (state + 1) << 16 | kind << 24
};

struct BatchMovesParams {
    const BatchDesc* desc;
    const BatchMovesDesc* mdesc;          // one workgroup each
    const int32_t* in;
    int32_t* sc;
    int32_t* out;
};

// The plan statistics of one batched problem (DESIGN.md §4.10 "k_batch_stats"): 1 + 7 M int64 values in its output slice,
// n_nodes_next, then load_min / load_max / load_sum / load_sumsq / nodes_used / unmet_slots / rule_violations [M] each.
constexpr int kBatchStatsThreads = 256;
constexpr int kBatchStatsArrays = 7;
struct BatchStatsDesc {
    int32_t desc;                         // index of the problem's BatchDesc
    int32_t o_stats;                      // output slice: first word of the values (a multiple of 4: 8-byte aligned)
};

struct BatchStatsParams {
    const BatchDesc* desc;
    const BatchStatsDesc* sdesc;          // one workgroup each
    const int32_t* in;
    int32_t* out;
};

// The PartitionMap document of one batched problem (DESIGN.md §4.16 "k_batch_wire_size / k_batch_wire_write").  The names
// block (a blance_batch_names' words, copied as they are) lies behind the problem's input slice: kBatchNamesHdr words with
// the word offsets of its eight tables inside the block, then the tables.
constexpr int kBatchWireThreads = 256;
constexpr int kBatchNamesHdr = 8;         // order [P], part_off [P + 1] (by rank), node_off [NX + 1], state_off [M + 1],
                                          // state_id [M], then the escaped bytes: partitions by rank, nodes by id, states
enum { kNamesOrder = 0, kNamesPartOff, kNamesNodeOff, kNamesStateOff, kNamesStateId, kNamesPartEsc, kNamesNodeEsc, kNamesStateEsc };
struct BatchWireDesc {
    int32_t desc;                         // index of the problem's BatchDesc
    int32_t i_names;                      // input slice: first word of the names block
    int32_t s_len;                        // scratch slice: [P + 1] byte offsets of the ranks (k_batch_wire_size's scan)
    int32_t o_total;                      // output slice: the document's length (one word of a region of four)
};

// The prevMap document of one batched problem (DESIGN.md §4.17 "k_batch_decode").  The dictionary block (a
// blance_batch_dict's words, copied as they are) lies behind the problem's input slice: kBatchDictHdr words, per kind of
// name (partitions, nodes, states) four -- slots (word offset in the block), mask, the raw bytes (word offset), their
// int32 offsets (word offset) --, then the three counts; then the tables, each at a multiple of 4 words.
constexpr int kBatchDecodeThreads = 256;
constexpr int kBatchDictHdr = 16;
// the hash of a name in a dictionary's tables (WdTable, k_wire_decode.h): FNV-1a over the unescaped bytes, the length folded
// in.  One definition for the host that builds the tables (host/wire_names.hpp) and both translation units that parse.
BLANCE_HOST_DEVICE inline uint32_t wd_hash_init() { return 2166136261u; }
BLANCE_HOST_DEVICE inline uint32_t wd_hash_step(uint32_t h, unsigned b) { return (h ^ b) * 16777619u; }     // FNV-1a
BLANCE_HOST_DEVICE inline uint32_t wd_hash_done(uint32_t h, int n) { h ^= (uint32_t)n; h ^= h >> 15; return h; }
constexpr int kBatchDecodeLdsHead = 4096;                   // scan and reduction words in front of the parse stage
// summary words of one document (k_batch_decode's place-and-sum), int32 unless said otherwise
enum { kBdRefusal = 0 /* 64 bit: all ones, or offset << 8 | reason */, kBdRecords = 2, kBdRefs = 3, kBdLongest = 4, kBdFresh = 5,
       kBdFirstMissing = 6, kBdFirstDup = 7, kBdFirstLong = 8, kBdCap = 10 /* 64 bit */, kBdPrevLoad = 12 /* 64 bit */,
       kBdSumWords = 16 };
struct BatchDocDesc {
    int32_t desc;                         // index of the problem's BatchDesc
    int32_t len;                          // the document's bytes
    int64_t doc_base;                     // its first byte in BatchDecodeParams::docs (a multiple of 16)
    int32_t i_dict;                       // input slice: first word of the dictionary block
    int32_t assign_too;
    // scratch slice: claim [P], the partitions' kinds [P] (bytes), the lists' kinds [P*M] (bytes), their lengths [P*M + 1],
    // the record starts [rec_cap]
    int32_t s_claim, s_pkind, s_kind, s_len, s_rec, rec_cap;
};

struct BatchDecodeParams {
    const BatchDesc* desc;
    const BatchDocDesc* ddesc;            // one workgroup each
    int32_t* in;                          // (the decoded lists go into the problems' input slices)
    int32_t* sc;
    const unsigned char* docs;            // all documents, each at a 16-byte aligned base, padded to 16
    int32_t* sum;                         // [n][kBdSumWords]
    int32_t tile, stage;                  // bytes of a thread's tile of the record split; bytes of the parse stage in LDS
};

struct BatchWireParams {
    const BatchDesc* desc;
    const BatchWireDesc* wdesc;           // one workgroup each
    const int32_t* in;
    int32_t* sc;
    int32_t* out;
    int32_t* wire_total;                  // [nw] scratch: every document's length rounded up to 16 (0: problem skipped)
    char* doc;                            // all documents, one after another at 16-byte aligned bases (k_batch_wire_write)
    int32_t stage;                        // bytes of k_batch_wire_write's LDS stage
};

}  // namespace blance
