// MI355X (gfx950) implementation of blance's planNextMapEx (plan.go:23-58) behind
// the C ABI of include/blance_hip.h.  One blance_plan() call runs the whole
// convergence loop on the device; the host only sequences kernels and reads
// one convergence word per sweep.  See DESIGN.md for the kernel inventory.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -shared -fPIC
// (fp64 scores must keep the reference's operation order, plan.go:634-689).
#include "dev_prelude.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <type_traits>
#include <string>
#include <vector>

#include "k_sweep.h"
#include "k_flat.h"
#include "k_period.h"
#include "k_cycle.h"
#include "k_plan_moves.h"
#include "k_plan_wire.h"
#include "k_wire_decode.h"
#include "k_adopt.h"
#include "k_wire_adopt.h"
#include "host/json_escape.hpp"
#include "host/problem_facts.hpp"
#include "host/batch_layout.hpp"
#include "host/wire_names.hpp"
#ifdef BLANCE_SIMT_EMU          /* the emulator build is one translation unit */
#include "tu_seq.hip"
#include "tu_tree.hip"
#include "tu_queue.hip"
#include "tu_chain.hip"
#include "tu_batch.hip"
#endif


// ============================================================================
// Host side: context, upload, the sweep driver, download
// ============================================================================
using namespace blance;

static thread_local std::string g_last_error;

static int fail(int code, const char* fmt, const char* a = "", long b = 0) {
    char buf[512];
    snprintf(buf, sizeof buf, fmt, a, b);
    g_last_error = buf;
    return code;
}

#define HIPTRY(expr)                                                                  \
    do {                                                                              \
        hipError_t e_ = (expr);                                                       \
        if (e_ != hipSuccess)                                                         \
            return fail(BLANCE_ERR_DEVICE, "%s failed: line %ld", hipGetErrorString(e_), __LINE__); \
    } while (0)

struct DevBuf {                                     // device memory, freed with its owner
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    int reserve(size_t bytes) {
        if (bytes <= cap && p) return 0;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        size_t want = bytes < 256 ? 256 : bytes;
        if (hipMalloc(&p, want) != hipSuccess) { p = nullptr; return -1; }
        cap = want;
        return 0;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <class T> T* as() const { return (T*)p; }
};

// ---- page-locked host memory (include/blance_hip.h: blance_host_alloc).  hipHostMalloc costs milliseconds for the
// sizes of a plan, so freed blocks are kept (up to kPinCacheMax bytes) and handed out again.
struct CopySeg { void* dst; const void* src; size_t bytes; };
namespace {
constexpr size_t kPinCacheMax = (size_t)2 << 30;
struct PinBlock { void* p; size_t cap; };
std::mutex g_pin_mu;
std::vector<PinBlock> g_pin_free;
std::map<uintptr_t, size_t> g_pin_live;          // blocks handed out: base -> capacity
size_t g_pin_cached = 0;

void* pin_alloc(size_t bytes) {
    const size_t want = ((bytes ? bytes : 1) + 65535) & ~(size_t)65535;
    {
        std::lock_guard<std::mutex> g(g_pin_mu);
        size_t best = g_pin_free.size();
        for (size_t i = 0; i < g_pin_free.size(); i++)
            if (g_pin_free[i].cap >= want && g_pin_free[i].cap <= 2 * want + (1u << 20) &&
                (best == g_pin_free.size() || g_pin_free[i].cap < g_pin_free[best].cap)) best = i;
        if (best < g_pin_free.size()) {
            PinBlock b = g_pin_free[best];
            g_pin_free.erase(g_pin_free.begin() + (long)best);
            g_pin_cached -= b.cap;
            g_pin_live[(uintptr_t)b.p] = b.cap;
            return b.p;
        }
    }
    void* p = nullptr;
    if (hipHostMalloc(&p, want) != hipSuccess || !p) { (void)hipGetLastError(); return nullptr; }
    std::lock_guard<std::mutex> g(g_pin_mu);
    g_pin_live[(uintptr_t)p] = want;
    return p;
}
void pin_free(void* p) {
    if (!p) return;
    size_t cap = 0;
    {
        std::lock_guard<std::mutex> g(g_pin_mu);
        auto it = g_pin_live.find((uintptr_t)p);
        if (it == g_pin_live.end()) return;          // not one of ours
        cap = it->second;
        g_pin_live.erase(it);
        if (g_pin_cached + cap <= kPinCacheMax) { g_pin_free.push_back(PinBlock{p, cap}); g_pin_cached += cap; return; }
    }
    (void)hipHostFree(p);
}
void pin_trim() {
    std::vector<PinBlock> drop;
    {
        std::lock_guard<std::mutex> g(g_pin_mu);
        drop.swap(g_pin_free);
        g_pin_cached = 0;
    }
    for (const PinBlock& b : drop) (void)hipHostFree(b.p);
}
// does [p, p + bytes) lie in page-locked memory the device can copy from / to directly?
bool host_ptr_pinned(const void* p, size_t bytes) {
    const uintptr_t a = (uintptr_t)p;
    {
        std::lock_guard<std::mutex> g(g_pin_mu);
        auto it = g_pin_live.upper_bound(a);
        if (it != g_pin_live.begin()) {
            --it;
            if (a >= it->first && a + bytes <= it->first + it->second) return true;
        }
    }
#ifndef BLANCE_SIMT_EMU
    if (bytes >= ((size_t)1 << 20)) {                // (memory the caller registered itself: worth a query for big arrays only)
        // both ends: an array that only starts inside a registered range is not DMA'd as if all of it were page-locked
        hipPointerAttribute_t at, at_end;
        if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
        if (at.type != hipMemoryTypeHost) return false;
        if (hipPointerGetAttributes(&at_end, (const char*)p + bytes - 1) != hipSuccess) { (void)hipGetLastError(); return false; }
        return at_end.type == hipMemoryTypeHost && at_end.hostPointer != nullptr && at.hostPointer != nullptr &&
               (const char*)at_end.hostPointer - (const char*)at.hostPointer == (ptrdiff_t)(bytes - 1);
    }
#endif
    return false;
}

// n bytes copied by a few threads (a pageable array on its way into / out of the staging buffer: one core moves ~10 GB/s,
// the link five times that)
void copy_threaded(const std::vector<CopySeg>& segs) {
    size_t total = 0;
    for (const CopySeg& g : segs) total += g.bytes;
    unsigned T = 1;
    if (total >= ((size_t)4 << 20)) {
        const unsigned hw = std::thread::hardware_concurrency();
        T = hw >= 16 ? 6 : hw >= 8 ? 4 : hw >= 4 ? 2 : 1;
        const unsigned by_size = (unsigned)(total >> 21);
        if (by_size < T) T = by_size ? by_size : 1;
    }
    auto work = [&](unsigned t) {
        const size_t lo = total * t / T, hi = total * (t + 1) / T;
        size_t pos = 0;
        for (const CopySeg& g : segs) {
            const size_t b = pos, e = pos + g.bytes;
            pos = e;
            if (e <= lo || b >= hi) continue;
            const size_t from = lo > b ? lo - b : 0, to = (hi < e ? hi : e) - b;
            memcpy((char*)g.dst + from, (const char*)g.src + from, to - from);
        }
    };
    std::vector<std::thread> th;
    struct Join { std::vector<std::thread>& v; ~Join() { for (auto& t : v) if (t.joinable()) t.join(); } } join{th};
    unsigned started = 1;
    try {
        for (unsigned t = 1; t < T; t++) { th.emplace_back(work, t); started++; }
    } catch (...) {}                                  // (no more threads: this one does the rest)
    work(0);
    for (unsigned t = started; t < T; t++) work(t);
}
}  // namespace

extern "C" void* blance_host_alloc(size_t bytes) { return pin_alloc(bytes); }
extern "C" void blance_host_free(void* p) { pin_free(p); }
extern "C" void blance_host_trim(void) { pin_trim(); }
static std::atomic<int> g_live_contexts{0};

struct HostStage {                                   // a page-locked staging buffer of the context
    void* p = nullptr;
    size_t cap = 0, used = 0;
    HostStage() = default;
    HostStage(const HostStage&) = delete;
    HostStage& operator=(const HostStage&) = delete;
    ~HostStage() { release(); }
    void release() { if (p) pin_free(p); p = nullptr; cap = used = 0; }
};

// What one plan did, written once when it ends (plan_locked's finish_plan); blance_result's counters are filled from it.
struct PlanStats {
    int32_t iterations = 0, converged = 0;
    int64_t n_warnings = 0, steps_total = 0, steps_batched = 0, kernel_launches = 0, host_syncs = 0;
    int64_t pass_launches = 0, flat_passes = 0, blank_launches = 0, stay_launches = 0;
    double device_ms = 0.0, pass_ms = 0.0, flat_ms = 0.0, blank_ms = 0.0, stay_ms = 0.0;
};

// The context's streams and events.  A base of blance_ctx, so that they go after its members: ~blance_ctx synchronises the
// streams and releases the communicator, the buffers free themselves, then events and streams are destroyed.
struct CtxHandles {
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipStream_t side = nullptr;     // the second stream (run_chain_pass_once: group_ahead)
    hipEvent_t side_go = nullptr, side_done = nullptr;
    std::vector<hipEvent_t> pass_events;     // begin/end pairs around every pass kernel
    std::vector<hipEvent_t> comm_events;     // begin / end pairs around the collectives of the current plan (RCCL path)
    ~CtxHandles() {
        for (hipEvent_t e : pass_events) (void)hipEventDestroy(e);
        for (hipEvent_t e : comm_events) (void)hipEventDestroy(e);
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (stream) (void)hipStreamDestroy(stream);
        if (side_go) (void)hipEventDestroy(side_go);
        if (side_done) (void)hipEventDestroy(side_done);
        if (side) (void)hipStreamDestroy(side);
    }
};

// The fewest remaining steps a region's chain hands off by default (profiles/chain_handoff_ab.txt).  Chains shorter than
// this plus a stage never hand off: the driver then plans the pass as before.
constexpr int kChainHandoffMin = 8192;

// blance_wire_dict_create: per kind of name (partitions, nodes, states) the hash table, the raw names and
// their offsets on the device.  Owned by the context it was made on.
struct blance_wire_dict {
    blance_ctx* owner = nullptr;
    int32_t n[3] = {0, 0, 0};       // P, NX, M
    uint32_t mask[3] = {0, 0, 0};
    DevBuf slots[3], bytes[3], off[3];
};

// blance_calc_moves: inputs, per-partition slices, offsets, compacted outputs.  blance_plan_moves_get reads both maps where the
// plan left them and keeps beg_other's CSR in the two buffers of the begin map (other_off / other_nodes); n_moves then has
// its counters in front, c_* the moves at their final places.
struct MovesBufs {
    DevBuf beg_off, beg_nodes, end_off, end_nodes, op_node, op_state, op_kind, n_moves, c_node, c_state, c_kind;
    DevBuf& other_off() { return beg_off; }
    DevBuf& other_nodes() { return beg_nodes; }
};
// blance_plan_wire_names' eight tables (WireTables has the same names), k_wire_size's lengths, the document
struct WireOutBufs { DevBuf order, part_esc, part_off, node_esc, node_off, state_esc, state_off, state_id, len, doc; };
// the decoder: the document's copy, the record split's scratch, the claims, the decoded CSR (part_kind, kind, off, nodes)
struct WireInBufs { DevBuf doc, tb, qbits, quotes, depth, count, rec, claim, part_kind, kind, off, nodes, refusal; };

struct Mover;
enum PassKind { kPassKernel = 0, kPassFlatBulk = 1, kPassBlank = 2, kPassStayTop = 3 };   // what ran a state pass (statistics)

struct blance_ctx : CtxHandles {
    int device = 0;
    int engine = BLANCE_ENGINE_AUTO;
    int force_threads = 0;
    std::mutex mu;
    bool uploaded = false;
    bool planned = false;
    // one plan on several ranks (include/blance_hip.h "one plan on several GPUs")
    blance_comm comm{0, 1, nullptr, nullptr, nullptr};
    void* rccl_comm = nullptr;      // ncclComm_t of blance_comm_init_rccl
    DevBuf scan_sums;               // tile totals of launch_scan_excl
    DevBuf scan_part;               // k_flat_scan's per-wave results
    DevBuf topkey, top_counts, top_off, top_order;   // k_stay_by_top: steps grouped by the leaf of their top priority node
    // That grouping made AHEAD of the sweep that wants it: on a second stream, beside the chain kernel of the sweep before (a
    // few dozen workgroups on 256 CUs).  It holds as long as the grouping by region it was made from does (group_epoch).
    // (CtxHandles: side, side_go, side_done)
    DevBuf side_sums;               // (launch_scan_excl's tile totals on that stream)
    bool side_pending = false;      // work on `side` the planner's stream has not waited for yet
    int top_group_state = -1;       // top_off / top_order are those of this state's chain order ...
    int64_t top_group_epoch = -1, group_epoch = 0;   // ... as grouped at this count of regroupings
    std::vector<int64_t> last_stays; // [state] steps the last chain pass of that state committed as verified stays
    // The chain kernel's hand-off: a region's walk ends at the first stage boundary behind a stage of stay
    // rounds only, when at least this many steps remain; k_stay_by_top checks the rest.  0: off (BLANCE_CHAIN_HANDOFF=0|<n>).
    int chain_handoff = kChainHandoffMin;
    DevBuf handoff;                 // [regions] chain index of the first step a region's walk did not do
    bool no_stay_top = false;       // test knob (kKnobNoStayTop): never k_stay_by_top
    bool force_stay_top = false;    // test knob (kKnobForceStayTop): try k_stay_by_top in every chain pass with NumPartitions > 0
    bool periodic = true;           // an all-blank chain pass with periodic records walks two periods (k_period.h); off: kKnobNoPeriodic, or BLANCE_PERIODIC=0
    int periodic_cut = 0;           // test knob BLANCE_PERIODIC_CUT (k_period_segments)
    // the periodic pass behind a round robin takes its period from the upload, not from a search (k_period_find's known
    // mode); off: kKnobNoPeriodKnown, or BLANCE_PERIOD_KNOWN=0.  What the upload contributes:
    bool period_known = true;
    uint32_t assign_kinds = 0;      // k_validate_parts: bit m -- some list to assign of state m is absent, bit 16 + m -- some is not
    bool cycle_order_stands = false; // sweep 1's second pass runs in the order of its first (one partitionSorter category in both)
    bool leaves_distinct = false;   // no two nodes share a leaf of the hierarchy
    // The chain pass behind a round robin takes its grouping by region and k_stay_by_top's work list from tables of the upload
    // (k_cycle.h, RuleRegions::cyc), not from two counting sorts.  0: off (kKnobNoCycleGroup, or BLANCE_CYCLE_GROUP=0); 2: the test knob
    // BLANCE_CYCLE_GROUP=refute -- the kernel's check of the premise fails for step 0, the pass goes in order.
    int cycle_group = 1;
    int64_t cycle_group_epoch = -1; // the count of regroupings at which the grouping by region was taken from those tables (-1: it was not)
    DevBuf cnt_base, xbuf, gath;    // sharded pass: loads at pass start, [flags | load change], gathered output slices
    std::vector<int32_t> h_reg_off; // host copy of the chain offsets (slice sizes of the all-gather)
    int chain_group_state = -1;     // the state whose chain pass last grouped the steps by region (chain_order, chain_oi, reg_off) ...
    bool chain_group_static = false; // ... and whether it did so from the static order (sweeps >= 2)
    bool tops_moved = true;         // this sweep's top-state pass was not (known to be) one run of stays
    uint32_t top_gate = 0;          // the words of scal + kScalFlags every launch behind a top-state pass assumed to be one run of stays waits
                                    // for (plan_locked: kFlagTopMoved, kFlagForced), 0 when that pass's verdict is known
    bool flags_clean = false;       // the chain flags (scalars[kScalFlags ..], kChainFlags words) are zero: nothing has set one since the last fill
    bool rowcount_clean = false;    // f_row_count is zero (k_flat_row_count adds to it)
    bool top_prio_strict = false;   // every other state with constraints > 0 has a priority strictly behind the top state's
    // every partition gets the same partitionSorter category in sweep 1 (decided at upload): the pass order IS the static
    // order, no k_category / stable partition (plan.go:542-561) -- in the sweep's first state pass / in all of them
    bool uniform_first = false, uniform_all = false;
    bool trace = false;             // BLANCE_TRACE, read once at context creation
    int dump_sweep = -1;            // BLANCE_DUMP_SWEEP (developer aid), likewise
    DevBuf dl_off, dl_nodes;        // blance_download: the result as CSR, compacted on the device
    HostStage stage;                // pageable arrays of the caller pass through this page-locked buffer
    // small readbacks (flag words, counts) land in a page-locked block first: a D2H copy into pageable memory is staged by
    // the runtime and costs several microseconds more, thirteen times per call
    void* rb_buf = nullptr;
    size_t rb_used = 0;
    struct RbItem { void* dst; size_t off, bytes; };
    std::vector<RbItem> rb_items;
    DevBuf vres, vseen;             // blance_upload: the device's part of the validation (k_validate_parts)
    MovesBufs mv;                   // blance_calc_moves, blance_plan_moves_get (kept between calls)
    // blance_plan_wire_names / blance_plan_wire_get: the names of the problem the context holds in their
    // escaped forms and document order, the byte offsets of the ranks, the document
    bool wire_names = false;        // `wire` holds the names of the problem uploaded last
    int wire_stage = kWireStageDefault;   // bytes of k_wire_write's LDS stage (test knob BLANCE_WIRE_STAGE lowers it)
    WireOutBufs wire;
    // blance_wire_dict_create / blance_wire_decode_device: the dictionaries made on this context, the
    // document's copy and the scratch of the decoder (kept between calls)
    int wd_tile = kWdTileDefault;   // bytes of a tile of the record split (test knob BLANCE_WIRE_IN_TILE lowers it)
    int wd_stage = kWdStageDefault; // bytes of k_wd_parse's LDS stage (test knob BLANCE_WIRE_IN_STAGE)
    std::vector<blance_wire_dict*> wd_dicts;
    WireInBufs wd;
    int64_t comm_calls = 0, comm_bytes = 0;
    size_t comm_events_used = 0;             // (comm_events: CtxHandles)
    double comm_ms = 0.0;                    // device time between those pairs, all plans so far
    int64_t n_syncs = 0;                     // stream_sync() calls so far
    // known at upload (no readback needed for them in the first sweep's first pass): the partitions to assign hold no node at
    // all; no load counter starts above zero (no extra loads, nothing counted from prevMap)
    bool assign_empty = false, counts_start_zero = false;
    int chain_waves = 0;                     // k_pass_chain's workgroup: 0 = 8 waves when the LDS is there, else 4 (BLANCE_CHAIN_WAVES=4|8)
    int speculate = 1;                       // host decisions taken before their words are read back (BLANCE_SPECULATE=0|1|fail)
    bool fused_tail = true;                  // a sweep ends with k_sweep_tail instead of k_scatter + k_converge (BLANCE_FUSED_TAIL=0: off)

    // host copy of the small parts of the problem
    blance_problem h{};
    std::vector<int32_t> state_priority, state_constraints, rule_off;
    int L = 1, np_later = 0, n_alive = 0, any_removed = 0;
    int chain_min_parts = 2048;
    int any_node_weight = 0;
    bool no_fast_keys = false;      // a chain left the packed keys' range during this pass
    bool no_seq_spec = false;       // test knob (kKnobNoSeqSpec): k_pass_seq without stay speculation
    bool no_tree = false;           // test knob (kKnobNoTree): flat passes never on k_pass_tree
    bool tree_dense = false;        // test knob (kKnobTreeDense): k_pass_tree scores every node in every general step
    bool tree_always = false;       // test knob (kKnobTreeAlways): k_pass_tree even when a k_pass_seq workgroup size is forced
    bool tree_long = false;         // test knob (kKnobTreeLong): k_pass_tree decodes the record in every general step
    bool no_planes = false;         // test knob (kKnobNoPlanes): the all-blank chain pass on k_pass_chain_blank, not k_pass_chain_planes
    bool no_queue = false;          // test knob (kKnobNoQueue): flat passes with k <= 2 on k_pass_tree, never on k_pass_queue
    bool queue_general = false;     // test knob (kKnobQueueGeneral): k_pass_queue without its lean walk
    bool queue_no_asm = false;      // test knob (kKnobQueueNoAsm): k_pass_queue's lean walk as compiled C++ only
    bool queue_force_dense = false; // test knob (kKnobQueueForceDense): every general step of k_pass_queue scores every node
    bool queue_exact_rebuild = false; // test knob (kKnobQueueExactRebuild): k_pass_queue's window always rebuilt by the exact selection
    bool queue_bits_self = false;   // test knob (kKnobQueueBitsSelf): k_pass_queue's walking wave copies the row bit maps itself (no helper)
    bool shard_one_rank = false;    // test knob (kKnobShardOneRank): a communicator of ONE rank takes the sharded branch of a chain pass, so that
                                    // both collectives really execute (ncclAllReduce / ncclAllGather on a one-GPU box)
    DevBuf ntn_bits;                // k_pass_queue: one bit per nodeToNodeCounts entry, zeroed with the matrix
    bool bits_stale = false;        // another kernel bumped the matrix in this pass: k_ntn_bits before k_pass_queue goes on
    // nodeToNodeCounts (67 MB at config 3) is zeroed lazily: only a pass that reads or bumps the matrix in HBM pays for it
    // (region chains keep their rows in LDS, a pass that is one run of stays needs none of it)
    bool pass_ntn_ready = false;    // this pass has been given its zeroed matrix already (plan.go:266)
    int64_t queue_launches = 0, queue_stops = 0, queue_moved = 0, queue_exact = 0, queue_rebuilds = 0, queue_dense = 0;
    struct RuleRegions {           // regions the rule cuts the leaves into (chains), if it does
        bool ok = false;
        int n_regions = 0, max_size = 0;
        DevBuf node_region, reg_lo, reg_hi, leaf_cls, cls_size;
        DevBuf wg_region, wg_chunk;     // k_stay_by_top: entry b of its work table = the tops at leaves reg_lo + 64 chunk .. + 63 of its region
        int n_stay_wgs = 0, n_leaves = 0;
        int cls_run = 0;                // S if every exclude class is an aligned run of S = 2^e <= 64 node-carrying leaves, else 0
        // k_cycle.h: where step j of a round robin over nodesNext lies in the region chains and in k_stay_by_top's work list,
        // for the upload's partition count.  Built when no two nodes share a leaf and every node of nodesNext lies in a region.
        bool cyc_ok = false;
        DevBuf cyc, cyc_reg_off, cyc_top_off;   // [n_alive][kCycWords], [n_regions + 1], [n_leaves + 1]
        std::vector<int32_t> h_cyc_reg_off;     // the host's copy of the chain offsets
        int put(Mover& up, const RuleTables& t, int leaves);   // the analysis of host/problem_facts.hpp, onto the device
    };
    std::vector<RuleRegions> rule_regions;
    DevBuf leaf_node, regid, chain_order, bucket_counts, reg_off, cnt_save, crec;
    DevBuf chain_inv;               // chain_inv[p]: p's place in chain_order (k_invert, with every regrouping)
    DevBuf period, cnt_p1;          // k_period.h: per-region period tables, the counters after the first period
    DevBuf fl_iota, fl_zero, fl_one, fl_reglo, fl_reghi;   // the whole cluster as one region (flat single chain)
    DevBuf n_ev, chain_oi, ev_key, ev_oi, ev_leaf, ev_w, ev_perm, ev_off, ev_counts;   // chain events
    bool flat_chain_ok = false;
    DevBuf f_tot, f_g, f_top_g, f_top_n, f_row_count, f_m, f_moff, f_keys_a, f_keys_b, f_vals_a, f_vals_b, f_hist, f_comp;
    int64_t out_capacity = 0;
    DevBuf batch_in, batch_sc, batch_out;   // blance_plan_batch: descriptors + packed problems, working state, results
    DevBuf batch_doc;                       // blance_plan_batch_wire: the documents of the batched problems, one after another
    DevBuf batch_doc_in, batch_doc_sum;     // blance_plan_batch_docs: the prevMap documents coming in, k_batch_decode's summary words

    // device: problem
    DevBuf node_removed, node_added, node_weight, node_has_weight, alive, zeros_nx, node_leaf_pos;
    DevBuf alive_ids, alive_rank;   // the nodes of nodesNext in id order; a node's place in that list (-1: not in it)
    DevBuf part_order, part_weight, part_has_weight, part_in_prev, part_never_equal;
    DevBuf a_off, a_nodes, a_kind, p_off, p_nodes, p_kind;
    DevBuf load_state, load_node, load_weight, load_first;
    DevBuf rule_inc, rule_exc, vparent, vlo, vhi, anchors;
    DevBuf state_stick, state_has_stick;
    // device: working state
    DevBuf live, live_len, live_kind, prv, prv_len, prv_kind, in_prev, never_equal;
    DevBuf cnt, ntn, cat, order, chunk_counts, rec, out, warn_part, warn_state, scalars;
    DevBuf cnt_next;                // stateNodeCounts of the next sweep, counted by this sweep's k_sweep_tail (swapped with cnt)
    bool tail_counted = false;      // the last sweep's k_sweep_tail counted cnt_next and refreshed the kinds (plan.go:94, 418)
    // blance_plan_adopt.  Host copies of the small arrays the upload's analysis reads (host/problem_facts.hpp:
    // O(NX + VX + rules), never the lists), so that a node change is analysed again without the caller's problem; the two
    // sums of blance_validate's load bound that an adoption leaves as they are; the summary block of k_adopt_len.
    std::vector<uint8_t> h_node_has_weight;
    std::vector<int32_t> h_node_weight, h_node_leaf_pos, h_vparent, h_vlo, h_vhi, h_rule_inc, h_rule_exc;
    long long sum_abs_weight = 0;   // of the partitions' weights (k_validate_parts)
    long long kept_load_abs = 0;    // of the load entries of partitions that are only in prevMap (load_first_sweep_only == 0)
    // an adoption with keep_prev_only: the load entries stay where they are, k_count_loads skips the first-sweep-only ones
    // in EVERY sweep (the adopted map replaced the keys they stood for)
    bool loads_later_only = false;
    DevBuf adopt_res;
    DevBuf wire_adopt_res;          // blance_wire_adopt: the summary block of k_wire_adopt_sum
    PlanStats stats;                         // of the last plan
    ~blance_ctx();
    std::vector<PassKind> pass_kind;         // of every pass so far in this plan (pass_events holds their begin / end pairs)
};

static void comm_release(blance_ctx* c);
// no exception crosses the C boundary (std::bad_alloc from a staging vector, say)
template <class F>
static int guarded(F f) {
    try {
        return f();
    } catch (const std::bad_alloc&) {
        return fail(BLANCE_ERR_DEVICE, "out of host memory");
    } catch (...) {
        return fail(BLANCE_ERR_DEVICE, "unexpected exception");
    }
}
extern "C" int blance_abi_version(void) { return BLANCE_ABI_VERSION; }
extern "C" const char* blance_last_error(void) { return g_last_error.c_str(); }

extern "C" int64_t blance_result_capacity(const blance_problem* pb) {
    if (!pb || !pb->assign_off || !pb->state_constraints) return 0;
    int64_t cap = 0;
    const int64_t PM = (int64_t)pb->n_parts * pb->n_states;
    for (int64_t idx = 0; idx < PM; idx++) {
        int len = pb->assign_off[idx + 1] - pb->assign_off[idx];
        int k = pb->state_constraints[idx % pb->n_states];
        cap += len > k ? len : k;
    }
    return cap;
}

// blance_validate in four parts, in the order of its checks: head (sizes, pointers), parts (the O(P) loops: CSR shape, ids,
// the order's permutation -- blance_upload runs these on the device, k_validate_parts), tail_a (loads, rules, hierarchy),
// tail_b (what needs the longest list and the weight sums).
static int validate_head(const blance_problem* pb) {
    if (!pb) return fail(BLANCE_ERR_BAD_ARG, "null problem");
    const int N = pb->n_nodes, NX = pb->n_nodes_ext, M = pb->n_states, P = pb->n_parts;
    if (N < 0 || NX < N || M < 0 || P < 0 || pb->n_prev < 0 || pb->n_loads < 0 || pb->n_rules < 0 ||
        pb->max_iterations < 0)
        return fail(BLANCE_ERR_BAD_ARG, "negative or inconsistent sizes");
    if ((int64_t)P * (M > 0 ? M : 1) > (int64_t)INT32_MAX / 4) return fail(BLANCE_ERR_UNSUPPORTED, "P*M too large");
    if (M > kMaxStates) return fail(BLANCE_ERR_UNSUPPORTED, "more than 16 model states");
    if (M > 0 && (pb->top_state < 0 || pb->top_state >= M)) return fail(BLANCE_ERR_BAD_ARG, "top_state out of range");
    const void* need[] = {pb->state_priority, pb->state_constraints, pb->state_stickiness, pb->state_has_stickiness,
                          pb->node_removed, pb->node_added, pb->node_weight, pb->node_has_weight, pb->part_order,
                          pb->part_weight, pb->part_has_weight, pb->part_in_prev, pb->part_prev_never_equal,
                          pb->assign_off, pb->assign_nodes, pb->assign_kind, pb->prev_off, pb->prev_nodes,
                          pb->prev_kind, pb->load_state, pb->load_node, pb->load_weight, pb->load_first_sweep_only,
                          pb->rule_off, pb->rule_inc, pb->rule_exc, pb->node_leaf_pos};
    for (const void* q : need) if (!q) return fail(BLANCE_ERR_BAD_ARG, "null array pointer");
    if (pb->assign_off[0] != 0 || pb->prev_off[0] != 0) return fail(BLANCE_ERR_BAD_ARG, "CSR offsets must start at 0");
    return BLANCE_OK;
}

struct PartsSummary { int L; long long fresh, cap, sumw, aprev; };

static int validate_parts_host(const blance_problem* pb, PartsSummary* ps) {
    const int NX = pb->n_nodes_ext, M = pb->n_states, P = pb->n_parts;
    const int64_t PM = (int64_t)P * M;
    for (int64_t i = 0; i < PM; i++) {
        if (pb->assign_off[i + 1] < pb->assign_off[i] || pb->prev_off[i + 1] < pb->prev_off[i])
            return fail(BLANCE_ERR_BAD_ARG, "CSR offsets not monotone");
        if (pb->assign_kind[i] > BLANCE_LIST_SET || pb->prev_kind[i] > BLANCE_LIST_SET)
            return fail(BLANCE_ERR_BAD_ARG, "bad list kind");
        if (pb->assign_off[i + 1] - pb->assign_off[i] > 0xffff || pb->prev_off[i + 1] - pb->prev_off[i] > 0xffff)
            return fail(BLANCE_ERR_UNSUPPORTED, "state list longer than 65535");
    }
    for (int64_t i = 0; i < pb->assign_off[PM]; i++)
        if (pb->assign_nodes[i] < 0 || pb->assign_nodes[i] >= NX) return fail(BLANCE_ERR_BAD_ARG, "assign node id out of range");
    for (int64_t i = 0; i < pb->prev_off[PM]; i++)
        if (pb->prev_nodes[i] < 0 || pb->prev_nodes[i] >= NX) return fail(BLANCE_ERR_BAD_ARG, "prev node id out of range");
    {
        std::vector<uint8_t> seen((size_t)P, 0);
        for (int i = 0; i < P; i++) {
            int p = pb->part_order[i];
            if (p < 0 || p >= P || seen[p]) return fail(BLANCE_ERR_BAD_ARG, "part_order is not a permutation");
            seen[p] = 1;
        }
    }
    ps->L = 0; ps->fresh = ps->cap = ps->sumw = ps->aprev = 0;
    for (int64_t i = 0; i < PM; i++) {
        int a = pb->assign_off[i + 1] - pb->assign_off[i], b = pb->prev_off[i + 1] - pb->prev_off[i];
        if (a > ps->L) ps->L = a;
        if (b > ps->L) ps->L = b;
        const int k = pb->state_constraints[i % M];
        ps->cap += a > k ? a : k;
    }
    auto la = [](long long v) { return v < 0 ? -v : v; };
    for (int p = 0; p < P; p++) {
        const long long w = (!pb->partition_weights_nil && pb->part_has_weight[p]) ? la(pb->part_weight[p]) : 1;
        ps->sumw += w;
        if (pb->part_in_prev[p]) ps->aprev += w * (pb->prev_off[(int64_t)(p + 1) * M] - pb->prev_off[(int64_t)p * M]);
        else ps->fresh++;
    }
    return BLANCE_OK;
}

static int validate_tail_a(const blance_problem* pb) {
    const int NX = pb->n_nodes_ext, M = pb->n_states;
    for (int i = 0; i < pb->n_loads; i++)
        if (pb->load_state[i] < 0 || pb->load_state[i] > M || pb->load_node[i] < 0 || pb->load_node[i] >= NX)
            return fail(BLANCE_ERR_BAD_ARG, "load entry out of range");
    if (pb->rule_off[0] != 0) return fail(BLANCE_ERR_BAD_ARG, "rule_off must start at 0");
    for (int m = 0; m < M; m++) {
        int k = pb->state_constraints[m];
        if (k > kMaxK) return fail(BLANCE_ERR_UNSUPPORTED, "constraints > 8 for a state");
        if (pb->rule_off[m + 1] < pb->rule_off[m]) return fail(BLANCE_ERR_BAD_ARG, "rule_off not monotone");
        if (!pb->hierarchy_rules_nil && k > 0 && (pb->rule_off[m + 1] - pb->rule_off[m]) * k > kMaxAnchors - 1)
            return fail(BLANCE_ERR_UNSUPPORTED, "more than 8 hierarchy picks per partition and state");
    }
    if (M > 0 && pb->rule_off[M] > pb->n_rules) return fail(BLANCE_ERR_BAD_ARG, "rule_off exceeds n_rules");
    if (!pb->hierarchy_rules_nil) {
        const int VX = pb->n_vertices;
        if (VX <= NX || !pb->vertex_parent || !pb->vertex_leaf_lo || !pb->vertex_leaf_hi)
            return fail(BLANCE_ERR_BAD_ARG, "hierarchy arrays missing");
        if (pb->vertex_empty < 0 || pb->vertex_empty >= VX) return fail(BLANCE_ERR_BAD_ARG, "vertex_empty out of range");
        for (int v = 0; v < VX; v++) {
            if (pb->vertex_parent[v] < 0 || pb->vertex_parent[v] >= VX) return fail(BLANCE_ERR_BAD_ARG, "vertex_parent out of range");
            if (pb->vertex_leaf_lo[v] < 0 || pb->vertex_leaf_hi[v] <= pb->vertex_leaf_lo[v] || pb->vertex_leaf_hi[v] > VX)
                return fail(BLANCE_ERR_BAD_ARG, "vertex leaf interval empty or beyond the number of vertices");
        }
        for (int n = 0; n < NX; n++)
            if (pb->node_leaf_pos[n] < -1 || pb->node_leaf_pos[n] >= VX) return fail(BLANCE_ERR_BAD_ARG, "node_leaf_pos out of range");
        for (int r = 0; r < pb->n_rules; r++)
            if (pb->rule_inc[r] < 0 || pb->rule_exc[r] < 0 || pb->rule_inc[r] > 64 || pb->rule_exc[r] > 64)
                return fail(BLANCE_ERR_UNSUPPORTED, "hierarchy rule level outside 0..64");
    }
    if (pb->booster_kind != BLANCE_BOOSTER_NONE && pb->booster_kind != BLANCE_BOOSTER_CBGT)
        return fail(BLANCE_ERR_UNSUPPORTED, "unknown booster kind");
    if (NX > 1024 * 8) return fail(BLANCE_ERR_UNSUPPORTED, "more than 8192 node names (register-resident tables)");
    return BLANCE_OK;
}

static int validate_tail_b(const blance_problem* pb, const PartsSummary& ps) {
    const int N = pb->n_nodes, NX = pb->n_nodes_ext, M = pb->n_states;
    int L = 1;
    for (int m = 0; m < M; m++) if (pb->state_constraints[m] > L) L = pb->state_constraints[m];
    if (ps.L > L) L = ps.L;
    if (kRecHead + M * (1 + L) > 64) return fail(BLANCE_ERR_UNSUPPORTED, "step record wider than 64 words (states x list length)");
    {   // the load tables are int32: bound every sum a plan can form (a shim doing its own interning gets the check too)
        long long loads = 0, ksum = 0;
        auto la = [](long long v) { return v < 0 ? -v : v; };
        for (int i = 0; i < pb->n_loads; i++) loads += la(pb->load_weight[i]);
        for (int m = 0; m < M; m++) ksum += pb->state_constraints[m] > 0 ? pb->state_constraints[m] : 0;
        if (adopt_load_bound_exceeded(ps.aprev, loads, ps.sumw, ksum)) return fail(BLANCE_ERR_UNSUPPORTED, "partition weights overflow the int32 load tables");
    }
    if ((int64_t)(NX + 1) * (N > 0 ? N : 1) * 4 > (int64_t)64 << 30) return fail(BLANCE_ERR_UNSUPPORTED, "nodeToNodeCounts matrix > 64 GiB");
    return BLANCE_OK;
}

extern "C" int blance_validate(const blance_problem* pb) {
    return guarded([&]() -> int {
    int st = validate_head(pb);
    if (st) return st;
    PartsSummary ps;
    if ((st = validate_parts_host(pb, &ps))) return st;
    if ((st = validate_tail_a(pb))) return st;
    return validate_tail_b(pb, ps);
    });
}

// The test knobs of blance_options::reserved[2] and the environment variables a context reads once, when it is made.
// (BLANCE_NO_UNIFORM_CATEGORY is read by every upload, BLANCE_QUEUE_STATS at the end of every plan.)
enum TestKnob : uint32_t {
    kKnobNoSeqSpec = 1, kKnobNoTree = 2, kKnobTreeDense = 4, kKnobTreeAlways = 8, kKnobTreeLong = 16, kKnobNoPlanes = 32,
    kKnobNoStayTop = 64, kKnobForceStayTop = 128, kKnobNoPeriodic = 256, kKnobNoQueue = 512, kKnobQueueGeneral = 1024,
    kKnobQueueForceDense = 2048, kKnobQueueNoAsm = 4096, kKnobQueueExactRebuild = 8192, kKnobShardOneRank = 16384,
    kKnobQueueBitsSelf = 32768, kKnobNoPeriodKnown = 65536, kKnobNoCycleGroup = 131072,
};
static void read_knobs(const blance_options* opt, blance_ctx* c) {
    const uint32_t bits = opt ? (uint32_t)opt->reserved[2] : 0;
    auto on = [bits](TestKnob k) { return (bits & k) != 0; };
    auto env_int = [](const char* name, int* v) { const char* e = getenv(name); if (e) *v = atoi(e); return e != nullptr; };
    auto clamp = [](int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; };
    int v = 0;
    c->no_seq_spec = on(kKnobNoSeqSpec);
    c->no_tree = on(kKnobNoTree);
    c->tree_dense = on(kKnobTreeDense);
    c->tree_always = on(kKnobTreeAlways);
    c->tree_long = on(kKnobTreeLong);
    c->no_planes = on(kKnobNoPlanes);
    c->no_queue = on(kKnobNoQueue);
    c->queue_general = on(kKnobQueueGeneral);
    c->queue_force_dense = on(kKnobQueueForceDense);
    c->queue_no_asm = on(kKnobQueueNoAsm);
    c->queue_exact_rebuild = on(kKnobQueueExactRebuild);
    c->shard_one_rank = on(kKnobShardOneRank);
    c->queue_bits_self = on(kKnobQueueBitsSelf);
    c->no_stay_top = on(kKnobNoStayTop);
    c->force_stay_top = on(kKnobForceStayTop);
    c->periodic = !on(kKnobNoPeriodic);
    if (env_int("BLANCE_PERIODIC", &v)) c->periodic = v != 0;                  // BLANCE_PERIODIC=0: the way out
    (void)env_int("BLANCE_PERIODIC_CUT", &c->periodic_cut);
    c->period_known = !on(kKnobNoPeriodKnown);
    if (env_int("BLANCE_PERIOD_KNOWN", &v)) c->period_known = v != 0;
    c->cycle_group = on(kKnobNoCycleGroup) ? 0 : 1;
    if (const char* cg = getenv("BLANCE_CYCLE_GROUP")) c->cycle_group = !strcmp(cg, "refute") ? 2 : atoi(cg) != 0;
    c->trace = getenv("BLANCE_TRACE") != nullptr;
    (void)env_int("BLANCE_CHAIN_WAVES", &c->chain_waves);
    if (env_int("BLANCE_CHAIN_HANDOFF", &v)) c->chain_handoff = v > 0 ? v : 0;   // 0: the way out; n: hand off n steps or more
    if (const char* sp = getenv("BLANCE_SPECULATE")) c->speculate = !strcmp(sp, "fail") ? 2 : atoi(sp) != 0;   // 0: every decision read back first
    if (env_int("BLANCE_FUSED_TAIL", &v)) c->fused_tail = v != 0;               // BLANCE_FUSED_TAIL=0: the unfused tail
    (void)env_int("BLANCE_DUMP_SWEEP", &c->dump_sweep);
    if (env_int("BLANCE_WIRE_STAGE", &v)) c->wire_stage = clamp(v, kWireStageMin, kWireStageMax);
    if (env_int("BLANCE_WIRE_IN_TILE", &v)) c->wd_tile = clamp(v & ~63, kWdTileMin, kWdTileMax);
    if (env_int("BLANCE_WIRE_IN_STAGE", &v)) c->wd_stage = clamp(v & ~15, kWdStageMin, kWdStageMax);
}

extern "C" int blance_ctx_create(const blance_options* opt, blance_ctx** out) {
    if (!out) return fail(BLANCE_ERR_BAD_ARG, "null out");
    *out = nullptr;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0)
        return fail(BLANCE_ERR_NO_DEVICE, "no HIP device visible");
    int dev = opt ? opt->device_id : 0;
    if (dev < 0 || dev >= n_dev) return fail(BLANCE_ERR_BAD_ARG, "device_id out of range");
    HIPTRY(hipSetDevice(dev));
    blance_ctx* c = new blance_ctx();
    c->device = dev;
    c->engine = opt ? opt->engine : BLANCE_ENGINE_AUTO;
    c->force_threads = opt ? opt->reserved[0] : 0;
    if (opt && opt->reserved[1] > 0) c->chain_min_parts = opt->reserved[1];
    read_knobs(opt, c);
    if (hipStreamCreate(&c->stream) != hipSuccess || hipEventCreate(&c->ev0) != hipSuccess ||
        hipEventCreate(&c->ev1) != hipSuccess ||
        hipEventCreate(&c->side_go) != hipSuccess || hipEventCreate(&c->side_done) != hipSuccess) {
        delete c;                                    // (releases what was made)
        return fail(BLANCE_ERR_DEVICE, "stream/event creation failed");
    }
    *out = c;
    g_live_contexts++;
    return BLANCE_OK;
}

// Nothing is in flight when the buffers go: both streams are synchronised first.  The members free themselves after this body,
// events and streams last (CtxHandles).
blance_ctx::~blance_ctx() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    if (side) (void)hipStreamSynchronize(side);
    comm_release(this);
    if (rb_buf) pin_free(rb_buf);
    for (blance_wire_dict* d : wd_dicts) delete d;
}

extern "C" void blance_ctx_destroy(blance_ctx* c) {
    if (!c) return;
    delete c;
    if (--g_live_contexts == 0) pin_trim();          // the process's last context: the cache of page-locked blocks goes too
}

constexpr size_t kRbBytes = 64 * 1024;
// device -> host of a few words, complete after the next stream_sync()
static hipError_t read_back(blance_ctx* c, void* dst, const void* dev, size_t bytes) {
    if (!bytes) return hipSuccess;
    if (!c->rb_buf) c->rb_buf = pin_alloc(kRbBytes);
    const size_t need = (bytes + 15) & ~(size_t)15;
    if (!c->rb_buf || c->rb_used + need > kRbBytes) return hipMemcpyAsync(dst, dev, bytes, hipMemcpyDeviceToHost, c->stream);
    char* at = (char*)c->rb_buf + c->rb_used;
    hipError_t e = hipMemcpyAsync(at, dev, bytes, hipMemcpyDeviceToHost, c->stream);
    if (e != hipSuccess) return e;
    c->rb_items.push_back(blance_ctx::RbItem{dst, c->rb_used, bytes});
    c->rb_used += need;
    return hipSuccess;
}
static hipError_t stream_sync(blance_ctx* c) {
    c->n_syncs++;
    if (c->trace) fprintf(stderr, "[blance] host synchronisation %lld (%zu words read back)\n", (long long)c->n_syncs, c->rb_used / 4);
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess)
        for (const blance_ctx::RbItem& it : c->rb_items) memcpy(it.dst, (const char*)c->rb_buf + it.off, it.bytes);
    c->rb_items.clear();
    c->rb_used = 0;
    return e;
}

// An entry point's error exit: nothing is in flight any more (no DMA into the caller's arrays after the call returns) and
// no read-back is left queued -- its destination is a local of a frame that is gone by now, so it is dropped, not copied.
static void rb_discard(blance_ctx* c) {
    c->rb_items.clear();
    c->rb_used = 0;
}
static int settle(blance_ctx* c, int st) {
    if (st) {
        if (c->stream && hipStreamSynchronize(c->stream) != hipSuccess) (void)hipGetLastError();
        rb_discard(c);
    }
    return st;
}

// Every entry point that takes a context runs its body through here (all but create, destroy and the communicator's
// setters, which enqueue nothing): one call at a time on a context, no read-back left over from the call before, and
// never a return with copies in flight -- not with an error status, not behind an exception either.
template <class F>
static int enter(blance_ctx* c, F f) {
    if (!c) return fail(BLANCE_ERR_BAD_ARG, "null ctx");
    return guarded([&]() -> int {
        std::lock_guard<std::mutex> g(c->mu);
        rb_discard(c);
        try {
            return settle(c, f());
        } catch (...) {
            (void)settle(c, BLANCE_ERR_DEVICE);
            throw;                                   // (guarded names it)
        }
    });
}

// ---- host <-> device copies.  An array in page-locked memory (blance_host_alloc, or registered by the caller) is copied by
// DMA where it lies; a pageable one passes through the context's page-locked staging buffer -- small ones at once, big ones
// (>= 1 MB) by a few threads at flush().  Nothing of the caller's is read after the stream synchronisation that ends the call.
struct Mover {
    blance_ctx* c;
    bool to_device;
    std::vector<CopySeg> host_copy;                 // pending host side copies (caller <-> staging)
    std::vector<CopySeg> dma;                       // the DMAs that go with them (to_device: after the host copy; else before)
    Mover(blance_ctx* ctx, bool up) : c(ctx), to_device(up) {}
    int reserve(size_t bytes);                       // staging space for `bytes` more
    int copy(void* dst, const void* src, size_t bytes);
    int flush();                                     // to_device: host copies done and DMAs enqueued on return
    int finish();                                    // device -> host: DMAs done, then the host copies
};
static int stage_grow(blance_ctx* c, size_t need) {  // (the stream is idle, nothing pending)
    HostStage& st = c->stage;
    size_t cap = st.cap * 2 > need ? st.cap * 2 : need;
    cap = (cap + ((size_t)1 << 20)) & ~(((size_t)1 << 20) - 1);
    st.release();
    st.p = pin_alloc(cap);
    if (!st.p) return fail(BLANCE_ERR_DEVICE, "page-locked staging buffer: hipHostMalloc failed");
    st.cap = cap;
    st.used = 0;
    return 0;
}
int Mover::reserve(size_t bytes) {
    HostStage& st = c->stage;
    if (st.used + bytes <= st.cap) return 0;
    int e = to_device ? flush() : finish();
    if (e) return e;
    HIPTRY(stream_sync(c));
    if (bytes <= st.cap) { st.used = 0; return 0; }
    return stage_grow(c, bytes);
}
int Mover::copy(void* dst, const void* src, size_t bytes) {
    if (!bytes) return 0;
    const void* host = to_device ? src : dst;
    if (host_ptr_pinned(host, bytes)) {
        HIPTRY(hipMemcpyAsync(dst, src, bytes, to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, c->stream));
        return 0;
    }
    const size_t need = (bytes + 255) & ~(size_t)255;
    int e = reserve(need);
    if (e) return e;
    HostStage& st = c->stage;
    char* at = (char*)st.p + st.used;
    st.used += need;
    if (to_device) {
        if (bytes < ((size_t)1 << 20)) {
            memcpy(at, src, bytes);
            HIPTRY(hipMemcpyAsync(dst, at, bytes, hipMemcpyHostToDevice, c->stream));
        } else {
            host_copy.push_back(CopySeg{at, src, bytes});
            dma.push_back(CopySeg{dst, at, bytes});
        }
    } else {
        HIPTRY(hipMemcpyAsync(at, src, bytes, hipMemcpyDeviceToHost, c->stream));
        host_copy.push_back(CopySeg{dst, at, bytes});
    }
    return 0;
}
int Mover::flush() {
    if (!to_device) return 0;
    if (!host_copy.empty()) copy_threaded(host_copy);
    host_copy.clear();
    for (const CopySeg& g : dma) HIPTRY(hipMemcpyAsync(g.dst, g.src, g.bytes, hipMemcpyHostToDevice, c->stream));
    dma.clear();
    return 0;
}
int Mover::finish() {
    if (to_device) return flush();
    if (host_copy.empty()) return 0;
    HIPTRY(stream_sync(c));
    copy_threaded(host_copy);
    host_copy.clear();
    return 0;
}

template <class T>
static int put(Mover& mv, DevBuf& b, const T* src, size_t n) {
    if (b.reserve(n * sizeof(T))) return fail(BLANCE_ERR_DEVICE, "hipMalloc failed");
    return mv.copy(b.p, src, n * sizeof(T));
}
#define PUT(buf, src, n) do { int e__ = put(up, c->buf, src, (size_t)(n)); if (e__) return e__; } while (0)
#define RESERVE(buf, bytes) do { if (c->buf.reserve((size_t)(bytes))) return fail(BLANCE_ERR_DEVICE, "hipMalloc failed"); } while (0)

static inline int cdiv(int64_t a, int b) { return (int)((a + b - 1) / b); }

// up to four zero fills and one copy of int32 words in one launch (k_sweep.h: k_fill_copy)
struct FillCopyJob {
    FillCopy a{};
    int nz = 0;
    int64_t most = 0;
    bool over = false;              // more zero fills than kFillZeros, or a range past INT32_MAX words: run_fill_copy refuses
    void zero(void* p, int64_t words) {
        if (words <= 0) return;
        if (nz == kFillZeros || words > INT32_MAX) { over = true; return; }
        a.z[nz] = (int32_t*)p; a.zn[nz] = (int32_t)words; nz++;
        if (words > most) most = words;
    }
    void copy(void* dst, const void* src, int64_t words) {
        if (words > INT32_MAX) { over = true; return; }
        a.cd = (int32_t*)dst; a.cs = (const int32_t*)src; a.cn = (int32_t)words;
        if (words > most) most = words;
    }
};
static int run_fill_copy(blance_ctx* c, FillCopyJob& j) {
    if (j.over) return fail(BLANCE_ERR_DEVICE, "k_fill_copy job over its slots");
    if (j.most > 0) BLANCE_LAUNCH_NOSYNC(k_fill_copy, cdiv(j.most, 256), 256, 0, c->stream, j.a);
    return 0;
}

// The tables of one rule on their way to the device.  `t` (and the LeafTables n_leaves comes from) must outlive the next
// up.flush(): a big array is only noted here and copied into the staging buffer there.  upload_rule_tables keeps that rule
// for every vector of host/problem_facts.hpp; nothing else in the upload hands the Mover memory of a shorter life.
int blance_ctx::RuleRegions::put(Mover& up, const RuleTables& t, int leaves) {
    ok = t.ok;
    n_regions = t.n_regions;
    max_size = t.max_size;
    n_leaves = leaves;
    cls_run = t.cls_run;
    n_stay_wgs = t.n_stay_wgs;
    cyc_ok = t.cyc_ok;
    if (cyc_ok) h_cyc_reg_off = t.cyc_reg_off;
    struct { DevBuf* b; const std::vector<int32_t>* v; bool on; } rows[] = {
        {&wg_region, &t.wg_region, ok}, {&wg_chunk, &t.wg_chunk, ok}, {&node_region, &t.node_region, ok},
        {&reg_lo, &t.reg_lo, ok}, {&reg_hi, &t.reg_hi, ok}, {&leaf_cls, &t.leaf_cls, ok}, {&cls_size, &t.cls_size, ok},
        {&cyc, &t.cyc, cyc_ok}, {&cyc_reg_off, &t.cyc_reg_off, cyc_ok}, {&cyc_top_off, &t.cyc_top_off, cyc_ok}};
    for (auto& r : rows)
        if (r.on && ::put(up, *r.b, r.v->data(), r.v->size())) return BLANCE_ERR_DEVICE;
    return 0;
}

// ---- blance_upload, step by step.  Copies may still be reading the caller's arrays (and the staging buffer) when an error
// cuts a step short: enter() never returns with copies in flight.

// what the device's half of the validation yields beside its verdict
struct UploadSummary { PartsSummary ps; uint32_t assign_kinds; int64_t na; };

static int upload_arrays(blance_ctx* c, const blance_problem* pb, const NodeFacts& nodes, Mover& up) {
    const int NX = pb->n_nodes_ext, M = pb->n_states, P = pb->n_parts;
    const int64_t PM = (int64_t)P * M;
    c->stage.used = 0;                               // (the stream is idle between calls)
    {   // staging space for everything that may be pageable, asked for once
        const size_t per_part = 4 + 4 + 1 + 1 + 1, per_pm = 4 + 1 + 4 + 1;
        const size_t want = (size_t)P * per_part + (size_t)(PM + 1) * per_pm + (size_t)NX * 32 + (size_t)pb->n_loads * 13 + ((size_t)4 << 20);
        int st;
        if (c->stage.cap < want && (st = stage_grow(c, want))) return st;
    }
    PUT(node_removed, pb->node_removed, NX);
    PUT(node_added, pb->node_added, NX);
    PUT(node_weight, pb->node_weight, NX);
    PUT(node_has_weight, pb->node_has_weight, NX);
    PUT(alive, nodes.alive.data(), NX);
    PUT(alive_ids, nodes.alive_ids.data(), nodes.alive_ids.size());
    PUT(alive_rank, nodes.alive_rank.data(), NX);
    PUT(node_leaf_pos, pb->node_leaf_pos, NX);
    RESERVE(zeros_nx, NX + 1);
    HIPTRY(hipMemsetAsync(c->zeros_nx.p, 0, (size_t)NX + 1, c->stream));
    PUT(part_order, pb->part_order, P);
    PUT(part_weight, pb->part_weight, P);
    PUT(part_has_weight, pb->part_has_weight, P);
    PUT(part_in_prev, pb->part_in_prev, P);
    PUT(part_never_equal, pb->part_prev_never_equal, P);
    PUT(a_off, pb->assign_off, PM + 1);
    PUT(a_kind, pb->assign_kind, PM);
    PUT(p_off, pb->prev_off, PM + 1);
    PUT(p_kind, pb->prev_kind, PM);
    PUT(load_state, pb->load_state, pb->n_loads);
    PUT(load_node, pb->load_node, pb->n_loads);
    PUT(load_weight, pb->load_weight, pb->n_loads);
    PUT(load_first, pb->load_first_sweep_only, pb->n_loads);
    PUT(state_stick, pb->state_stickiness, M);
    PUT(state_has_stick, pb->state_has_stickiness, M);
    PUT(rule_inc, pb->rule_inc, pb->n_rules);
    PUT(rule_exc, pb->rule_exc, pb->n_rules);
    return up.flush();
}

// The O(P) checks of blance_validate and the sizes they yield, on the device (k_validate_parts, k_validate_ids), the rest
// of blance_validate on the host meanwhile; the lists' payloads go up between the two device checks.
static int upload_validate(blance_ctx* c, const blance_problem* pb, Mover& up, UploadSummary* sum) {
    const int NX = pb->n_nodes_ext, M = pb->n_states, P = pb->n_parts;
    const int64_t PM = (int64_t)P * M;
    int st;
    RESERVE(vres, 64);
    RESERVE(vseen, sizeof(uint32_t) * ((size_t)P / 32 + 2));
    HIPTRY(hipMemsetAsync(c->vres.p, 0, 64, c->stream));
    HIPTRY(hipMemsetAsync(c->vseen.p, 0, sizeof(uint32_t) * ((size_t)P / 32 + 1), c->stream));
    if (P > 0) {
        ValidateParams vp;
        memset(&vp, 0, sizeof vp);
        vp.P = P; vp.M = M; vp.weights_nil = pb->partition_weights_nil;
        for (int m = 0; m < M; m++) vp.k[m] = pb->state_constraints[m];
        vp.a_off = c->a_off.as<int32_t>(); vp.a_kind = c->a_kind.as<uint8_t>();
        vp.p_off = c->p_off.as<int32_t>(); vp.p_kind = c->p_kind.as<uint8_t>();
        vp.part_order = c->part_order.as<int32_t>(); vp.part_weight = c->part_weight.as<int32_t>();
        vp.part_has_weight = c->part_has_weight.as<uint8_t>(); vp.part_in_prev = c->part_in_prev.as<uint8_t>();
        vp.seen = c->vseen.as<uint32_t>(); vp.res = c->vres.as<int32_t>();
        const int vblocks = cdiv(PM > P ? PM : P, 256);
        BLANCE_LAUNCH(k_validate_parts, vblocks < 1024 ? vblocks : 1024, 256, 4 * 8 * sizeof(unsigned long long), c->stream, vp);
    }
    int32_t vr[16] = {0};
    HIPTRY(read_back(c, vr, c->vres.p, sizeof vr));
    const int tail_a = validate_tail_a(pb);          // (the host's share, while the device works)
    const std::string tail_a_text = g_last_error;
    HIPTRY(stream_sync(c));
    if (vr[3]) {                                      // the first list the host's loop would have refused, and why
        const int check = (INT_MAX - vr[3]) & 3;
        if (check == 0) return fail(BLANCE_ERR_BAD_ARG, "CSR offsets not monotone");
        if (check == 1) return fail(BLANCE_ERR_BAD_ARG, "bad list kind");
        return fail(BLANCE_ERR_UNSUPPORTED, "state list longer than 65535");
    }
    // the lists' payloads: their lengths are the last offsets, which are sound now
    const int64_t na = pb->assign_off[PM], np = pb->prev_off[PM];
    PUT(a_nodes, pb->assign_nodes, na);
    PUT(p_nodes, pb->prev_nodes, np);
    if ((st = up.flush())) return st;
    if (na > 0) BLANCE_LAUNCH(k_validate_ids, cdiv(na, 256), 256, 0, c->stream, (long long)na, NX, c->a_nodes.as<int32_t>(), kVErrAssignId, c->vres.as<int32_t>());
    if (np > 0) BLANCE_LAUNCH(k_validate_ids, cdiv(np, 256), 256, 0, c->stream, (long long)np, NX, c->p_nodes.as<int32_t>(), kVErrPrevId, c->vres.as<int32_t>());
    if (na > 0 || np > 0) {
        HIPTRY(read_back(c, vr, c->vres.p, sizeof(int32_t)));
        HIPTRY(stream_sync(c));
    }
    if (vr[0] & kVErrAssignId) return fail(BLANCE_ERR_BAD_ARG, "assign node id out of range");
    if (vr[0] & kVErrPrevId) return fail(BLANCE_ERR_BAD_ARG, "prev node id out of range");
    if (vr[0] & kVErrOrder) return fail(BLANCE_ERR_BAD_ARG, "part_order is not a permutation");
    if (tail_a) { g_last_error = tail_a_text; return tail_a; }
    long long r64[3];
    memcpy(r64, vr + 4, sizeof r64);
    sum->ps = PartsSummary{vr[1], vr[2], r64[0], r64[1], r64[2]};
    sum->assign_kinds = (uint32_t)vr[10];
    sum->na = na;
    return validate_tail_b(pb, sum->ps);
}

// what the sweep driver's shortcuts rest on
static void upload_facts(blance_ctx* c, const blance_problem* pb, const NodeFacts& nodes, const UploadSummary& sum) {
    const int M = pb->n_states;
    c->n_alive = nodes.n_alive;
    c->any_removed = nodes.any_removed;
    c->any_node_weight = nodes.any_node_weight;
    const OrderFacts o = order_facts(*pb, nodes, sum.na);
    c->top_prio_strict = o.top_prio_strict;
    c->cycle_order_stands = o.cycle_order_stands;
    c->uniform_first = o.uniform_first;
    c->uniform_all = o.uniform_all;
    if (getenv("BLANCE_NO_UNIFORM_CATEGORY")) c->uniform_first = c->uniform_all = false;   // (tests: the partition kernels on such inputs too)
    int L = 1;
    for (int m = 0; m < M; m++) if (pb->state_constraints[m] > L) L = pb->state_constraints[m];
    if (sum.ps.L > L) L = sum.ps.L;
    c->L = L;
    c->np_later = pb->n_prev + (int)sum.ps.fresh;          // plan.go:50
    c->assign_empty = sum.na == 0;
    c->assign_kinds = sum.assign_kinds;
    c->counts_start_zero = pb->n_loads == 0 && sum.ps.aprev == 0;
    c->out_capacity = sum.ps.cap;
    c->flat_chain_ok = pb->n_nodes_ext >= 1 && pb->n_nodes_ext <= 256 && L <= kChainOwn;   // wider: k_pass_seq is faster (measured)
    c->last_stays.assign((size_t)M, 0);
}

// what blance_plan_adopt analyses a node change from (the problem has passed validation: the arrays are there)
static void upload_keep_small(blance_ctx* c, const blance_problem* pb, const UploadSummary& sum) {
    const int NX = pb->n_nodes_ext;
    c->h_node_has_weight.assign(pb->node_has_weight, pb->node_has_weight + NX);
    c->h_node_weight.assign(pb->node_weight, pb->node_weight + NX);
    c->h_node_leaf_pos.assign(pb->node_leaf_pos, pb->node_leaf_pos + NX);
    c->h_rule_inc.assign(pb->rule_inc, pb->rule_inc + pb->n_rules);
    c->h_rule_exc.assign(pb->rule_exc, pb->rule_exc + pb->n_rules);
    const int VX = pb->hierarchy_rules_nil ? 0 : pb->n_vertices;
    c->h_vparent.assign(pb->vertex_parent, pb->vertex_parent + VX);
    c->h_vlo.assign(pb->vertex_leaf_lo, pb->vertex_leaf_lo + VX);
    c->h_vhi.assign(pb->vertex_leaf_hi, pb->vertex_leaf_hi + VX);
    c->sum_abs_weight = sum.ps.sumw;
    c->kept_load_abs = 0;
    for (int i = 0; i < pb->n_loads; i++)
        if (!pb->load_first_sweep_only[i]) c->kept_load_abs += pb->load_weight[i] < 0 ? -(long long)pb->load_weight[i] : pb->load_weight[i];
}

// the anchor and leaf tables and every rule's RuleRegions
static int upload_rule_tables(blance_ctx* c, const blance_problem* pb, const NodeFacts& nodes, Mover& up) {
    int st;
    const LeafTables leaf = leaf_tables(*pb);
    c->leaves_distinct = leaf.leaves_distinct;
    PUT(anchors, leaf.anchors.data(), leaf.anchors.size());
    PUT(leaf_node, leaf.leaf_node.data(), leaf.leaf_node.size());
    c->rule_regions.resize(pb->n_rules);
    for (int r = 0; r < pb->n_rules; r++) {
        const RuleTables t = analyse_rule(*pb, leaf, nodes, r);
        if ((st = c->rule_regions[r].put(up, t, leaf.n_leaves))) return st;
        if ((st = up.flush())) return st;                 // before `t` goes
    }
    return up.flush();                                    // ... and before `leaf` does
}

// the whole cluster as one region (flat single chain)
static int upload_flat_chain_tables(blance_ctx* c, int NX, Mover& up) {
    std::vector<int32_t> iota((size_t)NX + 1), zero((size_t)NX + 1, 0), one((size_t)NX + 1, 1);
    for (int i = 0; i <= NX; i++) iota[i] = i;
    int32_t lo0 = 0, hi0 = NX;
    PUT(fl_iota, iota.data(), iota.size());
    PUT(fl_zero, zero.data(), zero.size());
    PUT(fl_one, one.data(), one.size());
    PUT(fl_reglo, &lo0, 1);
    PUT(fl_reghi, &hi0, 1);
    return up.flush();                                    // before these locals go
}

static int upload_reserve(blance_ctx* c, const blance_problem* pb, Mover& up) {
    const int N = pb->n_nodes, NX = pb->n_nodes_ext, M = pb->n_states, P = pb->n_parts, L = c->L;
    const int64_t PM = (int64_t)P * M;
    const int RW = kRecHead + M * (1 + L);       // header + per-state lists
    int kmax = 1, maxB = 1;
    for (int m = 0; m < M; m++) if (pb->state_constraints[m] > kmax) kmax = pb->state_constraints[m];
    for (auto& rr : c->rule_regions) if (rr.ok && rr.n_regions > maxB) maxB = rr.n_regions;
    RESERVE(live, sizeof(int32_t) * (size_t)(PM * L + 1));
    RESERVE(live_len, sizeof(int32_t) * (size_t)(PM + 1));
    RESERVE(live_kind, (size_t)PM + 1);
    RESERVE(prv, sizeof(int32_t) * (size_t)(PM * L + 1));
    RESERVE(prv_len, sizeof(int32_t) * (size_t)(PM + 1));
    RESERVE(prv_kind, (size_t)PM + 1);
    RESERVE(in_prev, (size_t)P + 1);
    RESERVE(never_equal, (size_t)P + 1);
    RESERVE(cnt, sizeof(int32_t) * (size_t)(M + 1) * (NX + 1));
    RESERVE(cnt_next, sizeof(int32_t) * (size_t)(M + 1) * (NX + 1));
    RESERVE(ntn, sizeof(int32_t) * (size_t)(NX + 1) * (N > 0 ? N : 1));
    RESERVE(cat, (size_t)P + 1);
    RESERVE(order, sizeof(int32_t) * ((size_t)P + 1));
    RESERVE(chunk_counts, sizeof(int32_t) * 3 * (size_t)(cdiv(P, kPartChunk) + 1));
    RESERVE(rec, sizeof(int32_t) * ((size_t)P * RW + 64));
    RESERVE(out, sizeof(int32_t) * ((size_t)P * (1 + kmax) + 1));
    RESERVE(warn_part, sizeof(int32_t) * (size_t)(PM + 1));
    RESERVE(warn_state, sizeof(int32_t) * (size_t)(PM + 1));
    RESERVE(scalars, sizeof(int32_t) * kScalWords);   // (blance_kernels.h: ScalarWord)
    RESERVE(ntn_bits, sizeof(uint32_t) * (queue_bits_words(NX) + 4));
    RESERVE(regid, sizeof(int32_t) * ((size_t)P + 1));
    RESERVE(chain_order, sizeof(int32_t) * ((size_t)P + 1));
    RESERVE(chain_inv, sizeof(int32_t) * ((size_t)P + 1));
    RESERVE(bucket_counts, sizeof(int32_t) * ((size_t)maxB * (cdiv(P, kPartChunk) + 1) + 1));
    RESERVE(reg_off, sizeof(int32_t) * ((size_t)maxB + 2));
    RESERVE(cnt_save, sizeof(int32_t) * (size_t)(M + 1) * (NX + 1));
    if (maxB > 1) {
        const size_t emax = (size_t)P * L + 1;
        RESERVE(n_ev, sizeof(int32_t) * ((size_t)P + 2));
        RESERVE(chain_oi, sizeof(int32_t) * ((size_t)P + 1));
        RESERVE(ev_key, sizeof(int32_t) * emax);
        RESERVE(ev_oi, sizeof(int32_t) * emax);
        RESERVE(ev_leaf, sizeof(int32_t) * emax);
        RESERVE(ev_w, sizeof(int32_t) * emax);
        RESERVE(ev_perm, sizeof(int32_t) * emax);
        RESERVE(ev_off, sizeof(int32_t) * ((size_t)maxB + 2));
        RESERVE(ev_counts, sizeof(int32_t) * ((size_t)maxB * (cdiv((int64_t)emax, kPartChunk) + 1) + 1));
    }
    if (maxB > 1 || c->flat_chain_ok) RESERVE(crec, sizeof(int32_t) * ((size_t)P * kCW + 64));
    if (c->flat_chain_ok) {
        int st = upload_flat_chain_tables(c, NX, up);
        if (st) return st;
    }
    RESERVE(f_tot, sizeof(int32_t) * ((size_t)NX + 1));
    RESERVE(f_g, sizeof(double) * ((size_t)NX + 1));
    RESERVE(f_top_g, sizeof(double) * kTopList);
    RESERVE(f_top_n, sizeof(int32_t) * kTopList);
    RESERVE(f_row_count, sizeof(int32_t) * ((size_t)NX + 2));
    RESERVE(f_m, sizeof(int32_t) * ((size_t)N + 2));
    RESERVE(f_moff, sizeof(int32_t) * ((size_t)N + 2));
    RESERVE(f_keys_a, sizeof(unsigned long long) * (2 * (size_t)P + 4));      // fresh runs: up to 2 picks per step, + 1
    RESERVE(f_keys_b, sizeof(unsigned long long) * (2 * (size_t)P + 4));
    RESERVE(f_vals_a, sizeof(int32_t) * (2 * (size_t)P + 4));
    RESERVE(f_vals_b, sizeof(int32_t) * (2 * (size_t)P + 4));
    RESERVE(f_hist, sizeof(int32_t) * 256 * ((size_t)cdiv(2 * (int64_t)P + 4, kSortTile) + 1));
    return 0;
}

static int upload_inner(blance_ctx* c, const blance_problem* pb) {
    int st = validate_head(pb);
    if (st) return st;
    HIPTRY(hipSetDevice(c->device));
    c->uploaded = false;
    c->planned = false;
    c->wire_names = false;                           // (they were the names of the problem this one replaces)
    c->loads_later_only = false;
    c->h = *pb;
    const int M = pb->n_states;
    c->state_priority.assign(pb->state_priority, pb->state_priority + M);
    c->state_constraints.assign(pb->state_constraints, pb->state_constraints + M);
    c->rule_off.assign(pb->rule_off, pb->rule_off + M + 1);
    c->rule_regions.clear();
    const NodeFacts nodes = node_facts(*pb);         // (copied from by every flush below: it lives to the end)
    Mover up(c, true);
    UploadSummary sum;
    if ((st = upload_arrays(c, pb, nodes, up))) return st;
    if ((st = upload_validate(c, pb, up, &sum))) return st;
    upload_facts(c, pb, nodes, sum);
    upload_keep_small(c, pb, sum);
    if (!pb->hierarchy_rules_nil && (st = upload_rule_tables(c, pb, nodes, up))) return st;
    if ((st = upload_reserve(c, pb, up))) return st;
    if ((st = up.flush())) return st;
    HIPTRY(stream_sync(c));
    // the caller's arrays are not retained: drop the host pointers
    blance_problem& h = c->h;
    h.state_priority = h.state_constraints = h.state_stickiness = nullptr;
    h.state_has_stickiness = h.node_removed = h.node_added = nullptr;
    c->uploaded = true;
    return BLANCE_OK;
}

// is a collective of this context's communicator more than a no-op? / does a chain pass over n_regions regions run sharded?
static bool comm_active(const blance_ctx* c) { return c->comm.n_ranks > 1 || c->shard_one_rank; }
static bool pass_sharded(const blance_ctx* c, int n_regions) { return comm_active(c) && n_regions >= c->comm.n_ranks; }

// The fields the parameter blocks of the pass kernels (PassParams, ChainParams, StayParams, FlatParams) share, for the pass
// of state s with k constraints; everything else is zero.
template <class Q>
static void fill_pass_common(const blance_ctx* c, Q& q, int s, int k, int NP) {
    const blance_problem& h = c->h;
    memset(&q, 0, sizeof q);
    q.N = h.n_nodes; q.NX = h.n_nodes_ext; q.M = h.n_states; q.s = s; q.k = k; q.NP = NP; q.OW = 1 + k;
    q.booster_kind = h.booster_kind;
    q.alive = c->alive.as<uint8_t>(); q.node_weight = c->node_weight.as<int32_t>(); q.node_has_weight = c->node_has_weight.as<uint8_t>();
    q.cnt = c->cnt.as<int32_t>();
}
// ... and a rule's region tables (ChainParams, StayParams)
template <class Q>
static void fill_region_tables(const blance_ctx* c, const blance_ctx::RuleRegions& rr, Q& q) {
    q.reg_lo = rr.reg_lo.as<int32_t>(); q.reg_hi = rr.reg_hi.as<int32_t>();
    q.leaf_node = c->leaf_node.as<int32_t>(); q.leaf_cls = rr.leaf_cls.as<int32_t>(); q.cls_size = rr.cls_size.as<int32_t>();
}

// (the launch shapes of the sweep's record, list-edit and tail kernels, named once: tests/kernels/sweep_cases.inc runs the same)
struct LaunchShape { int grid, block; size_t lds; };
// a workgroup stages its records in LDS at a row stride of RW | 1 words
static LaunchShape shape_gather(int P, int RW) { return {cdiv(P, 256), 256, sizeof(int32_t) * 256 * (size_t)(RW | 1) + 64}; }
static LaunchShape shape_gather_chain(int P) { return {cdiv(P, 256), 256, sizeof(int32_t) * 256 * (kCW + 1) + 64}; }
static LaunchShape shape_chain_classify(int P) { return {cdiv(P + 1, 256), 256, 0}; }     // (one thread more: n_ev[P])
static LaunchShape shape_ntn_bits(int rows) { return {cdiv(rows, 4), 256, 0}; }           // (a wave64 per row)
static LaunchShape shape_scatter(int P) { return {cdiv(P, 256), 256, 0}; }
static LaunchShape shape_converge(int P) { return {cdiv(P, 256), 256, 0}; }
static LaunchShape shape_sweep_tail(int P) { return {cdiv(P, 256), 256, 0}; }

// f_row_count zeroed for a kernel that adds to it (k_flat_row_count, k_flat_row_count_live, k_gather)
static int rowcount_reset(blance_ctx* c) {
    if (!c->rowcount_clean) HIPTRY(hipMemsetAsync(c->f_row_count.p, 0, sizeof(int32_t) * ((size_t)c->h.n_nodes_ext + 1), c->stream));
    c->rowcount_clean = false;
    return 0;
}

// plan.go:266: a state pass starts from an empty nodeToNodeCounts.  Called by whatever is about to read or bump the matrix
// in HBM (NumPartitions > 0); the first such call of a pass zeroes it (a pass that never calls this -- region chains with their
// rows in LDS, a pass that is one run of stays -- does not pay for the 67 MB).
static int ntn_prepare(blance_ctx* c) {
    if (!c->pass_ntn_ready) {
        const blance_problem& h = c->h;
        HIPTRY(hipMemsetAsync(c->ntn.p, 0, sizeof(int32_t) * (size_t)(h.n_nodes_ext + 1) * (h.n_nodes > 0 ? h.n_nodes : 1), c->stream));
        HIPTRY(hipMemsetAsync(c->ntn_bits.p, 0, sizeof(uint32_t) * queue_bits_words(h.n_nodes_ext), c->stream));
        c->pass_ntn_ready = true;
        c->bits_stale = false;
    }
    return 0;
}
#define NTNTRY() do { int e__ = ntn_prepare(c); if (e__) return e__; } while (0)

// A state pass (or a sub-range of one) in order.  Flat passes (no hierarchy rule for the state) of up
// to kTreeMaxNodes node names: one wave64 with bound-ordered candidates (k_pass_tree.h) -- the cost
// of a step does not grow with the cluster; everything else: the workgroup pass k_pass_seq.
static int dispatch_pass_tree_or_seq(blance_ctx* c, const PassParams& q) {
    if (q.NP > 0) NTNTRY();
    c->bits_stale = true;
    const bool tree = !c->no_tree && c->engine != BLANCE_ENGINE_SEQUENTIAL && (c->force_threads == 0 || c->tree_always);
    if (tree && launch_pass_tree(c->stream, q, (c->tree_dense ? 1 : 0) | (c->tree_long ? 2 : 0))) {
        if (c->trace) fprintf(stderr, "[blance] k_pass_tree state %d steps [%d, %d) k %d\n", q.s, q.beg, q.end, q.k);
        return 0;
    }
    if (launch_pass_seq(c->stream, q, c->force_threads, !c->no_seq_spec && c->engine != BLANCE_ENGINE_SEQUENTIAL))
        return fail(BLANCE_ERR_UNSUPPORTED, "too many nodes for the register-resident pass");
    return 0;
}

// Flat passes with k <= 2 first go to k_pass_queue (k_pass_queue.h: the candidates as a sorted window over the lanes of
// one wave64).  It stops at a step it does not take (q.stop); k_pass_tree / k_pass_seq then do a few steps -- more after
// every stop that comes soon after the last one -- and the queue kernel takes over again.
static int dispatch_pass(blance_ctx* c, const PassParams& q0) {
    const bool queue = !c->no_queue && !c->no_tree && c->engine != BLANCE_ENGINE_SEQUENTIAL && (c->force_threads == 0 || c->tree_always) &&
                       !c->tree_dense && !c->tree_long && q0.k <= 2 && q0.rule_begin >= q0.rule_end && q0.NX >= 1 && q0.NX <= 4096;
    if (!queue) return dispatch_pass_tree_or_seq(c, q0);
    PassParams q = q0;
    if (q.NP > 0) NTNTRY();
    int32_t* scal = c->scalars.as<int32_t>();
    q.ntn_bits = c->ntn_bits.as<uint32_t>();
    q.stop = scal + kScalQueueStop;
    q.qstats = (long long*)(scal + kScalQueueStats);
    q.spec = (c->queue_general ? 8 : 0) | (c->queue_force_dense ? 16 : 0) | (c->queue_no_asm ? 32 : 0) | (c->queue_exact_rebuild ? 64 : 0) |
             (c->queue_bits_self ? 128 : 0);
    int pos = q0.beg, chunk = 64;
    while (pos < q0.end) {
        q.beg = pos; q.end = q0.end;
        if (q.NP > 0 && c->bits_stale) {
            const long long words = (long long)queue_bits_words(q.NX);
            const LaunchShape bs = shape_ntn_bits(q.NX + 1);
            BLANCE_LAUNCH(k_ntn_bits, bs.grid, bs.block, bs.lds, c->stream, q.N, q.NX + 1, (int)(words / (q.NX + 1)), q.ntn, q.ntn_bits);
            c->bits_stale = false;
        }
        if (!launch_pass_queue(c->stream, q)) { q.beg = pos; return dispatch_pass_tree_or_seq(c, q); }
        int32_t st[2] = {0, 0};
        HIPTRY(read_back(c, st, scal + kScalQueueStop, sizeof st));
        HIPTRY(stream_sync(c));
        c->queue_launches++;
        if (c->trace) fprintf(stderr, "[blance] k_pass_queue state %d steps [%d, %d) k %d: stopped at %d (%d)\n", q.s, pos, q0.end, q.k, st[0], st[1]);
        if (st[0] < pos || st[0] > q0.end) return fail(BLANCE_ERR_DEVICE, "k_pass_queue returned a position outside its range");
        if (st[0] >= q0.end) break;
        c->queue_stops++;
        chunk = st[0] - pos < 4096 ? (chunk < 65536 ? chunk * 2 : chunk) : 64;
        PassParams t = q0;
        t.beg = st[0];
        t.end = q0.end - st[0] < chunk ? q0.end : st[0] + chunk;
        const int e = dispatch_pass_tree_or_seq(c, t);
        if (e) return e;
        pos = t.end;
    }
    return 0;
}

// exclusive scan of n ints on the planner's stream (k_sweep.h: one workgroup for short arrays, tile
// totals + per-tile scans over the whole chip for long ones)
static int launch_scan_excl_on(blance_ctx* c, hipStream_t stream, DevBuf& sums, int n, int32_t* data) {
    if (n <= 4 * kScanTile) {
        BLANCE_LAUNCH(k_scan_excl, 1, 1024, 256, stream, n, data);
        return 0;
    }
    const int tiles = cdiv(n, kScanTile);
    if (sums.reserve(sizeof(int32_t) * ((size_t)tiles + 1))) return fail(BLANCE_ERR_DEVICE, "hipMalloc failed");
    BLANCE_LAUNCH(k_scan_tile_sums, tiles, 1024, 256, stream, n, data, sums.as<int32_t>());
    BLANCE_LAUNCH(k_scan_excl, 1, 1024, 256, stream, tiles, sums.as<int32_t>());
    BLANCE_LAUNCH(k_scan_apply, tiles, 1024, 256, stream, n, data, sums.as<int32_t>());
    return 0;
}
// Stable counting sort of n items by key[i] < B: offs[B + 1] = where each key's items begin, out[] = src[i] (or i, src null)
// in key order, out_oi[] (or null) = i in that order.  counts: B * cdiv(n, kPartChunk) + 1 words of scratch.
static int group_by_key(blance_ctx* c, hipStream_t st, DevBuf& sums, int n, const int32_t* key, const int32_t* src, int B,
                        int32_t* counts, int32_t* offs, int32_t* out, int32_t* out_oi) {
    const int nch = cdiv(n, kPartChunk);
    int bits = 1;
    while ((1 << bits) < B) bits++;
    BLANCE_LAUNCH(k_part_count, nch, 64, sizeof(int32_t) * B + 64, st, n, key, (const uint8_t*)nullptr, (const int32_t*)nullptr, nch, B, counts);
    const int se = launch_scan_excl_on(c, st, sums, B * nch, counts);
    if (se) return se;
    BLANCE_LAUNCH_NOSYNC(k_region_offsets, cdiv(B + 1, 64), 64, 0, st, B, nch, n, counts, offs);
    BLANCE_LAUNCH(k_part_scatter, nch, 64, sizeof(int32_t) * B + 64, st, n, key, (const uint8_t*)nullptr, (const int32_t*)nullptr, src, nch, B, bits,
                  counts, out, out_oi);
    return 0;
}
static int launch_scan_excl(blance_ctx* c, int n, int32_t* data) { return launch_scan_excl_on(c, c->stream, c->scan_sums, n, data); }
#define SCANTRY(n, data) do { int e__ = launch_scan_excl(c, (n), (data)); if (e__) return e__; } while (0)

// The launch shapes of the bulk primitives below, each named once: the driver and the single-kernel cases of
// tests/kernels/kernel_cases.inc go through the same lines.
// pass_order's stable partition of the static order by partitionSorter category (plan.go:542-561): item i has category
// cat[index[i]] < kCatBuckets, out[] = index[] in category order.  counts: kCatBuckets * cdiv(n, kPartChunk) words.
constexpr int kCatBuckets = 3, kCatBits = 2;
static int partition_by_category(blance_ctx* c, int n, const uint8_t* cat, const int32_t* index, int32_t* counts, int32_t* out) {
    const int n_chunks = cdiv(n, kPartChunk);
    hipStream_t sm = c->stream;
    BLANCE_LAUNCH(k_part_count, n_chunks, 64, 64, sm, n, (const int32_t*)nullptr, cat, index, n_chunks, kCatBuckets, counts);
    SCANTRY(kCatBuckets * n_chunks, counts);
    BLANCE_LAUNCH(k_part_scatter, n_chunks, 64, 64, sm, n, (const int32_t*)nullptr, cat, index, index, n_chunks, kCatBuckets, kCatBits,
                  counts, out, (int32_t*)nullptr);
    return 0;
}
static void launch_sort_varbits(hipStream_t sm, int n, const unsigned long long* keys, unsigned long long* vbits) {
    BLANCE_LAUNCH(k_sort_varbits, cdiv(n, 256 * kVarbitsPer), 256, 0, sm, n, keys, vbits);
}
static void launch_flat_row_count(hipStream_t sm, const FlatParams& fq, int32_t* row_count) {
    BLANCE_LAUNCH(k_flat_row_count, cdiv(fq.P, 256), 256, 0, sm, fq, row_count);
}
static void launch_flat_scan_min(hipStream_t sm, int n_waves, const int32_t* part, int32_t* scan, int32_t* not_whole, int end) {
    BLANCE_LAUNCH(k_flat_scan_min, 1, 1024, 256, sm, n_waves, part, scan, not_whole, end);
}
// (the launch shapes of run_flat_pass's stay side, named once: tests/kernels/kernel_cases.inc runs the same)
static void launch_flat_prepare(hipStream_t sm, const FlatParams& fq, int32_t* tot, double* g, double* top_g, int32_t* top_n) {
    BLANCE_LAUNCH(k_flat_prepare, 1, 1024, sizeof(RedSlot) * 32 + 64, sm, fq, tot, g, top_g, top_n);
}
static void launch_flat_prepare_count_live(hipStream_t sm, const FlatParams& fq, int32_t* tot, double* g, double* top_g, int32_t* top_n,
                                           const DevProblem& d, int32_t* row_count) {
    BLANCE_LAUNCH(k_flat_prepare_count_live, 1 + cdiv(fq.P, 1024), 1024, sizeof(RedSlot) * 32 + 64, sm, fq, tot, g, top_g, top_n, d, row_count);
}
static void launch_flat_stay_live(hipStream_t sm, const FlatParams& fq, const DevProblem& d, const int32_t* order,
                                  const int32_t* state_stickiness, const uint8_t* state_has_stickiness, int32_t* moved) {
    BLANCE_LAUNCH(k_flat_stay_live, cdiv(fq.P, 256), 256, 0, sm, fq, d, order, state_stickiness, state_has_stickiness, moved);   // (uses a wave ballot)
}
static int flat_scan_waves(int beg, int end) { return cdiv(end - beg, 256) * 4; }
// (fq.scan_waves = flat_scan_waves(beg, end), fq.scan_part sized for it)
static void launch_flat_scan(hipStream_t sm, const FlatParams& fq, int beg, int end) {
    BLANCE_LAUNCH(k_flat_scan, cdiv(end - beg, 256), 256, 0, sm, fq, beg, end);
}
static void launch_flat_commit_stay(hipStream_t sm, const FlatParams& fq, int beg, int end, int bump) {
    BLANCE_LAUNCH_NOSYNC(k_flat_commit_stay, cdiv(end - beg, 256), 256, 0, sm, fq, beg, end, bump);
}


// stable LSD radix sort of the n (key, value) pairs in the f_*_a buffers; *sorted_vals = the buffer the sorted
// values ended in (a or b: no copy back), *other_vals = the other one (free for the caller)
// (known_varying: the key bits that can differ at all, when the caller can tell -- no varbits launch, no round trip)
static int radix_sort_pairs(blance_ctx* c, int n, int64_t* launches, int32_t** sorted_vals, int32_t** other_vals,
                            const unsigned long long* known_varying) {
    const int n_tiles = cdiv(n, kSortTile);
    unsigned long long* ka = c->f_keys_a.as<unsigned long long>();
    unsigned long long* kb = c->f_keys_b.as<unsigned long long>();
    int32_t* va = c->f_vals_a.as<int32_t>();
    int32_t* vb = c->f_vals_b.as<int32_t>();
    // byte positions equal in every key need no pass (scores of one pass share most of their bits)
    unsigned long long* vbits = (unsigned long long*)(c->scalars.as<int32_t>() + kScalSortVarying);
    unsigned long long varying = 0;
    if (known_varying) {
        varying = *known_varying;
    } else {
        HIPTRY(hipMemsetAsync(vbits, 0, sizeof varying, c->stream));
        launch_sort_varbits(c->stream, n, ka, vbits);
        HIPTRY(read_back(c, &varying, vbits, sizeof varying));
        HIPTRY(stream_sync(c));
        *launches += 1;
    }
    for (int shift = 0; shift < 64; shift += 8) {
        if (((varying >> shift) & 0xff) == 0) continue;
        BLANCE_LAUNCH(k_sort_hist, n_tiles, 64, 1024 + 64, c->stream, n, shift, ka, n_tiles, c->f_hist.as<int32_t>());
        SCANTRY(256 * n_tiles, c->f_hist.as<int32_t>());
        BLANCE_LAUNCH(k_sort_scatter, n_tiles, 64, 1024 + 64, c->stream, n, shift, ka, va, kb, vb, n_tiles,
                      c->f_hist.as<int32_t>());
        std::swap(ka, kb);
        std::swap(va, vb);
        *launches += 3;
    }
    *sorted_vals = va;                               // (the loop swapped the roles after every pass)
    *other_vals = vb;
    return 0;
}

// The first RS picks of a fresh run from step `pos` on, sorted: how many each node receives (f_m, f_moff), the (score, node)
// elements in node-major order, the stable sort (k_flat.h "fresh identical run")
static int fresh_run_sorted(blance_ctx* c, const FlatParams& fq, int pos, int RS, int64_t* launches, int32_t** sorted_vals,
                            int32_t** other_vals) {
    hipStream_t sm = c->stream;
    BLANCE_LAUNCH(k_fresh_threshold, 1, 1024, 16384 + 64, sm, fq, pos, RS, c->f_m.as<int32_t>(),
                  c->f_moff.as<int32_t>());
    BLANCE_LAUNCH_NOSYNC(k_fresh_emit, cdiv(RS, 256), 256, 0, sm, fq, pos, RS, c->f_moff.as<int32_t>(),
                         c->f_keys_a.as<unsigned long long>(), c->f_vals_a.as<int32_t>());
    return radix_sort_pairs(c, RS, launches, sorted_vals, other_vals, nullptr);
}
// ... its closed form (k_fresh_cycle): the nodes of nodesNext by id, again and again
static void fresh_cycle_sorted(blance_ctx* c, int N, int RS, int32_t** sorted_vals, int32_t** other_vals) {
    *sorted_vals = c->f_vals_a.as<int32_t>();
    *other_vals = c->f_vals_b.as<int32_t>();
    BLANCE_LAUNCH_NOSYNC(k_fresh_cycle, cdiv(RS > N ? RS : N, 256), 256, 0, c->stream, RS, c->n_alive, N,
                         c->alive_ids.as<int32_t>(), c->alive_rank.as<int32_t>(), *sorted_vals, c->f_m.as<int32_t>());
}
// The exclusion automaton over the R steps from `pos` (k_flat.h, above fresh_excluded): S = the exclusion-free sequence,
// picks[k R] = what the steps take, *bad = the first step that is not exact (INT_MAX: none), read back through bad_word.
// (threads of a few steps each: coalesced record reads; up to 64 workgroups)
static int fresh_excl_groups(int R) {
    const int G = cdiv(R, 4 * 1024);
    return G < 1 ? 1 : G > 64 ? 64 : G;
}
static int fresh_excl_resolve(blance_ctx* c, const FlatParams& fq, int pos, int R, const int32_t* S, int32_t* picks,
                              int32_t* bad_word, int32_t* bad) {
    hipStream_t sm = c->stream;
    *bad = INT_MAX;
    HIPTRY(hipMemcpyAsync(bad_word, bad, sizeof *bad, hipMemcpyHostToDevice, sm));
    const int G = fresh_excl_groups(R);
    RESERVE(f_comp, (size_t)G * 1024 + 64 + 64);
    unsigned char* comp = c->f_comp.as<unsigned char>();
    BLANCE_LAUNCH(k_fresh_excl_scan, G, 1024, 2048 + 64, sm, fq, pos, R, S, comp, comp + (size_t)G * 1024);
    BLANCE_LAUNCH_NOSYNC(k_fresh_excl_apply, G, 1024, 0, sm, fq, pos, R, S, comp, comp + (size_t)G * 1024, picks, bad_word);
    HIPTRY(read_back(c, bad, bad_word, sizeof *bad));
    HIPTRY(stream_sync(c));
    return 0;
}

static bool dispatch_chain(blance_ctx* c, ChainParams& q, int max_size, const ChainHandoff& ho = ChainHandoff{nullptr, 0});

// Steps [beg, end) of a flat pass on ONE wave64 (clusters of <= 256 node names): the
// chain kernel with the whole cluster as its region and every node its own exclude
// class.  Where the chain cannot go on exactly it stops; k_pass_seq does a few steps
// and the chain resumes.  crec must hold the pass's compact records in pass order.
static int run_flat_chain(blance_ctx* c, PassParams q, int beg, int end, bool lds_rows, int32_t* scal,
                          int64_t* launches) {
    hipStream_t sm = c->stream;
    if (q.NP > 0) NTNTRY();
    c->bits_stale = true;
    int32_t* flags = scal + kScalFlags;
    ChainParams cq;
    fill_pass_common(c, cq, q.s, q.k, q.NP);
    cq.L = q.L;
    cq.n_regions = 1; cq.n_launch = 1; cq.flat = 1; cq.waves = c->chain_waves;
    cq.reg_lo = c->fl_reglo.as<int32_t>(); cq.reg_hi = c->fl_reghi.as<int32_t>();
    cq.reg_off = c->reg_off.as<int32_t>();
    cq.leaf_node = c->fl_iota.as<int32_t>(); cq.leaf_cls = c->fl_iota.as<int32_t>(); cq.cls_size = c->fl_one.as<int32_t>();
    cq.ntn = q.ntn; cq.crec = c->crec.as<int32_t>(); cq.out = q.out; cq.flags = flags;
    int pos = beg;
    c->chain_group_state = -1;                       // (reg_off is this chain's range from here on)
    c->group_epoch++;
    while (pos < end) {
        int32_t range[2] = {pos, end};
        HIPTRY(hipMemcpyAsync(c->reg_off.p, range, sizeof range, hipMemcpyHostToDevice, sm));
        HIPTRY(hipMemsetAsync(flags, 0, sizeof(int32_t) * kChainFlags, sm));
        c->flags_clean = false;
        cq.ntn_in_lds = lds_rows ? 1 : 0;
        if (!dispatch_chain(c, cq, q.NX)) return fail(BLANCE_ERR_UNSUPPORTED, "flat chain shape");
        int32_t fl[kChainFlags] = {0};
        HIPTRY(read_back(c, fl, flags, sizeof fl));
        HIPTRY(stream_sync(c));
        *launches += 1;
        lds_rows = false;                          // a stopped chain handed its rows to global memory
        if (fl[kFlagNotLocal]) return 1;           // a step the compact record cannot hold: caller falls back
        if (!fl[kFlagEscaped]) break;              // ran to the end
        if (fl[kFlagStopRange]) c->no_fast_keys = true;
        int stop = fl[kFlagStopAt];
        int nseq = end - stop < 16 ? end - stop : 16;
        q.beg = stop; q.end = stop + nseq;
        int e = dispatch_pass(c, q);
        if (e) return e;
        *launches += 1;
        pos = stop + nseq;
    }
    return 0;
}

// The compact records a flat single chain walks (clusters of <= 256 names), made when a pass first needs them: a pass the
// bulk runs settle entirely (config 2: every pass) never pays for the gather and its round trip.
struct FlatChainPrep {
    bool possible = false, done = false, ok = false;
    DevProblem d;
    int m = 0, higher_mask = 0;
    const int32_t* order = nullptr;
};
static int flat_chain_prepare(blance_ctx* c, FlatChainPrep& fc, int64_t* launches) {
    if (fc.done || !fc.possible) return 0;
    fc.done = true;
    const blance_problem& h = c->h;
    hipStream_t sm = c->stream;
    int32_t* flags = c->scalars.as<int32_t>() + kScalFlags;
    HIPTRY(hipMemsetAsync(flags, 0, sizeof(int32_t) * kChainFlags, sm));
    c->flags_clean = false;
    const LaunchShape gs = shape_gather_chain(h.n_parts);
    BLANCE_LAUNCH(k_gather_chain, gs.grid, gs.block, gs.lds, sm, fc.d, fc.m, h.top_state, fc.higher_mask,
                         fc.order, (const int32_t*)nullptr, c->state_stick.as<int32_t>(),
                         c->state_has_stick.as<uint8_t>(), c->fl_iota.as<int32_t>(),
                         c->fl_zero.as<int32_t>(), c->fl_reglo.as<int32_t>(), c->fl_iota.as<int32_t>(),
                         c->fl_one.as<int32_t>(), 1, 0,
                         c->crec.as<int32_t>(), flags, (int32_t*)nullptr, kNoGate);
    int32_t bad = 0;
    HIPTRY(read_back(c, &bad, flags + kFlagNotLocal, sizeof bad));
    HIPTRY(stream_sync(c));
    *launches += 1;
    fc.ok = !bad;                                  // (bad: some step does not fit the compact record)
    return 0;
}

// The opening pass of a plan from nothing that run_flat_pass settles as one fresh run in (key, node) order without looking at
// a step record: every partition to assign holds no node and has no weight of its own, so no step is a stay and every step
// is fresh with weight 1 (known_run); integer keys from counters that all start at zero make the run a round robin over
// nodesNext (k_fresh_cycle); and no step excludes a node.  Asked by run_pass_in_order before it gathers, and by run_flat_pass.
// (NumPartitions == 0 here: the stay test's row bound, which would ride on the gather, is not wanted.)
static bool fresh_cycle_whole(const blance_ctx* c, bool opening, int NP, int k, int higher_mask) {
    return opening && c->assign_empty && c->h.partition_weights_nil && c->speculate > 0 && NP == 0 && !c->any_node_weight &&
           c->counts_start_zero && higher_mask == 0 && k == 1 && c->n_alive > 0 && c->h.n_parts > 0;
}

// A flat pass (no hierarchy rule for the state): runs of certain stays and of
// fresh identical partitions are resolved in bulk, the rest by k_pass_seq in
// order on sub-ranges.  See the "Flat bulk engine" comment above the kernels.
// opening: a pass of a plan's first sweep whose steps the host knows to be fresh and alike without looking -- the first pass
// over partitions that hold nothing, or the second when the first gave every partition ONE node in a state of higher priority
// and NumPartitions == 0 (k_flat_scan's test for "fresh": such a node is just not a candidate).  *whole_known: the pass was
// such a run from its first step to its last.
// assume_stays: a `settled` pass whose stay test is enqueued and NOT read back: the pass is taken to be one run of stays, and
// k_flat_stay_live's verdict goes to scal[kScalFlags + kFlagTopMoved] for the caller's gates and its sweep's readback (plan_locked).
static int run_flat_pass(blance_ctx* c, PassParams q, int32_t* scal, int64_t* launches, int64_t* batched,
                         FlatChainPrep& fc, bool opening, bool* whole_known, bool settled, bool assume_stays,
                         bool* nothing_to_apply, bool rows_counted) {
    *whole_known = false;
    *nothing_to_apply = false;
    hipStream_t sm = c->stream;
    c->bits_stale = true;                           // (the bulk kernels below bump nodeToNodeCounts, not k_pass_queue's bit maps)
    const int P = q.P;
    // (the driver's own words: outside the chain flags, which only chain code writes -- blance_ctx::flags_clean)
    int32_t* scan_words = scal + kScalFlatScan;
    int32_t* bad_word = scal + kScalFlatBad;
    FlatParams fq;
    fill_pass_common(c, fq, q.s, q.k, q.NP);
    fq.L = q.L; fq.P = P; fq.top_state = q.top_state; fq.RW = q.RW; fq.higher_mask = q.higher_mask;
    fq.tot = c->f_tot.as<int32_t>(); fq.g = c->f_g.as<double>();
    fq.top_g = c->f_top_g.as<double>(); fq.top_n = c->f_top_n.as<int32_t>();
    fq.row_count = c->f_row_count.as<int32_t>();
    fq.ntn = q.ntn; fq.rec = q.rec; fq.out = q.out; fq.scan = scan_words;
    fq.int_keys = (q.NP == 0 && !c->any_node_weight) ? 1 : 0;
    // the load totals and the smallest partition-independent scores: what the scan and the fresh run's threshold test against
    auto prepare = [&]() {
        launch_flat_prepare(sm, fq, c->f_tot.as<int32_t>(), c->f_g.as<double>(), c->f_top_g.as<double>(), c->f_top_n.as<int32_t>());
    };
    if (assume_stays) {
        // The stay test of the whole pass on the live lists (no step records: k_gather is not run), its row bound counted
        // from them as well; the verdict stays on the device.  What the pass would then do -- nothing, see `settled` below --
        // is done: no output, no k_scatter, and the top priority nodes are where they were.
        // One launch for what the test reads (the row bound only when NP > 0), one for the test, which leaves its verdict
        // word itself: open_sweep's fill zeroes kFlagTopMoved with the chain flags, nothing between that fill and this pass
        // writes it, and nobody needs the first step that moved.
        if (q.NP > 0) {
            if (rowcount_reset(c)) return BLANCE_ERR_DEVICE;
            launch_flat_prepare_count_live(sm, fq, c->f_tot.as<int32_t>(), c->f_g.as<double>(), c->f_top_g.as<double>(),
                                           c->f_top_n.as<int32_t>(), fc.d, c->f_row_count.as<int32_t>());
            if (c->trace) fprintf(stderr, "[blance] flat pass state %d: the row count rides on k_flat_prepare's launch\n", q.s);
        } else {
            prepare();
        }
        launch_flat_stay_live(sm, fq, fc.d, fc.order, c->state_stick.as<int32_t>(), c->state_has_stick.as<uint8_t>(),
                              scal + kScalFlags + kFlagTopMoved);
        if (c->trace) fprintf(stderr, "[blance] flat pass state %d: k_flat_stay_live leaves the verdict word, no k_flat_scan_min\n", q.s);
        // (kernel_launches is the driver's own tally, pinned mode by mode in tests/test_driver_decisions_emulated.py; the steps
        // folded away here and in the other shortcuts still count in it.  What runs on the stream is in profiles/.)
        *launches += q.NP > 0 ? 4 : 3;
        if (q.s == q.top_state) c->tops_moved = false;
        *nothing_to_apply = true;
        *batched += P;
        return 0;
    }
    if (fresh_cycle_whole(c, opening, q.NP, q.k, q.higher_mask)) {       // (q.rec has NOT been gathered)
        BLANCE_LAUNCH_NOSYNC(k_fresh_cycle_commit, cdiv(P > q.N ? P : q.N, 256), 256, 0, sm, fq, P, c->n_alive,
                             c->alive_ids.as<int32_t>(), c->alive_rank.as<int32_t>(), q.cnt);
        if (c->trace) fprintf(stderr, "[blance] flat pass state %d: a plan from nothing, the pass committed as a round robin without its records\n", q.s);
        *launches += 5;                            // (the tally of the path it replaces, see assume_stays above)
        *batched += P;
        *whole_known = true;
        return 0;
    }
    if (q.NP > 0 && !rows_counted) {                // only read by the stay test when NP > 0; (else: k_gather has counted)
        if (rowcount_reset(c)) return BLANCE_ERR_DEVICE;
        launch_flat_row_count(sm, fq, c->f_row_count.as<int32_t>());
        *launches += 1;
    }
    // bulk paths have fixed costs (a host round trip, a sort): short runs stay sequential
    const int kMinStayRun = c->chain_min_parts < 64 ? c->chain_min_parts : 64;
    const int kMinFreshRun = c->chain_min_parts < 512 ? c->chain_min_parts : 512;
    int pos = 0, seq_batch = 256;
    bool dirty = true;
    while (pos < P) {
        c->bits_stale = true;                       // (conservative: a bulk commit may have run since the last k_pass_queue)
        int32_t got[2] = {0, 0};
        // A plan from nothing: the partitions to assign hold no node and have no weights of their own -- no step of the
        // opening pass is a stay (k_flat_scan: a stay keeps the ONE node the partition holds) and every step is fresh and
        // identical to the first (weight 1, nothing held anywhere): the scan's answer without the scan.
        const bool known_run = opening && pos == 0 && c->assign_empty && c->h.partition_weights_nil && c->speculate > 0;
        if (known_run) {
            got[0] = 0; got[1] = P;
        } else {
            if (dirty) {
                prepare();
                dirty = false;
                *launches += 1;
            }
            fq.scan_waves = flat_scan_waves(pos, P);
            if (c->scan_part.reserve(sizeof(int32_t) * 2 * ((size_t)fq.scan_waves + 1))) return fail(BLANCE_ERR_DEVICE, "hipMalloc failed");
            fq.scan_part = c->scan_part.as<int32_t>();
            launch_flat_scan(sm, fq, pos, P);
            launch_flat_scan_min(sm, fq.scan_waves, fq.scan_part, scan_words, nullptr, P);
            HIPTRY(read_back(c, got, scan_words, sizeof got));
            HIPTRY(stream_sync(c));
            *launches += 1;
        }
        int first_nonstay = got[0] > P ? P : got[0], first_nonfresh = got[1] > P ? P : got[1];
        if (first_nonstay - pos >= kMinStayRun || (first_nonstay == P && first_nonstay > pos)) {
            const bool whole = pos == 0 && first_nonstay == P;      // the pass is one run of stays: no one reads the matrix
            if (whole && q.s == q.top_state && q.k == 1) c->tops_moved = false;      // (k > 1: a stay may still reorder the list, plan.go:126-138 reads its first node)
            if (q.NP > 0 && !whole) NTNTRY();
            // One run of certain stays with ONE node each, as the first pass of a sweep >= 2 (`settled`: every present list is a
            // non-nil slice, plan.go:418): applying it (plan.go:290-299) changes nothing -- the partition keeps the node it holds,
            // which is in no other list of the partition (k_flat_scan's test), so no list is filtered and no kind changes.
            // Neither the outputs nor k_scatter are needed then.
            if (whole && q.k == 1 && settled) {
                *nothing_to_apply = true;
                *batched += P;
                break;
            }
            launch_flat_commit_stay(sm, fq, pos, first_nonstay, whole ? 0 : 1);
            *launches += 1;
            *batched += first_nonstay - pos;
            pos = first_nonstay;
            continue;
        }
        if (first_nonfresh - pos >= kMinFreshRun && c->n_alive > 0) {
            int R = first_nonfresh - pos;
            // NumPartitions == 0: steps may each exclude one node (k_fresh_excl); one more element of the
            // exclusion-free sequence is needed then
            // NumPartitions == 0: steps may exclude one node each and take two (k_fresh_excl); the exclusion-free
            // sequence then needs k elements per step and one more
            const bool excl = q.NP == 0 && (q.higher_mask != 0 || q.k == 2);
            const int RS = excl ? q.k * R + q.k : R;
            if (q.NP > 0) NTNTRY();                 // (the fresh run reads and bumps row "" of the matrix)
            int32_t *sorted_vals = nullptr, *other_vals = nullptr;
            // Integer keys (NumPartitions == 0, no node weights) from counters that all start at zero, step weight 1
            // (known_run): node n's elements are (0, n), (1, n), (2, n) ..; the RS smallest in (key, node) order are the A
            // nodes of nodesNext by id, again and again -- the sorted sequence and every node's share of it without
            // threshold search, emission and sort (the empty cluster's greedy plan is a round robin).
            if (known_run && fq.int_keys && c->counts_start_zero) {
                fresh_cycle_sorted(c, q.N, RS, &sorted_vals, &other_vals);
                *launches += 1;
            } else {
                if (dirty) {
                    prepare();
                    dirty = false;
                    *launches += 1;
                }
                const int e = fresh_run_sorted(c, fq, pos, RS, launches, &sorted_vals, &other_vals);
                if (e) return e;
            }
            const int32_t* picks = sorted_vals;
            if (excl) {
                int32_t bad = INT_MAX;
                const int e = fresh_excl_resolve(c, fq, pos, R, sorted_vals, other_vals, bad_word, &bad);
                if (e) return e;
                *launches += 1;
                if (bad < R) R = bad;               // a pending node came up again: the run ends before that step
                picks = other_vals;
                HIPTRY(hipMemsetAsync(c->f_m.p, 0, sizeof(int32_t) * ((size_t)q.N + 1), sm));
                if (R > 0) BLANCE_LAUNCH_NOSYNC(k_fresh_hist, cdiv((int64_t)q.k * R, 256), 256, 0, sm, q.k * R, picks, c->f_m.as<int32_t>());
            }
            if (R > 0) {
                BLANCE_LAUNCH_NOSYNC(k_fresh_commit_steps, cdiv(R, 256), 256, 0, sm, fq, pos, R, picks);
                BLANCE_LAUNCH_NOSYNC(k_fresh_commit_nodes, cdiv(q.N, 256), 256, 0, sm, fq, pos, c->f_m.as<int32_t>(), q.cnt);
                *launches += 4;
                *batched += R;
                if (known_run && R == P) *whole_known = true;
                pos += R;
                dirty = true;
                seq_batch = 256;
                continue;
            }
        }
        int B = P - pos < seq_batch ? P - pos : seq_batch;
        int e = flat_chain_prepare(c, fc, launches);
        if (e) return e;
        if (fc.ok) {                                  // small cluster: one wave64 walks the batch
            e = run_flat_chain(c, q, pos, pos + B, false, scal, launches);
            if (e < 0) return e;
        } else {
            q.beg = pos; q.end = pos + B;
            e = dispatch_pass(c, q);
            if (e) return e;
            *launches += 1;
        }
        pos += B;
        dirty = true;
        if (seq_batch < (1 << 20)) seq_batch *= 2;
    }
    return 0;
}

static bool dispatch_chain(blance_ctx* c, ChainParams& q, int max_size, const ChainHandoff& ho) {
    const bool fast = q.NP == 0 && !c->any_node_weight && !c->no_fast_keys;
    return launch_chain(c->stream, q, max_size, fast, ho);
}

// developer aid: BLANCE_DUMP_SWEEP=<i> prints every step's choice of sweep i (pass order)
static int dump_pass(blance_ctx* c, int sweep, int state, int P, int OW, const int32_t* idx_dev /* or null */) {
    if (c->dump_sweep != sweep) return 0;
    std::vector<int32_t> out((size_t)P * OW), idx((size_t)P);
    HIPTRY(hipMemcpyAsync(out.data(), c->out.p, sizeof(int32_t) * out.size(), hipMemcpyDeviceToHost, c->stream));
    if (idx_dev) HIPTRY(hipMemcpyAsync(idx.data(), idx_dev, sizeof(int32_t) * P, hipMemcpyDeviceToHost, c->stream));
    HIPTRY(stream_sync(c));
    std::vector<int> at((size_t)P);
    for (int i = 0; i < P; i++) at[idx_dev ? idx[i] : i] = i;
    for (int oi = 0; oi < P; oi++) {
        const int32_t* o = &out[(size_t)at[oi] * OW];
        fprintf(stderr, "[dump] sweep %d state %d step %d:", sweep, state, oi);
        for (int j = 0; j < OW; j++) fprintf(stderr, " %d", o[j]);
        fprintf(stderr, "\n");
    }
    return 0;
}

// ---- collectives of a sharded plan ---------------------------------------------------------
#ifndef BLANCE_SIMT_EMU
#include <dlfcn.h>
struct Id128 { char b[128]; };                  // ncclUniqueId, passed by value
namespace {
// RCCL is bound at run time (dlopen): a single-GPU caller never loads it.  The two enum values
// this file passes are part of NCCL's stable ABI (nccl.h: ncclDataType_t, ncclRedOp_t).
constexpr int kNcclInt32 = 2;                   // ncclInt32 == ncclInt
constexpr int kNcclSum = 0;                     // ncclSum
struct Rccl {
    void* lib = nullptr;
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, Id128, int) = nullptr;
    int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*CommAbort)(void*) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};
}
static Rccl g_rccl;
static std::mutex g_rccl_mu;
static int rccl_load() {
    std::lock_guard<std::mutex> g(g_rccl_mu);
    if (g_rccl.lib) return 0;
    void* lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) lib = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) return fail(BLANCE_ERR_COMM, "librccl.so not found: %s", dlerror());
    g_rccl.GetUniqueId = (decltype(g_rccl.GetUniqueId))dlsym(lib, "ncclGetUniqueId");
    g_rccl.CommInitRank = (decltype(g_rccl.CommInitRank))dlsym(lib, "ncclCommInitRank");
    g_rccl.AllReduce = (decltype(g_rccl.AllReduce))dlsym(lib, "ncclAllReduce");
    g_rccl.AllGather = (decltype(g_rccl.AllGather))dlsym(lib, "ncclAllGather");
    g_rccl.CommDestroy = (decltype(g_rccl.CommDestroy))dlsym(lib, "ncclCommDestroy");
    g_rccl.CommAbort = (decltype(g_rccl.CommAbort))dlsym(lib, "ncclCommAbort");
    g_rccl.GetErrorString = (decltype(g_rccl.GetErrorString))dlsym(lib, "ncclGetErrorString");
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllReduce || !g_rccl.AllGather || !g_rccl.CommDestroy)
        return fail(BLANCE_ERR_COMM, "librccl.so lacks an entry point");
    g_rccl.lib = lib;
    return 0;
}
#endif

extern "C" int blance_is_emulated(void) {
#ifdef BLANCE_SIMT_EMU
    return 1;
#else
    return 0;
#endif
}

extern "C" int blance_comm_unique_id(void* id_out_128) {
#ifndef BLANCE_SIMT_EMU
    if (!id_out_128) return fail(BLANCE_ERR_BAD_ARG, "null id buffer");
    int st = rccl_load();
    if (st) return st;
    int e = g_rccl.GetUniqueId(id_out_128);
    if (e) return fail(BLANCE_ERR_COMM, "ncclGetUniqueId: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(e) : "?");
    return BLANCE_OK;
#else
    (void)id_out_128;
    return fail(BLANCE_ERR_COMM, "no RCCL in the emulator build");
#endif
}

extern "C" int blance_comm_init_rccl(blance_ctx* c, int32_t n_ranks, int32_t rank, const void* id_128) {
    return guarded([&]() -> int {
#ifndef BLANCE_SIMT_EMU
    if (!c || !id_128 || n_ranks < 1 || rank < 0 || rank >= n_ranks) return fail(BLANCE_ERR_BAD_ARG, "bad communicator arguments");
    std::lock_guard<std::mutex> g(c->mu);
    int st = rccl_load();
    if (st) return st;
    HIPTRY(hipSetDevice(c->device));
    if (c->rccl_comm) { g_rccl.CommDestroy(c->rccl_comm); c->rccl_comm = nullptr; }
    Id128 id;
    memcpy(id.b, id_128, sizeof id.b);
    void* comm = nullptr;
    int e = g_rccl.CommInitRank(&comm, n_ranks, id, rank);
    if (e) return fail(BLANCE_ERR_COMM, "ncclCommInitRank: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(e) : "?");
    c->rccl_comm = comm;
    c->comm = blance_comm{rank, n_ranks, nullptr, nullptr, nullptr};
    return BLANCE_OK;
#else
    (void)c; (void)n_ranks; (void)rank; (void)id_128;
    return fail(BLANCE_ERR_COMM, "no RCCL in the emulator build");
#endif
    });
}

extern "C" int blance_comm_set(blance_ctx* c, const blance_comm* comm) {
    return guarded([&]() -> int {
    if (!c) return fail(BLANCE_ERR_BAD_ARG, "null ctx");
    std::lock_guard<std::mutex> g(c->mu);
    if (!comm) { c->comm = blance_comm{0, 1, nullptr, nullptr, nullptr}; return BLANCE_OK; }
    if (comm->n_ranks < 1 || comm->rank < 0 || comm->rank >= comm->n_ranks || (comm->n_ranks > 1 && !comm->allreduce_sum_i32))
        return fail(BLANCE_ERR_BAD_ARG, "bad communicator");
    c->comm = *comm;
    return BLANCE_OK;
    });
}

extern "C" int blance_comm_stats(blance_ctx* c, int64_t* calls, int64_t* words) {
    return enter(c, [&]() -> int {
        if (calls) *calls = c->comm_calls;
        if (words) *words = c->comm_bytes / 4;
        return BLANCE_OK;
    });
}

extern "C" int blance_comm_time_ms(blance_ctx* c, double* ms) {
    return enter(c, [&]() -> int {
        if (!ms) return fail(BLANCE_ERR_BAD_ARG, "null argument");
        *ms = c->comm_ms;
        return BLANCE_OK;
    });
}

static void comm_release(blance_ctx* c) {
#ifndef BLANCE_SIMT_EMU
    if (c->rccl_comm && g_rccl.CommDestroy) g_rccl.CommDestroy(c->rccl_comm);
#endif
    c->rccl_comm = nullptr;
}

// a sharded call failed on this rank after the others may have entered a collective: RCCL
// communicators are aborted so that no rank waits forever (the communicator is invalid afterwards)
static void comm_abort(blance_ctx* c) {
#ifndef BLANCE_SIMT_EMU
    if (c->rccl_comm && g_rccl.CommAbort) { g_rccl.CommAbort(c->rccl_comm); c->rccl_comm = nullptr; }
#endif
    (void)c;
}

// the device time a collective takes on the planner's stream: an event on either side (summed up when the plan ends)
static int comm_mark(blance_ctx* c) {
    if (c->comm_events_used == c->comm_events.size()) {
        hipEvent_t ev;
        HIPTRY(hipEventCreate(&ev));
        c->comm_events.push_back(ev);
    }
    HIPTRY(hipEventRecord(c->comm_events[c->comm_events_used++], c->stream));
    return 0;
}
static void comm_sum_up(blance_ctx* c) {            // (after the stream has been synchronised)
    for (size_t i = 0; i + 1 < c->comm_events_used; i += 2) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, c->comm_events[i], c->comm_events[i + 1]) == hipSuccess) c->comm_ms += ms;
        else (void)hipGetLastError();
    }
    c->comm_events_used = 0;
}

// in-place int32 sum over the ranks, ordered with the kernels of the planner's stream
static int comm_allreduce(blance_ctx* c, int32_t* buf, int64_t n) {
    if (!comm_active(c) || n <= 0) return 0;
    c->comm_calls++;
    c->comm_bytes += n * 4;
    if (c->comm.allreduce_sum_i32) {
        HIPTRY(stream_sync(c));
        if (c->comm.allreduce_sum_i32(c->comm.user, buf, n)) return fail(BLANCE_ERR_COMM, "the caller's all-reduce failed");
        return 0;
    }
#ifndef BLANCE_SIMT_EMU
    if (!c->rccl_comm) return fail(BLANCE_ERR_COMM, "no communicator");
    if (comm_mark(c)) return BLANCE_ERR_DEVICE;
    int e = g_rccl.AllReduce(buf, buf, (size_t)n, kNcclInt32, kNcclSum, c->rccl_comm, c->stream);
    if (e) return fail(BLANCE_ERR_COMM, "ncclAllReduce: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(e) : "?");
    if (comm_mark(c)) return BLANCE_ERR_DEVICE;
    return 0;
#else
    return fail(BLANCE_ERR_COMM, "no communicator");
#endif
}

// in-place all-gather of n_ranks blocks of `per_rank` int32 values (this rank's block filled in)
static int comm_allgather(blance_ctx* c, int32_t* buf, int64_t per_rank) {
    if (!comm_active(c) || per_rank <= 0) return 0;
    c->comm_calls++;
    c->comm_bytes += per_rank * 4 * c->comm.n_ranks;
    if (c->comm.allreduce_sum_i32) {
        HIPTRY(stream_sync(c));
        if (!c->comm.allgather_i32) return fail(BLANCE_ERR_COMM, "no all-gather hook");
        if (c->comm.allgather_i32(c->comm.user, buf, per_rank)) return fail(BLANCE_ERR_COMM, "the caller's all-gather failed");
        return 0;
    }
#ifndef BLANCE_SIMT_EMU
    if (!c->rccl_comm) return fail(BLANCE_ERR_COMM, "no communicator");
    if (comm_mark(c)) return BLANCE_ERR_DEVICE;
    int e = g_rccl.AllGather(buf + (size_t)c->comm.rank * per_rank, buf, (size_t)per_rank, kNcclInt32, c->rccl_comm, c->stream);
    if (e) return fail(BLANCE_ERR_COMM, "ncclAllGather: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(e) : "?");
    if (comm_mark(c)) return BLANCE_ERR_DEVICE;
    return 0;
#else
    return fail(BLANCE_ERR_COMM, "no communicator");
#endif
}
#define COMMTRY(expr) do { int e__ = (expr); if (e__) return e__; } while (0)

static DevProblem dev_problem(blance_ctx* c);
// The planned map, for the readers after a plan: prevMap as the last sweep wrote it back (k_converge / k_sweep_tail).  It is
// the live lists as planned, but for their kinds: k_sweep_tail has already made the live ones the next sweep's (plan.go:418).
static DevProblem result_problem(blance_ctx* c) {
    DevProblem d = dev_problem(c);
    d.live = d.prv; d.live_len = d.prv_len; d.live_kind = d.prv_kind;
    return d;
}

static DevProblem dev_problem(blance_ctx* c) {
    const blance_problem& h = c->h;
    DevProblem d;
    d.N = h.n_nodes; d.NX = h.n_nodes_ext; d.M = h.n_states; d.L = c->L; d.P = h.n_parts;
    d.weights_nil = h.partition_weights_nil;
    d.node_removed = c->zeros_nx.as<uint8_t>();
    d.node_added = c->zeros_nx.as<uint8_t>();
    d.part_weight = c->part_weight.as<int32_t>();
    d.part_has_weight = c->part_has_weight.as<uint8_t>();
    d.live = c->live.as<int32_t>(); d.live_len = c->live_len.as<int32_t>(); d.live_kind = c->live_kind.as<uint8_t>();
    d.prv = c->prv.as<int32_t>(); d.prv_len = c->prv_len.as<int32_t>(); d.prv_kind = c->prv_kind.as<uint8_t>();
    d.in_prev = c->in_prev.as<uint8_t>(); d.never_equal = c->never_equal.as<uint8_t>();
    return d;
}

// ---- one state pass as region chains ----------------------------------------
// Header of the buffer the ranks of a sharded plan sum up after such a pass (collective A):
// [0 .. kChainFlags) the chain kernels' flags, [kXPoison] poison (a rank failed), then the load-vector change.
constexpr int kXHead = 16, kXPoison = kChainFlags;
// The sweep's last pass hands its list edits (k_scatter's arguments) to the sweep's tail, k_sweep_tail, instead of launching
// them: plan_locked launches the tail after the pass.  scatter = false: the pass changed no list (run_flat_pass's
// nothing_to_apply).  inv: the inverse of `order` (k_sweep_tail goes by partition), or null -- then k_scatter runs first.
struct SweepTail {
    bool set = false, scatter = false;
    int m = 0, OW = 0;
    const int32_t* order = nullptr;
    const int32_t* inv = nullptr;
    Gate gate = kNoGate;
};
struct ChainPassArgs {
    int m, k, NP, higher_mask, r0, it;
    const int32_t* order;          // the pass order: the stable partition of sweep 1, the static order itself afterwards
    bool same_tops;                // no partition has changed its top priority node since this state's last chain pass
    SweepTail* tail;               // non-null: the sweep's last pass, its k_scatter goes to the sweep's tail
    bool known_cycle = false;      // the pass behind a round robin: its periodic form knows its period (run_state_pass)
    bool round_robin = false;      // ... the same, whether or not the period is taken from it: step j of `order` has top
                                   // priority node alive_ids[j % n_alive] (the grouping from the upload's tables, k_cycle.h)
};

// this rank failed before collective A of a sharded chain pass: take part in it with the poison word set
static void comm_poison(blance_ctx* c) {
    const blance_problem& h = c->h;
    const size_t n = kXHead + (size_t)(h.n_states + 1) * h.n_nodes_ext;
    if (c->xbuf.reserve(sizeof(int32_t) * (n + 1))) return;
    if (hipMemsetAsync(c->xbuf.p, 0, sizeof(int32_t) * n, c->stream) != hipSuccess) return;
    const int32_t one = 1;
    if (hipMemcpyAsync(c->xbuf.as<int32_t>() + kXPoison, &one, sizeof one, hipMemcpyHostToDevice, c->stream) != hipSuccess) return;
    if (stream_sync(c) != hipSuccess) return;
    (void)comm_allreduce(c, c->xbuf.as<int32_t>(), (int64_t)n);
    (void)stream_sync(c);
}

// What a plan has done so far.  Saved by value where a sweep or a pass may have to run again, and put back then.
struct Progress {
    int64_t steps = 0, batched = 0;
    int n_pass = 0;                // passes timed so far (pass_events, pass_kind)
    int passes_this_sweep = 0;
};
// One plan, from plan_locked's first line to its last.
struct PlanRun {
    DevProblem d;
    int64_t launches = 0;
    Progress at;
    int32_t hs[kScalReadback] = {0};   // the scalar words read back after every sweep
    int m_last = -1;               // the last state a sweep makes a pass for
    // Each sweep ends with k_sweep_tail (the last pass's list edits, the convergence test and write-back, and the next
    // sweep's counters and kinds) -- not on a sharded plan, whose ranks scatter the pass's gathered outputs one by one.
    bool fuse = false;
    bool top_spec_plan = true;     // (no sweep of this plan has refuted it: see Sweep::top_spec_off)
    bool handoff_plan = true;      // (no chain pass of this plan has had its hand-off refuted: ChainPass::handoff)
    int iterations = 0, converged = 0;
};

// The host round trips a chain pass may save, and what it left open.
//   allow_spec: the classification of a pass that reuses its grouping is ASSUMED clean (no events, no orphans) instead of
//     read back; the words are checked with the pass's own flags, and `redo` says the assumption was wrong: nothing of the
//     pass stands, the caller runs it again without.
//   defer: the pass's own verdict (k_stay_by_top's, the all-blank kernel's, the chain kernel's flags) is not read here
//     either: the pass is taken to stand, k_scatter is enqueued behind a Gate on those words, and `pending` tells the
//     caller which words to look at with its next readback (the sweep's convergence word: one round trip for both).  A
//     verdict that comes back bad has changed nothing but the counters (cnt_save holds them): the caller runs the pass
//     again with no_stay / no_lean / skip set accordingly.
enum class Pending { kNone, kStayTop, kBlank, kChain };   // whose verdict is still on the device
struct ChainRun {
    bool allow_spec = true, defer = false, no_stay = false, no_lean = false, skip = false;
    bool no_handoff = false;       // the chain kernel walks every region to its end (a pass that runs again always does)
    bool handoff = false;          // the pass was launched with the hand-off: kFlagStayMoved is part of its verdict
    bool redo_handoff = false;     // (with redo: it was the hand-off that did not hold, not the classification)
    bool redo = false;
    Pending pending = Pending::kNone;
    bool spec = false;             // the classification was assumed
    Gate gate = kNoGate;
    bool done = false;             // the pass was made; if not (and no redo), the counters are as before and the caller
                                   // runs the pass in order
    bool a_done = false;           // collective A of a sharded pass has been entered
};

// One attempt at a chain pass: what its phases share.  Every phase returns 0 or an error; a phase that finds the attempt's
// assumptions refuted sets run.redo (run() then ends at once).
struct ChainPass {
    blance_ctx* const c;
    PlanRun& pr;
    const ChainPassArgs& a;
    ChainRun& run;
    const blance_problem& h;
    const DevProblem& d;
    blance_ctx::RuleRegions& rr;
    const int m, OW, P, B, nbc, G, rank;
    const bool sharded;
    const size_t cnt_words;
    const hipStream_t sm;
    int32_t* const flags;                    // the chain flags on the device
    Gate top_gate = kNoGate;
    bool regroup = false, spec = false, defer = false, gather_out = false;
    bool cycle = false;                      // the grouping by region comes from the upload's tables (k_cycle_group)
    int32_t cfl[kChainFlags] = {0};          // the classification's flags (all zero when they were assumed)
    int32_t n_events = 0;
    bool stay_fits = false, try_stay = false, group_stands = false, group_ahead = false;
    bool handoff = false;                    // k_pass_chain may hand a calm region's remaining steps to k_stay_by_top
    ChainParams cq;

    ChainPass(blance_ctx* c_, PlanRun& pr_, const ChainPassArgs& a_, ChainRun& run_)
        : c(c_), pr(pr_), a(a_), run(run_), h(c_->h), d(pr_.d), rr(c_->rule_regions[a_.r0]), m(a_.m), OW(1 + a_.k), P(c_->h.n_parts), B(rr.n_regions),
          nbc(cdiv(c_->h.n_parts, kPartChunk)), G(c_->comm.n_ranks), rank(c_->comm.rank), sharded(pass_sharded(c_, rr.n_regions)),
          cnt_words((size_t)(c_->h.n_states + 1) * c_->h.n_nodes_ext), sm(c_->stream),
          flags(c_->scalars.as<int32_t>() + kScalFlags) {}

    int slice_lo(int r) const { return (int)((int64_t)B * r / G); }   // a sharded plan: rank r walks regions [slice_lo(r), slice_lo(r + 1))
    Gate gate_on(uint32_t words) const {               // (the flag words a deferred verdict depends on)
        return Gate{flags, words | (1u << kFlagForced) | (spec ? (1u << kFlagOrphans) | (1u << kFlagEvents) : 0u) | c->top_gate};
    }
    // (speculate == 2, tests: every assumption is treated as refuted)
    bool refuted(const int32_t* f) const { return spec && (f[kFlagOrphans] || f[kFlagEvents] || c->speculate == 2); }
    void uncount_orphans() {                           // nodes of this state that lie in no region
        BLANCE_LAUNCH_NOSYNC(k_chain_orphans, cdiv(P, 256), 256, 0, sm, d, m, h.top_state, a.order,
                             rr.node_region.as<int32_t>(), c->cnt.as<int32_t>());
    }
    int restore_counters() {
        HIPTRY(hipMemcpyAsync(c->cnt.p, c->cnt_save.p, sizeof(int32_t) * cnt_words, hipMemcpyDeviceToDevice, sm));
        return 0;
    }
    int open_timing() { HIPTRY(hipEventRecord(c->pass_events[2 * pr.at.n_pass], sm)); return 0; }
    int close_timing(PassKind kind) {
        HIPTRY(hipEventRecord(c->pass_events[2 * pr.at.n_pass + 1], sm));
        c->pass_kind.resize(pr.at.n_pass + 1);
        c->pass_kind[pr.at.n_pass] = kind;
        pr.at.n_pass++;
        return 0;
    }

    int classify_and_group();
    int events();
    int gather_records();
    int group_by_top(hipStream_t st, DevBuf& sums);
    bool top_from_tables() const;
    int top_by_tables();
    void fill_chain_params();
    int start_counters();
    void fill_stay_params(StayParams& sq);
    int stay_attempt(bool* stayed);
    int stay_behind_handoff();
    int trace_handoff();
    int longest_chain() const {
        int mx = 0;
        if (c->h_reg_off.size() == (size_t)B + 1)
            for (int r = 0; r < B; r++) mx = std::max(mx, (int)(c->h_reg_off[r + 1] - c->h_reg_off[r]));
        return mx;
    }
    int blank_walk(bool* lean);
    int periodic_walk(bool* walked);
    int collective_a(int32_t* fl);
    int collective_b();
    int commit();
    int run_once();
};

// The pass's steps classified by the region of their top priority node and grouped by it; the classification's flags read
// back, or assumed.
int ChainPass::classify_and_group() {
    if (!c->flags_clean) HIPTRY(hipMemsetAsync(flags, 0, sizeof(int32_t) * kChainFlags, sm));
    c->flags_clean = false;
    // (c->top_gate: the sweep's first pass is taken to be one run of stays -- plan_locked -- and every launch of this pass
    // waits for that verdict: closed, it returns at once)
    top_gate = Gate{flags, c->top_gate};
    // The steps grouped by the region of their top priority node (a stable counting sort of the pass order).  A sweep whose
    // top-state pass was one run of stays has moved no top priority node, and from sweep 2 on the pass order is the static
    // order: the grouping of this state's last chain pass -- chain_order, chain_oi, reg_off -- still stands (config 3's
    // third sweep: six launches less).
    regroup = !(a.same_tops && c->chain_group_state == m && c->chain_group_static && a.order == c->part_order.as<int32_t>() &&
                c->h_reg_off.size() == (size_t)B + 1);
    // A pass that reuses its grouping has nothing else to learn from the classification's round trip: with the top priority
    // nodes where they were, events and orphans come from this state's own nodes having left their partition's region since --
    // rare enough to assume there are none and to look at flags[kFlagOrphans], flags[kFlagEvents] only when the pass's own
    // flags come back.  Such a pass reads neither the region ids nor the event counts, and k_gather_chain, which walks the
    // same lists right behind, raises the two words itself (gather_chain_record's `classify`): no k_chain_classify.
    spec = run.allow_spec && !regroup && !sharded && c->speculate > 0;
    // The pass behind a round robin (run_state_pass): the region of step j's top priority node is that of alive_ids[j % A], and
    // the stable sort by it a closed form over the upload's tables -- k_cycle_group classifies, places every step and inverts
    // the order in one launch, and checks the premise step by step (kFlagNotLocal: the pass goes in order, run_once drops the
    // grouping).  The tallies count the launches it replaces.
    cycle = a.round_robin && regroup && !sharded && rr.cyc_ok && c->cycle_group > 0 && a.order != nullptr;
    if (cycle) {
        const LaunchShape cs = shape_chain_classify(P);
        BLANCE_LAUNCH_NOSYNC(k_cycle_group, cs.grid, cs.block, cs.lds, sm, d, m, h.top_state, a.order, rr.node_region.as<int32_t>(),
                             c->n_alive, B, c->alive_ids.as<int32_t>(), rr.cyc.as<int32_t>(), rr.cyc_reg_off.as<int32_t>(),
                             c->cycle_group == 2 ? 1 : 0, c->regid.as<int32_t>(), c->n_ev.as<int32_t>(),
                             c->chain_order.as<int32_t>(), c->chain_oi.as<int32_t>(), c->chain_inv.as<int32_t>(),
                             c->reg_off.as<int32_t>(), flags, top_gate);
        pr.launches++;
        c->chain_group_state = m;
        c->group_epoch++;
        c->chain_group_static = a.order == c->part_order.as<int32_t>();
        c->cycle_group_epoch = c->group_epoch;
        if (c->trace) fprintf(stderr, "[blance] chain pass state %d: the steps grouped by region from the round robin's tables, no sort\n", m);
    } else if (!spec) {
        const LaunchShape cs = shape_chain_classify(P);
        BLANCE_LAUNCH_NOSYNC(k_chain_classify, cs.grid, cs.block, cs.lds, sm, d, m, h.top_state,
                             a.order, rr.node_region.as<int32_t>(), c->regid.as<int32_t>(),
                             c->n_ev.as<int32_t>(), flags, top_gate);
    } else {
        if (c->trace) fprintf(stderr, "[blance] chain pass state %d: no k_chain_classify, k_gather_chain raises its flag words\n", m);
    }
    if (regroup && !cycle) {
        const int ge = group_by_key(c, sm, c->scan_sums, P, c->regid.as<int32_t>(), a.order, B, c->bucket_counts.as<int32_t>(),
                                    c->reg_off.as<int32_t>(), c->chain_order.as<int32_t>(), c->chain_oi.as<int32_t>());
        if (ge) return ge;
        BLANCE_LAUNCH_NOSYNC(k_invert, cdiv(P, 256), 256, 0, sm, P, c->chain_order.as<int32_t>(), c->chain_inv.as<int32_t>());
        pr.launches++;
        c->chain_group_state = m;
        c->group_epoch++;
        c->chain_group_static = a.order == c->part_order.as<int32_t>();
    } else if (!regroup && c->trace) fprintf(stderr, "[blance] chain pass state %d: the grouping by region of the last sweep stands\n", m);
    // events: how many?  (also: is every step region-local at all, are there orphan nodes); a sharded
    // plan reads the chain offsets in the same round trip (the slice sizes of collective B)
    defer = run.defer && !sharded && c->speculate > 0;
    if (c->top_gate && (regroup || !spec || !defer))               // (top_spec_fits rules these out)
        return fail(BLANCE_ERR_DEVICE, "a chain pass behind the top-state pass's verdict would read back");
    run.spec = spec;
    run.pending = Pending::kNone;
    run.redo = false;
    if (!spec) {
        HIPTRY(read_back(c, cfl, flags, sizeof cfl));
        if (cycle) {                                       // (the chain offsets are the upload's)
            c->h_reg_off = rr.h_cyc_reg_off;
        } else if (regroup) {                              // (always: the next sweep may reuse the grouping, the host's copy with it)
            c->h_reg_off.resize((size_t)B + 1);
            HIPTRY(read_back(c, c->h_reg_off.data(), c->reg_off.p, sizeof(int32_t) * ((size_t)B + 1)));
        }
        HIPTRY(stream_sync(c));
    }
    if (cycle && cfl[kFlagNotLocal]) {                     // the premise did not hold: chain_order is a permutation, not a grouping
        c->chain_group_state = -1;
        c->top_group_state = -1;
        c->cycle_group_epoch = -1;
        if (c->trace) fprintf(stderr, "[blance] chain pass state %d: the round robin's tables do not describe this pass, the grouping is dropped\n", m);
    }
    return 0;
}

// The pass's events (nodes a partition holds in this state outside its region) counted and grouped by the region that owns
// them; and the one launch every attempt starts with.
int ChainPass::events() {
    if (!cfl[kFlagNotLocal] && cfl[kFlagEvents]) {      // rare: nodes outside their partition's region
        SCANTRY(P + 1, c->n_ev.as<int32_t>());   // -> event slots
        HIPTRY(read_back(c, &n_events, c->n_ev.as<int32_t>() + P, sizeof n_events));
        HIPTRY(stream_sync(c));
    }
    if (c->trace)
        fprintf(stderr, spec ? "[blance] chain pass state %d: classification assumed clean (checked with the pass's flags)\n" :
                               "[blance] chain pass state %d: %d events, not-local %d, orphans %d\n", m, n_events, cfl[kFlagNotLocal], cfl[kFlagOrphans]);
    {   // one launch: no events yet, the counters this pass starts from (what a redo restores), k_stay_by_top's flag
        FillCopyJob fj;
        fj.zero(c->ev_off.p, (int64_t)B + 1);
        fj.zero(flags + kFlagStayMoved, 1);
        fj.zero(flags + kFlagHandedOff, 1);
        fj.copy(c->cnt_save.p, c->cnt.p, (int64_t)cnt_words);
        if (run_fill_copy(c, fj)) return BLANCE_ERR_DEVICE;
    }
    if (!cfl[kFlagNotLocal] && n_events > 0) {
        BLANCE_LAUNCH_NOSYNC(k_chain_ev_fill, cdiv(P, 256), 256, 0, sm, d, m, h.top_state, a.order,
                             rr.node_region.as<int32_t>(), rr.reg_lo.as<int32_t>(), c->node_leaf_pos.as<int32_t>(),
                             c->regid.as<int32_t>(), c->n_ev.as<int32_t>(), c->ev_key.as<int32_t>(),
                             c->ev_oi.as<int32_t>(), c->ev_leaf.as<int32_t>(), c->ev_w.as<int32_t>());
        const int ge = group_by_key(c, sm, c->scan_sums, n_events, c->ev_key.as<int32_t>(), nullptr, B, c->ev_counts.as<int32_t>(),
                                    c->ev_off.as<int32_t>(), c->ev_perm.as<int32_t>(), nullptr);
        if (ge) return ge;
        pr.launches += 5;
    }
    return 0;
}

// steps grouped by the leaf of their top priority node, pass order inside a group (stable counting sort)
int ChainPass::group_by_top(hipStream_t st, DevBuf& sums) {
    const int ge = group_by_key(c, st, sums, P, c->topkey.as<int32_t>(), nullptr, rr.n_leaves, c->top_counts.as<int32_t>(),
                                c->top_off.as<int32_t>(), c->top_order.as<int32_t>(), nullptr);
    if (ge) return ge;
    c->top_group_state = m;
    c->top_group_epoch = c->group_epoch;
    pr.launches += 5;
    return 0;
}

// k_stay_by_top's work list from the upload's tables (k_cycle_top) where group_by_top would sort for it: the grouping by region
// in force is the one k_cycle_group made.  On the planner's stream; counted as the five launches it replaces.
bool ChainPass::top_from_tables() const {
    return c->cycle_group > 0 && rr.cyc_ok && !sharded && c->chain_group_state == m && c->cycle_group_epoch == c->group_epoch &&
           !cfl[kFlagNotLocal];
}
int ChainPass::top_by_tables() {
    const int A = c->n_alive, wpa = std::max(1, cdiv(cdiv(P, A), 64));
    BLANCE_LAUNCH_NOSYNC(k_cycle_top, cdiv((int64_t)A * wpa, 4), 256, 0, sm, P, A, wpa, rr.n_leaves, rr.cyc.as<int32_t>(),
                         rr.cyc_reg_off.as<int32_t>(), rr.cyc_top_off.as<int32_t>(), c->top_off.as<int32_t>(),
                         c->top_order.as<int32_t>(), top_gate);
    c->top_group_state = m;
    c->top_group_epoch = c->group_epoch;
    pr.launches += 5;
    if (c->trace) fprintf(stderr, "[blance] chain pass state %d: the steps grouped by top priority node from the round robin's tables, no sort\n", m);
    return 0;
}

// The compact records of the pass in chain order (k_gather_chain); whether k_stay_by_top is worth a try, and its work list
// made on the second stream for the next sweep when it is not.
int ChainPass::gather_records() {
    // A pass of stays only (the last sweep of every plan that converges)?  Worth a try when the state's pass of the
    // sweep before was one but for a few steps: k_stay_by_top checks every step in parallel.
    const bool fits_but_np = !sharded && !c->no_stay_top && !cfl[kFlagNotLocal] && !cfl[kFlagOrphans] && !cfl[kFlagEvents] &&
                             rr.max_size <= kStayMaxLeaves && rr.n_stay_wgs > 0;
    stay_fits = fits_but_np && a.NP > 0;
    try_stay = stay_fits && !run.no_stay && (c->force_stay_top || c->last_stays[m] * 100 >= (int64_t)P * 99);
    // THE HAND-OFF.  A pass that walks its chains lets k_pass_chain stop in every region that has calmed
    // down and hands the rest to k_stay_by_top, launched right behind: when k_stay_by_top fits, nothing of the pass is being
    // run again, no hand-off of this plan has been refuted, the stay test's rows are in LDS (else no stay round is ever
    // tried) and some chain is long enough to have handoff_min steps left behind its first stage.
    const bool handoff_plan_ok = c->chain_handoff > 0 && pr.handoff_plan && c->speculate > 0 && !run.no_handoff && run.allow_spec &&
                                 longest_chain() - 64 * 4 >= c->chain_handoff;
    handoff = stay_fits && !try_stay && handoff_plan_ok && chain_rows_in_lds(cq, rr.max_size);
    // (... and a pass with NumPartitions == 0 -- a fresh plan's first sweep -- whose next sweep's pass will fit makes the work
    // list for it: that pass's chain kernel is too short to hide the grouping behind)
    const bool handoff_next = fits_but_np && a.NP == 0 && c->np_later > 0 && handoff_plan_ok && a.it + 1 < h.max_iterations;
    // k_stay_by_top's work list (the steps grouped by the leaf of their top priority node: four launches over all steps)
    // depends on the grouping by region and on the top priority nodes only.  One made for this state at the same count of
    // regroupings still holds; and a pass that does NOT try k_stay_by_top makes it for the next sweep's on the second
    // stream, beside its own chain kernel.
    group_stands = c->top_group_state == m && c->top_group_epoch == c->group_epoch;
    // (The second stream is made when it is first wanted, and only in a process of one or two planners: a stream is a
    // hardware queue, and with many contexts planning at once on one GPU -- bench.py's replicas: 16 contexts, 32 queues -- the
    // planners' own streams end up sharing queues and their long kernels run one after the other.)
    const bool for_next = stay_fits && !try_stay && c->speculate > 0 && a.it + 1 < h.max_iterations;
    group_ahead = (for_next || handoff || handoff_next) && !group_stands && (c->side || g_live_contexts.load() <= 2);
    // (the tables of the round robin give the list in one small launch on this stream: no second stream, no keys)
    const bool by_tables = top_from_tables();
    const bool list_by_tables = by_tables && (group_ahead || ((handoff || handoff_next) && !group_stands));
    if (by_tables) group_ahead = false;
    if (group_ahead && !c->side && hipStreamCreate(&c->side) != hipSuccess) { c->side = nullptr; group_ahead = false; (void)hipGetLastError(); }
    // (no second stream: a list the hand-off needs is made on this one, a list for the next sweep's k_stay_by_top alone is not)
    const bool group_here = (handoff || handoff_next) && !group_stands && !group_ahead && !by_tables;
    if (try_stay || group_ahead || handoff || group_here || list_by_tables) {
        RESERVE(topkey, sizeof(int32_t) * ((size_t)P + 1));
        RESERVE(top_order, sizeof(int32_t) * ((size_t)P + 1));
        RESERVE(top_off, sizeof(int32_t) * ((size_t)rr.n_leaves + 2));
        RESERVE(top_counts, sizeof(int32_t) * ((size_t)rr.n_leaves * nbc + 1));
        if (c->side_pending) {                         // (what the second stream reads and writes is about to be used here)
            HIPTRY(hipStreamWaitEvent(sm, c->side_done, 0));
            c->side_pending = false;
        }
    }
    const bool group_now = (try_stay && !group_stands && !by_tables) || group_ahead || group_here;
    const LaunchShape gs = shape_gather_chain(P);
    BLANCE_LAUNCH(k_gather_chain, gs.grid, gs.block, gs.lds, sm, d, m, h.top_state, a.higher_mask,
                         c->chain_order.as<int32_t>(), c->chain_oi.as<int32_t>(), c->state_stick.as<int32_t>(),
                         c->state_has_stick.as<uint8_t>(), c->node_leaf_pos.as<int32_t>(),
                         rr.node_region.as<int32_t>(), rr.reg_lo.as<int32_t>(), rr.leaf_cls.as<int32_t>(),
                         rr.cls_size.as<int32_t>(), 0, spec ? 1 : 0,
                         c->crec.as<int32_t>(), flags, group_now ? c->topkey.as<int32_t>() : (int32_t*)nullptr, top_gate);
    if (group_ahead) {
        HIPTRY(hipEventRecord(c->side_go, sm));        // (the keys are written)
        HIPTRY(hipStreamWaitEvent(c->side, c->side_go, 0));
        const int ge = group_by_top(c->side, c->side_sums);
        if (ge) return ge;
        HIPTRY(hipEventRecord(c->side_done, c->side));
        c->side_pending = true;
        if (c->trace) fprintf(stderr, "[blance] chain pass state %d: the steps grouped by top priority node for the next sweep, on the second stream\n", m);
    } else if (group_here) {
        const int ge = group_by_top(sm, c->scan_sums);
        if (ge) return ge;
        if (c->trace) fprintf(stderr, "[blance] chain pass state %d: the steps grouped by top priority node for the hand-off\n", m);
    } else if (list_by_tables) {
        const int ge = top_by_tables();
        if (ge) return ge;
    }
    return 0;
}

void ChainPass::fill_chain_params() {
    fill_pass_common(c, cq, m, a.k, a.NP);
    fill_region_tables(c, rr, cq);
    cq.L = c->L;
    cq.n_regions = B;
    // (a plan's first sweep is where the moves are: a stay round of 512 steps that commits a short prefix costs more than one of
    // 256 -- the last wave looks its node up in seven tables; the rebalance of config 3 after a tenth of the nodes left: 59.5
    // against 56.7 ms for that pass.  Eight waves from the second sweep on, when the LDS is there.)
    cq.waves = c->chain_waves ? c->chain_waves : (a.it == 0 ? 4 : 0);
    cq.cls_run = rr.cls_run;
    // a sharded plan: this rank walks the chains of its slice of the regions
    cq.region_base = sharded ? slice_lo(rank) : 0;
    cq.n_launch = sharded ? slice_lo(rank + 1) - cq.region_base : B;
    cq.reg_off = c->reg_off.as<int32_t>();
    cq.ntn = c->ntn.as<int32_t>();
    cq.crec = c->crec.as<int32_t>(); cq.out = c->out.as<int32_t>();
    cq.flags = flags;
    cq.gate = c->top_gate;
    cq.ev_off = c->ev_off.as<int32_t>(); cq.ev_perm = c->ev_perm.as<int32_t>();
    cq.ev_oi = c->ev_oi.as<int32_t>(); cq.ev_leaf = c->ev_leaf.as<int32_t>(); cq.ev_w = c->ev_w.as<int32_t>();
    cq.cnt_out = cq.cnt;
}

// the counters every walk of this pass starts from: the orphans' loads gone, and a sharded plan's copy of them
int ChainPass::start_counters() {
    if (cfl[kFlagOrphans]) uncount_orphans();
    gather_out = sharded && (c->comm.allgather_i32 || !c->comm.allreduce_sum_i32);
    if (sharded) {                                     // the loads every rank starts this pass from (orphans included)
        RESERVE(cnt_base, sizeof(int32_t) * (cnt_words + 1));
        RESERVE(xbuf, sizeof(int32_t) * (kXHead + cnt_words + 1));
        HIPTRY(hipMemcpyAsync(c->cnt_base.p, c->cnt.p, sizeof(int32_t) * cnt_words, hipMemcpyDeviceToDevice, sm));
        if (!gather_out) HIPTRY(hipMemsetAsync(c->out.p, 0, sizeof(int32_t) * (size_t)P * OW, sm));
    }
    return 0;
}

void ChainPass::fill_stay_params(StayParams& sq) {
    fill_pass_common(c, sq, m, a.k, a.NP);
    fill_region_tables(c, rr, sq);
    sq.wg_region = rr.wg_region.as<int32_t>(); sq.wg_chunk = rr.wg_chunk.as<int32_t>();
    sq.crec = c->crec.as<int32_t>();
    sq.top_off = c->top_off.as<int32_t>(); sq.top_order = c->top_order.as<int32_t>();
    sq.out = c->out.as<int32_t>(); sq.flag = flags + kFlagStayMoved;
    sq.gate = top_gate;
}

// k_stay_by_top behind a chain kernel that handed off: every region from the step its walk stopped at.  The launch waits
// for the chain kernel's own words as well: a chain that escaped has left its outputs unwritten, and the pass does not stand.
int ChainPass::stay_behind_handoff() {
    if (c->side_pending) {                             // (the work list made beside the chain kernel)
        HIPTRY(hipStreamWaitEvent(sm, c->side_done, 0));
        c->side_pending = false;
    }
    StayParams sq;
    fill_stay_params(sq);
    sq.gate.mask |= (1u << kFlagNotLocal) | (1u << kFlagEscaped);
    sq.from = c->handoff.as<int32_t>();
    sq.node_leaf_pos = c->node_leaf_pos.as<int32_t>();
    int e;
    if ((e = open_timing())) return e;
    if (!launch_stay_by_top(sm, sq, rr.n_stay_wgs, rr.max_size)) return fail(BLANCE_ERR_UNSUPPORTED, "k_stay_by_top shape behind a hand-off");
    pr.launches += 1;
    return close_timing(kPassStayTop);
}

// BLANCE_TRACE: where every region's walk stopped
int ChainPass::trace_handoff() {
    std::vector<int32_t> at((size_t)B), ro((size_t)B + 1);
    HIPTRY(hipMemcpyAsync(at.data(), c->handoff.p, sizeof(int32_t) * at.size(), hipMemcpyDeviceToHost, sm));
    HIPTRY(hipMemcpyAsync(ro.data(), c->reg_off.p, sizeof(int32_t) * ro.size(), hipMemcpyDeviceToHost, sm));
    HIPTRY(stream_sync(c));
    std::string line;
    int n = 0;
    if (B > 0 && at[0] < 0) {
        fprintf(stderr, "[blance] chain pass state %d: hand-off (%d steps or more): the launch returned at its gate, no region walked\n", m, c->chain_handoff);
        return 0;
    }
    for (int r = 0; r < B; r++) {
        char buf[96];
        if (at[r] >= ro[r] && at[r] < ro[r + 1]) {
            snprintf(buf, sizeof buf, " region %d at step %d of %d;", r, at[r] - ro[r], ro[r + 1] - ro[r]);
            n++;
        } else {
            snprintf(buf, sizeof buf, " region %d walked to its end (%d);", r, ro[r + 1] - ro[r]);
        }
        line += buf;
    }
    fprintf(stderr, "[blance] chain pass state %d: hand-off (%d steps or more) in %d of %d regions:%s\n", m, c->chain_handoff, n, B, line.c_str());
    return 0;
}

// k_stay_by_top: every step of the pass checked as a stay, one thread per top priority node.  *stayed: the pass is done
// (or, its verdict deferred, taken to be).
int ChainPass::stay_attempt(bool* stayed) {
    *stayed = false;
    if (!group_stands) {
        const int ge = top_from_tables() ? top_by_tables() : group_by_top(sm, c->scan_sums);
        if (ge) return ge;
    } else if (c->trace) fprintf(stderr, "[blance] chain pass state %d: the steps' grouping by top priority node stands\n", m);
    StayParams sq;
    fill_stay_params(sq);
    if (!launch_stay_by_top(sm, sq, rr.n_stay_wgs, rr.max_size)) return 0;
    pr.launches += 1;
    if (defer) {
        *stayed = true;                                 // (until the caller's readback says otherwise)
        run.pending = Pending::kStayTop;
        run.gate = gate_on((1u << kFlagNotLocal) | (1u << kFlagStayMoved));
        if (c->trace) fprintf(stderr, "[blance] chain pass state %d: stays per top priority node, the verdict is read with the sweep's\n", m);
        return 0;
    }
    int32_t sf[kChainFlags] = {0}, moved = 0;           // sf[kFlagNotLocal]: k_gather_chain's; moved: not all stays
    HIPTRY(read_back(c, sf, flags, sizeof sf));
    HIPTRY(read_back(c, &moved, flags + kFlagStayMoved, sizeof moved));
    HIPTRY(stream_sync(c));
    if (refuted(sf)) {                                  // (k_stay_by_top changes no counter)
        run.redo = true;
        return 0;
    }
    *stayed = !sf[kFlagNotLocal] && !moved;
    if (c->trace) fprintf(stderr, "[blance] chain pass state %d: stays verified per top priority node: %s\n", m, *stayed ? "all of them" : "no");
    return 0;
}

// k_period.h: regions whose records repeat are walked for two periods; the rest of the periodic stretch is copied, what
// lies behind it is walked -- all decided on the device, region by region.  *walked: the walk has been launched.
int ChainPass::periodic_walk(bool* walked) {
    const int N = h.n_nodes, NX = h.n_nodes_ext;
    *walked = false;
    int max_len = 0;
    for (int r = 0; r < B; r++) max_len = std::max(max_len, (int)(c->h_reg_off[r + 1] - c->h_reg_off[r]));
    if (max_len < kPeriodMinRounds * 2) return 0;
    RESERVE(period, sizeof(int32_t) * ((size_t)kPWords * B + 1));
    RESERVE(cnt_p1, sizeof(int32_t) * (cnt_words + 1));
    int32_t* pb = c->period.as<int32_t>();
    const int gx = cdiv(max_len, 256);
    // (a known cycle, run_state_pass: the period is the region's count of nodes of nodesNext and nothing breaks it -- one
    // trip over the region's leaves, no record read, no k_period_verify)
    const bool known = a.known_cycle;
    BLANCE_LAUNCH(k_period_find, B, known ? 256 : 1024, 64, sm, B, known ? 1 : 0, N, cq.reg_off, cq.reg_lo, cq.reg_hi, cq.leaf_node,
                  cq.alive, cq.crec, pb);
    if (!known) {
        const int gv = cdiv((long long)max_len * (kCW / 4), 256);
        BLANCE_LAUNCH_NOSYNC(k_period_verify, gv * B, 256, 0, sm, B, gv, cq.reg_off, cq.crec, pb);
    } else if (c->trace) {
        fprintf(stderr, "[blance] chain pass state %d: the period taken from the round robin of the pass before, no search and no k_period_verify\n", m);
    }
    BLANCE_LAUNCH_NOSYNC(k_period_segments, cdiv(B, 64), 64, 0, sm, B, c->periodic_cut > 0 ? c->periodic_cut : 0, cq.reg_off, pb);
    ChainParams sq = cq;
    // (the plane automaton for regions of up to 128 leaves, the lane-minimum kernel for wider ones)
    auto walk = [&](int beg_row, int end_row) {
        sq.seg_beg = pb + (size_t)beg_row * B; sq.seg_end = pb + (size_t)end_row * B;
        if (c->no_planes || !launch_chain_planes(sm, sq, rr.max_size)) launch_chain_blank(sm, sq, rr.max_size);
    };
    walk(kPBeg1, kPEnd1);
    *walked = true;
    HIPTRY(hipMemcpyAsync(c->cnt_p1.p, c->cnt.p, sizeof(int32_t) * cnt_words, hipMemcpyDeviceToDevice, sm));
    walk(kPBeg2, kPEnd2);
    // (128 threads: a trip over the leaves of config 3's regions; wider regions take two)
    BLANCE_LAUNCH(k_period_judge, B, 128, 64, sm, B, m, N, NX, OW, cq.reg_off, cq.reg_lo, cq.reg_hi, cq.leaf_node, cq.alive,
                  cq.crec, cq.out, cq.flags, c->cnt_p1.as<int32_t>(), cq.cnt, pb);
    BLANCE_LAUNCH_NOSYNC(k_period_replicate, gx * B, 256, 0, sm, B, gx, OW, cq.reg_off, pb, cq.out);
    if (c->trace) fprintf(stderr, "[blance] chain pass state %d: periodic walk, the regions set up by k_period_find and judged by k_period_judge\n", m);
    walk(kPBeg3, kPEnd3);
    pr.launches += 11;
    if (c->trace) {
        std::vector<int32_t> hp((size_t)kPWords * B);
        HIPTRY(hipMemcpyAsync(hp.data(), pb, sizeof(int32_t) * hp.size(), hipMemcpyDeviceToHost, sm));
        HIPTRY(stream_sync(c));
        int64_t copied = 0; int n_ok = 0, n_refused = 0;     // refused: joined, then failed k_period_judge -- walked on behind 2T
        for (int r = 0; r < B; r++) {
            const int32_t T = hp[(size_t)kPT * B + r], limit = hp[(size_t)kPLimit * B + r];
            if (hp[(size_t)kPOk * B + r]) { n_ok++; copied += limit - 2 * T; }
            else if (T >= 1 && T <= kPeriodCap && (long long)limit >= (long long)kPeriodMinRounds * T) n_refused++;
        }
        fprintf(stderr, "[blance] chain pass state %d: periodic records in %d of %d regions (period %d in the first), %lld of %d steps copied, "
                        "%d joined and were refused\n", m, n_ok, B, hp[(size_t)kPT * B], (long long)copied, P, n_refused);
    }
    return 0;
}

// a fresh plan's first sweep: every step blank -> the lean kernel; it either does this rank's
// whole slice or changes nothing that is not restored below (a rank-local decision: the full
// kernel makes the same choices).  *lean: it did the pass (or, its verdict deferred, is taken to have).
int ChainPass::blank_walk(bool* lean) {
    *lean = false;
    if (!(a.NP == 0 && !run.no_lean && !c->any_node_weight && rr.max_size <= 256 && a.k <= 4 && !cfl[kFlagNotLocal])) return 0;
    bool walked = false;
    if (c->periodic && !sharded && n_events == 0 && !cfl[kFlagOrphans] && !cfl[kFlagEvents]) {
        const int pe = periodic_walk(&walked);
        if (pe) return pe;
    }
    if (!walked && (c->no_planes || !launch_chain_planes(sm, cq, rr.max_size))) launch_chain_blank(sm, cq, rr.max_size);
    int32_t fl[kChainFlags] = {0};
    pr.launches++;
    if (defer) {                                        // (taken to have done the pass until the caller's readback says otherwise)
        run.pending = Pending::kBlank;
        run.gate = gate_on((1u << kFlagNotLocal) | (1u << kFlagEscaped));
    } else {
        HIPTRY(read_back(c, fl, flags, sizeof fl));
        HIPTRY(stream_sync(c));
        if (refuted(fl)) {
            run.redo = true;
            return restore_counters();
        }
    }
    if (c->trace) fprintf(stderr, "[blance] chain pass state %d: all-blank kernel (%s) %s\n", m, c->no_planes ? "lanes" : "planes",
                          run.pending != Pending::kNone ? "launched, its flags are read with the sweep's" :
                          !fl[kFlagNotLocal] && !fl[kFlagEscaped] ? "did the pass" : "escaped");
    if (!fl[kFlagNotLocal] && !fl[kFlagEscaped]) {
        *lean = true;
    } else if (!fl[kFlagNotLocal]) {                    // not all blank: the full kernel, from the same state
        HIPTRY(hipMemcpyAsync(c->cnt.p, sharded ? c->cnt_base.p : c->cnt_save.p, sizeof(int32_t) * cnt_words,
                              hipMemcpyDeviceToDevice, sm));
        if (cfl[kFlagOrphans] && !sharded) uncount_orphans();
        HIPTRY(hipMemsetAsync(flags, 0, sizeof(int32_t) * (kFlagStayBatches + 1), sm));
    }
    return 0;
}

// collective A of a sharded pass: [flags | this rank's change of the load vector], summed over the ranks; fl: the header
int ChainPass::collective_a(int32_t* fl) {
    int32_t* xb = c->xbuf.as<int32_t>();
    HIPTRY(hipMemsetAsync(xb, 0, sizeof(int32_t) * kXHead, sm));
    HIPTRY(hipMemcpyAsync(xb, flags, sizeof(int32_t) * kChainFlags, hipMemcpyDeviceToDevice, sm));
    BLANCE_LAUNCH_NOSYNC(k_vec_sub, cdiv((int64_t)cnt_words, 256), 256, 0, sm, (int)cnt_words, c->cnt.as<int32_t>(),
                         c->cnt_base.as<int32_t>(), xb + kXHead);
    run.a_done = true;
    COMMTRY(comm_allreduce(c, xb, (int64_t)(kXHead + cnt_words)));
    HIPTRY(read_back(c, fl, xb, sizeof(int32_t) * kXHead));
    pr.launches++;
    return 0;
}

// A sharded pass that stands: every rank's chains wrote their own regions' loads and their own steps' outputs.  The loads
// are those of collective A; collective B brings the outputs together.
int ChainPass::collective_b() {
    int32_t* xb = c->xbuf.as<int32_t>();
    BLANCE_LAUNCH_NOSYNC(k_vec_add, cdiv((int64_t)cnt_words, 256), 256, 0, sm, (int)cnt_words, c->cnt_base.as<int32_t>(),
                         xb + kXHead, c->cnt.as<int32_t>());
    pr.launches++;
    if (!gather_out) {
        COMMTRY(comm_allreduce(c, c->out.as<int32_t>(), (int64_t)P * OW));
        return 0;
    }
    // a rank's steps are contiguous in chain order
    const int32_t* ro = c->h_reg_off.data();
    int64_t per = 0;
    for (int r = 0; r < G; r++) {
        const int64_t len = (int64_t)(ro[slice_lo(r + 1)] - ro[slice_lo(r)]) * OW;
        if (len > per) per = len;
    }
    if (per <= 0) return 0;
    RESERVE(gath, sizeof(int32_t) * ((size_t)per * G + 1));
    int32_t* gb = c->gath.as<int32_t>();
    const int64_t mine = (int64_t)(ro[slice_lo(rank + 1)] - ro[slice_lo(rank)]) * OW;
    if (mine > 0)
        HIPTRY(hipMemcpyAsync(gb + (size_t)rank * per, c->out.as<int32_t>() + (size_t)ro[slice_lo(rank)] * OW,
                              sizeof(int32_t) * (size_t)mine, hipMemcpyDeviceToDevice, sm));
    COMMTRY(comm_allgather(c, gb, per));
    for (int r = 0; r < G; r++) {
        const int64_t len = (int64_t)(ro[slice_lo(r + 1)] - ro[slice_lo(r)]) * OW;
        if (r != rank && len > 0)
            HIPTRY(hipMemcpyAsync(c->out.as<int32_t>() + (size_t)ro[slice_lo(r)] * OW, gb + (size_t)r * per,
                                  sizeof(int32_t) * (size_t)len, hipMemcpyDeviceToDevice, sm));
    }
    return 0;
}

// The pass stands (or is taken to): its list edits go to the sweep's tail or are launched, behind the pending verdict's gate.
int ChainPass::commit() {
    if (dump_pass(c, a.it, m, P, OW, c->chain_oi.as<int32_t>())) return BLANCE_ERR_DEVICE;
    const Gate gate = run.pending != Pending::kNone ? run.gate : kNoGate;
    if (a.tail) {
        *a.tail = SweepTail{true, true, m, OW, c->chain_order.as<int32_t>(), c->chain_inv.as<int32_t>(), gate};
    } else {
        BLANCE_LAUNCH_NOSYNC(k_scatter, shape_scatter(P).grid, shape_scatter(P).block, shape_scatter(P).lds, sm, d, m, OW, c->chain_order.as<int32_t>(), c->out.as<int32_t>(), gate);
        pr.launches++;
    }
    pr.at.batched += P;
    run.done = true;
    return 0;
}

// 0 = ok (run.done tells whether the pass was made; if not, the counters are as before and the caller
// runs the pass in order), < 0 = error.
int ChainPass::run_once() {
    int e;
    if ((e = classify_and_group()) || (e = events())) return e;
    fill_chain_params();
    if ((e = gather_records()) || (e = start_counters()) || (e = open_timing())) return e;
    if (try_stay) {
        bool stayed = false;
        if ((e = stay_attempt(&stayed)) || run.redo) return e;
        if (stayed) {
            if ((e = close_timing(kPassStayTop))) return e;
            c->last_stays[m] = P;
            return commit();
        }
    }
    bool lean = false;
    if ((e = blank_walk(&lean)) || run.redo) return e;
    if (!lean) {
        if (a.NP > 0 && !chain_rows_in_lds(cq, rr.max_size)) NTNTRY();      // (rows in LDS: the matrix in HBM is not touched)
        ChainHandoff ch{nullptr, 0};
        if (handoff) {
            RESERVE(handoff, sizeof(int32_t) * ((size_t)B + 1));
            // (the trace reads the stops back: a launch that returns at its gate writes none, and says so by these -1s)
            if (c->trace) HIPTRY(hipMemsetAsync(c->handoff.p, 0xff, sizeof(int32_t) * (size_t)B, sm));
            ch = ChainHandoff{c->handoff.as<int32_t>(), c->chain_handoff};
        }
        if (!dispatch_chain(c, cq, rr.max_size, ch)) return fail(BLANCE_ERR_UNSUPPORTED, "region chain shape");
    } else {
        handoff = false;
    }
    pr.launches += 8;
    if ((e = close_timing(lean ? kPassBlank : kPassKernel))) return e;
    if (handoff && (e = stay_behind_handoff())) return e;
    run.handoff = handoff;
    if (c->trace && !lean) {
        if (handoff) { if ((e = trace_handoff())) return e; }
        else if (c->chain_handoff > 0) fprintf(stderr, "[blance] chain pass state %d: no hand-off\n", m);
    }
    int32_t fl[kXHead] = {0}, ho[2] = {0, 0};        // ho: k_stay_by_top's "not all stays" behind a hand-off, the steps it verified
    if (sharded) {
        if ((e = collective_a(fl))) return e;
    } else if (!lean) {                              // (the all-blank kernel's flags were read above: all clear)
        if (defer) {
            run.pending = Pending::kChain;
            run.gate = gate_on((1u << kFlagNotLocal) | (1u << kFlagEscaped) | (handoff ? 1u << kFlagStayMoved : 0u));
        } else {
            HIPTRY(read_back(c, fl, flags, sizeof(int32_t) * kChainFlags));
            if (handoff) {
                HIPTRY(read_back(c, &ho[0], flags + kFlagStayMoved, sizeof(int32_t)));
                HIPTRY(read_back(c, &ho[1], flags + kFlagHandedOff, sizeof(int32_t)));
            }
        }
    }
    const bool pending = run.pending != Pending::kNone;
    if (!pending && (sharded || !lean)) HIPTRY(stream_sync(c));
    if (fl[kXPoison]) return fail(BLANCE_ERR_COMM, "another rank of the sharded plan failed");
    // (a hand-off whose rest was not all stays: nothing of the pass stands, it runs again with every region walked to its end)
    const bool handoff_refuted = !pending && handoff && !fl[kFlagNotLocal] && !fl[kFlagEscaped] && (ho[0] || c->speculate == 2);
    if (!pending && !lean && (refuted(fl) || handoff_refuted)) {          // (the all-blank kernel's words were checked above)
        c->pass_ntn_ready = false;
        pr.at.n_pass -= handoff ? 2 : 1;
        if (handoff_refuted && !refuted(fl)) {
            pr.handoff_plan = false;
            run.redo_handoff = true;
        }
        run.redo = true;
        return restore_counters();
    }
    if (c->trace && !pending)
        fprintf(stderr, "[blance] chain pass state %d: %d of %d steps committed as verified stays in %d batches\n",
                m, fl[kFlagStaySteps], P, fl[kFlagStayBatches]);
    const bool stands = !fl[kFlagNotLocal] && !fl[kFlagEscaped];
    c->last_stays[m] = stands ? (int64_t)fl[kFlagStaySteps] + ho[1] : 0;   // (a pending verdict: the caller fills this in)
    if (!stands) {                                  // not region-local after all: redo in order
        c->pass_ntn_ready = false;                  // (chains of big regions keep their rows in global memory: zeroed again on demand)
        return restore_counters();
    }
    if (sharded && (e = collective_b())) return e;
    return commit();
}

static int run_chain_pass(blance_ctx* c, PlanRun& pr, const ChainPassArgs& a, ChainRun& run) {
    int e = ChainPass(c, pr, a, run).run_once();
    if (e || !run.redo) return e;
    if (c->trace)
        fprintf(stderr, run.redo_handoff ? "[blance] chain pass state %d: a step behind the hand-off moved, the pass runs again without\n" :
                                           "[blance] chain pass state %d: the assumed classification did not hold, the pass runs again\n", a.m);
    if (!run.redo_handoff) run.allow_spec = false;
    run.no_handoff = true;
    run.defer = false;
    return ChainPass(c, pr, a, run).run_once();
}

// One sweep of the plan (plan.go:32's loop body), and what its retries need.
struct Sweep {
    int it = 0;
    bool first = false;
    int NP = 0, add_nil = 0, any_removed = 0;
    bool opened = false;           // the last sweep's k_sweep_tail counted this sweep's prevMap into cnt_next and made every
                                   // present list a non-nil slice
    int known_passes = 0, known_state = -1, known_k = 0;        // run_flat_pass's `opening`
    bool known_broken = false;
    bool known_cycle = false;      // the known pass was committed as a round robin over nodesNext (fresh_cycle_whole)
    // The sweep's last pass, when it is a chain pass, leaves its verdict on the device (ChainRun::defer) and the words
    // come back with the convergence word: one round trip for both.  A bad verdict brings the sweep back for that
    // state alone (retry says how), with everything the pass enqueued behind its gate undone by never having run.
    int m_from = 0;
    ChainRun retry;
    bool retrying = false, counted = false;
    bool restore_counters = false;     // the pass that runs again starts from cnt_save
    // The sweep's first pass, when it is `settled` (run_state_pass), need not be read back either: its stay test leaves a word
    // on the device (kFlagTopMoved), everything behind it waits for that word, and the word comes back with the convergence
    // word.  Set, the whole sweep runs again from its first pass with that pass read back (top_spec_off).  This holds only
    // when every later pass of the sweep keeps its own verdict on the device as well (top_spec_fits), so that nothing of the
    // sweep is read before its one readback.
    bool top_spec_off = false;
    Progress at_open, at_last_pass;    // the plan's progress when the sweep / its last state's pass began
    std::vector<int64_t> last_stays_open;
    // of the current round of passes:
    ChainRun pend;                 // the last pass's deferred verdict
    SweepTail tail;
    bool tail_counts = false;      // (this round ended with a counting tail)
};

// run_chain_pass makes the pass of every state behind m0 from the grouping by region it made last sweep, assumes its
// classification and defers its verdict: no readback inside
static bool top_spec_fits(const blance_ctx* c, const PlanRun& pr, const Sweep& sw, int m0) {
    const blance_problem& h = c->h;
    if (sw.NP == 0 || !c->top_prio_strict || m0 != h.top_state) return false;
    for (int t = m0 + 1; t < h.n_states; t++) {
        const int kt = c->state_constraints[t];
        if (kt <= 0) continue;
        if (t != pr.m_last) return false;
        const int q0 = c->rule_off[t], q1 = c->rule_off[t + 1];
        if (c->engine == BLANCE_ENGINE_SEQUENTIAL || h.hierarchy_rules_nil || q1 - q0 != 1 || !c->rule_regions[q0].ok ||
            h.n_parts < c->chain_min_parts || kt > 4)
            return false;
        const int B = c->rule_regions[q0].n_regions;
        if (pass_sharded(c, B)) return false;
        if (c->chain_group_state != t || !c->chain_group_static || c->h_reg_off.size() != (size_t)B + 1) return false;
    }
    return true;
}

// The sweep's working state as plan.go:53-55, :94 set it up: the live lists, stateNodeCounts = countStateNodes(prevMap).
static int open_sweep(blance_ctx* c, PlanRun& pr, Sweep& sw) {
    const blance_problem& h = c->h;
    const int NX = h.n_nodes_ext, M = h.n_states;
    const int64_t PM = (int64_t)h.n_parts * M;
    hipStream_t sm = c->stream;
    int32_t* scal = c->scalars.as<int32_t>();
    DevProblem& d = pr.d;
    d.node_removed = sw.first ? c->node_removed.as<uint8_t>() : c->zeros_nx.as<uint8_t>();   // plan.go:53-55
    d.node_added = sw.first ? c->node_added.as<uint8_t>() : c->zeros_nx.as<uint8_t>();
    c->tops_moved = true;                                       // until this sweep's top-state pass turns out to be one run of stays
    sw.opened = c->tail_counted;
    c->tail_counted = false;
    if (sw.opened) std::swap(c->cnt, c->cnt_next);
    {   // one launch: warn_count / not_match, the chain flags, the settled pass's verdict word, stateNodeCounts (plan.go:94) unless counted already, the flat
        // passes' row counts, and the counters this sweep's tail counts the next sweep's into
        FillCopyJob fj;
        fj.zero(scal + kScalWarnCount, 2);
        fj.zero(scal + kScalFlags, kChainFlags);
        fj.zero(scal + kScalFlags + kFlagTopMoved, 1);      // (k_flat_stay_live only ever stores a 1 there)
        if (!sw.opened) fj.zero(c->cnt.p, (int64_t)(M + 1) * (NX + 1));
        if (sw.NP > 0 && c->f_row_count.p) fj.zero(c->f_row_count.p, (int64_t)NX + 1);
        if (pr.fuse) fj.zero(c->cnt_next.p, (int64_t)(M + 1) * (NX + 1));
        if (run_fill_copy(c, fj)) return BLANCE_ERR_DEVICE;
        c->flags_clean = true;
        c->rowcount_clean = sw.NP > 0 && c->f_row_count.p;
    }
    if (PM > 0 && !sw.opened) {
        if (sw.first)
            BLANCE_LAUNCH_NOSYNC(k_live_init, cdiv(PM, 256), 256, 0, sm, d, c->a_off.as<int32_t>(),
                                 c->a_nodes.as<int32_t>(), c->a_kind.as<uint8_t>(), c->p_off.as<int32_t>(),
                                 c->p_nodes.as<int32_t>(), c->p_kind.as<uint8_t>());
        else
            BLANCE_LAUNCH_NOSYNC(k_live_refresh, cdiv(PM, 256), 256, 0, sm, d);
        pr.launches++;
    }
    // stateNodeCounts = countStateNodes(prevMap), plan.go:94 (zeroed above)
    if (h.n_loads > 0) {
        BLANCE_LAUNCH_NOSYNC(k_count_loads, cdiv(h.n_loads, 256), 256, 0, sm, h.n_loads, NX, sw.first && !c->loads_later_only ? 0 : 1,
                             c->load_state.as<int32_t>(), c->load_node.as<int32_t>(),
                             c->load_weight.as<int32_t>(), c->load_first.as<uint8_t>(), c->cnt.as<int32_t>());
        pr.launches++;
    }
    if (PM > 0 && !sw.opened) {
        BLANCE_LAUNCH_NOSYNC(k_count_prev, cdiv(PM, 256), 256, 0, sm, d, c->cnt.as<int32_t>());
        pr.launches++;
    }
    return 0;
}

// The order of state m's pass (plan.go:542-561): the static order stably partitioned by category in sweep 1, the static
// order itself wherever every partition has the same category.
static int pass_order(blance_ctx* c, PlanRun& pr, const Sweep& sw, int m, const int32_t** order) {
    const int P = c->h.n_parts;
    hipStream_t sm = c->stream;
    const bool sort_cat = sw.first && !(pr.at.passes_this_sweep == 0 ? c->uniform_first : c->uniform_all);
    if (sort_cat) {
        BLANCE_LAUNCH_NOSYNC(k_category, cdiv(P, 256), 256, 0, sm, pr.d, m, sw.any_removed, sw.add_nil, c->cat.as<uint8_t>());
        const int pe = partition_by_category(c, P, c->cat.as<uint8_t>(), c->part_order.as<int32_t>(), c->chunk_counts.as<int32_t>(),
                                             c->order.as<int32_t>());
        if (pe) return pe;
    } else {
        // sweeps >= 2 run with nodesToRemove = nodesToAdd = [] (non-nil, plan.go:53-55): no partition's
        // nodes are in either, so every category is "1" (plan.go:542-561) and the pass order is the
        // static order itself
    }
    // (the same holds in sweep 1 when every partition has one category, known at upload: uniform_category)
    *order = sort_cat ? c->order.as<int32_t>() : c->part_order.as<int32_t>();
    return 0;
}

struct StatePass {                 // what the paths of one state's pass share
    int m, k, higher_mask, r0, r1;
    const int32_t* order;
};

// State m's pass without region chains: the flat bulk driver, the flat single chain, or the pass kernels in order.
static int run_pass_in_order(blance_ctx* c, PlanRun& pr, Sweep& sw, const StatePass& sp) {
    const blance_problem& h = c->h;
    const int NX = h.n_nodes_ext, M = h.n_states, P = h.n_parts, L = c->L;
    const int RW = kRecHead + M * (1 + L);       // header + per-state lists
    const int m = sp.m, k = sp.k;
    hipStream_t sm = c->stream;
    int32_t* scal = c->scalars.as<int32_t>();
    const DevProblem& d = pr.d;
    int& n_pass = pr.at.n_pass;
    // (what kind of pass this will be, before its records are made: the flat bulk driver's row bound rides on the gather)
    const bool flat_state = h.hierarchy_rules_nil || sp.r1 == sp.r0;
    const bool bulk = c->engine != BLANCE_ENGINE_SEQUENTIAL && flat_state && (k == 1 || (k == 2 && sw.NP == 0)) &&
                      P >= c->chain_min_parts;
    const bool count_rows = bulk && sw.NP > 0 && c->f_row_count.p;
    const bool settled = bulk && !sw.first && pr.at.passes_this_sweep == 1 && !sw.retrying && c->dump_sweep < 0 && c->speculate > 0;
    const bool assume_stays = settled && pr.top_spec_plan && !sw.top_spec_off && k == 1 && top_spec_fits(c, pr, sw, m);
    // (what the sweep's passes so far have been: known_passes of them fresh runs known in advance, the last one
    // of state known_state with known_k picks a step)
    const bool opening = bulk && sw.first && !sw.retrying && !sw.known_broken &&
                         (sw.known_passes == 0 || (sw.known_passes == 1 && sw.known_k == 1 && sw.NP == 0 && ((sp.higher_mask >> sw.known_state) & 1)));
    const bool ungathered = assume_stays || fresh_cycle_whole(c, opening, sw.NP, k, sp.higher_mask);   // (no step record is read)
    if (count_rows && !assume_stays && rowcount_reset(c)) return BLANCE_ERR_DEVICE;
    const LaunchShape gs = shape_gather(P, RW);
    if (!ungathered)
        BLANCE_LAUNCH(k_gather, gs.grid, gs.block, gs.lds, sm, d, m, h.top_state, RW, sp.order,
                             c->state_stick.as<int32_t>(), c->state_has_stick.as<uint8_t>(), c->rec.as<int32_t>(),
                             count_rows ? c->f_row_count.as<int32_t>() : (int32_t*)nullptr, NX);
    PassParams q;
    fill_pass_common(c, q, m, k, sw.NP);
    q.L = L; q.P = P; q.top_state = h.top_state;
    q.RW = RW;
    q.higher_mask = sp.higher_mask;
    q.hier = !h.hierarchy_rules_nil;
    q.rule_begin = sp.r0; q.rule_end = sp.r1;
    q.n_alive = c->n_alive;
    q.vertex_empty_anchor = NX;
    q.node_leaf_pos = c->node_leaf_pos.as<int32_t>();
    q.anchors = c->anchors.as<AnchorSet>();
    q.ntn = c->ntn.as<int32_t>();
    q.rec = c->rec.as<int32_t>();
    q.out = c->out.as<int32_t>();
    q.warn_part = c->warn_part.as<int32_t>();
    q.warn_state = c->warn_state.as<int32_t>();
    q.warn_count = scal + kScalWarnCount;
    q.err = scal + kScalErr;
    q.spec_count = (long long*)(scal + kScalSpecCount);
    q.beg = 0; q.end = P;
    // a flat pass (no rule for the state) of a small cluster can run on one wave64
    bool flat_chain = c->engine != BLANCE_ENGINE_SEQUENTIAL && flat_state && c->flat_chain_ok && k <= 4 &&
                      P >= c->chain_min_parts;
    c->no_fast_keys = false;
    FlatChainPrep fc;
    fc.possible = flat_chain; fc.d = d; fc.m = m; fc.higher_mask = sp.higher_mask; fc.order = sp.order;
    if (flat_chain && !bulk) {               // (the bulk driver asks for the records when a sub-range needs them)
        const int pe = flat_chain_prepare(c, fc, &pr.launches);
        if (pe) return pe;
        flat_chain = fc.ok;
    }
    HIPTRY(hipEventRecord(c->pass_events[2 * n_pass], sm));
    int e;
    bool nothing_to_apply = false;               // (run_flat_pass: a pass of stays that leaves every list as it is)
    c->pass_kind.resize(n_pass + 1);
    // the flat bulk driver: k = 1, and the first sweep of a fresh plan (NumPartitions == 0) with k = 2
    if (bulk) {
        c->pass_kind[n_pass] = kPassFlatBulk;
        bool whole_known = false;
        if (assume_stays) sw.last_stays_open = c->last_stays;
        e = run_flat_pass(c, q, scal, &pr.launches, &pr.at.batched, fc, opening, &whole_known, settled, assume_stays, &nothing_to_apply,
                          count_rows);
        if (assume_stays) {
            c->top_gate = (1u << kFlagTopMoved) | (1u << kFlagForced);
            if (c->trace) fprintf(stderr, "[blance] sweep %d: state %d's pass taken to be one run of stays, checked with the sweep's readback\n", sw.it, m);
        }
        if (whole_known) { sw.known_passes++; sw.known_state = m; sw.known_k = k; sw.known_cycle = ungathered && !assume_stays; }
        else sw.known_broken = true;
    } else if (flat_chain) {
        sw.known_broken = true;
        c->pass_kind[n_pass] = kPassKernel;
        const size_t rows = sizeof(int32_t) * (size_t)(NX + 1) * (NX + 1);
        e = run_flat_chain(c, q, 0, P, sw.NP > 0 && rows <= 100 * 1024, scal, &pr.launches);
        if (e > 0) e = fail(BLANCE_ERR_DEVICE, "flat chain refused a checked pass");
        if (!e) pr.at.batched += P;
    } else {
        sw.known_broken = true;
        c->pass_kind[n_pass] = kPassKernel;
        e = dispatch_pass(c, q);
    }
    if (e) return e;
    HIPTRY(hipEventRecord(c->pass_events[2 * n_pass + 1], sm));
    n_pass++;
    if (dump_pass(c, sw.it, m, P, q.OW, nullptr)) return BLANCE_ERR_DEVICE;
    if (pr.fuse && m == pr.m_last)
        sw.tail = SweepTail{true, !nothing_to_apply, m, q.OW, sp.order, nullptr, kNoGate};
    else if (!nothing_to_apply)
        BLANCE_LAUNCH_NOSYNC(k_scatter, shape_scatter(P).grid, shape_scatter(P).block, shape_scatter(P).lds, sm, d, m, q.OW, sp.order, c->out.as<int32_t>(), kNoGate);
    return 0;
}

// State m's pass (assignStateToPartitions, plan.go:253-303): as region chains when the state's single hierarchy rule allows
// them, else in order.
static int run_state_pass(blance_ctx* c, PlanRun& pr, Sweep& sw, int m) {
    const blance_problem& h = c->h;
    const int M = h.n_states, P = h.n_parts;
    StatePass sp;
    sp.m = m;
    sp.k = c->state_constraints[m];
    if (sw.restore_counters) {                                  // (a pass whose deferred verdict came back bad)
        HIPTRY(hipMemcpyAsync(c->cnt.p, c->cnt_save.p, sizeof(int32_t) * (size_t)(M + 1) * h.n_nodes_ext, hipMemcpyDeviceToDevice, c->stream));
        sw.restore_counters = false;
    }
    const int oe = pass_order(c, pr, sw, m, &sp.order);
    if (oe) return oe;
    pr.at.passes_this_sweep++;
    c->pass_ntn_ready = false;                              // nodeToNodeCounts := fresh (plan.go:266), zeroed when first needed
    sp.higher_mask = 0;
    for (int t = 0; t < M; t++)
        if (c->state_priority[t] < c->state_priority[m]) sp.higher_mask |= 1 << t;
    sp.r0 = c->rule_off[m]; sp.r1 = c->rule_off[m + 1];
    while (c->pass_events.size() < 2 * (size_t)(pr.at.n_pass + 3)) {    // (a pass that hands off times two kernels)
        hipEvent_t ev;
        HIPTRY(hipEventCreate(&ev));
        c->pass_events.push_back(ev);
    }
    // ---- region chains, when the state's single hierarchy rule allows them
    bool done = false;
    if (c->engine != BLANCE_ENGINE_SEQUENTIAL && !h.hierarchy_rules_nil && sp.r1 - sp.r0 == 1 &&
        c->rule_regions[sp.r0].ok && P >= c->chain_min_parts && sp.k <= 4 && !(sw.retrying && sw.retry.skip)) {
        // (same_tops: the top state's pass was one run of stays AND no other state can take a partition's top priority
        // node away in between -- plan.go:146-154 keeps only nodes of STRICTLY higher priority states out of a pass)
        ChainPassArgs ca{m, sp.k, sw.NP, sp.higher_mask, sp.r0, sw.it, sp.order,
                         !sw.first && !c->tops_moved && m != h.top_state && c->top_prio_strict,
                         pr.fuse && m == pr.m_last ? &sw.tail : nullptr};
        // A KNOWN CYCLE (k_period.h): the sweep's second pass, behind a top-state pass that
        // k_fresh_cycle_commit settled as a round robin over nodesNext -- step j of the pass order took alive_ids[j % A] --
        // and in the same order.  No partition holds anything else (assign_empty), none has a weight of its own, and the
        // record's `present` bit is one and the same (every list to assign of this state is absent, or none is): words 1..23
        // of a step's record are then a function of its top priority node alone (gather_chain_record), distinct nodes give
        // distinct records (their leaves differ), and the chain of a region repeats its nodes of nodesNext from its first
        // step to its last.  All known before the pass is enqueued.
        const uint32_t kinds_m = (c->assign_kinds >> m) & 0x10001u;
        ca.round_robin = sw.first && !sw.retrying && !sw.known_broken && pr.at.passes_this_sweep == 2 &&
                         sw.known_passes == 1 && sw.known_cycle && sw.known_state == h.top_state && sw.known_k == 1 &&
                         m != h.top_state && sw.NP == 0 && c->assign_empty && h.partition_weights_nil && c->cycle_order_stands &&
                         c->leaves_distinct && kinds_m != 0x10001u;
        ca.known_cycle = c->period_known && ca.round_robin;
        ChainRun run;
        if (sw.retrying) run = sw.retry;
        run.defer = !sw.retrying && m == pr.m_last;
        sw.known_broken = true;
        const int e = run_chain_pass(c, pr, ca, run);
        if (e) {
            const bool sharded = pass_sharded(c, c->rule_regions[sp.r0].n_regions);
            if (sharded && !run.a_done) comm_poison(c);       // the other ranks are (or will be) in collective A
            if (sharded) comm_abort(c);
            return e;
        }
        if (run.pending != Pending::kNone) sw.pend = run;
        done = run.done;
    }
    if (!done) {
        const int e = run_pass_in_order(c, pr, sw, sp);
        if (e) return e;
    }
    pr.launches += 7;
    pr.at.steps += P;
    return 0;
}

// The sweep's end: convergence (plan.go:36-45) + write-back (plan.go:49-52), with the last pass's list edits when it left
// them to the tail.
static int close_sweep(blance_ctx* c, PlanRun& pr, Sweep& sw) {
    const blance_problem& h = c->h;
    const int P = h.n_parts;
    if (P <= 0) return 0;
    hipStream_t sm = c->stream;
    int32_t* scal = c->scalars.as<int32_t>();
    const DevProblem& d = pr.d;
    SweepTail& tail = sw.tail;
    const Gate cg = sw.pend.pending != Pending::kNone ? sw.pend.gate : c->top_gate ? Gate{scal + kScalFlags, c->top_gate} : kNoGate;
    if (tail.set && tail.scatter && (!tail.inv || tail.gate.flags != cg.flags || tail.gate.mask != cg.mask)) {
        // (no inverse of the pass order -- a flat pass --, or the list edits wait for other words than the convergence
        // test: on their own, as before)
        BLANCE_LAUNCH_NOSYNC(k_scatter, shape_scatter(P).grid, shape_scatter(P).block, shape_scatter(P).lds, sm, d, tail.m, tail.OW, tail.order, c->out.as<int32_t>(), tail.gate);
        pr.launches++;
        tail.scatter = false;
    }
    if (tail.set) {
        // the sweep's tail: the list edits, the convergence test and write-back, and -- when another sweep may follow --
        // that sweep's counters and kinds, in one pass over the partitions
        int32_t* next = sw.it + 1 < h.max_iterations ? c->cnt_next.as<int32_t>() : nullptr;
        const LaunchShape ts = shape_sweep_tail(P);
        BLANCE_LAUNCH(k_sweep_tail, ts.grid, ts.block, ts.lds, sm, d, tail.m, tail.OW, tail.scatter ? tail.inv : nullptr,
                      tail.scatter ? c->out.as<int32_t>() : nullptr, scal + kScalNotMatch, next, cg);   // (uses a wave ballot)
        sw.tail_counts = next != nullptr;
    } else {
        BLANCE_LAUNCH(k_converge, shape_converge(P).grid, shape_converge(P).block, shape_converge(P).lds, sm, d, scal + kScalNotMatch, cg);   // (uses a wave ballot)
    }
    pr.launches++;
    return 0;
}

// What the sweep's one readback says about the verdicts the sweep left on the device.
enum class Verdict {
    kStands,
    kSweepAgain,       // the top-state pass was not one run of stays: from the sweep's first pass, that pass read back
    kPassAgain,        // the last pass's deferred verdict was bad: that state's pass alone, as sw.retry says
};
static Verdict sweep_verdict(blance_ctx* c, PlanRun& pr, Sweep& sw) {
    const int32_t* f = pr.hs + kScalFlags;
    if (c->top_gate) {
        const bool moved = f[kFlagTopMoved] || c->speculate == 2;
        c->top_gate = 0;
        if (c->trace) fprintf(stderr, "[blance] sweep %d: the first pass %s\n", sw.it, moved ? "was not one run of stays: the sweep runs again" : "was one run of stays");
        if (moved) {
            // Nothing behind the gate ran: the live lists, prevMap, the counters and the flag words are as the sweep's
            // first pass found them.  What the host assumed or cached along the way is dropped.
            c->last_stays = sw.last_stays_open;
            c->tops_moved = true;
            c->chain_group_state = -1;                          // (a gated k_chain_classify wrote no region ids ...)
            c->group_epoch++;
            c->top_group_state = -1;                            // (... and a gated k_gather_chain no top priority keys)
            c->pass_ntn_ready = false;
            pr.at = sw.at_open;
            sw.known_passes = 0; sw.known_state = -1; sw.known_k = 0; sw.known_broken = false; sw.known_cycle = false;
            sw.retry = ChainRun();
            sw.retrying = false;
            sw.top_spec_off = true;
            pr.top_spec_plan = false;                           // (a plan whose top-state pass moves steps in one later
                                                                // sweep tends to do so in the next: read them back)
            sw.m_from = 0;
            return Verdict::kSweepAgain;
        }
    }
    const Pending pending = sw.pend.pending;
    if (pending == Pending::kNone) return Verdict::kStands;
    const bool refuted = (sw.pend.spec && (f[kFlagOrphans] || f[kFlagEvents])) || f[kFlagForced];
    const bool handed = sw.pend.handoff;                        // (k_stay_by_top behind the chain kernel: both verdicts count)
    const bool bad = f[kFlagNotLocal] || (pending == Pending::kStayTop ? f[kFlagStayMoved] : f[kFlagEscaped]) || (handed && f[kFlagStayMoved]);
    if (c->trace)
        fprintf(stderr, "[blance] chain pass state %d: deferred verdict (%s): %s; %d verified stays in %d batches\n", pr.m_last,
                pending == Pending::kStayTop ? "k_stay_by_top" : pending == Pending::kBlank ? "all-blank kernel" : "chain kernel",
                refuted ? "assumption refuted" : bad ? "the pass did not stand" : "stands", f[kFlagStaySteps], f[kFlagStayBatches]);
    if (!refuted && !bad) {
        if (pending == Pending::kChain) c->last_stays[pr.m_last] = (int64_t)f[kFlagStaySteps] + (handed ? f[kFlagHandedOff] : 0);
        return Verdict::kStands;
    }
    // nothing behind the gate ran: the live lists and prevMap are as the pass found them; the counters are not
    sw.retry = ChainRun();
    sw.retry.no_handoff = true;
    if (refuted) sw.retry.allow_spec = false;
    else if (pending == Pending::kStayTop) sw.retry.no_stay = true;
    else if (pending == Pending::kBlank) sw.retry.no_lean = true;
    else if (handed && !f[kFlagNotLocal] && !f[kFlagEscaped]) {
        // a step behind the hand-off moved: the chain kernel alone, every region to its end -- and for the rest of the plan
        pr.handoff_plan = false;
        if (c->trace) fprintf(stderr, "[blance] chain pass state %d: a step behind the hand-off moved, the pass runs again without\n", pr.m_last);
    }
    else sw.retry.skip = true;                                  // (straight to the pass in order)
    if (pending != Pending::kStayTop || refuted) {              // (k_stay_by_top changes no counter)
        c->pass_ntn_ready = false;
        sw.restore_counters = true;
    }
    pr.at = sw.at_last_pass;
    sw.retrying = true;
    sw.m_from = pr.m_last;
    return Verdict::kPassAgain;
}

static void fill_result(const PlanStats& s, blance_result* res) {
    res->n_warnings = s.n_warnings;
    res->iterations = s.iterations;
    res->converged = s.converged;
    res->device_ms = s.device_ms;
    res->steps_total = s.steps_total;
    res->steps_sequential = s.steps_total - s.steps_batched;
    res->steps_batched = s.steps_batched;
    res->kernel_launches = s.kernel_launches;
    res->pass_kernel_ms = s.pass_ms;
    res->pass_kernel_launches = s.pass_launches;
    res->flat_pass_ms = s.flat_ms;
    res->flat_passes = s.flat_passes;
    res->blank_pass_ms = s.blank_ms;
    res->blank_pass_launches = s.blank_launches;
    res->stay_pass_ms = s.stay_ms;
    res->stay_pass_launches = s.stay_launches;
    res->host_syncs = s.host_syncs;
}

// The plan's end: event times and statistics into c->stats.
static int finish_plan(blance_ctx* c, PlanRun& pr, int64_t syncs0) {
    PlanStats& s = c->stats;
    const int64_t n_warnings = pr.iterations == 0 ? 0 : s.n_warnings;     // (counted sweep by sweep)
    s = PlanStats();
    HIPTRY(hipEventRecord(c->ev1, c->stream));
    long long spec = 0, qs[4] = {0, 0, 0, 0};
    memcpy(&spec, pr.hs + kScalSpecCount, sizeof spec);
    memcpy(qs, pr.hs + kScalQueueStats, sizeof qs);
    HIPTRY(hipEventSynchronize(c->ev1));
    comm_sum_up(c);
    c->queue_moved = qs[0]; c->queue_exact = qs[1]; c->queue_rebuilds = qs[2]; c->queue_dense = qs[3];
    if (c->trace || getenv("BLANCE_QUEUE_STATS"))
        fprintf(stderr, "[blance] k_pass_queue: %lld launches, %lld stops, %lld moving steps (%lld with matrix reads, %lld scoring every node), %lld window rebuilds\n",
                (long long)c->queue_launches, (long long)c->queue_stops, qs[0], qs[1], qs[3], qs[2]);
    int64_t batched = pr.at.batched + spec;
    if (batched > pr.at.steps) batched = pr.at.steps;     // the flat chain counts its whole pass already
    if (c->trace) fprintf(stderr, "[blance] sequential passes: %lld verified stays\n", spec);
    float ms = 0.f;
    HIPTRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    for (int i = 0; i < pr.at.n_pass; i++) {
        float pm = 0.f;
        HIPTRY(hipEventElapsedTime(&pm, c->pass_events[2 * i], c->pass_events[2 * i + 1]));
        const PassKind kind = c->pass_kind[i];
        if (kind != kPassFlatBulk) { s.pass_ms += pm; s.pass_launches++; } else { s.flat_ms += pm; s.flat_passes++; }
        if (kind == kPassBlank) { s.blank_ms += pm; s.blank_launches++; }
        if (kind == kPassStayTop) { s.stay_ms += pm; s.stay_launches++; }
        if (c->trace)
            fprintf(stderr, "[blance] pass %d (%s): %.3f ms\n", i,
                    kind == kPassFlatBulk ? "flat bulk driver" : kind == kPassBlank ? "all-blank chain kernel" :
                    kind == kPassStayTop ? "k_stay_by_top" : "pass kernel", pm);
    }
    s.iterations = pr.iterations;
    s.converged = pr.converged;
    s.n_warnings = n_warnings;
    s.device_ms = ms;
    s.host_syncs = c->n_syncs - syncs0;
    s.steps_total = pr.at.steps;
    s.steps_batched = batched;
    s.kernel_launches = pr.launches;
    return 0;
}

static int plan_locked(blance_ctx* c, blance_result* res) {
    if (!c->uploaded) return fail(BLANCE_ERR_BAD_ARG, "no problem uploaded");
    HIPTRY(hipSetDevice(c->device));
    const blance_problem& h = c->h;
    const int M = h.n_states, P = h.n_parts;
    hipStream_t sm = c->stream;
    int32_t* scal = c->scalars.as<int32_t>();

    PlanRun pr;
    pr.d = dev_problem(c);
    c->last_stays.assign((size_t)(M > 0 ? M : 1), 0);
    c->queue_launches = c->queue_stops = 0;
    c->comm_events_used = 0;
    c->chain_group_state = -1;
    c->group_epoch++;
    c->top_group_state = -1;
    c->tail_counted = false;
    if (c->side_pending) { HIPTRY(hipStreamSynchronize(c->side)); c->side_pending = false; }
    const int64_t syncs0 = c->n_syncs;
    pr.fuse = c->fused_tail && !comm_active(c);

    HIPTRY(hipEventRecord(c->ev0, sm));
    HIPTRY(hipMemsetAsync(scal, 0, sizeof(int32_t) * kScalWords, sm));
    if (c->speculate == 2) {                                         // (tests: every deferred verdict comes back bad, every gate is closed)
        static const int32_t one = 1;
        HIPTRY(hipMemcpyAsync(scal + kScalFlags + kFlagForced, &one, sizeof one, hipMemcpyHostToDevice, sm));
    }
    if (P > 0) {
        BLANCE_LAUNCH_NOSYNC(k_flags_init, cdiv(P, 256), 256, 0, sm, P, c->part_in_prev.as<uint8_t>(), c->part_never_equal.as<uint8_t>(),
                             pr.d.in_prev, pr.d.never_equal);
    }
    for (int m = 0; m < M; m++)
        if (c->state_constraints[m] > 0 && P > 0) pr.m_last = m;
    for (int it = 0; it < h.max_iterations; it++) {                 // plan.go:32
        Sweep sw;
        sw.it = it;
        sw.first = it == 0;
        sw.add_nil = sw.first ? h.nodes_to_add_nil : 0;
        sw.any_removed = sw.first ? c->any_removed : 0;
        sw.NP = sw.first ? h.n_prev : c->np_later;
        int e = open_sweep(c, pr, sw);
        if (e) return e;
        pr.at.passes_this_sweep = 0;
        sw.at_open = pr.at;
        Verdict v;
        do {
            sw.pend = ChainRun();
            sw.tail = SweepTail();
            sw.tail_counts = false;
            c->top_gate = 0;
            sw.at_last_pass = pr.at;
            for (int m = sw.m_from; m < M; m++) {                   // plan.go:307-324
                if (c->state_constraints[m] <= 0 || P == 0) continue;
                if (m == pr.m_last) sw.at_last_pass = pr.at;
                if ((e = run_state_pass(c, pr, sw, m))) return e;
            }
            if (!sw.counted) pr.iterations++;
            sw.counted = true;
            if ((e = close_sweep(c, pr, sw))) return e;
            // one readback per sweep: the convergence word with the warnings count, the chain flags (a deferred verdict) and --
            // complete with the last sweep -- the statistics words behind them (steps k_pass_seq committed as verified stays,
            // the queue kernel's counters)
            HIPTRY(read_back(c, pr.hs, scal, sizeof pr.hs));
            HIPTRY(stream_sync(c));
            HIPTRY(hipGetLastError());
            v = sweep_verdict(c, pr, sw);
        } while (v != Verdict::kStands);
        c->tail_counted = sw.tail_counts;                           // (the tail that stood: a closed gate's wrote nothing)
        if (pr.hs[kScalErr]) return fail(BLANCE_ERR_UNSUPPORTED, "hierarchy fold overflowed the device's interval budget");
        c->stats.n_warnings = pr.hs[kScalWarnCount];
        if (!pr.hs[kScalNotMatch]) { pr.converged = 1; break; }
    }
    const int fe = finish_plan(c, pr, syncs0);
    if (fe) return fe;
    c->planned = true;
    if (res) {
        fill_result(c->stats, res);
        res->total_ms = res->device_ms;
    }
    return BLANCE_OK;
}

static int download_locked(blance_ctx* c, blance_result* res) {
    if (!c->planned) return fail(BLANCE_ERR_BAD_ARG, "nothing planned yet");
    if (!res || !res->out_off || !res->out_nodes || !res->out_kind || !res->warn_part || !res->warn_state)
        return fail(BLANCE_ERR_BAD_ARG, "null result buffers");
    HIPTRY(hipSetDevice(c->device));
    const blance_problem& h = c->h;
    const int M = h.n_states, P = h.n_parts, L = c->L;
    const size_t PM = (size_t)P * M;
    if (c->stats.n_warnings > res->warn_capacity) return fail(BLANCE_ERR_CAPACITY, "warn_capacity too small");
    if (c->stats.iterations == 0) {
        // MaxIterationsPerPlan <= 0: planNextMapEx returns (nil, nil) -- nothing to report (plan.go:32-58)
        for (size_t i = 0; i <= PM; i++) res->out_off[i] = 0;
        for (size_t i = 0; i < PM; i++) res->out_kind[i] = BLANCE_LIST_ABSENT;
        res->n_warnings = 0;
        res->iterations = 0;
        res->converged = 0;
        return BLANCE_OK;
    }
    res->out_off[0] = 0;
    Mover down(c, false);
    c->stage.used = 0;
    int e = 0;
    if (PM) {
        // the CSR is made on the device (lengths -> exclusive scan -> gather) and lands in the caller's arrays: directly when
        // they are page-locked, through the staging buffer otherwise
        DevProblem d = result_problem(c);
        RESERVE(dl_off, sizeof(int32_t) * (PM + 2));
        BLANCE_LAUNCH_NOSYNC(k_result_len, cdiv((int64_t)PM + 1, 256), 256, 0, c->stream, d, c->dl_off.as<int32_t>());
        SCANTRY((int)PM + 1, c->dl_off.as<int32_t>());
        int32_t total = 0;
        HIPTRY(read_back(c, &total, c->dl_off.as<int32_t>() + PM, sizeof total));
        HIPTRY(stream_sync(c));
        if (total > res->out_capacity) return fail(BLANCE_ERR_CAPACITY, "out_capacity too small");
        RESERVE(dl_nodes, sizeof(int32_t) * ((size_t)total + 1));
        BLANCE_LAUNCH_NOSYNC(k_result_gather, cdiv((int64_t)PM, 256), 256, 0, c->stream, d, c->dl_off.as<int32_t>(),
                             c->dl_nodes.as<int32_t>());
        if ((e = down.copy(res->out_off, c->dl_off.p, sizeof(int32_t) * (PM + 1)))) return e;
        if (total && (e = down.copy(res->out_nodes, c->dl_nodes.p, sizeof(int32_t) * (size_t)total))) return e;
        if ((e = down.copy(res->out_kind, c->prv_kind.p, PM))) return e;
    }
    if (c->stats.n_warnings) {
        if ((e = down.copy(res->warn_part, c->warn_part.p, sizeof(int32_t) * (size_t)c->stats.n_warnings))) return e;
        if ((e = down.copy(res->warn_state, c->warn_state.p, sizeof(int32_t) * (size_t)c->stats.n_warnings))) return e;
    }
    if ((e = down.finish())) return e;
    HIPTRY(stream_sync(c));
    fill_result(c->stats, res);
    return BLANCE_OK;
}

static int calc_moves_locked(blance_ctx* c, const blance_moves_problem* pb, blance_moves_result* res) {
    const int P = pb->n_parts, M = pb->n_states;
    if (P < 0 || M < 0 || !pb->beg_off || !pb->end_off || !pb->beg_nodes || !pb->end_nodes || !res->op_off ||
        !res->op_node || !res->op_state || !res->op_kind)
        return fail(BLANCE_ERR_BAD_ARG, "null array pointer or negative size");
    const size_t PS = (size_t)P * (M + 1);
    if (pb->beg_off[0] != 0 || pb->end_off[0] != 0) return fail(BLANCE_ERR_BAD_ARG, "CSR offsets must start at 0");
    for (size_t i = 0; i < PS; i++)
        if (pb->beg_off[i + 1] < pb->beg_off[i] || pb->end_off[i + 1] < pb->end_off[i])
            return fail(BLANCE_ERR_BAD_ARG, "CSR offsets not monotone");
    const int64_t nb = pb->beg_off[PS], ne = pb->end_off[PS], cap = nb + ne;
    if (cap > res->capacity) return fail(BLANCE_ERR_CAPACITY, "moves capacity too small");
    if (cap > (int64_t)INT32_MAX) return fail(BLANCE_ERR_UNSUPPORTED, "more than 2^31 list entries");
    HIPTRY(hipSetDevice(c->device));
    MovesBufs& mb = c->mv;
    DevBuf &boff = mb.beg_off, &bnod = mb.beg_nodes, &eoff = mb.end_off, &enod = mb.end_nodes, &onode = mb.op_node, &ostate = mb.op_state,
           &okind = mb.op_kind, &nmov = mb.n_moves, &cnode = mb.c_node, &cstate = mb.c_state, &ckind = mb.c_kind;
    auto up = [&](DevBuf& b, const int32_t* src, size_t n) -> int {
        if (b.reserve(sizeof(int32_t) * (n + 1))) return fail(BLANCE_ERR_DEVICE, "hipMalloc failed");
        if (n) HIPTRY(hipMemcpyAsync(b.p, src, sizeof(int32_t) * n, hipMemcpyHostToDevice, c->stream));
        return 0;
    };
    int e;
    if ((e = up(boff, pb->beg_off, PS + 1)) || (e = up(bnod, pb->beg_nodes, (size_t)nb)) ||
        (e = up(eoff, pb->end_off, PS + 1)) || (e = up(enod, pb->end_nodes, (size_t)ne)))
        return e;
    if (onode.reserve(sizeof(int32_t) * ((size_t)cap + 1)) || ostate.reserve(sizeof(int32_t) * ((size_t)cap + 1)) ||
        okind.reserve(sizeof(int32_t) * ((size_t)cap + 1)) || nmov.reserve(sizeof(int32_t) * ((size_t)P + 2)) ||
        cnode.reserve(sizeof(int32_t) * ((size_t)cap + 1)) || cstate.reserve(sizeof(int32_t) * ((size_t)cap + 1)) ||
        ckind.reserve(sizeof(int32_t) * ((size_t)cap + 1)))
        return fail(BLANCE_ERR_DEVICE, "hipMalloc failed");
    MovesParams q;
    q.P = P; q.M = M; q.favor_min_nodes = pb->favor_min_nodes;
    q.beg_off = boff.as<int32_t>(); q.beg_nodes = bnod.as<int32_t>();
    q.end_off = eoff.as<int32_t>(); q.end_nodes = enod.as<int32_t>();
    q.op_node = onode.as<int32_t>(); q.op_state = ostate.as<int32_t>(); q.op_kind = okind.as<int32_t>();
    q.n_moves = nmov.as<int32_t>();
    HIPTRY(hipEventRecord(c->ev0, c->stream));
    res->op_off[0] = 0;
    if (P > 0) {
        // per-partition slices -> offsets (exclusive scan of the move counts) -> packed on the device
        HIPTRY(hipMemsetAsync(nmov.as<int32_t>() + P, 0, sizeof(int32_t), c->stream));
        BLANCE_LAUNCH_NOSYNC(k_calc_moves, cdiv(P, 256), 256, 0, c->stream, q);
        SCANTRY(P + 1, nmov.as<int32_t>());
        BLANCE_LAUNCH_NOSYNC(k_moves_compact, cdiv(P, 256), 256, 0, c->stream, q, nmov.as<int32_t>(), cnode.as<int32_t>(),
                             cstate.as<int32_t>(), ckind.as<int32_t>());
    }
    HIPTRY(hipEventRecord(c->ev1, c->stream));
    if (P > 0) {
        HIPTRY(hipMemcpyAsync(res->op_off, nmov.p, sizeof(int32_t) * ((size_t)P + 1), hipMemcpyDeviceToHost, c->stream));
        HIPTRY(stream_sync(c));
        const int64_t total = res->op_off[P];
        if (total > 0) {
            HIPTRY(hipMemcpyAsync(res->op_node, cnode.p, sizeof(int32_t) * total, hipMemcpyDeviceToHost, c->stream));
            HIPTRY(hipMemcpyAsync(res->op_state, cstate.p, sizeof(int32_t) * total, hipMemcpyDeviceToHost, c->stream));
            HIPTRY(hipMemcpyAsync(res->op_kind, ckind.p, sizeof(int32_t) * total, hipMemcpyDeviceToHost, c->stream));
        }
    }
    HIPTRY(stream_sync(c));
    float ms = 0.f;
    HIPTRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    res->device_ms = ms;
    return BLANCE_OK;
}

extern "C" int blance_calc_moves(blance_ctx* c, const blance_moves_problem* pb, blance_moves_result* res) {
    return enter(c, [&]() -> int {
        if (!pb || !res) return fail(BLANCE_ERR_BAD_ARG, "null argument");
        return calc_moves_locked(c, pb, res);
    });
}

extern "C" int blance_upload(blance_ctx* c, const blance_problem* pb) {
    return enter(c, [&]() -> int { return upload_inner(c, pb); });
}

extern "C" int blance_plan_resident(blance_ctx* c, blance_result* res) {
    return enter(c, [&]() -> int { return plan_locked(c, res); });
}

// ---- what blance_plan_adopt and blance_wire_adopt share.
// P' as a blance_problem, but for its lists, n_prev and n_loads: the pure analysis reads nothing else.  Every array pointer
// of it is one of the context's copies, the call's two arrays, or NULL: c->h still carries the upload's pointers to the
// caller's lists and weights, which are gone.
static blance_problem adopt_shell(const blance_ctx* c, const uint8_t* node_removed, const uint8_t* node_added, int nodes_to_add_nil) {
    blance_problem q = c->h;
    q.state_stickiness = nullptr; q.state_has_stickiness = nullptr;
    q.part_order = nullptr; q.part_weight = nullptr; q.part_has_weight = nullptr;
    q.part_in_prev = nullptr; q.part_prev_never_equal = nullptr;
    q.assign_off = nullptr; q.assign_nodes = nullptr; q.assign_kind = nullptr;
    q.prev_off = nullptr; q.prev_nodes = nullptr; q.prev_kind = nullptr;
    q.load_state = nullptr; q.load_node = nullptr; q.load_weight = nullptr; q.load_first_sweep_only = nullptr;
    q.node_weight = c->h_node_weight.data();
    q.state_priority = c->state_priority.data();
    q.state_constraints = c->state_constraints.data();
    q.rule_off = c->rule_off.data();
    q.node_removed = node_removed;
    q.node_added = node_added;
    q.node_has_weight = c->h_node_has_weight.data();
    q.node_leaf_pos = c->h_node_leaf_pos.data();
    q.rule_inc = c->h_rule_inc.data();
    q.rule_exc = c->h_rule_exc.data();
    q.vertex_parent = c->h_vparent.data();
    q.vertex_leaf_lo = c->h_vlo.data();
    q.vertex_leaf_hi = c->h_vhi.data();
    q.nodes_to_add_nil = nodes_to_add_nil ? 1 : 0;
    return q;
}

// validate_tail_b's load bound for P' (its other checks depend on sizes that do not change; L' <= L)
static bool adopt_load_overflows(const blance_ctx* c, const PartsSummary& ps, bool keep) {
    long long ksum = 0;
    for (int32_t k : c->state_constraints) ksum += k > 0 ? k : 0;
    return adopt_load_bound_exceeded(ps.aprev, keep ? c->kept_load_abs : 0, ps.sumw, ksum);
}

// neither adopts on a context with a communicator; who: the entry point, for the text
static int comm_refuse(const blance_ctx* c, const char* who) {
    if (comm_active(c) || c->rccl_comm || c->comm.allreduce_sum_i32 || c->comm.allgather_i32)
        return fail(BLANCE_ERR_UNSUPPORTED, "%s on a context with a communicator", who);
    return BLANCE_OK;
}

// Where a summary block keeps what validate_tail_b and upload_facts want of P' (k_adopt_len: kAdoptRes*, k_wire_adopt_sum:
// kWaRes*): int32 words, and 64-bit words counted from word 4 of the block.  fresh < 0: the block has no such word, no
// partition of P' is outside its prevMap
struct SummaryWords { int longest, fresh, kinds, cap64, prev64, total64; };
constexpr SummaryWords kAdoptSummary{kAdoptResLongest, -1, kAdoptResKinds, kAdoptRes64Cap, kAdoptRes64Prev, kAdoptRes64Total};
constexpr SummaryWords kWaSummary{kWaResLongest, kWaResFresh, kWaResKinds, kWaRes64Cap, kWaRes64Prev, kWaRes64Total};
static UploadSummary adopt_summary(const blance_ctx* c, const int32_t* vr, const SummaryWords& w) {
    long long r64[5];
    memcpy(r64, vr + 4, sizeof r64);
    UploadSummary sum;
    sum.ps = PartsSummary{vr[w.longest], w.fresh < 0 ? 0 : vr[w.fresh], r64[w.cap64], c->sum_abs_weight, r64[w.prev64]};
    sum.assign_kinds = (uint32_t)vr[w.kinds];
    sum.na = r64[w.total64];
    return sum;
}

// The second half of both: from here on the problem is rewritten, a failure leaves the context without one, as a failed
// upload does.  q: adopt_shell's problem with n_prev and n_loads set; na / np: the entries a_nodes / p_nodes must hold (-1:
// the buffer stays as it is); write_lists launches the kernel that writes the lists and the partitions' flags.
template <class F>
static int adopt_swap(blance_ctx* c, const blance_problem& q, const UploadSummary& sum, bool keep, int64_t na, int64_t np, F write_lists) {
    const int NX = q.n_nodes_ext;
    c->uploaded = false;
    c->planned = false;
    c->h.nodes_to_add_nil = q.nodes_to_add_nil;
    c->h.n_prev = q.n_prev;
    c->h.n_loads = q.n_loads;
    c->loads_later_only = keep;
    if (!keep) c->kept_load_abs = 0;                     // (the load entries are gone for every later adoption too)
    const NodeFacts nodes = node_facts(q);               // (copied from by every flush below: it lives to the end)
    Mover up(c, true);
    c->stage.used = 0;                                   // (the stream is idle here)
    int st;
    PUT(node_removed, q.node_removed, NX);
    PUT(node_added, q.node_added, NX);
    PUT(alive, nodes.alive.data(), NX);
    PUT(alive_ids, nodes.alive_ids.data(), nodes.alive_ids.size());
    PUT(alive_rank, nodes.alive_rank.data(), NX);
    if ((st = up.flush())) return st;
    if (na >= 0) RESERVE(a_nodes, sizeof(int32_t) * (size_t)na);
    if (np >= 0) RESERVE(p_nodes, sizeof(int32_t) * (size_t)np);
    if ((st = write_lists())) return st;
    // what the sweep driver's shortcuts rest on, as a fresh upload of P' decides it -- but for L, which stays the stride of
    // the working state's rows (L' <= L; every buffer of upload_reserve is sized by it)
    const int L = c->L;
    const bool flat_chain_ok = c->flat_chain_ok;
    upload_facts(c, &q, nodes, sum);
    c->L = L;
    c->flat_chain_ok = flat_chain_ok;
    if (!q.hierarchy_rules_nil && (st = upload_rule_tables(c, &q, nodes, up))) return st;
    if ((st = up.flush())) return st;
    // the caches of the sweep driver that outlive a plan (plan_locked drops the rest when it starts)
    c->h_reg_off.clear();
    c->chain_group_state = -1;
    c->chain_group_static = false;
    c->top_group_state = -1;
    c->group_epoch++;
    c->cycle_group_epoch = -1;
    c->top_group_epoch = -1;
    c->tail_counted = false;
    c->flags_clean = c->rowcount_clean = false;
    c->pass_ntn_ready = false;
    c->bits_stale = true;
    c->no_fast_keys = false;
    c->tops_moved = true;
    c->top_gate = 0;
    HIPTRY(stream_sync(c));                              // nothing of the caller's or of this frame is read after the call
    HIPTRY(hipGetLastError());
    c->uploaded = true;
    return BLANCE_OK;
}

// ---- blance_plan_adopt: the planned map becomes assign_* and prev_* of the problem the context holds,
// the node change is analysed again from the host's copies of the small arrays.  Everything that can refuse is decided
// before the problem is touched: the argument checks at once, P''s share of blance_validate (validate_tail_b) from the
// summary k_adopt_len leaves in a scratch buffer -- the call's one host round trip.
static int adopt_locked(blance_ctx* c, const blance_adopt* ad) {
    if (!c->planned) return fail(BLANCE_ERR_BAD_ARG, "nothing planned yet");
    if (c->stats.iterations == 0) return fail(BLANCE_ERR_BAD_ARG, "the plan made no sweep (max_iterations <= 0): there is no map to adopt");
    if (!ad->node_removed || !ad->node_added) return fail(BLANCE_ERR_BAD_ARG, "null array pointer");
    for (int32_t r : ad->reserved) if (r) return fail(BLANCE_ERR_BAD_ARG, "blance_adopt::reserved must be zero");
    if (int st = comm_refuse(c, "blance_plan_adopt")) return st;
    HIPTRY(hipSetDevice(c->device));
    const blance_problem& h = c->h;
    const int M = h.n_states, P = h.n_parts;
    const int64_t PM = (int64_t)P * M;
    const bool keep = ad->keep_prev_only != 0;
    hipStream_t sm = c->stream;
    if (c->side_pending) { HIPTRY(hipStreamSynchronize(c->side)); c->side_pending = false; }

    blance_problem q = adopt_shell(c, ad->node_removed, ad->node_added, ad->nodes_to_add_nil);
    q.n_prev = keep ? c->np_later : P;                  // (np_later: the old n_prev + the partitions that were not in prevMap)
    q.n_loads = keep ? h.n_loads : 0;

    // the length-and-summary pass and the scan, into scratch (blance_download's offsets: nothing is planned after this call)
    AdoptParams ap;
    memset(&ap, 0, sizeof ap);
    UploadSummary sum;
    sum.ps = PartsSummary{0, 0, 0, c->sum_abs_weight, 0};
    sum.assign_kinds = 0;
    sum.na = 0;
    if (PM > 0) {
        const DevProblem d = result_problem(c);
        RESERVE(dl_off, sizeof(int32_t) * ((size_t)PM + 2));
        RESERVE(adopt_res, sizeof(int32_t) * kAdoptResWords);
        ap.P = P; ap.M = M; ap.L = c->L; ap.weights_nil = h.partition_weights_nil;
        for (int m = 0; m < M; m++) ap.k[m] = c->state_constraints[m];
        ap.prv = d.live; ap.prv_len = d.live_len; ap.prv_kind = d.live_kind;
        ap.part_weight = c->part_weight.as<int32_t>(); ap.part_has_weight = c->part_has_weight.as<uint8_t>();
        ap.len = c->dl_off.as<int32_t>(); ap.res = c->adopt_res.as<int32_t>();
        HIPTRY(hipMemsetAsync(ap.res, 0, sizeof(int32_t) * kAdoptResWords, sm));
        const int wgs = cdiv(PM + 1, 256);
        BLANCE_LAUNCH(k_adopt_len, wgs < kAdoptMaxWgs ? wgs : kAdoptMaxWgs, 256, 4 * 5 * sizeof(unsigned long long), sm, ap);
        SCANTRY((int)PM + 1, ap.len);
        int32_t vr[kAdoptResWords] = {0};
        HIPTRY(read_back(c, vr, ap.res, sizeof vr));
        HIPTRY(stream_sync(c));
        HIPTRY(hipGetLastError());
        sum = adopt_summary(c, vr, kAdoptSummary);
        if (sum.na > (long long)INT32_MAX) return fail(BLANCE_ERR_UNSUPPORTED, "more than 2^31 list entries");
    }
    if (adopt_load_overflows(c, sum.ps, keep)) return fail(BLANCE_ERR_UNSUPPORTED, "partition weights overflow the int32 load tables");

    return adopt_swap(c, q, sum, keep, PM > 0 ? sum.na : -1, PM > 0 ? sum.na : -1, [&]() -> int {
        if (PM > 0) {
            ap.a_off = c->a_off.as<int32_t>(); ap.a_nodes = c->a_nodes.as<int32_t>(); ap.a_kind = c->a_kind.as<uint8_t>();
            ap.p_off = c->p_off.as<int32_t>(); ap.p_nodes = c->p_nodes.as<int32_t>(); ap.p_kind = c->p_kind.as<uint8_t>();
            ap.part_in_prev = c->part_in_prev.as<uint8_t>(); ap.part_never_equal = c->part_never_equal.as<uint8_t>();
            BLANCE_LAUNCH(k_adopt_write, cdiv(PM, kAdoptLists), kAdoptLists, adopt_write_lds(c->L), sm, ap);
        } else if (P > 0) {                                  // (no states: no list, the flags alone)
            HIPTRY(hipMemsetAsync(c->part_in_prev.p, 1, (size_t)P, sm));
            HIPTRY(hipMemsetAsync(c->part_never_equal.p, 0, (size_t)P, sm));
        }
        return BLANCE_OK;
    });
}

extern "C" int blance_plan_adopt(blance_ctx* c, const blance_adopt* ad) {
    return enter(c, [&]() -> int {
        if (!ad) return fail(BLANCE_ERR_BAD_ARG, "null argument");
        return adopt_locked(c, ad);
    });
}

// a statistics request: the six mandatory arrays, their capacity (blance_plan_stats_get and every problem of a batch)
static int stats_arrays_check(const blance_plan_stats* st, int n_states) {
    if (st->n_states < n_states || !st->load_min || !st->load_max || !st->load_sum || !st->load_sumsq || !st->nodes_used ||
        !st->unmet_slots)
        return fail(BLANCE_ERR_BAD_ARG, "stats arrays missing or shorter than n_states");
    return BLANCE_OK;
}

// the statistics of the map the context holds (blance_plan_stats_get; a batch's single-path problems); *launches grows by
// the kernels launched
static int plan_stats_locked(blance_ctx* c, blance_plan_stats* st, int64_t* launches = nullptr) {
    if (!c->planned) return fail(BLANCE_ERR_BAD_ARG, "nothing planned yet");
    const blance_problem& h = c->h;
    const int N = h.n_nodes, NX = h.n_nodes_ext, M = h.n_states, P = h.n_parts;
    if (int e = stats_arrays_check(st, M)) return e;
    HIPTRY(hipSetDevice(c->device));
    hipStream_t sm = c->stream;
    DevBuf load, out, cons, unmet, roff;
    if (load.reserve(sizeof(int32_t) * ((size_t)M * (NX > 0 ? NX : 1) + 1)) || out.reserve(sizeof(long long) * ((size_t)M * 5 + 1)) ||
        cons.reserve(sizeof(int32_t) * ((size_t)M + 1)) || unmet.reserve(sizeof(long long) * (2 * (size_t)M + 1)) ||
        roff.reserve(sizeof(int32_t) * ((size_t)M + 2)))
        return fail(BLANCE_ERR_DEVICE, "hipMalloc failed");
    std::vector<long long> host((size_t)M * 5 + 1), hun(2 * (size_t)M + 1, 0);
    int n_next = 0;
    if (c->stats.iterations > 0 && M > 0) {
        HIPTRY(hipMemsetAsync(load.p, 0, sizeof(int32_t) * (size_t)M * (NX > 0 ? NX : 1), sm));
        HIPTRY(hipMemsetAsync(unmet.p, 0, sizeof(long long) * 2 * (size_t)M, sm));
        HIPTRY(hipMemcpyAsync(cons.p, c->state_constraints.data(), sizeof(int32_t) * (size_t)M, hipMemcpyHostToDevice, sm));
        DevProblem d = result_problem(c);
        int n_launched = 1;
        if ((int64_t)P * M > 0) {
            BLANCE_LAUNCH_NOSYNC(k_stats_load, cdiv((int64_t)P * M, 256), 256, 0, sm, d, load.as<int32_t>(), cons.as<int32_t>(),
                                 unmet.as<unsigned long long>());
            n_launched++;
        }
        if (!h.hierarchy_rules_nil && h.n_rules > 0 && (int64_t)P * M > 0) {      // rule violations (words M .. 2M - 1 of `unmet`)
            HIPTRY(hipMemcpyAsync(roff.p, c->rule_off.data(), sizeof(int32_t) * ((size_t)M + 1), hipMemcpyHostToDevice, sm));
            BLANCE_LAUNCH_NOSYNC(k_stats_rules, cdiv((int64_t)P * M, 256), 256, 0, sm, d, h.top_state, roff.as<int32_t>(),
                                 c->anchors.as<AnchorSet>(), c->node_leaf_pos.as<int32_t>(), unmet.as<unsigned long long>() + M);
            n_launched++;
        }
        BLANCE_LAUNCH(k_stats_reduce, M, 256, sizeof(long long) * 5 * 256 + 64, sm, N, NX, c->alive.as<uint8_t>(), load.as<int32_t>(), out.as<long long>());
        if (launches) *launches += n_launched;
        // (into the context's read-back block, not into these locals: an error exit drops what is queued there)
        HIPTRY(read_back(c, host.data(), out.p, sizeof(long long) * (size_t)M * 5));
        HIPTRY(read_back(c, hun.data(), unmet.p, sizeof(long long) * 2 * (size_t)M));
        HIPTRY(stream_sync(c));
    }
    if (c->stats.iterations > 0) n_next = c->n_alive;
    st->n_nodes_next = n_next;
    for (int m = 0; m < M; m++) {
        const bool any = c->stats.iterations > 0 && n_next > 0;
        st->load_min[m] = any ? host[(size_t)m * 5 + 0] : 0;
        st->load_max[m] = any ? host[(size_t)m * 5 + 1] : 0;
        st->load_sum[m] = any ? host[(size_t)m * 5 + 2] : 0;
        st->load_sumsq[m] = any ? host[(size_t)m * 5 + 3] : 0;
        st->nodes_used[m] = any ? (int32_t)host[(size_t)m * 5 + 4] : 0;
        st->unmet_slots[m] = c->stats.iterations > 0 ? hun[(size_t)m] : 0;
        if (st->rule_violations) st->rule_violations[m] = c->stats.iterations > 0 ? hun[(size_t)M + m] : 0;
    }
    return BLANCE_OK;
}

extern "C" int blance_plan_stats_get(blance_ctx* c, blance_plan_stats* st) {
    return enter(c, [&]() -> int {
        if (!st) return fail(BLANCE_ERR_BAD_ARG, "null argument");
        return plan_stats_locked(c, st);
    });
}

// the CSR of the prevMap keys outside the model, where a moves request has one (blance_plan_moves_get and every problem of
// a batch): P + 1 offsets from 0, not falling, every node an id of the problem's
static int beg_other_check(const int32_t* off, const int32_t* nodes, int P, int NX) {
    if (!off) return BLANCE_OK;
    if (off[0] != 0) return fail(BLANCE_ERR_BAD_ARG, "beg_other offsets must start at 0");
    for (int p = 0; p < P; p++)
        if (off[p + 1] < off[p]) return fail(BLANCE_ERR_BAD_ARG, "beg_other offsets not monotone");
    for (int32_t j = 0; j < off[P]; j++)
        if (nodes[j] < 0 || nodes[j] >= NX) return fail(BLANCE_ERR_BAD_ARG, "beg_other node id outside [0, n_nodes_ext)");
    return BLANCE_OK;
}

// prev_off[P*M] + beg_other_off[P] + blance_result_capacity(pb) (blance_plan_moves_capacity, blance_batch_moves_capacity)
static int64_t moves_capacity(const blance_problem* pb, const int32_t* beg_other_off) {
    if (!pb || !pb->prev_off || pb->n_parts < 0 || pb->n_states < 0) return 0;
    int64_t cap = pb->prev_off[(size_t)pb->n_parts * pb->n_states] + blance_result_capacity(pb);
    if (beg_other_off) cap += beg_other_off[pb->n_parts];
    return cap;
}

// the partition moves of the map the context holds (blance_plan_moves_get): both maps are read where the
// plan left them, k_plan_moves counts, the counts are scanned, k_plan_moves writes every move at its final place
static int plan_moves_locked(blance_ctx* c, blance_plan_moves* mv) {
    if (!c->planned) return fail(BLANCE_ERR_BAD_ARG, "nothing planned yet");
    if (c->stats.iterations == 0) return fail(BLANCE_ERR_BAD_ARG, "the plan made no sweep (max_iterations <= 0): there is no map to move to");
    blance_moves_result& o = mv->out;
    const bool count_only = !o.op_node && !o.op_state && !o.op_kind && o.capacity == 0;
    if (!count_only && (!o.op_node || !o.op_state || !o.op_kind || o.capacity < 0))
        return fail(BLANCE_ERR_BAD_ARG, "null moves buffers (count only: all three NULL and capacity 0)");
    if (!count_only && !o.op_off) return fail(BLANCE_ERR_BAD_ARG, "op_off is NULL but the move arrays are given");
    if (!mv->beg_other_off != !mv->beg_other_nodes)
        return fail(BLANCE_ERR_BAD_ARG, "beg_other_off and beg_other_nodes: both or neither");
    const blance_problem& h = c->h;
    const int P = h.n_parts, M = h.n_states;
    if (int e = beg_other_check(mv->beg_other_off, mv->beg_other_nodes, P, h.n_nodes_ext)) return e;
    const int64_t n_other = mv->beg_other_off ? mv->beg_other_off[P] : 0;
    HIPTRY(hipSetDevice(c->device));
    hipStream_t sm = c->stream;
    unsigned long long cnt[6] = {0, 0, 0, 0, 0, 0};
    float ms = 0.f;
    if (P > 0) {
        constexpr size_t kHead = 1024;             // the six counter words, a cache line each, in front of n_moves [P + 1]
        static_assert(6 * kPlanMovesCounterStride * sizeof(unsigned long long) <= kHead, "counters outgrew their block");
        DevBuf &ooff = c->mv.other_off(), &onod = c->mv.other_nodes(), &nmov = c->mv.n_moves, &cnode = c->mv.c_node,
               &cstate = c->mv.c_state, &ckind = c->mv.c_kind;
        if (nmov.reserve(kHead + sizeof(int32_t) * ((size_t)P + 2)) || ooff.reserve(sizeof(int32_t) * ((size_t)P + 2)) ||
            onod.reserve(sizeof(int32_t) * ((size_t)n_other + 1)))
            return fail(BLANCE_ERR_DEVICE, "hipMalloc failed");
        int e = 0;
        if (mv->beg_other_off) {                   // the call's only upload
            Mover up(c, true);
            c->stage.used = 0;                     // (the stream is idle between calls)
            if ((e = up.copy(ooff.p, mv->beg_other_off, sizeof(int32_t) * ((size_t)P + 1)))) return e;
            if ((e = up.copy(onod.p, mv->beg_other_nodes, sizeof(int32_t) * (size_t)n_other))) return e;
            if ((e = up.flush())) return e;
        }
        const DevProblem d = result_problem(c);
        PlanMovesParams q;
        memset(&q, 0, sizeof q);
        q.P = P; q.M = M; q.L = d.L; q.favor_min_nodes = mv->favor_min_nodes ? 1 : 0;
        q.beg_off = c->p_off.as<int32_t>(); q.beg_nodes = c->p_nodes.as<int32_t>(); q.in_prev = c->part_in_prev.as<uint8_t>();
        if (mv->beg_other_off) { q.other_off = ooff.as<int32_t>(); q.other_nodes = onod.as<int32_t>(); }
        q.end = d.live; q.end_len = d.live_len; q.end_kind = d.live_kind;
        q.counters = nmov.as<unsigned long long>();
        q.n_moves = (int32_t*)((char*)nmov.p + kHead);
        HIPTRY(hipMemsetAsync(nmov.p, 0, kHead, sm));
        HIPTRY(hipEventRecord(c->ev0, sm));
        const int wgs1 = cdiv((int64_t)P + 1, 256);
        BLANCE_LAUNCH(k_plan_moves<false>, wgs1 < kPlanMovesMaxWgs ? wgs1 : kPlanMovesMaxWgs, 256, sizeof(int) * 5 * 4, sm, q);
        const bool scanned = !count_only || o.op_off;
        if (scanned) SCANTRY(P + 1, q.n_moves);
        if (count_only) HIPTRY(hipEventRecord(c->ev1, sm));
        // the one host round trip: the total sizes the download, the six counter words come with it
        int32_t total = 0;
        unsigned long long lines[6 * kPlanMovesCounterStride];
        HIPTRY(read_back(c, lines, q.counters, sizeof lines));
        if (scanned) HIPTRY(read_back(c, &total, q.n_moves + P, sizeof total));
        HIPTRY(stream_sync(c));
        HIPTRY(hipGetLastError());
        for (int k = 0; k < 6; k++) cnt[k] = lines[k * kPlanMovesCounterStride];
        if (cnt[0] > (unsigned long long)INT32_MAX) return fail(BLANCE_ERR_UNSUPPORTED, "more than 2^31 moves");
        if (scanned && (unsigned long long)total != cnt[0]) return fail(BLANCE_ERR_DEVICE, "k_plan_moves: the counts and the counters disagree");
        if (!count_only && (int64_t)cnt[0] > o.capacity) {
            mv->n_moves = (int64_t)cnt[0];
            for (int k = 0; k < 4; k++) mv->n_by_kind[k] = (int64_t)cnt[1 + k];
            mv->n_parts_moved = (int64_t)cnt[5];
            return fail(BLANCE_ERR_CAPACITY, "moves capacity too small");
        }
        Mover down(c, false);
        c->stage.used = 0;
        if (!count_only) {
            const size_t n = (size_t)cnt[0];
            if (cnode.reserve(sizeof(int32_t) * (n + 1)) || cstate.reserve(sizeof(int32_t) * (n + 1)) || ckind.reserve(sizeof(int32_t) * (n + 1)))
                return fail(BLANCE_ERR_DEVICE, "hipMalloc failed");
            q.op_node = cnode.as<int32_t>(); q.op_state = cstate.as<int32_t>(); q.op_kind = ckind.as<int32_t>();
            if (n) BLANCE_LAUNCH_NOSYNC(k_plan_moves<true>, cdiv(P, 256), 256, 0, sm, q);
            HIPTRY(hipEventRecord(c->ev1, sm));
            if (n && ((e = down.copy(o.op_node, cnode.p, sizeof(int32_t) * n)) || (e = down.copy(o.op_state, cstate.p, sizeof(int32_t) * n)) ||
                      (e = down.copy(o.op_kind, ckind.p, sizeof(int32_t) * n))))
                return e;
        }
        if (o.op_off && (e = down.copy(o.op_off, q.n_moves, sizeof(int32_t) * ((size_t)P + 1)))) return e;
        if ((e = down.finish())) return e;
        HIPTRY(stream_sync(c));
        HIPTRY(hipGetLastError());
        HIPTRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    } else if (o.op_off) {
        o.op_off[0] = 0;
    }
    o.device_ms = ms;
    mv->n_moves = (int64_t)cnt[0];
    for (int k = 0; k < 4; k++) mv->n_by_kind[k] = (int64_t)cnt[1 + k];
    mv->n_parts_moved = (int64_t)cnt[5];
    return BLANCE_OK;
}

extern "C" int64_t blance_plan_moves_capacity(const blance_problem* pb, const blance_plan_moves* mv) {
    return moves_capacity(pb, mv ? mv->beg_other_off : nullptr);
}

extern "C" int blance_plan_moves_get(blance_ctx* c, blance_plan_moves* mv) {
    return enter(c, [&]() -> int {
        if (!mv) return fail(BLANCE_ERR_BAD_ARG, "null argument");
        return plan_moves_locked(c, mv);
    });
}

// ---- the planned map as PartitionMap JSON bytes (blance_plan_wire_names / blance_plan_wire_get)

// What a caller is told of a failure of host/wire_names.hpp, where all the tables of the four entry points are made.  The
// encoder's two (blance_plan_wire_names, blance_batch_names_create) and the dictionaries' two (blance_wire_dict_create,
// blance_batch_dict_create) word a negative count and the 2^31 bytes differently; kDupNode comes from the dictionaries alone.
enum class WireSide { kEncoder, kDict };
static int wire_fail(WireErr e, WireSide side) {
    const bool enc = side == WireSide::kEncoder;
    switch (e) {
    case WireErr::kNone: return BLANCE_OK;
    case WireErr::kNegativeSize: return fail(BLANCE_ERR_BAD_ARG, enc ? "negative size" : "negative count");
    case WireErr::kTooManyLists: return fail(BLANCE_ERR_BAD_ARG, "n_parts * n_states of 2^31 - 1 or more");
    case WireErr::kNullOffsets: return fail(BLANCE_ERR_BAD_ARG, "null offsets");
    case WireErr::kFirstOffset: return fail(BLANCE_ERR_BAD_ARG, "name offsets must start at 0");
    case WireErr::kNotMonotone: return fail(BLANCE_ERR_BAD_ARG, "name offsets not monotone");
    case WireErr::kNullBytes: return fail(BLANCE_ERR_BAD_ARG, "null name bytes");
    case WireErr::kDupPartition:
        return fail(BLANCE_ERR_UNSUPPORTED, "two partitions with one name (the reference's map would keep one of them)");
    case WireErr::kDupNode: return fail(BLANCE_ERR_BAD_ARG, "two nodes with one name");
    case WireErr::kDupState: return fail(BLANCE_ERR_BAD_ARG, "two states with one name");
    case WireErr::kTooLong:
        return fail(BLANCE_ERR_UNSUPPORTED, enc ? "the escaped names take 2^31 bytes or more" : "names of 2^31 bytes or more");
    }
    return fail(BLANCE_ERR_BAD_ARG, "unknown failure of the names");
}

static int wire_tables_upload_locked(blance_ctx* c, const WireTables& t) {
    HIPTRY(hipSetDevice(c->device));
    c->wire_names = false;                               // (the buffers are written again from here on)
    Mover up(c, true);
    c->stage.used = 0;                                   // (the stream is idle between calls)
    int e = 0;
    WireOutBufs& w = c->wire;
    const struct { DevBuf& buf; const WireTable& tab; } pairs[8] = {
        {w.order, t.order}, {w.part_esc, t.part_esc}, {w.part_off, t.part_off}, {w.node_esc, t.node_esc},
        {w.node_off, t.node_off}, {w.state_esc, t.state_esc}, {w.state_off, t.state_off}, {w.state_id, t.state_id}};
    for (const auto& x : pairs) {
        if (x.buf.reserve(x.tab.bytes + 16)) return fail(BLANCE_ERR_DEVICE, "hipMalloc failed");
        if ((e = up.copy(x.buf.p, x.tab.p, x.tab.bytes))) return e;
    }
    if ((e = up.flush())) return e;
    HIPTRY(stream_sync(c));                              // nothing of this frame is read after the call
    HIPTRY(hipGetLastError());
    c->wire_names = true;
    return BLANCE_OK;
}

static int wire_names_locked(blance_ctx* c, const blance_wire_names* nm) {
    if (!c->uploaded) return fail(BLANCE_ERR_BAD_ARG, "no problem on the context (blance_upload or blance_plan first)");
    const blance_problem& h = c->h;
    WirePrepared w;
    if (int st = wire_fail(wire_prepare(nm, h.n_parts, h.n_nodes_ext, h.n_states, w), WireSide::kEncoder)) return st;
    return wire_tables_upload_locked(c, wire_tables_of(w));
}

extern "C" int blance_plan_wire_names(blance_ctx* c, const blance_wire_names* nm) {
    return enter(c, [&]() -> int {
        if (!nm) return fail(BLANCE_ERR_BAD_ARG, "null argument");
        return wire_names_locked(c, nm);
    });
}

static int plan_wire_locked(blance_ctx* c, char* buf, size_t cap, size_t* need, double* device_ms) {
    if (!c->planned) return fail(BLANCE_ERR_BAD_ARG, "nothing planned yet");
    if (c->stats.iterations == 0) return fail(BLANCE_ERR_BAD_ARG, "the plan made no sweep (max_iterations <= 0): there is no map to encode");
    if (!c->wire_names) return fail(BLANCE_ERR_BAD_ARG, "no names set for the problem the context holds (blance_plan_wire_names)");
    const bool size_only = !buf && cap == 0;
    const blance_problem& h = c->h;
    const int P = h.n_parts;
    float ms = 0.f;
    if (P == 0) {                                        // json.Marshal of an empty, non-nil map
        *need = 2;
        if (!size_only) {
            if (cap < 2) return fail(BLANCE_ERR_CAPACITY, "the caller's buffer is too small (see *need)");
            memcpy(buf, "{}", 2);
        }
        if (device_ms) *device_ms = 0.0;
        return BLANCE_OK;
    }
    HIPTRY(hipSetDevice(c->device));
    hipStream_t sm = c->stream;
    constexpr size_t kHead = 256;                        // the 64-bit total on a cache line of its own, in front of len [P + 1]
    WireOutBufs& w = c->wire;
    DevBuf &wlen = w.len, &wdoc = w.doc;
    if (wlen.reserve(kHead + sizeof(int32_t) * ((size_t)P + 2))) return fail(BLANCE_ERR_DEVICE, "hipMalloc failed");
    const DevProblem d = result_problem(c);
    PlanWireParams q;
    memset(&q, 0, sizeof q);
    q.P = P; q.M = h.n_states; q.L = d.L; q.NX = h.n_nodes_ext;
    q.order = w.order.as<int32_t>();
    q.part_esc = w.part_esc.as<char>(); q.part_off = w.part_off.as<int32_t>();
    q.node_esc = w.node_esc.as<char>(); q.node_off = w.node_off.as<int32_t>();
    q.state_esc = w.state_esc.as<char>(); q.state_off = w.state_off.as<int32_t>(); q.state_id = w.state_id.as<int32_t>();
    q.lists = d.live; q.list_len = d.live_len; q.list_kind = d.live_kind;
    q.total = wlen.as<unsigned long long>();
    q.len = (int32_t*)((char*)wlen.p + kHead);
    q.stage = c->wire_stage;
    HIPTRY(hipMemsetAsync(wlen.p, 0, kHead, sm));
    HIPTRY(hipEventRecord(c->ev0, sm));
    const int wgs1 = cdiv((int64_t)P + 1, 256);
    const size_t lds1 = (((size_t)q.NX * 4 + 15) & ~(size_t)15) + sizeof(unsigned long long) * 256;
    BLANCE_LAUNCH(k_wire_size, wgs1 < kWireMaxWgs ? wgs1 : kWireMaxWgs, 256, lds1, sm, q);
    SCANTRY(P + 1, q.len);
    if (size_only) HIPTRY(hipEventRecord(c->ev1, sm));
    // the one host round trip: the total sizes the document; the scan's last offset is checked against it
    unsigned long long total = 0;
    int32_t scanned = 0;
    HIPTRY(read_back(c, &total, q.total, sizeof total));
    HIPTRY(read_back(c, &scanned, q.len + P, sizeof scanned));
    HIPTRY(stream_sync(c));
    HIPTRY(hipGetLastError());
    if (total > (unsigned long long)INT32_MAX) return fail(BLANCE_ERR_UNSUPPORTED, "a document of 2^31 bytes or more");
    if ((unsigned long long)scanned != total) return fail(BLANCE_ERR_DEVICE, "k_wire_size: the lengths and the total disagree");
    *need = (size_t)total;
    if (!size_only) {
        if (cap < (size_t)total) return fail(BLANCE_ERR_CAPACITY, "the caller's buffer is too small (see *need)");
        if (wdoc.reserve((size_t)total + 16)) return fail(BLANCE_ERR_DEVICE, "hipMalloc failed");
        q.doc = wdoc.as<char>();
        BLANCE_LAUNCH(k_wire_write, cdiv(P, kWireRun), kWireRun, (size_t)q.stage, sm, q);
        HIPTRY(hipEventRecord(c->ev1, sm));
        Mover down(c, false);
        c->stage.used = 0;
        int e = 0;
        if ((e = down.copy(buf, wdoc.p, (size_t)total))) return e;
        if ((e = down.finish())) return e;
    }
    HIPTRY(stream_sync(c));
    HIPTRY(hipGetLastError());
    HIPTRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    if (device_ms) *device_ms = ms;
    return BLANCE_OK;
}

extern "C" int blance_plan_wire_get(blance_ctx* c, char* buf, size_t cap, size_t* need, double* device_ms) {
    return enter(c, [&]() -> int {
        if (!need || (!buf && cap)) return fail(BLANCE_ERR_BAD_ARG, "null argument");
        return plan_wire_locked(c, buf, cap, need, device_ms);
    });
}

// ---- a PartitionMap document decoded on the device (blance_wire_dict_create / blance_wire_decode_device)
// the tables as a dictionary of the context
static int wire_dict_upload_locked(blance_ctx* c, const WdHostTables& t, blance_wire_dict** out) {
    std::unique_ptr<blance_wire_dict> d(new blance_wire_dict());
    d->owner = c;
    for (int k = 0; k < 3; k++) { d->n[k] = t.n[k]; d->mask[k] = t.mask[k]; }
    HIPTRY(hipSetDevice(c->device));
    Mover up(c, true);
    c->stage.used = 0;                                   // (the stream is idle between calls)
    int e = 0;
    for (int k = 0; k < 3; k++) {
        const size_t nb = (size_t)t.off32[k][(size_t)t.n[k]];
        if (d->slots[k].reserve(sizeof(int32_t) * t.slots[k].size()) || d->bytes[k].reserve(nb + 16) ||
            d->off[k].reserve(sizeof(int32_t) * t.off32[k].size()))
            return fail(BLANCE_ERR_DEVICE, "hipMalloc failed");
        if ((e = up.copy(d->slots[k].p, t.slots[k].data(), sizeof(int32_t) * t.slots[k].size()))) return e;
        if ((e = up.copy(d->bytes[k].p, t.bytes[k], nb))) return e;
        if ((e = up.copy(d->off[k].p, t.off32[k].data(), sizeof(int32_t) * t.off32[k].size()))) return e;
    }
    if ((e = up.flush())) return e;
    HIPTRY(stream_sync(c));                              // nothing of this frame is read after the call
    HIPTRY(hipGetLastError());
    c->wd_dicts.push_back(d.get());
    *out = d.release();
    return BLANCE_OK;
}

static int wire_dict_locked(blance_ctx* c, const blance_wire_names* nm, int32_t P, int32_t NX, int32_t M, blance_wire_dict** out) {
    WdHostTables t;
    const int e = wire_fail(wd_host_tables(nm, P, NX, M, t), WireSide::kDict);
    return e ? e : wire_dict_upload_locked(c, t, out);
}

extern "C" int blance_wire_dict_create(blance_ctx* c, const blance_wire_names* nm, int32_t n_parts, int32_t n_nodes_ext,
                                       int32_t n_states, blance_wire_dict** out) {
    return enter(c, [&]() -> int {
        if (!nm || !out) return fail(BLANCE_ERR_BAD_ARG, "null argument");
        *out = nullptr;
        return wire_dict_locked(c, nm, n_parts, n_nodes_ext, n_states, out);
    });
}

extern "C" void blance_wire_dict_destroy(blance_ctx* c, blance_wire_dict* d) {
    if (!c || !d) return;
    (void)enter(c, [&]() -> int {
        auto it = std::find(c->wd_dicts.begin(), c->wd_dicts.end(), d);
        if (it == c->wd_dicts.end()) return BLANCE_OK;   // not one of this context's
        c->wd_dicts.erase(it);
        (void)hipSetDevice(c->device);
        if (c->stream) (void)hipStreamSynchronize(c->stream);
        delete d;
        return BLANCE_OK;
    });
}

// what a decode says of its document before it has looked
static void wire_lists_reset(blance_wire_lists* out) {
    out->n_node_refs = out->n_parts_seen = 0;
    out->refusal = 0; out->refusal_at = -1;
    out->device_ms = out->total_ms = 0.0;
}

// The decoder's device part: the record split, both parse passes, the decoded CSR left in c->wd (part_kind, off, kind,
// nodes) -- blance_wire_decode_device downloads it from there, blance_wire_adopt makes it the problem's lists.
// The counters, the refusal and the first pass's device_ms go to `out`; its arrays are not touched.  count_only: pass 1
// alone; check_capacity: out->capacity below the entries ends the call before pass 2.  On BLANCE_OK behind pass 2 the
// stream is idle and c->ev0 .. c->ev1 span the kernels.
static int wire_decode_device_part(blance_ctx* c, const blance_wire_dict* d, const char* json, size_t len, blance_wire_lists* out,
                                   bool count_only, bool check_capacity) {
    wire_lists_reset(out);
    if (len > (size_t)INT32_MAX) {                       // before anything is launched
        out->refusal = kWdDocumentTooLong; out->refusal_at = 0;
        return fail(BLANCE_ERR_UNSUPPORTED, "refused: a document of 2^31 bytes or more");
    }
    const int P = d->n[0], NX = d->n[1], M = d->n[2];
    const int64_t PM = (int64_t)P * M;
    HIPTRY(hipSetDevice(c->device));
    hipStream_t sm = c->stream;
    WireDecodeParams q;
    memset(&q, 0, sizeof q);
    q.len = (int32_t)len;
    q.tile = c->wd_tile;
    q.n_tiles = cdiv((int64_t)len, q.tile);
    q.P = P; q.NX = NX; q.M = M; q.stage = c->wd_stage;
    const size_t nt = (size_t)q.n_tiles;
    WireInBufs& w = c->wd;
    if (w.doc.reserve(len + 2 * kWdPad) || w.tb.reserve(4 * (nt + 1)) || w.qbits.reserve(nt * (size_t)q.tile / 8 + 16) ||
        w.quotes.reserve(4 * (nt + 2)) || w.depth.reserve(4 * (nt + 2)) || w.count.reserve(4 * (nt + 2)) ||
        w.claim.reserve(4 * ((size_t)P + 1)) || w.part_kind.reserve((size_t)P + 1) || w.kind.reserve((size_t)PM + 1) ||
        w.off.reserve(4 * ((size_t)PM + 2)) || w.refusal.reserve(256))
        return fail(BLANCE_ERR_DEVICE, "hipMalloc failed");
    q.doc = w.doc.as<unsigned char>();
    q.tb = w.tb.as<int32_t>(); q.qbits = w.qbits.as<uint32_t>();
    q.quotes = w.quotes.as<int32_t>(); q.depth = w.depth.as<int32_t>(); q.count = w.count.as<int32_t>();
    q.claim = w.claim.as<int32_t>(); q.part_kind = w.part_kind.as<uint8_t>(); q.kind = w.kind.as<uint8_t>();
    q.off = w.off.as<int32_t>(); q.refusal = w.refusal.as<unsigned long long>();
    const blance_wire_dict& dd = *d;
    WdTable* tabs[3] = {&q.part, &q.node, &q.state};
    for (int k = 0; k < 3; k++)
        *tabs[k] = WdTable{dd.slots[k].as<int32_t>(), dd.mask[k], dd.bytes[k].as<unsigned char>(), dd.off[k].as<int32_t>()};
    int e = 0;
    {
        Mover up(c, true);
        c->stage.used = 0;                               // (the stream is idle between calls)
        if ((e = up.copy(w.doc.p, json, len))) return e;
        if ((e = up.flush())) return e;
    }
    HIPTRY(hipMemsetAsync(w.claim.p, 0, 4 * ((size_t)P + 1), sm));
    HIPTRY(hipMemsetAsync(w.part_kind.p, 0, (size_t)P + 1, sm));
    HIPTRY(hipMemsetAsync(w.kind.p, 0, (size_t)PM + 1, sm));
    HIPTRY(hipMemsetAsync(w.off.p, 0, 4 * ((size_t)PM + 2), sm));
    HIPTRY(hipMemsetAsync(w.refusal.p, 0xFF, 8, sm));
    HIPTRY(hipEventRecord(c->ev0, sm));
    // stage 1: the record starts (a hint: k_wire_decode.h)
    int32_t R = 0;
    if (q.n_tiles > 0) {
        const int wgs = cdiv(q.n_tiles, 256);
        BLANCE_LAUNCH_NOSYNC(k_wd_tail, wgs, 256, 0, sm, q);
        BLANCE_LAUNCH_NOSYNC(k_wd_quotes, wgs, 256, 0, sm, q);
        SCANTRY(q.n_tiles + 1, q.quotes);
        BLANCE_LAUNCH_NOSYNC(k_wd_walk<0>, wgs, 256, 0, sm, q);
        SCANTRY(q.n_tiles + 1, q.depth);
        BLANCE_LAUNCH_NOSYNC(k_wd_walk<1>, wgs, 256, 0, sm, q);
        SCANTRY(q.n_tiles + 1, q.count);
        HIPTRY(read_back(c, &R, q.count + q.n_tiles, sizeof R));
        HIPTRY(stream_sync(c));
        HIPTRY(hipGetLastError());
        if (R < 0 || (size_t)R > len) return fail(BLANCE_ERR_DEVICE, "k_wd_walk: a record count outside the document");
        if (w.rec.reserve(4 * ((size_t)R + 1))) return fail(BLANCE_ERR_DEVICE, "hipMalloc failed");
        q.rec = w.rec.as<int32_t>();
        if (R > 0) BLANCE_LAUNCH_NOSYNC(k_wd_walk<2>, wgs, 256, 0, sm, q);
    }
    q.R = R;
    // stage 2, pass 1: every record parsed strictly; kinds and list lengths
    const int wgs2 = R > 0 ? cdiv(R, kWdRun) : 1;
    BLANCE_LAUNCH(k_wd_parse<false>, wgs2, kWdRun, (size_t)q.stage, sm, q);
    SCANTRY((int)(PM + 1), q.off);
    HIPTRY(hipEventRecord(c->ev1, sm));                  // (recorded again behind pass 2)
    unsigned long long refusal = 0;
    int32_t total = 0;
    HIPTRY(read_back(c, &refusal, q.refusal, sizeof refusal));
    HIPTRY(read_back(c, &total, q.off + PM, sizeof total));
    HIPTRY(stream_sync(c));
    HIPTRY(hipGetLastError());
    float ms = 0.f;
    HIPTRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    out->device_ms = ms;                                 // stage 1 and pass 1: all there is of a count, a refusal, a capacity error
    if (refusal != ~0ull) {
        out->refusal = (int32_t)(refusal & 255u);
        out->refusal_at = (int64_t)(refusal >> 8);
        return fail(BLANCE_ERR_UNSUPPORTED, "refused: the document is outside what the device decodes (reason %s%ld: BLANCE_WIRE_REFUSED_*)",
                    "", (long)out->refusal);             // (fail() formats a string, then a number)
    }
    if (total < 0) return fail(BLANCE_ERR_DEVICE, "k_wd_parse: the list lengths overflow");
    out->n_node_refs = total;
    out->n_parts_seen = R;
    if (count_only) return BLANCE_OK;
    if (check_capacity && out->capacity < (int64_t)total) return fail(BLANCE_ERR_CAPACITY, "the caller's nodes array is too small (see n_node_refs)");
    // pass 2: the node ids
    if (w.nodes.reserve(4 * ((size_t)total + 1))) return fail(BLANCE_ERR_DEVICE, "hipMalloc failed");
    q.nodes = w.nodes.as<int32_t>();
    if (total > 0) BLANCE_LAUNCH(k_wd_parse<true>, wgs2, kWdRun, (size_t)q.stage, sm, q);
    HIPTRY(hipEventRecord(c->ev1, sm));
    unsigned long long again = 0;
    HIPTRY(read_back(c, &again, q.refusal, sizeof again));
    HIPTRY(stream_sync(c));
    HIPTRY(hipGetLastError());
    if (again != ~0ull) return fail(BLANCE_ERR_DEVICE, "k_wd_parse: the two passes disagree");
    return BLANCE_OK;
}

static int wire_decode_locked(blance_ctx* c, const blance_wire_dict* d, const char* json, size_t len, blance_wire_lists* out) {
    wire_lists_reset(out);
    if (std::find(c->wd_dicts.begin(), c->wd_dicts.end(), d) == c->wd_dicts.end())
        return fail(BLANCE_ERR_BAD_ARG, "the dictionary is not one of this context's");
    if (out->capacity < 0 || (!out->nodes && out->capacity > 0)) return fail(BLANCE_ERR_BAD_ARG, "nodes NULL with a capacity, or a negative capacity");
    const bool count_only = !out->nodes && out->capacity == 0;
    if (!count_only && (!out->part_kind || !out->off || !out->kind)) return fail(BLANCE_ERR_BAD_ARG, "part_kind, off or kind NULL");
    int e = wire_decode_device_part(c, d, json, len, out, count_only, true);
    if (e || count_only) return e;
    const int P = d->n[0], M = d->n[2];
    const int64_t PM = (int64_t)P * M;
    const int64_t total = out->n_node_refs;
    {   // the download
        Mover down(c, false);
        c->stage.used = 0;
        if ((e = down.copy(out->part_kind, c->wd.part_kind.p, (size_t)P))) return e;
        if ((e = down.copy(out->off, c->wd.off.p, 4 * ((size_t)PM + 1)))) return e;
        if ((e = down.copy(out->kind, c->wd.kind.p, (size_t)PM))) return e;
        if ((e = down.copy(out->nodes, c->wd.nodes.p, 4 * (size_t)total))) return e;
        if ((e = down.finish())) return e;
    }
    HIPTRY(stream_sync(c));
    HIPTRY(hipGetLastError());
    float ms = 0.f;
    HIPTRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    out->device_ms = ms;
    return BLANCE_OK;
}

extern "C" int blance_wire_decode_device(blance_ctx* c, const blance_wire_dict* d, const char* json, size_t len, blance_wire_lists* out) {
    return enter(c, [&]() -> int {
        if (!d || !out || (!json && len)) return fail(BLANCE_ERR_BAD_ARG, "null argument");
        const auto t0 = std::chrono::steady_clock::now();
        const int st = wire_decode_locked(c, d, json, len, out);
        out->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();   // whatever the status
        return st;
    });
}

// ---- blance_wire_adopt: the decoder's device part, k_wire_adopt_sum with one more round trip for its
// summary words, the refusals -- and only then adopt_swap, whose write kernel reads the decoded CSR where the decoder left it.
static int wire_adopt_locked(blance_ctx* c, struct blance_wire_adopt* wa) {
    wa->refusal = 0; wa->refusal_at = -1;
    wa->n_node_refs = wa->n_parts_seen = wa->result_capacity = 0;
    wa->why = 0; wa->why_at = -1;
    wa->device_ms = wa->total_ms = 0.0;
    const blance_wire_dict* d = wa->dict;
    if (!d || (!wa->json && wa->len) || !wa->node_removed || !wa->node_added) return fail(BLANCE_ERR_BAD_ARG, "null argument");
    for (int32_t r : wa->reserved) if (r) return fail(BLANCE_ERR_BAD_ARG, "blance_wire_adopt::reserved must be zero");
    if (std::find(c->wd_dicts.begin(), c->wd_dicts.end(), d) == c->wd_dicts.end())
        return fail(BLANCE_ERR_BAD_ARG, "the dictionary is not one of this context's");
    if (!c->uploaded) return fail(BLANCE_ERR_BAD_ARG, "the context holds no problem (blance_upload first)");
    const blance_problem& h = c->h;
    const int NX = h.n_nodes_ext, M = h.n_states, P = h.n_parts;
    if (d->n[0] != P || d->n[1] != NX || d->n[2] != M)
        return fail(BLANCE_ERR_BAD_ARG, "the dictionary's sizes are not those of the problem the context holds");
    if (int st = comm_refuse(c, "blance_wire_adopt")) return st;
    HIPTRY(hipSetDevice(c->device));
    const int64_t PM = (int64_t)P * M;
    const bool keep = wa->keep_prev_only != 0, assign_too = wa->assign_too != 0;
    hipStream_t sm = c->stream;
    if (c->side_pending) { HIPTRY(hipStreamSynchronize(c->side)); c->side_pending = false; }

    blance_wire_lists wl;
    memset(&wl, 0, sizeof wl);
    int st = wire_decode_device_part(c, d, wa->json, wa->len, &wl, false, false);
    wa->refusal = wl.refusal; wa->refusal_at = wl.refusal_at;
    wa->n_node_refs = wl.n_node_refs; wa->n_parts_seen = wl.n_parts_seen;
    wa->device_ms = wl.device_ms;
    if (st) return st;
    const int64_t total = wl.n_node_refs;

    // the summary of the lists where they lie
    WireAdoptParams ap;
    memset(&ap, 0, sizeof ap);
    ap.P = P; ap.M = M; ap.L = c->L; ap.weights_nil = h.partition_weights_nil; ap.assign_too = assign_too ? 1 : 0;
    for (int m = 0; m < M; m++) ap.k[m] = c->state_constraints[m];
    ap.part_kind = c->wd.part_kind.as<uint8_t>(); ap.off = c->wd.off.as<int32_t>();
    ap.kind = c->wd.kind.as<uint8_t>(); ap.nodes = c->wd.nodes.as<int32_t>();
    ap.cur_a_off = c->a_off.as<int32_t>(); ap.cur_a_kind = c->a_kind.as<uint8_t>();
    ap.part_weight = c->part_weight.as<int32_t>(); ap.part_has_weight = c->part_has_weight.as<uint8_t>();
    RESERVE(wire_adopt_res, sizeof(int32_t) * kWireAdoptResWords);
    ap.res = c->wire_adopt_res.as<int32_t>();
    int32_t vr[kWireAdoptResWords] = {0};
    vr[kWaResFirstLong] = vr[kWaResFirstMissing] = vr[kWaResFirstDup] = INT_MAX;
    if (PM > 0 || P > 0) {
        {
            Mover up(c, true);
            c->stage.used = 0;                           // (the stream is idle here)
            if ((st = up.copy(ap.res, vr, sizeof vr))) return st;
            if ((st = up.flush())) return st;
        }
        const int wgs = cdiv(PM > P ? PM : P, 256);
        BLANCE_LAUNCH(k_wire_adopt_sum, wgs < kWireAdoptMaxWgs ? wgs : kWireAdoptMaxWgs, 256, 4 * 9 * sizeof(unsigned long long), sm, ap);
        HIPTRY(hipEventRecord(c->ev1, sm));
        HIPTRY(read_back(c, vr, ap.res, sizeof vr));
        HIPTRY(stream_sync(c));
        HIPTRY(hipGetLastError());
        float ms = 0.f;
        HIPTRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
        wa->device_ms = ms;
    }
    const UploadSummary sum = adopt_summary(c, vr, kWaSummary);

    // the refusals: all of them before the problem is touched
    auto refuse = [&](int why, int64_t at, const char* text) {
        wa->why = why; wa->why_at = at;
        return fail(BLANCE_ERR_UNSUPPORTED, "refused: %s (BLANCE_WIRE_ADOPT_* %ld)", text, (long)why);
    };
    bool any_removed = false, any_pass = false;
    for (int n = 0; n < NX; n++) any_removed |= wa->node_removed[n] != 0;
    for (int32_t k : c->state_constraints) any_pass |= k > 0;
    if (vr[kWaResFirstLong] != INT_MAX)
        return refuse(BLANCE_WIRE_ADOPT_LIST_TOO_LONG, vr[kWaResFirstLong], "a list longer than the uploaded problem's longest: upload again");
    // (what the batch refuses too, in that order: host/batch_layout.hpp)
    const AdoptRefusal rf = adopt_refusal(assign_too, vr[kWaResFirstMissing], vr[kWaResFirstDup], any_removed, any_pass,
                                          adopt_load_overflows(c, sum.ps, keep));
    switch (rf.why) {
    case BLANCE_WIRE_ADOPT_PARTITION_MISSING: return refuse(rf.why, rf.at, "a partition to assign is not in the document");
    case BLANCE_WIRE_ADOPT_DUPLICATE_NODE: return refuse(rf.why, rf.at, "a node twice in a list to assign");
    case BLANCE_WIRE_ADOPT_REMOVED_WITHOUT_PREV:
        return refuse(rf.why, rf.at, "nodesToRemove non-empty but a partition is missing from prevMap (plan.go:545)");
    case BLANCE_WIRE_ADOPT_LOAD_OVERFLOW: return refuse(rf.why, rf.at, "partition weights overflow the int32 load tables");
    }

    blance_problem q = adopt_shell(c, wa->node_removed, wa->node_added, wa->nodes_to_add_nil);
    q.n_prev = (int32_t)wl.n_parts_seen + (keep ? c->np_later - P : 0);   // (np_later - P: the old prevMap's keys outside partitionsToAssign)
    q.n_loads = keep ? h.n_loads : 0;
    ap.a_off = c->a_off.as<int32_t>(); ap.a_kind = c->a_kind.as<uint8_t>();
    ap.p_off = c->p_off.as<int32_t>(); ap.p_kind = c->p_kind.as<uint8_t>();
    ap.part_in_prev = c->part_in_prev.as<uint8_t>(); ap.part_never_equal = c->part_never_equal.as<uint8_t>();
    st = adopt_swap(c, q, sum, keep, assign_too ? total : -1, total, [&]() -> int {
        ap.a_nodes = c->a_nodes.as<int32_t>(); ap.p_nodes = c->p_nodes.as<int32_t>();
        BLANCE_LAUNCH_NOSYNC(k_wire_adopt_write, wire_adopt_write_wgs(P, M, total), 256, 0, sm, ap);
        HIPTRY(hipEventRecord(c->ev1, sm));
        return BLANCE_OK;
    });
    if (st) return st;
    float ms = 0.f;
    HIPTRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    wa->device_ms = ms;
    wa->result_capacity = sum.ps.cap;
    return BLANCE_OK;
}

extern "C" int blance_wire_adopt(blance_ctx* c, struct blance_wire_adopt* wa) {
    return enter(c, [&]() -> int {
        if (!wa) return fail(BLANCE_ERR_BAD_ARG, "null argument");
        const auto t0 = std::chrono::steady_clock::now();
        const int st = wire_adopt_locked(c, wa);
        wa->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();   // whatever the status
        return st;
    });
}

extern "C" int blance_download(blance_ctx* c, blance_result* res) {
    return enter(c, [&]() -> int { return download_locked(c, res); });
}

// upload, plan, download; total_ms is the device's time for all three
static int plan_whole_locked(blance_ctx* c, const blance_problem* pb, blance_result* res) {
    HIPTRY(hipSetDevice(c->device));
    struct Ev { hipEvent_t a = nullptr, b = nullptr; ~Ev() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); } } ev;
    HIPTRY(hipEventCreate(&ev.a));
    HIPTRY(hipEventCreate(&ev.b));
    HIPTRY(hipEventRecord(ev.a, c->stream));
    int st = upload_inner(c, pb);
    if (!st) st = plan_locked(c, res);
    if (!st) st = download_locked(c, res);
    if (st) return st;
    (void)hipEventRecord(ev.b, c->stream);
    (void)hipEventSynchronize(ev.b);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ev.a, ev.b);
    res->total_ms = ms;
    return BLANCE_OK;
}

extern "C" int blance_plan(blance_ctx* c, const blance_problem* pb, blance_result* res) {
    return enter(c, [&]() -> int {
        if (!res) return fail(BLANCE_ERR_BAD_ARG, "null result");
        return plan_whole_locked(c, pb, res);
    });
}

// ============================================================================
// blance_plan_batch: many small problems, one upload, one launch per size class (k_plan_batch, one workgroup per
// problem), one download.  Problems outside the batched envelope go through upload / plan / download one by one.
// The layout of the slices, the pack, the documents' verdict and the unpack are host/batch_layout.hpp's pure functions;
// BatchCall below is the call as a record with one step per stage.
// ============================================================================
namespace {
enum DocState : int8_t { kNoDoc, kDocToPlan, kDocRefused };  // kDocRefused: said in dc, nothing of the problem is written

// One problem of a batch call: what the caller passed for it -- NULL where the call has no such array or no entry for this
// problem: nothing behind BatchCall::check asks again -- and what the checks learnt.  The capacities are a document
// problem's bounds (blance_batch_doc_bounds), else the ordinary ones (blance_result_capacity, blance_batch_moves_capacity,
// blance_batch_wire_capacity); moves_cap and wire_cap only where mv / wr ask
struct BatchProblem {
    const blance_problem* pb = nullptr;
    blance_result* res = nullptr;
    blance_batch_moves* mv = nullptr;
    blance_plan_stats* ps = nullptr;
    blance_batch_wire* wr = nullptr;
    blance_batch_doc* dc = nullptr;
    int64_t result_cap = 0, moves_cap = 0;
    size_t wire_cap = 0;
    DocState doc = kNoDoc;
};

// the moves request of one problem: buffers, the beg_other CSR, the capacity
int batch_moves_check(BatchProblem& b) {
    const blance_problem* pb = b.pb;
    const blance_batch_moves* mv = b.mv;
    const blance_moves_result& o = mv->out;
    if (!o.op_off || !o.op_node || !o.op_state || !o.op_kind) return fail(BLANCE_ERR_BAD_ARG, "null moves buffers");
    if (!mv->beg_other_off != !mv->beg_other_nodes)
        return fail(BLANCE_ERR_BAD_ARG, "beg_other_off and beg_other_nodes: both or neither");
    if (pb->max_iterations <= 0) return fail(BLANCE_ERR_BAD_ARG, "moves asked for a problem with max_iterations <= 0 (no map)");
    if (int e = beg_other_check(mv->beg_other_off, mv->beg_other_nodes, pb->n_parts, pb->n_nodes_ext)) return e;
    if (!b.dc) b.moves_cap = blance_batch_moves_capacity(pb, mv);
    if (o.capacity < b.moves_cap) return fail(BLANCE_ERR_CAPACITY, "moves capacity too small");
    return BLANCE_OK;
}

// the result buffers of one (valid) problem and their capacities: with blance_validate, every check blance_plan would make
// before it writes a result
int batch_result_check(const BatchProblem& b) {
    const blance_problem* pb = b.pb;
    const blance_result* r = b.res;
    if (!r || !r->out_off || !r->out_nodes || !r->out_kind || !r->warn_part || !r->warn_state)
        return fail(BLANCE_ERR_BAD_ARG, "null result buffers");
    if (pb->max_iterations > 0) {
        int passes = 0;
        for (int m = 0; m < pb->n_states; m++) if (pb->state_constraints[m] > 0) passes++;
        if (r->out_capacity < b.result_cap) return fail(BLANCE_ERR_CAPACITY, "out_capacity too small");
        if (r->warn_capacity < (int64_t)pb->n_parts * passes) return fail(BLANCE_ERR_CAPACITY, "warn_capacity too small");
    }
    return BLANCE_OK;
}
}  // namespace

// the launches of a single-path reader over P > 0 partitions: its two kernels and between them the scan of P + 1 words
static int64_t reader_launches(int64_t P) { return 2 + (P + 1 <= 4 * kScanTile ? 1 : 3); }

// the moves of a problem the single path planned: blance_calc_moves's path on its prevMap lists (keys outside the model
// as pseudo state M) and its downloaded result
static int batch_moves_single(blance_ctx* c, const blance_problem* pb, const blance_result* r, blance_batch_moves* mv,
                              int64_t* launches) {
    const int P = pb->n_parts, M = pb->n_states;
    std::vector<int32_t> boff(1, 0), bnod, eoff(1, 0), enod;
    boff.reserve((size_t)P * (M + 1) + 1);
    eoff.reserve((size_t)P * (M + 1) + 1);
    bnod.reserve((size_t)pb->prev_off[(size_t)P * M] + (mv->beg_other_off ? mv->beg_other_off[P] : 0) + 1);
    enod.reserve((size_t)r->out_off[(size_t)P * M] + 1);       // (+ 1: data() is never NULL)
    for (int p = 0; p < P; p++) {
        for (int m = 0; m < M; m++) {
            const size_t idx = (size_t)p * M + m;
            bnod.insert(bnod.end(), pb->prev_nodes + pb->prev_off[idx], pb->prev_nodes + pb->prev_off[idx + 1]);
            boff.push_back((int32_t)bnod.size());
            enod.insert(enod.end(), r->out_nodes + r->out_off[idx], r->out_nodes + r->out_off[idx + 1]);
            eoff.push_back((int32_t)enod.size());
        }
        if (mv->beg_other_off)
            bnod.insert(bnod.end(), mv->beg_other_nodes + mv->beg_other_off[p], mv->beg_other_nodes + mv->beg_other_off[p + 1]);
        boff.push_back((int32_t)bnod.size());
        eoff.push_back((int32_t)enod.size());
    }
    blance_moves_problem q;
    q.n_parts = P; q.n_states = M; q.favor_min_nodes = mv->favor_min_nodes ? 1 : 0;
    q.beg_off = boff.data(); q.beg_nodes = bnod.data(); q.end_off = eoff.data(); q.end_nodes = enod.data();
    const int st = calc_moves_locked(c, &q, &mv->out);
    if (!st && P > 0) *launches += reader_launches(P);   // k_calc_moves, the scan, k_moves_compact
    return st;
}

extern "C" int64_t blance_batch_moves_capacity(const blance_problem* pb, const blance_batch_moves* mv) {
    return moves_capacity(pb, mv ? mv->beg_other_off : nullptr);
}

// ---- the prepared names of one index (blance_batch_names): wire_prepare's tables as one block of int32
// words (host/wire_names.hpp: NamesBlock), the block a batch copies behind a problem's packed input slice
struct blance_batch_names : NamesBlock {
    int32_t n_parts = 0, n_nodes_ext = 0, n_states = 0;
};

extern "C" int blance_batch_names_create(const blance_wire_names* names, int32_t n_parts, int32_t n_nodes_ext, int32_t n_states,
                                         blance_batch_names** out) {
    return guarded([&]() -> int {
        if (!names || !out) return fail(BLANCE_ERR_BAD_ARG, "null argument");
        std::unique_ptr<blance_batch_names> nm(new blance_batch_names);
        if (int st = wire_fail(names_block_build(names, n_parts, n_nodes_ext, n_states, *nm), WireSide::kEncoder)) return st;
        nm->n_parts = n_parts; nm->n_nodes_ext = n_nodes_ext; nm->n_states = n_states;
        *out = nm.release();
        return BLANCE_OK;
    });
}

extern "C" void blance_batch_names_destroy(blance_batch_names* nm) { delete nm; }

extern "C" size_t blance_batch_wire_capacity(const blance_problem* pb, const blance_batch_names* nm) {
    if (!pb || !nm || pb->n_parts < 0 || pb->n_states < 0) return 0;
    return batch_wire_cap_of(pb, *nm, blance_result_capacity(pb));
}

// ---- the dictionary of one index for blance_plan_batch_docs (blance_batch_dict): wd_host_tables' tables
// as one block of int32 words (host/wire_names.hpp: DictBlock), the block a batch copies behind a problem's packed input
// slice; `tables` is the same as blance_wire_dict_create wants it (the single path), its names in the block
struct blance_batch_dict : DictBlock {
    int32_t n_parts = 0, n_nodes_ext = 0, n_states = 0;
};

extern "C" int blance_batch_dict_create(const blance_wire_names* names, int32_t n_parts, int32_t n_nodes_ext, int32_t n_states,
                                        blance_batch_dict** out) {
    return guarded([&]() -> int {
        if (!names || !out) return fail(BLANCE_ERR_BAD_ARG, "null argument");
        *out = nullptr;
        std::unique_ptr<blance_batch_dict> d(new blance_batch_dict);
        if (int st = wire_fail(dict_block_build(names, n_parts, n_nodes_ext, n_states, *d), WireSide::kDict)) return st;
        d->n_parts = n_parts; d->n_nodes_ext = n_nodes_ext; d->n_states = n_states;
        *out = d.release();
        return BLANCE_OK;
    });
}

extern "C" void blance_batch_dict_destroy(blance_batch_dict* d) { delete d; }

extern "C" int blance_batch_doc_bounds(const blance_problem* pb, const blance_batch_doc* dc, const blance_batch_names* nm,
                                       int64_t* result_cap, int64_t* moves_cap, size_t* wire_cap) {
    if (!pb || !dc || !pb->state_constraints || pb->n_parts < 0 || pb->n_states < 0) return fail(BLANCE_ERR_BAD_ARG, "null argument");
    const DocBounds b = batch_doc_bounds(pb, dc->len, dc->assign_too != 0, nm, blance_result_capacity(pb));
    if (result_cap) *result_cap = b.result_cap;
    if (moves_cap) *moves_cap = b.moves_cap;
    if (wire_cap) *wire_cap = b.wire_cap;
    return BLANCE_OK;
}

namespace {
// the document request of one problem: the names object made for its sizes, the buffer, its capacity
int batch_wire_check(BatchProblem& b) {
    const blance_problem* pb = b.pb;
    const blance_batch_wire* wr = b.wr;
    if (!wr->names || !wr->buf) return fail(BLANCE_ERR_BAD_ARG, "null names or null document buffer");
    if (wr->names->n_parts != pb->n_parts || wr->names->n_nodes_ext != pb->n_nodes_ext || wr->names->n_states != pb->n_states)
        return fail(BLANCE_ERR_BAD_ARG, "the names were made for other sizes than the problem's");
    if (pb->max_iterations <= 0) return fail(BLANCE_ERR_BAD_ARG, "a document asked for a problem with max_iterations <= 0 (no map)");
    b.wire_cap = batch_wire_cap_of(pb, *wr->names, b.result_cap);
    if (wr->cap < b.wire_cap) return fail(BLANCE_ERR_CAPACITY, "document capacity too small");
    return BLANCE_OK;
}
}  // namespace

// the last error as that of problem i of a batch
static int fail_problem(int st, int i) {
    const std::string why = g_last_error;
    return fail(st, "problem %s", (std::to_string(i) + ": " + why).c_str());
}

// the arguments of a document problem that refuse the whole call (blance_plan_batch_docs)
static int batch_doc_check(const blance_problem* pb, const blance_batch_moves* mv, const blance_batch_doc* dc) {
    if (!dc->dict || (!dc->json && dc->len)) return fail(BLANCE_ERR_BAD_ARG, "null dictionary or null document");
    if (dc->dict->n_parts != pb->n_parts || dc->dict->n_nodes_ext != pb->n_nodes_ext || dc->dict->n_states != pb->n_states)
        return fail(BLANCE_ERR_BAD_ARG, "the dictionary was made for other sizes than the problem's");
    for (int32_t r : dc->reserved) if (r) return fail(BLANCE_ERR_BAD_ARG, "blance_batch_doc::reserved must be zero");
    if (mv && mv->beg_other_off) return fail(BLANCE_ERR_BAD_ARG, "beg_other with a document: its prevMap has no keys outside the model");
    if (pb->max_iterations <= 0) return fail(BLANCE_ERR_BAD_ARG, "a document for a problem with max_iterations <= 0 (no map)");
    return BLANCE_OK;
}

// A document problem's way to a problem the context holds, on the single path, from the original bytes: blance_upload(pb),
// a temporary dictionary of the context made from the batch dictionary's tables, blance_wire_adopt.  What the document
// decides goes to dc (*refused); any other failure is the call's.
static int batch_doc_adopt(blance_ctx* c, const blance_problem* pb, blance_batch_doc* dc, double* device_ms, bool* refused) {
    *refused = false;
    int st = upload_inner(c, pb);
    if (st) return st;
    blance_wire_dict* d = nullptr;
    if ((st = wire_dict_upload_locked(c, dc->dict->tables, &d))) return st;
    struct blance_wire_adopt wa;
    memset(&wa, 0, sizeof wa);
    wa.dict = d; wa.json = dc->json; wa.len = dc->len;
    wa.node_removed = pb->node_removed; wa.node_added = pb->node_added; wa.nodes_to_add_nil = pb->nodes_to_add_nil;
    wa.assign_too = dc->assign_too; wa.keep_prev_only = dc->keep_prev_only;
    st = wire_adopt_locked(c, &wa);
    c->wd_dicts.erase(std::find(c->wd_dicts.begin(), c->wd_dicts.end(), d));
    (void)hipStreamSynchronize(c->stream);
    delete d;
    dc->refusal = wa.refusal; dc->refusal_at = wa.refusal_at;
    dc->why = wa.why; dc->why_at = wa.why_at;
    dc->n_node_refs = wa.n_node_refs; dc->n_parts_seen = wa.n_parts_seen;
    *device_ms += wa.device_ms;
    if (st == BLANCE_ERR_UNSUPPORTED && (wa.refusal || wa.why)) {
        dc->status = BLANCE_ERR_UNSUPPORTED;
        *refused = true;
        return BLANCE_OK;
    }
    return st;
}

namespace {
struct Pinned {                                          // page-locked staging, freed with its owner
    void* p = nullptr;
    ~Pinned() { pin_free(p); }
    void release() { pin_free(p); p = nullptr; }
};

// One call of blance_plan_batch*, as run() reads: every step has one job and leaves what the later ones need in the record.
struct BatchCall {
    blance_ctx* c;
    blance_batch_info* info;
    const std::chrono::steady_clock::time_point t_start = std::chrono::steady_clock::now();
    std::vector<BatchProblem> pr;                        // check
    // classify: every 64-class item in call order, then every 256-class item; the single path's problems in the order they
    // are planned -- outside the envelope (call order), then a document's list too long (descriptor order, decode_round),
    // then what k_plan_batch did not finish (item order, collect)
    std::vector<BatchItem> items;
    std::vector<int> fallback;
    int n64 = 0;
    // lay_out
    std::vector<BatchMovesDesc> mds;
    std::vector<BatchStatsDesc> sds;
    std::vector<BatchWireDesc> wds;
    std::vector<BatchDocDesc> dds;
    std::vector<int> dd_item;                            // the item of every BatchDocDesc
    BatchHead head;
    int64_t in_words = 0, sc_words = 0, out_words = 0;
    size_t lds64 = 0, lds256 = 0, lds_stats = 0;
    size_t doc_cap = 0;                                  // the bounds of the documents to write, each rounded to 16 bytes
    size_t docs_in_bytes = 0;                            // the documents to decode, likewise
    // stage
    Pinned host, h_docs, h_sum, docs;
    char* h_in = nullptr;
    int32_t* h_out = nullptr;
    size_t in_bytes = 0, out_bytes = 0;
    BatchParams q;
    std::vector<size_t> doc_base;                        // collect: where every written document starts in docs
    // report
    int64_t launches = 0, steps = 0;
    double device_ms = 0.0;
    int n_refused_single = 0;

    BatchCall(blance_ctx* ctx, blance_batch_info* inf) : c(ctx), info(inf) {}

    int run(int32_t n, const blance_problem* const* pbs, blance_result* const* res, blance_batch_moves* const* mvs,
            blance_plan_stats* const* sts, blance_batch_wire* const* wrs, blance_batch_doc* const* dcs) {
        if (c->comm.n_ranks > 1 || c->rccl_comm) return fail(BLANCE_ERR_UNSUPPORTED, "blance_plan_batch on a context with a communicator");
        int st = check(n, pbs, res, mvs, sts, wrs, dcs);
        if (st) return st;
        HIPTRY(hipSetDevice(c->device));
        c->uploaded = false;                             // the context holds no problem after a batch
        c->planned = false;
        c->wire_names = false;
        classify();
        if (!items.empty()) {
            lay_out();
            if ((st = stage()) || (st = decode_round()) || (st = launch()) || (st = collect())) return st;
            unpack();
            docs.release(); h_sum.release(); h_docs.release(); host.release();
        }
        if ((st = single_path())) return st;
        report();
        return BLANCE_OK;
    }

    // every argument check of every problem, before anything runs: the first refusal is the call's
    int check(int32_t n, const blance_problem* const* pbs, blance_result* const* res, blance_batch_moves* const* mvs,
              blance_plan_stats* const* sts, blance_batch_wire* const* wrs, blance_batch_doc* const* dcs) {
        pr.resize((size_t)n);
        for (int i = 0; i < n; i++) {
            BatchProblem& b = pr[(size_t)i];
            b.pb = pbs[i]; b.res = res[i];
            b.mv = mvs ? mvs[i] : nullptr; b.ps = sts ? sts[i] : nullptr; b.wr = wrs ? wrs[i] : nullptr; b.dc = dcs ? dcs[i] : nullptr;
            int st = blance_validate(b.pb);
            if (!st && b.dc) st = batch_doc_check(b.pb, b.mv, b.dc);
            if (!st && b.dc) st = blance_batch_doc_bounds(b.pb, b.dc, nullptr, &b.result_cap, &b.moves_cap, nullptr);
            if (!st && !b.dc) b.result_cap = blance_result_capacity(b.pb);
            if (!st) st = batch_result_check(b);
            if (!st && b.mv) st = batch_moves_check(b);
            if (!st && b.ps) st = stats_arrays_check(b.ps, b.pb->n_states);
            if (!st && b.wr) st = batch_wire_check(b);
            if (st) return fail_problem(st, i);
        }
        return BLANCE_OK;
    }

    // which problems one launch plans: inside the batched envelope (batch_layout), its document inside the byte limits of a
    // call, its output document below 2^31 bytes; the rest goes the single path.  A document of 2^31 bytes or more is refused
    // here, before anything is launched, as blance_wire_decode_device refuses it.
    void classify() {
        constexpr size_t kBatchDocMaxLen = (size_t)1 << 28;  // (a longer document's record starts outgrow the int32 slice offsets)
        // ... and all documents decoded in one call stay below 2^31 bytes (their scratch is twice that): the excess, in call
        // order, goes the single path
        constexpr size_t kBatchDocsMaxBytes = (size_t)1 << 31;
        size_t docs_total = 0;
        std::vector<BatchItem> items256;
        for (size_t i = 0; i < pr.size(); i++) {
            BatchProblem& b = pr[i];
            if (b.dc) {
                blance_batch_doc* dc = b.dc;
                dc->status = BLANCE_OK;
                dc->refusal = 0; dc->refusal_at = -1; dc->why = 0; dc->why_at = -1;
                dc->n_node_refs = dc->n_parts_seen = 0;
                b.doc = kDocToPlan;
                if (dc->len > (size_t)INT32_MAX) {
                    dc->status = BLANCE_ERR_UNSUPPORTED;
                    dc->refusal = kWdDocumentTooLong; dc->refusal_at = 0;
                    b.doc = kDocRefused;
                    continue;
                }
            }
            BatchItem it;
            it.idx = (int)i;
            const size_t len = b.dc ? b.dc->len : 0;
            bool in_env = len <= kBatchDocMaxLen && docs_total + len <= kBatchDocsMaxBytes &&
                          batch_layout(b.pb, it, b.result_cap, b.dc != nullptr, b.dc ? batch_kept_loads(b.pb, b.dc->keep_prev_only != 0) : 0);
            if (in_env) docs_total += len;
            // (a document that may reach 2^31 bytes is the single path's to refuse: the batch's offsets are int32)
            if (in_env && b.wr && b.wire_cap > (size_t)INT32_MAX) in_env = false;
            if (!in_env) fallback.push_back((int)i);
            else (it.threads == 64 ? items : items256).push_back(it);
        }
        n64 = (int)items.size();
        items.insert(items.end(), items256.begin(), items256.end());
    }

    // the regions of what the batched problems ask for beside the plan, behind the plan's words of each slice: moves,
    // statistics, the document to write, the document to decode; then every slice's base and the descriptor header
    void lay_out() {
        for (int j = 0; j < (int)items.size(); j++) {
            BatchItem& it = items[(size_t)j];
            const BatchProblem& b = pr[(size_t)it.idx];
            if (b.mv) {
                it.mi = (int)mds.size();
                mds.push_back(batch_moves_regions(it, j, b.mv->favor_min_nodes != 0, b.mv->beg_other_off, b.moves_cap));
            }
            if (b.ps) {
                it.si = (int)sds.size();
                sds.push_back(batch_stats_regions(it, j));
                lds_stats = std::max(lds_stats, batch_stats_lds(it.d.M, it.d.NX));
            }
            if (b.wr && it.d.P > 0) {                    // (an empty map is written by the host)
                it.wi = (int)wds.size();
                wds.push_back(batch_wire_regions(it, j, (int64_t)b.wr->names->block.size(), b.wire_cap, doc_cap));
            }
            if (b.dc) {
                dd_item.push_back(j);
                dds.push_back(batch_doc_regions(it, j, b.dc->len, (int64_t)b.dc->dict->block.size(), b.dc->assign_too != 0, docs_in_bytes));
            }
            it.d.in_base = in_words; it.d.sc_base = sc_words; it.d.out_base = out_words;
            in_words += it.in_words; sc_words += it.sc_words; out_words += it.out_words;
            size_t& lds = it.threads == 64 ? lds64 : lds256;
            lds = std::max(lds, plan_batch_lds(it.threads, it.d.M, it.d.NX));
        }
        head = batch_head(items.size(), mds.size(), sds.size(), wds.size(), dds.size());
    }

    // the page-locked block (descriptors, input slices; the output behind them), every problem packed, the blocks of names
    // and dictionaries behind their slices; the device buffers; the input block's copy, and the documents'
    int stage() {
        const size_t nd = dds.size();
        in_bytes = head.head_bytes + sizeof(int32_t) * (size_t)in_words;
        out_bytes = sizeof(int32_t) * (size_t)out_words;
        host.p = pin_alloc(in_bytes + out_bytes);
        if (!host.p) return fail(BLANCE_ERR_DEVICE, "page-locked staging block: hipHostMalloc failed");
        h_in = (char*)host.p;
        h_out = (int32_t*)(h_in + in_bytes);
        for (size_t j = 0; j < items.size(); j++) {
            const BatchItem& it = items[j];
            const BatchProblem& b = pr[(size_t)it.idx];
            memcpy(h_in + head.desc + sizeof(BatchDesc) * j, &it.d, sizeof(BatchDesc));
            int32_t* dst = (int32_t*)(h_in + head.head_bytes) + it.d.in_base;
            batch_pack(b.pb, it.d, dst, b.dc ? (b.dc->assign_too ? 2 : 1) : 0, b.dc && b.dc->keep_prev_only);
            if (it.mi >= 0) {                            // beg_other behind the input slice
                const BatchMovesDesc& md = mds[(size_t)it.mi];
                const int P = it.d.P;
                if (b.mv->beg_other_off) {
                    memcpy(dst + md.i_ooff, b.mv->beg_other_off, sizeof(int32_t) * ((size_t)P + 1));
                    memcpy(dst + md.i_onodes, b.mv->beg_other_nodes, sizeof(int32_t) * (size_t)b.mv->beg_other_off[P]);
                } else {
                    memset(dst + md.i_ooff, 0, sizeof(int32_t) * ((size_t)P + 1));
                }
            }
            if (it.wi >= 0) {                            // the prepared names behind the input slice
                const std::vector<int32_t>& blk = b.wr->names->block;
                memcpy(dst + wds[(size_t)it.wi].i_names, blk.data(), sizeof(int32_t) * blk.size());
            }
        }
        if (!mds.empty()) memcpy(h_in + head.mdesc, mds.data(), sizeof(BatchMovesDesc) * mds.size());
        if (!sds.empty()) memcpy(h_in + head.sdesc, sds.data(), sizeof(BatchStatsDesc) * sds.size());
        if (!wds.empty()) memcpy(h_in + head.wdesc, wds.data(), sizeof(BatchWireDesc) * wds.size());
        // the documents in page-locked staging of their own, each at a 16-byte aligned base and padded to 16
        if (nd > 0) {
            memcpy(h_in + head.ddesc, dds.data(), sizeof(BatchDocDesc) * nd);
            h_docs.p = pin_alloc(docs_in_bytes + 16);
            h_sum.p = pin_alloc(sizeof(int32_t) * kBdSumWords * nd);
            if (!h_docs.p || !h_sum.p) return fail(BLANCE_ERR_DEVICE, "page-locked staging block: hipHostMalloc failed");
            for (size_t k = 0; k < nd; k++) {
                const BatchItem& it = items[(size_t)dd_item[k]];
                const blance_batch_doc* dc = pr[(size_t)it.idx].dc;
                char* at = (char*)h_docs.p + dds[k].doc_base;
                if (dc->len) memcpy(at, dc->json, dc->len);
                memset(at + dc->len, 0, ((dc->len + 15) & ~(size_t)15) - dc->len);
                const std::vector<int32_t>& blk = dc->dict->block;
                memcpy((int32_t*)(h_in + head.head_bytes) + it.d.in_base + dds[k].i_dict, blk.data(), sizeof(int32_t) * blk.size());
            }
            if (c->batch_doc_in.reserve(docs_in_bytes + 16) || c->batch_doc_sum.reserve(sizeof(int32_t) * kBdSumWords * nd))
                return fail(BLANCE_ERR_DEVICE, "hipMalloc failed");
        }
        // (scratch: wire_total [nw] behind the problems' slices)
        if (c->batch_in.reserve(in_bytes) || c->batch_sc.reserve(sizeof(int32_t) * ((size_t)sc_words + wds.size()) + 256) ||
            c->batch_out.reserve(out_bytes) || (!wds.empty() && c->batch_doc.reserve(doc_cap + 16)))
            return fail(BLANCE_ERR_DEVICE, "hipMalloc failed");
        HIPTRY(hipMemcpyAsync(c->batch_in.p, h_in, in_bytes, hipMemcpyHostToDevice, c->stream));
        q.desc = (const BatchDesc*)(c->batch_in.as<char>() + head.desc);
        q.in = (const int32_t*)(c->batch_in.as<char>() + head.head_bytes);
        q.sc = c->batch_sc.as<int32_t>();
        q.out = c->batch_out.as<int32_t>();
        HIPTRY(hipEventRecord(c->ev0, c->stream));
        if (docs_in_bytes > 0) HIPTRY(hipMemcpyAsync(c->batch_doc_in.p, h_docs.p, docs_in_bytes, hipMemcpyHostToDevice, c->stream));
        return BLANCE_OK;
    }

    // the documents: one launch, one round trip for the summary words, then what the host decides of them
    // (batch_doc_verdict) and the descriptors of the document problems again (n_prev, fresh, cap; skip for what is not
    // planned here)
    int decode_round() {
        const int nd = (int)dds.size();
        if (nd == 0) return BLANCE_OK;
        BatchDecodeParams qd;
        qd.desc = q.desc;
        qd.ddesc = (const BatchDocDesc*)(c->batch_in.as<char>() + head.ddesc);
        qd.in = (int32_t*)(c->batch_in.as<char>() + head.head_bytes);
        qd.sc = q.sc;
        qd.docs = c->batch_doc_in.as<unsigned char>();
        qd.sum = c->batch_doc_sum.as<int32_t>();
        qd.tile = c->wd_tile; qd.stage = c->wd_stage;
        launch_batch_decode(c->stream, qd, nd);
        launches++;
        HIPTRY(hipGetLastError());
        HIPTRY(hipMemcpyAsync(h_sum.p, c->batch_doc_sum.p, sizeof(int32_t) * kBdSumWords * (size_t)nd, hipMemcpyDeviceToHost, c->stream));
        HIPTRY(stream_sync(c));
        static const char* const kInconsistent[] = {"k_batch_decode: the list lengths overflow",
                                                    "k_batch_decode: the longest list and the first long list disagree",
                                                    "k_batch_decode: a result capacity above its bound"};
        for (int k = 0; k < nd; k++) {
            BatchItem& it = items[(size_t)dd_item[(size_t)k]];
            BatchProblem& b = pr[(size_t)it.idx];
            blance_batch_doc* dc = b.dc;
            const DocVerdict v = batch_doc_verdict((const int32_t*)h_sum.p + (size_t)k * kBdSumWords, b.pb, dc->assign_too != 0,
                                                   dc->keep_prev_only != 0, b.result_cap);
            dc->n_node_refs = v.n_node_refs; dc->n_parts_seen = v.n_parts_seen;
            switch (v.kind) {
            case DocVerdict::kInconsistent:
                return fail_problem(fail(BLANCE_ERR_DEVICE, "%s", kInconsistent[v.which]), it.idx);
            case DocVerdict::kParserRefused:
            case DocVerdict::kWhyRefused:
                dc->status = BLANCE_ERR_UNSUPPORTED;
                dc->refusal = v.refusal; dc->refusal_at = v.refusal_at;
                dc->why = v.why; dc->why_at = v.why_at;
                b.doc = kDocRefused;
                it.d.skip = 1;
                break;
            case DocVerdict::kSinglePath:                // from the bytes
                it.d.skip = 1;
                fallback.push_back(it.idx);
                break;
            case DocVerdict::kPlan:
                it.d.n_prev = v.n_prev; it.d.fresh = v.fresh; it.d.cap = v.cap;
                break;
            }
            memcpy(h_in + head.desc + sizeof(BatchDesc) * (size_t)dd_item[(size_t)k], &it.d, sizeof(BatchDesc));
        }
        HIPTRY(hipMemcpyAsync(c->batch_in.p, h_in, sizeof(BatchDesc) * items.size(), hipMemcpyHostToDevice, c->stream));
        return BLANCE_OK;
    }

    // one launch per size class, then one per kind of reader that some batched problem asks for (the documents: two)
    int launch() {
        const int nb = (int)items.size();
        q.first = 0;
        if (n64 > 0) { launch_plan_batch(c->stream, q, 64, n64, lds64); launches++; }
        q.first = n64;
        if (nb > n64) { launch_plan_batch(c->stream, q, 256, nb - n64, lds256); launches++; }
        if (!mds.empty()) {
            BatchMovesParams qm;
            qm.desc = q.desc;
            qm.mdesc = (const BatchMovesDesc*)(c->batch_in.as<char>() + head.mdesc);
            qm.in = q.in; qm.sc = q.sc; qm.out = q.out;
            launch_batch_moves(c->stream, qm, (int)mds.size());
            launches++;
        }
        if (!sds.empty()) {
            BatchStatsParams qs;
            qs.desc = q.desc;
            qs.sdesc = (const BatchStatsDesc*)(c->batch_in.as<char>() + head.sdesc);
            qs.in = q.in; qs.out = q.out;
            launch_batch_stats(c->stream, qs, (int)sds.size(), lds_stats);
            launches++;
        }
        if (!wds.empty()) {
            BatchWireParams qw;
            qw.desc = q.desc;
            qw.wdesc = (const BatchWireDesc*)(c->batch_in.as<char>() + head.wdesc);
            qw.in = q.in; qw.sc = q.sc; qw.out = q.out;
            qw.wire_total = q.sc + sc_words;
            qw.doc = c->batch_doc.as<char>();
            qw.stage = c->wire_stage;
            launch_batch_wire(c->stream, qw, (int)wds.size());
            launches += 2;
        }
        HIPTRY(hipGetLastError());
        HIPTRY(hipEventRecord(c->ev1, c->stream));
        return BLANCE_OK;
    }

    // the output block's download; what the kernel could not finish exactly (an interval budget of the hierarchy fold) goes
    // the single path; the written documents -- their 16-rounded lengths summed as k_batch_wire_write summed them -- in
    // one copy of exactly these bytes
    int collect() {
        HIPTRY(hipMemcpyAsync(h_out, c->batch_out.p, out_bytes, hipMemcpyDeviceToHost, c->stream));
        HIPTRY(stream_sync(c));
        float ms = 0.f;
        HIPTRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
        device_ms = ms;
        for (const BatchItem& it : items)
            if (!it.d.skip && !batch_planned(h_out + it.d.out_base)) fallback.push_back(it.idx);
        doc_base.assign(wds.size(), 0);
        size_t doc_bytes = 0;
        for (size_t w = 0; w < wds.size(); w++) {
            const BatchItem& it = items[(size_t)wds[w].desc];
            const int32_t* o = h_out + it.d.out_base;
            doc_base[w] = doc_bytes;
            if (!batch_planned(o) || o[kBoIterations] == 0) continue;
            const size_t total = (size_t)(uint32_t)o[wds[w].o_total];
            if (total > pr[(size_t)it.idx].wire_cap)
                return fail_problem(fail(BLANCE_ERR_DEVICE, "k_batch_wire_size: a document longer than its bound"), it.idx);
            doc_bytes += (total + 15) & ~(size_t)15;
        }
        if (doc_bytes > doc_cap) return fail(BLANCE_ERR_DEVICE, "k_batch_wire_size: the documents outgrow their buffer");
        if (doc_bytes > 0) {
            docs.p = pin_alloc(doc_bytes);
            if (!docs.p) return fail(BLANCE_ERR_DEVICE, "page-locked staging block: hipHostMalloc failed");
            HIPTRY(hipMemcpyAsync(docs.p, c->batch_doc.p, doc_bytes, hipMemcpyDeviceToHost, c->stream));
            HIPTRY(stream_sync(c));
        }
        return BLANCE_OK;
    }

    // every planned problem's output slice into the caller's structures
    void unpack() {
        const double total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
        for (const BatchItem& it : items) {
            const int32_t* o = h_out + it.d.out_base;
            if (!batch_planned(o)) continue;
            const BatchProblem& b = pr[(size_t)it.idx];
            batch_unpack_result(b.pb, it.d, o, device_ms, total_ms, b.res);
            steps += b.res->steps_total;
            if (it.mi >= 0) batch_unpack_moves(it.d, mds[(size_t)it.mi], o, b.mv->out);
            if (it.si >= 0) batch_unpack_stats(it.d, sds[(size_t)it.si], o, b.ps);
            if (b.wr && it.wi >= 0) {
                b.wr->need = (size_t)(uint32_t)o[wds[(size_t)it.wi].o_total];
                if (b.wr->need) memcpy(b.wr->buf, (const char*)docs.p + doc_base[(size_t)it.wi], b.wr->need);
            } else if (b.wr) {                           // an empty map is json.Marshal's "{}"
                b.wr->need = 2;
                memcpy(b.wr->buf, "{}", 2);
            }
        }
    }

    // One problem on the single path.  The two ways to a plan: blance_plan, or -- a document problem -- the document
    // adopted and blance_plan_resident; then the readers while the context still holds the plan: blance_plan_stats_get,
    // blance_plan_wire_names / blance_plan_wire_get, and the moves from where each way has the prevMap -- the adopted
    // lists on the device (blance_plan_moves_get), else the caller's arrays (blance_calc_moves).  *planned stays false for a
    // document refused here.
    // (Known inconsistency, DESIGN.md §4.17: the launches of the document's size / scan / write are counted for a problem
    // without a prevMap document only.)
    int plan_single(BatchProblem& b, bool* planned) {
        *planned = false;
        const bool doc = b.doc == kDocToPlan;
        int st;
        if (doc) {
            bool refused = false;
            if ((st = batch_doc_adopt(c, b.pb, b.dc, &device_ms, &refused)) || refused) return st;
            if ((st = plan_locked(c, b.res))) return st;
            if ((st = download_locked(c, b.res))) return st;
        } else if ((st = plan_whole_locked(c, b.pb, b.res))) {
            return st;
        }
        launches += b.res->kernel_launches;
        device_ms += b.res->device_ms;
        if (b.ps && (st = plan_stats_locked(c, b.ps, &launches))) return st;
        if (b.wr) {
            if ((st = wire_tables_upload_locked(c, b.wr->names->tables))) return st;
            double wire_ms = 0.0;
            st = plan_wire_locked(c, b.wr->buf, b.wr->cap, &b.wr->need, &wire_ms);
            c->wire_names = false;
            if (st) return st;
            if (!doc && b.pb->n_parts > 0) launches += reader_launches(b.pb->n_parts);   // size, scan, write
            device_ms += wire_ms;
        }
        if (b.mv && doc) {
            blance_plan_moves pm;
            memset(&pm, 0, sizeof pm);
            pm.favor_min_nodes = b.mv->favor_min_nodes;
            pm.out = b.mv->out;
            if ((st = plan_moves_locked(c, &pm))) return st;
            b.mv->out.device_ms = pm.out.device_ms;
        } else if (b.mv && (st = batch_moves_single(c, b.pb, b.res, b.mv, &launches))) {
            return st;
        }
        if (b.mv) device_ms += b.mv->out.device_ms;
        *planned = true;
        return BLANCE_OK;
    }

    int single_path() {
        for (int i : fallback) {
            BatchProblem& b = pr[(size_t)i];
            bool planned = false;
            const int st = plan_single(b, &planned);
            c->uploaded = c->planned = false;
            c->wire_names = false;
            if (st) return fail_problem(st, i);
            if (planned) steps += b.res->steps_total;
            else { b.doc = kDocRefused; n_refused_single++; }
        }
        return BLANCE_OK;
    }

    void report() {
        int n_planned = 0;                               // (a refused document's problem is in neither count)
        for (const BatchProblem& b : pr) {
            if (b.doc == kDocRefused) continue;
            n_planned++;
            if (b.mv) b.mv->out.device_ms = device_ms;
        }
        if (!info) return;
        const int n_fallback = (int)fallback.size() - n_refused_single;
        info->n_batched = n_planned - n_fallback;
        info->n_fallback = n_fallback;
        info->kernel_launches = launches;
        info->steps_total = steps;
        info->device_ms = device_ms;
        info->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    }
};
}  // namespace

// the one guard of the batch's entry points
static int batch_enter(blance_ctx* c, int32_t n, const blance_problem* const* pbs, blance_result* const* res,
                       blance_batch_moves* const* mvs, blance_plan_stats* const* sts, blance_batch_wire* const* wrs,
                       blance_batch_doc* const* dcs, blance_batch_info* info) {
    return enter(c, [&]() -> int {
        if (n < 0 || (n > 0 && (!pbs || !res))) return fail(BLANCE_ERR_BAD_ARG, "negative count or null arrays");
        return BatchCall(c, info).run(n, pbs, res, mvs, sts, wrs, dcs);
    });
}

extern "C" int blance_plan_batch(blance_ctx* c, int32_t n, const blance_problem* const* pbs, blance_result* const* res,
                                 blance_batch_info* info) {
    return batch_enter(c, n, pbs, res, nullptr, nullptr, nullptr, nullptr, info);
}

extern "C" int blance_plan_batch_moves(blance_ctx* c, int32_t n, const blance_problem* const* pbs, blance_result* const* res,
                                       blance_batch_moves* const* mvs, blance_batch_info* info) {
    return batch_enter(c, n, pbs, res, mvs, nullptr, nullptr, nullptr, info);
}

extern "C" int blance_plan_batch_stats(blance_ctx* c, int32_t n, const blance_problem* const* pbs, blance_result* const* res,
                                       blance_batch_moves* const* mvs, blance_plan_stats* const* sts, blance_batch_info* info) {
    return batch_enter(c, n, pbs, res, mvs, sts, nullptr, nullptr, info);
}

extern "C" int blance_plan_batch_wire(blance_ctx* c, int32_t n, const blance_problem* const* pbs, blance_result* const* res,
                                      blance_batch_moves* const* mvs, blance_plan_stats* const* sts,
                                      blance_batch_wire* const* wrs, blance_batch_info* info) {
    return batch_enter(c, n, pbs, res, mvs, sts, wrs, nullptr, info);
}

extern "C" int blance_plan_batch_docs(blance_ctx* c, int32_t n, const blance_problem* const* pbs, blance_result* const* res,
                                      blance_batch_moves* const* mvs, blance_plan_stats* const* sts, blance_batch_wire* const* wrs,
                                      blance_batch_doc* const* dcs, blance_batch_info* info) {
    return batch_enter(c, n, pbs, res, mvs, sts, wrs, dcs, info);
}
