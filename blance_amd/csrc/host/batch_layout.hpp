// The host arithmetic of a batch call (blance_plan_batch*): where every region of a
// problem's three slices lies, what the packed input slice holds, what the host decides of a decoded document's summary
// words, and how an output slice becomes the caller's structures.  Pure functions: no HIP, no context, no error text --
// blance_hip.hip's BatchCall calls them between its copies and launches, tests/simt/batch_layout_main.cpp prints them.
// The kernels trust these offsets blindly.  A problem has passed blance_validate.
#pragma once

#include <limits.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../../include/blance_hip.h"
#include "../../../include/blance_batch.h"
#include "../blance_kernels.h"

namespace blance {

struct BatchItem {
    int idx;            // index in the caller's arrays
    int threads;        // 64 / 256: k_plan_batch's size class
    BatchDesc d;
    int64_t in_words, sc_words, out_words;
    int mi = -1;        // its BatchMovesDesc, when the caller asks for its moves
    int si = -1;        // its BatchStatsDesc, when the caller asks for its statistics
    int wi = -1;        // its BatchWireDesc, when the caller asks for its document
};

// a region of n_words at the end of a slice of `words` words: every region starts at a multiple of 4 words
inline void batch_take(int32_t& field, int64_t& words, int64_t n_words) {
    field = (int32_t)words;
    words += (n_words + 3) & ~3ll;
}

inline int batch_list_len(const blance_problem* pb) {
    int L = 1;
    const int M = pb->n_states;
    for (int m = 0; m < M; m++) if (pb->state_constraints[m] > L) L = pb->state_constraints[m];
    const int64_t PM = (int64_t)pb->n_parts * M;
    for (int64_t i = 0; i < PM; i++) {
        const int a = pb->assign_off[i + 1] - pb->assign_off[i], b = pb->prev_off[i + 1] - pb->prev_off[i];
        if (a > L) L = a;
        if (b > L) L = b;
    }
    return L;
}

// the word layout of one problem's three slices (BatchDesc); false when the problem is outside the batched envelope.
// result_cap: the list entries the output slice holds (blance_result_capacity, or blance_batch_doc_bounds' of a document
// problem).  doc: a document problem (blance_plan_batch_docs) -- the row stride is kBatchMaxL, doc_loads load entries are
// packed; n_prev, fresh and cap are fixed after the decode
inline bool batch_layout(const blance_problem* pb, BatchItem& it, int64_t result_cap, bool doc, int doc_loads) {
    const int N = pb->n_nodes, NX = pb->n_nodes_ext, M = pb->n_states, P = pb->n_parts;
    if (NX > kBatchMaxNX || P > kBatchMaxP || M > kMaxStates) return false;
    int L = batch_list_len(pb);
    if (L > kBatchMaxL) return false;
    if (doc) {
        L = kBatchMaxL;
        if (result_cap > (int64_t)INT32_MAX / 2) return false;
    }
    BatchDesc& d = it.d;
    memset(&d, 0, sizeof d);
    const int PM = P * M;
    d.N = N; d.NX = NX; d.M = M; d.P = P; d.L = L;
    d.n_loads = doc ? doc_loads : pb->n_loads; d.n_rules = pb->hierarchy_rules_nil ? 0 : pb->n_rules;
    d.max_iterations = pb->max_iterations; d.n_prev = pb->n_prev;
    for (int p = 0; p < P; p++) if (!pb->part_in_prev[p]) d.fresh++;
    for (int n = 0; n < NX; n++) {
        if (pb->node_removed[n]) d.any_removed = 1;
        if (n < N && !pb->node_removed[n]) d.n_alive++;
    }
    d.weights_nil = pb->partition_weights_nil; d.add_nil = pb->nodes_to_add_nil; d.hier_nil = pb->hierarchy_rules_nil;
    d.booster_kind = pb->booster_kind; d.top_state = pb->top_state;
    d.cap = (int32_t)result_cap;
    int passes = 0;
    for (int m = 0; m < M; m++) if (pb->state_constraints[m] > 0) passes++;
    d.wcap = P * passes;
    int64_t o = 0;
    auto take = [&](int32_t& field, int64_t words) { batch_take(field, o, words); };
    take(d.i_state, 4 * M); take(d.i_rule_off, M + 1); take(d.i_node, 4 * (int64_t)NX); take(d.i_order, P);
    take(d.i_part, 2 * (int64_t)P); take(d.i_alist, (int64_t)PM * L); take(d.i_ahdr, PM); take(d.i_plist, (int64_t)PM * L);
    take(d.i_phdr, PM); take(d.i_loads, 4 * (int64_t)d.n_loads); take(d.i_anch, 4 * (int64_t)d.n_rules * (NX + 1));
    it.in_words = o;
    o = 0;
    take(d.s_live, (int64_t)PM * L); take(d.s_lhdr, PM); take(d.s_prv, (int64_t)PM * L); take(d.s_phdr, PM);
    take(d.s_pflag, P); take(d.s_order, P); take(d.s_cat, P); take(d.s_ntn, (int64_t)(NX + 1) * (N > 0 ? N : 1));
    it.sc_words = o;
    o = kBatchHdr;
    take(d.o_off, PM + 1); take(d.o_kind, PM); take(d.o_nodes, d.cap); take(d.o_wp, d.wcap); take(d.o_ws, d.wcap);
    it.out_words = o;
    it.threads = NX <= 64 ? 64 : 256;
    return true;
}

// ---- the optional region sets of a batched problem, each behind what the slices hold so far; desc: the item's index ----

// the moves (k_batch_moves): the beg_other CSR behind the input slice, counts and moves in scratch, op_off and the move
// words in the output slice.  beg_other_off: [P + 1] or NULL; cap: the moves the output region holds
inline BatchMovesDesc batch_moves_regions(BatchItem& it, int desc, bool favor_min_nodes, const int32_t* beg_other_off, int64_t cap) {
    const BatchDesc& d = it.d;
    BatchMovesDesc md;
    memset(&md, 0, sizeof md);
    md.desc = desc;
    md.favor_min_nodes = favor_min_nodes ? 1 : 0;
    int n_other = 0, other_len = 0;
    if (beg_other_off) {
        n_other = beg_other_off[d.P];
        for (int p = 0; p < d.P; p++) other_len = std::max(other_len, beg_other_off[p + 1] - beg_other_off[p]);
    }
    md.stride = std::min(2 * d.M * d.L + other_len, d.NX);   // >= the distinct nodes of a partition's two maps
    md.cap = (int32_t)cap;
    batch_take(md.i_ooff, it.in_words, d.P + 1); batch_take(md.i_onodes, it.in_words, n_other);
    batch_take(md.s_cnt, it.sc_words, d.P); batch_take(md.s_mv, it.sc_words, (int64_t)d.P * md.stride);
    batch_take(md.o_moff, it.out_words, d.P + 1); batch_take(md.o_mops, it.out_words, md.cap);
    return md;
}

// the statistics (k_batch_stats): 1 + 7 M int64 values in the output slice (a multiple of 4 words: 8-byte aligned)
inline BatchStatsDesc batch_stats_regions(BatchItem& it, int desc) {
    BatchStatsDesc sd;
    sd.desc = desc;
    batch_take(sd.o_stats, it.out_words, 2 * (1 + (int64_t)kBatchStatsArrays * it.d.M));
    return sd;
}

// the document (k_batch_wire_*): the names block (names_words words, a multiple of 4) behind the input slice, the ranks'
// offsets in scratch, the length in the output slice; doc_bytes grows by the document's bound wire_cap, rounded to 16
inline BatchWireDesc batch_wire_regions(BatchItem& it, int desc, int64_t names_words, size_t wire_cap, size_t& doc_bytes) {
    BatchWireDesc wd;
    wd.desc = desc;
    batch_take(wd.i_names, it.in_words, names_words);
    batch_take(wd.s_len, it.sc_words, (int64_t)it.d.P + 1);
    batch_take(wd.o_total, it.out_words, 1);
    doc_bytes += (wire_cap + 15) & ~(size_t)15;
    return wd;
}

// the prevMap document (k_batch_decode): the dictionary block (dict_words words, a multiple of 4) behind the input slice,
// the parser's claim / kinds / lengths and the record starts in scratch (one run of words: the kernel zeroes up to s_rec);
// docs_bytes: where the document lies among the call's documents, grows by len rounded to 16
inline BatchDocDesc batch_doc_regions(BatchItem& it, int desc, size_t len, int64_t dict_words, bool assign_too, size_t& docs_bytes) {
    BatchDocDesc dd;
    memset(&dd, 0, sizeof dd);
    dd.desc = desc;
    dd.len = (int32_t)len;
    dd.doc_base = (int64_t)docs_bytes;
    docs_bytes += (len + 15) & ~(size_t)15;
    dd.assign_too = assign_too ? 1 : 0;
    batch_take(dd.i_dict, it.in_words, dict_words);
    const int64_t P = it.d.P, PM = (int64_t)it.d.P * it.d.M;
    batch_take(dd.s_claim, it.sc_words, P); batch_take(dd.s_pkind, it.sc_words, (P + 3) / 4);
    batch_take(dd.s_kind, it.sc_words, (PM + 3) / 4); batch_take(dd.s_len, it.sc_words, PM + 1);
    dd.rec_cap = (int32_t)((len + 1) / 2 + 1);
    batch_take(dd.s_rec, it.sc_words, dd.rec_cap);
    return dd;
}

// the five descriptor arrays in front of the input block, each at a multiple of 256 bytes
struct BatchHead { size_t desc, mdesc, sdesc, wdesc, ddesc, head_bytes; };

inline BatchHead batch_head(size_t nb, size_t nm, size_t ns, size_t nw, size_t nd) {
    auto padded = [](size_t bytes) { return (bytes + 255) & ~(size_t)255; };
    BatchHead h;
    h.desc = 0;
    h.mdesc = h.desc + padded(sizeof(BatchDesc) * nb);
    h.sdesc = h.mdesc + padded(sizeof(BatchMovesDesc) * nm);
    h.wdesc = h.sdesc + padded(sizeof(BatchStatsDesc) * ns);
    h.ddesc = h.wdesc + padded(sizeof(BatchWireDesc) * nw);
    h.head_bytes = h.ddesc + padded(sizeof(BatchDocDesc) * nd);
    return h;
}

// the problem's input slice (BatchDesc) at dst.  doc: a document problem -- 0: none; 1: prevMap's lists and headers are
// k_batch_decode's to write; 2 (assign_too): the lists to assign as well; keep: its load entries that are not first sweep
// only stay (d.n_loads of them), else none
inline void batch_pack(const blance_problem* pb, const BatchDesc& d, int32_t* dst, int doc, bool keep) {
    const int NX = d.NX, M = d.M, P = d.P, L = d.L, PM = P * M;
    for (int m = 0; m < M; m++) {
        int32_t* s = dst + d.i_state + 4 * m;
        s[0] = pb->state_priority[m]; s[1] = pb->state_constraints[m];
        s[2] = pb->state_stickiness[m]; s[3] = pb->state_has_stickiness[m];
    }
    for (int m = 0; m <= M; m++) dst[d.i_rule_off + m] = d.hier_nil ? 0 : pb->rule_off[m];
    for (int n = 0; n < NX; n++) {
        int32_t* s = dst + d.i_node + 4 * n;
        s[0] = pb->node_weight[n];
        s[1] = (pb->node_removed[n] ? 1 : 0) | (pb->node_added[n] ? 2 : 0) | (pb->node_has_weight[n] ? 4 : 0);
        s[2] = pb->node_leaf_pos[n];
        s[3] = 0;
    }
    if (P > 0) memcpy(dst + d.i_order, pb->part_order, sizeof(int32_t) * (size_t)P);
    for (int p = 0; p < P; p++) {
        dst[d.i_part + 2 * p] = pb->part_weight[p];
        dst[d.i_part + 2 * p + 1] = (pb->part_has_weight[p] ? 1 : 0) | (pb->part_in_prev[p] ? 2 : 0) | (pb->part_prev_never_equal[p] ? 4 : 0);
    }
    for (int idx = 0; idx < PM; idx++) {
        const int a0 = pb->assign_off[idx], a1 = pb->assign_off[idx + 1], b0 = pb->prev_off[idx], b1 = pb->prev_off[idx + 1];
        if (doc < 2) {
            if (a1 > a0) memcpy(dst + d.i_alist + (int64_t)idx * L, pb->assign_nodes + a0, sizeof(int32_t) * (size_t)(a1 - a0));
            dst[d.i_ahdr + idx] = (a1 - a0) | (pb->assign_kind[idx] << 16);
        }
        if (doc < 1) {
            if (b1 > b0) memcpy(dst + d.i_plist + (int64_t)idx * L, pb->prev_nodes + b0, sizeof(int32_t) * (size_t)(b1 - b0));
            dst[d.i_phdr + idx] = (b1 - b0) | (pb->prev_kind[idx] << 16);
        }
    }
    for (int i = 0, at = 0; i < pb->n_loads && at < d.n_loads; i++) {
        if (doc && !(keep && !pb->load_first_sweep_only[i])) continue;
        int32_t* s = dst + d.i_loads + 4 * at++;
        s[0] = pb->load_state[i]; s[1] = pb->load_node[i]; s[2] = pb->load_weight[i]; s[3] = pb->load_first_sweep_only[i];
    }
    // leaf-interval table of every (rule, anchor), anchor NX = the "" vertex: plan.go:723-734, :755-774 (as blance_upload)
    AnchorSet* tab = (AnchorSet*)(dst + d.i_anch);
    for (int r = 0; r < d.n_rules; r++)
        for (int a = 0; a <= NX; a++) {
            const int v = a == NX ? pb->vertex_empty : a;
            int vi = v, ve = v;
            for (int l = pb->rule_inc[r]; l > 0; l--) vi = pb->vertex_parent[vi];
            for (int l = pb->rule_exc[r]; l > 0; l--) ve = pb->vertex_parent[ve];
            AnchorSet& s = tab[(size_t)r * (NX + 1) + a];
            s.alo = pb->vertex_leaf_lo[vi]; s.ahi = pb->vertex_leaf_hi[vi];
            s.blo = pb->vertex_leaf_lo[ve]; s.bhi = pb->vertex_leaf_hi[ve];
        }
}

// the load entries of a document problem that keep_prev_only keeps: those that are not first sweep only
inline int batch_kept_loads(const blance_problem* pb, bool keep) {
    int kept = 0;
    if (keep)
        for (int j = 0; j < pb->n_loads; j++) kept += !pb->load_first_sweep_only[j];
    return kept;
}

// ---- what refuses P', the problem a prevMap document defines: blance_wire_adopt and the batch decide it here ----

// blance_validate's bound on the int32 load tables for P': prevMap's loads, the kept load entries, and what a plan can add
// (aprev, kept, sumw: sums of absolute weights; ksum: the sum of the positive constraints)
inline bool adopt_load_bound_exceeded(long long aprev, long long kept, long long sumw, long long ksum) {
    return aprev + kept + sumw * (ksum > 1 ? ksum : 1) * 2 > 2147483647LL;
}

struct AdoptRefusal { int why; int64_t at; };        // why 0: not refused

// The refusals of P' in the order they are reported (BLANCE_WIRE_ADOPT_*, blance_hip.h; blance_wire_adopt has
// LIST_TOO_LONG in front of them).  first_missing / first_dup: the smallest offender, INT_MAX for none
inline AdoptRefusal adopt_refusal(bool assign_too, int first_missing, int first_dup, bool any_removed, bool any_pass, bool load_exceeded) {
    if (assign_too && first_missing != INT_MAX) return {BLANCE_WIRE_ADOPT_PARTITION_MISSING, first_missing};
    if (assign_too && first_dup != INT_MAX) return {BLANCE_WIRE_ADOPT_DUPLICATE_NODE, first_dup};
    if (first_missing != INT_MAX && any_removed && any_pass) return {BLANCE_WIRE_ADOPT_REMOVED_WITHOUT_PREV, first_missing};
    if (load_exceeded) return {BLANCE_WIRE_ADOPT_LOAD_OVERFLOW, -1};
    return {0, -1};
}

// What the host decides of one document from k_batch_decode's summary words
struct DocVerdict {
    enum Kind { kParserRefused,   // refusal, refusal_at: exactly blance_wire_decode_device's
                kWhyRefused,      // why, why_at: exactly blance_wire_adopt's
                kSinglePath,      // a list longer than the batch's rows: from the bytes, one by one
                kInconsistent,    // the summary contradicts itself or its bound (a device error): which
                kPlan } kind;     // n_prev, fresh, cap: the descriptor's words
    enum Which { kLengthsOverflow, kLongestDisagrees, kCapAboveBound };
    int32_t refusal = 0; int64_t refusal_at = -1;
    int32_t why = 0; int64_t why_at = -1;
    Which which = kLengthsOverflow;
    int32_t n_prev = 0, fresh = 0, cap = 0;
    int64_t n_node_refs = 0, n_parts_seen = 0;       // of every document the parser took and the batch keeps
};

// v: the kBdSumWords words; pb: the skeleton; result_cap: the problem's bound (blance_batch_doc_bounds)
inline DocVerdict batch_doc_verdict(const int32_t* v, const blance_problem* pb, bool assign_too, bool keep, int64_t result_cap) {
    DocVerdict r;
    unsigned long long refusal, cap64, aprev;
    memcpy(&refusal, v + kBdRefusal, 8); memcpy(&cap64, v + kBdCap, 8); memcpy(&aprev, v + kBdPrevLoad, 8);
    if (refusal != ~0ull) {
        r.kind = DocVerdict::kParserRefused;
        r.refusal = (int32_t)(refusal & 255u); r.refusal_at = (int64_t)(refusal >> 8);
        return r;
    }
    r.kind = DocVerdict::kInconsistent;
    if (v[kBdRefs] < 0) { r.which = DocVerdict::kLengthsOverflow; return r; }
    if ((v[kBdLongest] > kBatchMaxL) != (v[kBdFirstLong] != INT_MAX)) { r.which = DocVerdict::kLongestDisagrees; return r; }
    if (v[kBdLongest] > kBatchMaxL) { r.kind = DocVerdict::kSinglePath; return r; }
    r.n_node_refs = v[kBdRefs]; r.n_parts_seen = v[kBdRecords];
    bool any_removed = false, any_pass = false;
    long long ksum = 0, sumw = 0, kept_abs = 0;
    for (int x = 0; x < pb->n_nodes_ext; x++) any_removed |= pb->node_removed[x] != 0;
    for (int m = 0; m < pb->n_states; m++) { any_pass |= pb->state_constraints[m] > 0; ksum += pb->state_constraints[m] > 0 ? pb->state_constraints[m] : 0; }
    int in_prev = 0;
    for (int p = 0; p < pb->n_parts; p++) {
        const long long w = (!pb->partition_weights_nil && pb->part_has_weight[p]) ? pb->part_weight[p] : 1;
        sumw += w < 0 ? -w : w;
        in_prev += pb->part_in_prev[p] != 0;
    }
    if (keep)
        for (int j = 0; j < pb->n_loads; j++)
            if (!pb->load_first_sweep_only[j]) kept_abs += pb->load_weight[j] < 0 ? -(long long)pb->load_weight[j] : pb->load_weight[j];
    const AdoptRefusal rf = adopt_refusal(assign_too, v[kBdFirstMissing], v[kBdFirstDup], any_removed, any_pass,
                                          adopt_load_bound_exceeded((long long)aprev, kept_abs, sumw, ksum));
    if (rf.why) {
        r.kind = DocVerdict::kWhyRefused;
        r.why = rf.why; r.why_at = rf.at;
        return r;
    }
    if (assign_too && cap64 > (unsigned long long)result_cap) { r.which = DocVerdict::kCapAboveBound; return r; }
    r.kind = DocVerdict::kPlan;
    r.n_prev = v[kBdRecords] + (keep ? pb->n_prev - in_prev : 0);
    r.fresh = v[kBdFresh];
    r.cap = (int32_t)(assign_too ? (int64_t)cap64 : result_cap);
    return r;
}

// ---- one planned problem's output slice (o: its first word, batch_planned(o)) into the caller's structures ----

inline void batch_unpack_result(const blance_problem* pb, const BatchDesc& d, const int32_t* o, double device_ms, double total_ms,
                                blance_result* r) {
    const int PM = d.P * d.M;
    const int iters = o[kBoIterations], n_warn = o[kBoWarnings], entries = o[kBoEntries];
    memcpy(r->out_off, o + d.o_off, sizeof(int32_t) * ((size_t)PM + 1));
    for (int i = 0; i < PM; i++) r->out_kind[i] = (uint8_t)o[d.o_kind + i];
    if (entries > 0) memcpy(r->out_nodes, o + d.o_nodes, sizeof(int32_t) * (size_t)entries);
    if (n_warn > 0) {
        memcpy(r->warn_part, o + d.o_wp, sizeof(int32_t) * (size_t)n_warn);
        memcpy(r->warn_state, o + d.o_ws, sizeof(int32_t) * (size_t)n_warn);
    }
    int passes = 0;
    for (int m = 0; m < d.M; m++) if (pb->state_constraints[m] > 0) passes++;
    r->n_warnings = n_warn;
    r->iterations = iters;
    r->converged = o[kBoConverged];
    r->device_ms = device_ms;
    r->total_ms = total_ms;
    r->steps_total = (int64_t)iters * d.P * passes;
    r->steps_sequential = r->steps_batched = r->kernel_launches = 0;
    r->pass_kernel_ms = r->flat_pass_ms = r->blank_pass_ms = r->stay_pass_ms = 0.0;
    r->pass_kernel_launches = r->flat_passes = r->blank_pass_launches = r->stay_pass_launches = r->host_syncs = 0;
}

// moves: op_off [P + 1], then one word a move, node | (state + 1) << 16 | kind << 24
inline void batch_unpack_moves(const BatchDesc& d, const BatchMovesDesc& md, const int32_t* o, blance_moves_result& mo) {
    memcpy(mo.op_off, o + md.o_moff, sizeof(int32_t) * ((size_t)d.P + 1));
    const int32_t* w = o + md.o_mops;
    for (int32_t j = 0; j < mo.op_off[d.P]; j++) {
        mo.op_node[j] = w[j] & 0xffff;
        mo.op_state[j] = ((w[j] >> 16) & 0xff) - 1;
        mo.op_kind[j] = (w[j] >> 24) & 0xff;
    }
}

// statistics: n_nodes_next, then seven arrays [M], all int64; rule_violations may be NULL
inline void batch_unpack_stats(const BatchDesc& d, const BatchStatsDesc& sd, const int32_t* o, blance_plan_stats* ps) {
    const int M = d.M;
    std::vector<int64_t> v(1 + (size_t)kBatchStatsArrays * M);
    memcpy(v.data(), o + sd.o_stats, sizeof(int64_t) * v.size());
    ps->n_nodes_next = (int32_t)v[0];
    for (int m = 0; m < M; m++) {
        ps->load_min[m] = v[1 + m];
        ps->load_max[m] = v[1 + M + m];
        ps->load_sum[m] = v[1 + 2 * M + m];
        ps->load_sumsq[m] = v[1 + 3 * M + m];
        ps->nodes_used[m] = (int32_t)v[1 + 4 * M + m];
        ps->unmet_slots[m] = v[1 + 5 * M + m];
        if (ps->rule_violations) ps->rule_violations[m] = v[1 + 6 * M + m];
    }
}

}  // namespace blance
