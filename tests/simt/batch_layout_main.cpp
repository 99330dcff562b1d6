// TEST INFRASTRUCTURE ONLY: the batch's host arithmetic (blance_amd/csrc/host/batch_layout.hpp) alone, as a stand-alone program
// for plain g++ -- no HIP, no context.  It reads the commands tests/test_batch_layout.py writes (whitespace-separated words: a
// command's name, then integers), calls the header's functions and prints what they return, one "name values..." line each.
// Every array is a heap block of exactly its size, so that the build under AddressSanitizer sees an access past an end.
//
//   batch_layout_main <commands> <answers>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "../../blance_amd/csrc/host/batch_layout.hpp"

using namespace blance;

namespace {
FILE* g_in = nullptr;
FILE* g_out = nullptr;

long long next_int() {
    long long v = 0;
    if (fscanf(g_in, "%lld", &v) != 1) { fprintf(stderr, "command file ends early\n"); exit(2); }
    return v;
}
template <class T>
std::unique_ptr<T[]> next_array(long long n) {                  // exactly n elements (new T[0] is a valid, unreadable block)
    if (n < 0 || n > (1 << 24)) { fprintf(stderr, "bad array length\n"); exit(2); }
    std::unique_ptr<T[]> a(new T[(size_t)n]);
    for (long long i = 0; i < n; i++) a[(size_t)i] = (T)next_int();
    return a;
}
void line(const char* name, std::initializer_list<long long> v) {
    fprintf(g_out, "%s", name);
    for (long long x : v) fprintf(g_out, " %lld", x);
    fprintf(g_out, "\n");
}
template <class T>
void line(const char* name, const T* v, size_t n) {
    fprintf(g_out, "%s", name);
    for (size_t i = 0; i < n; i++) fprintf(g_out, " %lld", (long long)v[i]);
    fprintf(g_out, "\n");
}

// a blance_problem that owns its arrays
struct Problem {
    blance_problem pb{};
    std::unique_ptr<int32_t[]> prio, k, stick, nweight, leaf, order, pweight, aoff, anodes, poff, pnodes, lstate, lnode, lweight, roff, rinc,
        rexc, vparent, vlo, vhi;
    std::unique_ptr<uint8_t[]> hstick, removed, added, hweight, phweight, inprev, never, akind, pkind, lfirst;

    void read() {
        pb.n_nodes = (int32_t)next_int(); pb.n_nodes_ext = (int32_t)next_int(); pb.n_states = (int32_t)next_int();
        pb.n_parts = (int32_t)next_int(); pb.n_prev = (int32_t)next_int(); pb.n_loads = (int32_t)next_int();
        pb.n_rules = (int32_t)next_int(); pb.n_vertices = (int32_t)next_int(); pb.max_iterations = (int32_t)next_int();
        pb.partition_weights_nil = (int32_t)next_int(); pb.nodes_to_add_nil = (int32_t)next_int();
        pb.hierarchy_rules_nil = (int32_t)next_int(); pb.booster_kind = (int32_t)next_int(); pb.top_state = (int32_t)next_int();
        const long long NX = pb.n_nodes_ext, M = pb.n_states, P = pb.n_parts, PM = P * M;
        prio = next_array<int32_t>(M); k = next_array<int32_t>(M); stick = next_array<int32_t>(M); hstick = next_array<uint8_t>(M);
        removed = next_array<uint8_t>(NX); added = next_array<uint8_t>(NX); nweight = next_array<int32_t>(NX);
        hweight = next_array<uint8_t>(NX); leaf = next_array<int32_t>(NX);
        order = next_array<int32_t>(P); pweight = next_array<int32_t>(P); phweight = next_array<uint8_t>(P);
        inprev = next_array<uint8_t>(P); never = next_array<uint8_t>(P);
        aoff = next_array<int32_t>(PM + 1); anodes = next_array<int32_t>(aoff[(size_t)PM]); akind = next_array<uint8_t>(PM);
        poff = next_array<int32_t>(PM + 1); pnodes = next_array<int32_t>(poff[(size_t)PM]); pkind = next_array<uint8_t>(PM);
        lstate = next_array<int32_t>(pb.n_loads); lnode = next_array<int32_t>(pb.n_loads); lweight = next_array<int32_t>(pb.n_loads);
        lfirst = next_array<uint8_t>(pb.n_loads);
        roff = next_array<int32_t>(M + 1); rinc = next_array<int32_t>(pb.n_rules); rexc = next_array<int32_t>(pb.n_rules);
        pb.vertex_empty = (int32_t)next_int();
        vparent = next_array<int32_t>(pb.n_vertices); vlo = next_array<int32_t>(pb.n_vertices); vhi = next_array<int32_t>(pb.n_vertices);
        pb.state_priority = prio.get(); pb.state_constraints = k.get(); pb.state_stickiness = stick.get();
        pb.state_has_stickiness = hstick.get();
        pb.node_removed = removed.get(); pb.node_added = added.get(); pb.node_weight = nweight.get();
        pb.node_has_weight = hweight.get(); pb.node_leaf_pos = leaf.get();
        pb.part_order = order.get(); pb.part_weight = pweight.get(); pb.part_has_weight = phweight.get();
        pb.part_in_prev = inprev.get(); pb.part_prev_never_equal = never.get();
        pb.assign_off = aoff.get(); pb.assign_nodes = anodes.get(); pb.assign_kind = akind.get();
        pb.prev_off = poff.get(); pb.prev_nodes = pnodes.get(); pb.prev_kind = pkind.get();
        pb.load_state = lstate.get(); pb.load_node = lnode.get(); pb.load_weight = lweight.get(); pb.load_first_sweep_only = lfirst.get();
        pb.rule_off = roff.get(); pb.rule_inc = rinc.get(); pb.rule_exc = rexc.get();
        pb.vertex_parent = vparent.get(); pb.vertex_leaf_lo = vlo.get(); pb.vertex_leaf_hi = vhi.get();
    }
};

void print_desc(const BatchDesc& d) {
    line("sizes", {d.N, d.NX, d.M, d.P, d.L});
    line("scalars", {d.n_loads, d.n_rules, d.max_iterations, d.n_prev, d.fresh, d.n_alive, d.any_removed, d.weights_nil, d.add_nil,
                     d.hier_nil, d.booster_kind, d.top_state, d.cap, d.wcap, d.skip});
    line("in", {d.i_state, d.i_rule_off, d.i_node, d.i_order, d.i_part, d.i_alist, d.i_ahdr, d.i_plist, d.i_phdr, d.i_loads, d.i_anch});
    line("sc", {d.s_live, d.s_lhdr, d.s_prv, d.s_phdr, d.s_pflag, d.s_order, d.s_cat, d.s_ntn});
    line("out", {d.o_off, d.o_kind, d.o_nodes, d.o_wp, d.o_ws});
}

// layout <result_cap> <doc> <doc_loads>  <moves> [<favor> <has_other> [off P+1] <cap>]  <stats>  <wire> [<names_words> <wire_cap>]
//        <docd> [<len> <dict_words> <assign_too>]  <pack> [<pack_doc> <keep>]
void do_layout(const Problem& p) {
    BatchItem it;
    it.idx = 0;
    const long long result_cap = next_int();
    const bool doc = next_int() != 0;
    const int doc_loads = (int)next_int();
    const bool ok = batch_layout(&p.pb, it, result_cap, doc, doc_loads);
    const bool moves = next_int() != 0;
    bool favor = false;
    std::unique_ptr<int32_t[]> other;
    long long moves_cap = 0;
    if (moves) {
        favor = next_int() != 0;
        if (next_int()) other = next_array<int32_t>((long long)p.pb.n_parts + 1);
        moves_cap = next_int();
    }
    const bool stats = next_int() != 0;
    const bool wire = next_int() != 0;
    long long names_words = 0, wire_cap = 0;
    if (wire) { names_words = next_int(); wire_cap = next_int(); }
    const bool docd = next_int() != 0;
    long long len = 0, dict_words = 0, assign_too = 0;
    if (docd) { len = next_int(); dict_words = next_int(); assign_too = next_int(); }
    const bool pack = next_int() != 0;
    long long pack_doc = 0, keep = 0;
    if (pack) { pack_doc = next_int(); keep = next_int(); }
    line("ok", {ok});
    line("kept_loads", {batch_kept_loads(&p.pb, true), batch_kept_loads(&p.pb, false)});
    if (!ok) return;
    line("plan_words", {it.in_words, it.sc_words, it.out_words, it.threads});
    size_t doc_bytes = 7 * 16, docs_bytes = 3 * 16;                // (what earlier problems of the call took)
    if (moves) {
        const BatchMovesDesc md = batch_moves_regions(it, 5, favor, other.get(), moves_cap);
        line("moves", {md.desc, md.favor_min_nodes, md.i_ooff, md.i_onodes, md.s_cnt, md.s_mv, md.stride, md.o_moff, md.o_mops, md.cap});
    }
    if (stats) {
        const BatchStatsDesc sd = batch_stats_regions(it, 5);
        line("stats", {sd.desc, sd.o_stats});
    }
    if (wire) {
        const BatchWireDesc wd = batch_wire_regions(it, 5, names_words, (size_t)wire_cap, doc_bytes);
        line("wire", {wd.desc, wd.i_names, wd.s_len, wd.o_total});
    }
    if (docd) {
        const BatchDocDesc dd = batch_doc_regions(it, 5, (size_t)len, dict_words, assign_too != 0, docs_bytes);
        line("docd", {dd.desc, dd.len, dd.doc_base, dd.i_dict, dd.assign_too, dd.s_claim, dd.s_pkind, dd.s_kind, dd.s_len, dd.s_rec, dd.rec_cap});
    }
    line("bytes", {(long long)doc_bytes, (long long)docs_bytes});
    line("words", {it.in_words, it.sc_words, it.out_words});
    print_desc(it.d);
    if (pack) {
        std::unique_ptr<int32_t[]> dst(new int32_t[(size_t)it.in_words]);
        for (long long i = 0; i < it.in_words; i++) dst[(size_t)i] = 0x5A5A5A5A;
        batch_pack(&p.pb, it.d, dst.get(), (int)pack_doc, keep != 0);
        line("packed", dst.get(), (size_t)it.in_words);
    }
}

void do_verdict(const Problem& p) {
    auto v = next_array<int32_t>(kBdSumWords);
    const bool assign_too = next_int() != 0, keep = next_int() != 0;
    const long long result_cap = next_int();
    const DocVerdict r = batch_doc_verdict(v.get(), &p.pb, assign_too, keep, result_cap);
    line("verdict", {r.kind, r.refusal, r.refusal_at, r.why, r.why_at, r.kind == DocVerdict::kInconsistent ? r.which : -1,
                     r.n_prev, r.fresh, r.cap, r.n_node_refs, r.n_parts_seen});
}

// unpack_result <P> <M> <o_off> <o_kind> <o_nodes> <o_wp> <o_ws> <n> <words n>: into buffers of exactly what the slice says
void do_unpack_result(const Problem& p) {
    BatchDesc d;
    memset(&d, 0, sizeof d);
    d.P = (int32_t)next_int(); d.M = (int32_t)next_int();
    d.o_off = (int32_t)next_int(); d.o_kind = (int32_t)next_int(); d.o_nodes = (int32_t)next_int();
    d.o_wp = (int32_t)next_int(); d.o_ws = (int32_t)next_int();
    const long long n = next_int();
    auto o = next_array<int32_t>(n);
    const size_t PM = (size_t)d.P * d.M, entries = (size_t)o[kBoEntries], warn = (size_t)o[kBoWarnings];
    std::unique_ptr<int32_t[]> off(new int32_t[PM + 1]), nodes(new int32_t[entries]), wp(new int32_t[warn]), ws(new int32_t[warn]);
    std::unique_ptr<uint8_t[]> kind(new uint8_t[PM]);
    blance_result r;
    memset(&r, 0x77, sizeof r);
    r.out_off = off.get(); r.out_nodes = nodes.get(); r.out_kind = kind.get(); r.warn_part = wp.get(); r.warn_state = ws.get();
    batch_unpack_result(&p.pb, d, o.get(), 1.5, 2.5, &r);
    line("out_off", r.out_off, PM + 1);
    line("out_kind", r.out_kind, PM);
    line("out_nodes", r.out_nodes, entries);
    line("warn_part", r.warn_part, warn);
    line("warn_state", r.warn_state, warn);
    line("counters", {r.n_warnings, r.iterations, r.converged, (long long)r.steps_total, (long long)r.steps_sequential, (long long)r.steps_batched,
                      (long long)r.kernel_launches, (long long)r.pass_kernel_launches, (long long)r.flat_passes,
                      (long long)r.blank_pass_launches, (long long)r.stay_pass_launches, (long long)r.host_syncs,
                      (long long)(2 * r.device_ms), (long long)(2 * r.total_ms),
                      (long long)(r.pass_kernel_ms + r.flat_pass_ms + r.blank_pass_ms + r.stay_pass_ms)});
}

// unpack_moves <P> <o_moff> <o_mops> <n> <words n>
void do_unpack_moves() {
    BatchDesc d;
    memset(&d, 0, sizeof d);
    BatchMovesDesc md;
    memset(&md, 0, sizeof md);
    d.P = (int32_t)next_int(); md.o_moff = (int32_t)next_int(); md.o_mops = (int32_t)next_int();
    const long long n = next_int();
    auto o = next_array<int32_t>(n);
    const size_t total = (size_t)o[(size_t)md.o_moff + (size_t)d.P];
    std::unique_ptr<int32_t[]> off(new int32_t[(size_t)d.P + 1]), node(new int32_t[total]), state(new int32_t[total]), kind(new int32_t[total]);
    blance_moves_result mo;
    memset(&mo, 0, sizeof mo);
    mo.op_off = off.get(); mo.op_node = node.get(); mo.op_state = state.get(); mo.op_kind = kind.get();
    batch_unpack_moves(d, md, o.get(), mo);
    line("op_off", mo.op_off, (size_t)d.P + 1);
    line("op_node", mo.op_node, total);
    line("op_state", mo.op_state, total);
    line("op_kind", mo.op_kind, total);
}

// unpack_stats <M> <o_stats> <rule_violations?> <n> <words n>
void do_unpack_stats() {
    BatchDesc d;
    memset(&d, 0, sizeof d);
    BatchStatsDesc sd;
    d.M = (int32_t)next_int(); sd.desc = 0; sd.o_stats = (int32_t)next_int();
    const bool with_rv = next_int() != 0;
    const long long n = next_int();
    auto o = next_array<int32_t>(n);
    const size_t M = (size_t)d.M;
    std::unique_ptr<int64_t[]> mn(new int64_t[M]), mx(new int64_t[M]), sum(new int64_t[M]), sq(new int64_t[M]), unmet(new int64_t[M]),
        rv(new int64_t[M]);
    std::unique_ptr<int32_t[]> used(new int32_t[M]);
    blance_plan_stats ps;
    memset(&ps, 0, sizeof ps);
    ps.n_states = d.M;
    ps.load_min = mn.get(); ps.load_max = mx.get(); ps.load_sum = sum.get(); ps.load_sumsq = sq.get(); ps.nodes_used = used.get();
    ps.unmet_slots = unmet.get(); ps.rule_violations = with_rv ? rv.get() : nullptr;
    batch_unpack_stats(d, sd, o.get(), &ps);
    line("n_nodes_next", {ps.n_nodes_next});
    line("load_min", ps.load_min, M); line("load_max", ps.load_max, M); line("load_sum", ps.load_sum, M);
    line("load_sumsq", ps.load_sumsq, M); line("nodes_used", ps.nodes_used, M); line("unmet_slots", ps.unmet_slots, M);
    if (with_rv) line("rule_violations", ps.rule_violations, M);
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3 || !(g_in = fopen(argv[1], "r")) || !(g_out = fopen(argv[2], "w"))) {
        fprintf(stderr, "usage: batch_layout_main <commands> <answers>\n");
        return 2;
    }
    Problem p;
    long long n = 0;
    char cmd[32];
    while (fscanf(g_in, "%31s", cmd) == 1) {
        const std::string c = cmd;
        if (c != "problem") fprintf(g_out, "answer %lld\n", n++);
        if (c == "problem") p.read();
        else if (c == "layout") do_layout(p);
        else if (c == "head") {
            const size_t nb = (size_t)next_int(), nm = (size_t)next_int(), ns = (size_t)next_int(), nw = (size_t)next_int(), nd = (size_t)next_int();
            const BatchHead h = batch_head(nb, nm, ns, nw, nd);
            line("head", {(long long)h.desc, (long long)h.mdesc, (long long)h.sdesc, (long long)h.wdesc, (long long)h.ddesc, (long long)h.head_bytes});
            line("sizeof", {(long long)sizeof(BatchDesc), (long long)sizeof(BatchMovesDesc), (long long)sizeof(BatchStatsDesc),
                            (long long)sizeof(BatchWireDesc), (long long)sizeof(BatchDocDesc)});
        } else if (c == "verdict") do_verdict(p);
        else if (c == "refusal") {
            const bool assign_too = next_int() != 0;
            const int first_missing = (int)next_int(), first_dup = (int)next_int();
            const bool any_removed = next_int() != 0, any_pass = next_int() != 0, load = next_int() != 0;
            const AdoptRefusal r = adopt_refusal(assign_too, first_missing, first_dup, any_removed, any_pass, load);
            line("refusal", {r.why, r.at});
        } else if (c == "load_bound") {
            const long long aprev = next_int(), kept = next_int(), sumw = next_int(), ksum = next_int();
            line("load_bound", {adopt_load_bound_exceeded(aprev, kept, sumw, ksum)});
        } else if (c == "planned") {
            auto o = next_array<int32_t>(kBatchHdr);
            line("planned", {batch_planned(o.get())});
        } else if (c == "unpack_result") do_unpack_result(p);
        else if (c == "unpack_moves") do_unpack_moves();
        else if (c == "unpack_stats") do_unpack_stats();
        else { fprintf(stderr, "unknown command %s\n", cmd); return 2; }
    }
    fprintf(g_out, "ran %lld commands\n", n);
    return fclose(g_out) == 0 ? 0 : 1;
}
