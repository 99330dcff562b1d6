// TEST INFRASTRUCTURE ONLY: the upload's analysis (blance_amd/csrc/host/problem_facts.hpp) alone, as a stand-alone program for
// plain g++ -- no HIP, no context.  It reads the cases tests/test_problem_facts.py writes (the node, hierarchy and rule arrays of a
// small blance_problem, P and na; whitespace-separated integers), calls node_facts, order_facts, leaf_tables and analyse_rule,
// and prints every field and table, one "name values..." line each.  Every array is a heap block of exactly its size, so that
// the build under AddressSanitizer sees a read past an end.
//
//   problem_facts_main <cases> <answers>
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <vector>

#include "../../blance_amd/csrc/host/problem_facts.hpp"

using namespace blance;

namespace {
FILE* g_in = nullptr;
FILE* g_out = nullptr;

long long next_int() {
    long long v = 0;
    if (fscanf(g_in, "%lld", &v) != 1) { fprintf(stderr, "case file ends early\n"); exit(2); }
    return v;
}
template <class T>
std::unique_ptr<T[]> next_array(long long n) {                  // exactly n elements (new T[0] is a valid, unreadable block)
    if (n < 0 || n > (1 << 24)) { fprintf(stderr, "bad array length\n"); exit(2); }
    std::unique_ptr<T[]> a(new T[(size_t)n]);
    for (long long i = 0; i < n; i++) a[(size_t)i] = (T)next_int();
    return a;
}
void line(const char* name, long long v) { fprintf(g_out, "%s %lld\n", name, v); }
template <class T>
void line(const char* name, const std::vector<T>& v) {
    fprintf(g_out, "%s", name);
    for (const T& x : v) fprintf(g_out, " %lld", (long long)x);
    fprintf(g_out, "\n");
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3 || !(g_in = fopen(argv[1], "r")) || !(g_out = fopen(argv[2], "w"))) {
        fprintf(stderr, "usage: problem_facts_main <cases> <answers>\n");
        return 2;
    }
    const long long n_cases = next_int();
    for (long long k = 0; k < n_cases; k++) {
        blance_problem pb{};
        pb.n_nodes = (int32_t)next_int();
        pb.n_nodes_ext = (int32_t)next_int();
        pb.n_parts = (int32_t)next_int();
        pb.n_states = (int32_t)next_int();
        pb.top_state = (int32_t)next_int();
        pb.nodes_to_add_nil = (int32_t)next_int();
        const long long na = next_int();
        pb.hierarchy_rules_nil = (int32_t)next_int();
        const int NX = pb.n_nodes_ext;
        auto prio = next_array<int32_t>(pb.n_states);
        auto removed = next_array<uint8_t>(NX), added = next_array<uint8_t>(NX), has_weight = next_array<uint8_t>(NX);
        auto leaf_pos = next_array<int32_t>(NX);
        pb.state_priority = prio.get();
        pb.node_removed = removed.get(); pb.node_added = added.get(); pb.node_has_weight = has_weight.get();
        pb.node_leaf_pos = leaf_pos.get();
        pb.n_vertices = (int32_t)next_int();
        pb.vertex_empty = (int32_t)next_int();
        auto parent = next_array<int32_t>(pb.n_vertices), lo = next_array<int32_t>(pb.n_vertices), hi = next_array<int32_t>(pb.n_vertices);
        pb.vertex_parent = parent.get(); pb.vertex_leaf_lo = lo.get(); pb.vertex_leaf_hi = hi.get();
        pb.n_rules = (int32_t)next_int();
        auto inc = next_array<int32_t>(pb.n_rules), exc = next_array<int32_t>(pb.n_rules);
        pb.rule_inc = inc.get(); pb.rule_exc = exc.get();

        fprintf(g_out, "case %lld\n", k);
        const NodeFacts nodes = node_facts(pb);
        line("n_alive", nodes.n_alive);
        line("any_removed", nodes.any_removed);
        line("any_node_weight", nodes.any_node_weight);
        line("any_added", nodes.any_added);
        line("any_alive_added", nodes.any_alive_added);
        line("all_alive_added", nodes.all_alive_added);
        line("alive", nodes.alive);
        line("alive_ids", nodes.alive_ids);
        line("alive_rank", nodes.alive_rank);
        const OrderFacts o = order_facts(pb, nodes, na);
        line("top_prio_strict", o.top_prio_strict);
        line("cycle_order_stands", o.cycle_order_stands);
        line("uniform_first", o.uniform_first);
        line("uniform_all", o.uniform_all);
        if (pb.hierarchy_rules_nil) continue;
        const LeafTables leaf = leaf_tables(pb);
        line("n_leaves", leaf.n_leaves);
        line("leaves_distinct", leaf.leaves_distinct);
        line("leaf_node", leaf.leaf_node);
        std::vector<int32_t> flat;
        for (const AnchorSet& s : leaf.anchors) { flat.push_back(s.alo); flat.push_back(s.ahi); flat.push_back(s.blo); flat.push_back(s.bhi); }
        line("anchors", flat);
        for (int r = 0; r < pb.n_rules; r++) {
            const RuleTables t = analyse_rule(pb, leaf, nodes, r);
            fprintf(g_out, "rule %d\n", r);
            line("ok", t.ok);
            line("n_regions", t.n_regions);
            line("max_size", t.max_size);
            line("cls_run", t.cls_run);
            line("n_stay_wgs", t.n_stay_wgs);
            line("node_region", t.node_region);
            line("reg_lo", t.reg_lo);
            line("reg_hi", t.reg_hi);
            line("leaf_cls", t.leaf_cls);
            line("cls_size", t.cls_size);
            line("wg_region", t.wg_region);
            line("wg_chunk", t.wg_chunk);
            line("cyc_ok", t.cyc_ok);
            line("cyc", t.cyc);
            line("cyc_reg_off", t.cyc_reg_off);
            line("cyc_top_off", t.cyc_top_off);
        }
    }
    fprintf(g_out, "ran %lld cases\n", n_cases);
    return fclose(g_out) == 0 ? 0 : 1;
}
