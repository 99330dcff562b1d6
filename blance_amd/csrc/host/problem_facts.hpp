// What the upload learns from a problem before any kernel runs: which nodes are in nodesNext, which of the sweep
// driver's shortcuts the problem allows, and per hierarchy rule the region, exclude-class, k_stay_by_top and k_cycle.h
// tables.  Pure functions of a blance_problem: no HIP, no context, no error text -- blance_hip.hip copies the results to
// the device (RuleRegions::put) and tests/simt/problem_facts_main.cpp prints them.  The problem has passed blance_validate.
#pragma once

#include <limits.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../../../include/blance_hip.h"
#include "../blance_kernels.h"

namespace blance {

struct NodeFacts {
    std::vector<uint8_t> alive;           // [NX + 1] node is in nodesNext
    std::vector<int32_t> alive_ids;       // the nodes of nodesNext by id, then -1 (never empty)
    std::vector<int32_t> alive_rank;      // [NX + 1] a node's place in alive_ids, -1: not in it
    int n_alive = 0, any_removed = 0, any_node_weight = 0;
    // nodesToAdd names some node / some node of nodesNext / every node of nodesNext
    bool any_added = false, any_alive_added = false, all_alive_added = true;
};

inline NodeFacts node_facts(const blance_problem& pb) {
    const int N = pb.n_nodes, NX = pb.n_nodes_ext;
    NodeFacts f;
    f.alive.assign((size_t)NX + 1, 0);
    f.alive_rank.assign((size_t)NX + 1, -1);
    for (int n = 0; n < NX; n++) {
        if (pb.node_removed[n]) f.any_removed = 1;
        if (n < N && !pb.node_removed[n]) { f.alive[n] = 1; f.alive_rank[n] = f.n_alive++; f.alive_ids.push_back(n); }
        if (pb.node_has_weight[n]) f.any_node_weight = 1;
        if (pb.node_added[n]) { f.any_added = true; if (f.alive[n]) f.any_alive_added = true; }
        else if (f.alive[n]) f.all_alive_added = false;
    }
    f.alive_ids.push_back(-1);
    return f;
}

struct OrderFacts {
    bool top_prio_strict = false;     // every other state has a priority strictly behind the top state's
    bool cycle_order_stands = false;  // sweep 1's second pass runs in the order of its first
    // every partition gets the same partitionSorter category in sweep 1: in the sweep's first state pass / in all of them
    bool uniform_first = false, uniform_all = false;
};

// na: entries of the lists to assign (assign_off[P * M]).
inline OrderFacts order_facts(const blance_problem& pb, const NodeFacts& nodes, int64_t na) {
    OrderFacts o;
    const int M = pb.n_states;
    o.top_prio_strict = M > 0;
    for (int m = 0; m < M; m++)
        if (m != pb.top_state && pb.state_priority[m] <= pb.state_priority[pb.top_state]) o.top_prio_strict = false;
    // partitionSorter's category (plan.go:542-561) is "0" only for partitions with nodes in nodesToRemove.  Without any:
    // "2" for every partition when nodesToAdd == nil; "1" for every partition when nodesToAdd names no node.  A fresh
    // plan (the partitions to assign hold nothing): "1" for every partition in the sweep's first state pass (nothing held,
    // nothing in nodesToAdd), and -- when EVERY node of nodesNext is in nodesToAdd -- "2" for every partition in the later
    // ones: the first pass gave each partition at least one node (slot 0 always finds a candidate among >= 1 nodes, by
    // the rule or by the fallback of plan.go:216-218; nothing is excluded as "higher priority" yet) and that node is in
    // nodesToAdd.  The category is computed from the LIVE lists, so it changes from pass to pass of a sweep.
    //
    // (A plan from nothing whose first pass gave every partition ONE node of nodesNext: the second pass's category is "2"
    // where that node is in nodesToAdd, else "1" -- one category, and so the first pass's order again, when nodesToAdd is
    // nil, names every node of nodesNext or names none; "0" needs a removed node.  Not a matter of the caller's
    // BLANCE_NO_UNIFORM_CATEGORY: a stable partition by one category is the order it was given.)
    o.cycle_order_stands = !nodes.any_removed && (pb.nodes_to_add_nil || nodes.all_alive_added || !nodes.any_alive_added);
    const bool never = !nodes.any_removed && (pb.nodes_to_add_nil || !nodes.any_added);
    o.uniform_first = never || (!nodes.any_removed && na == 0);
    o.uniform_all = never || (!nodes.any_removed && na == 0 && nodes.all_alive_added && nodes.n_alive >= 1);
    return o;
}

struct LeafTables {
    std::vector<AnchorSet> anchors;   // [max(n_rules, 1)][NX + 1]: leaf intervals of every (rule, anchor), plan.go:723-734, :755-774
    std::vector<int32_t> leaf_node;   // [n_leaves] the node at a leaf (the last of them by id), -1: none
    int n_leaves = 1;
    bool leaves_distinct = true;      // no two nodes share a leaf of the hierarchy
};

// (only for a problem with hierarchy rules: the vertex arrays are there)
inline LeafTables leaf_tables(const blance_problem& pb) {
    const int NX = pb.n_nodes_ext, R = pb.n_rules;
    LeafTables f;
    f.anchors.resize((size_t)(R > 0 ? R : 1) * (NX + 1));
    for (int r = 0; r < R; r++)
        for (int a = 0; a <= NX; a++) {
            int v = a == NX ? pb.vertex_empty : a;
            int vi = v, ve = v;
            for (int l = pb.rule_inc[r]; l > 0; l--) vi = pb.vertex_parent[vi];   // findAncestor
            for (int l = pb.rule_exc[r]; l > 0; l--) ve = pb.vertex_parent[ve];
            AnchorSet st;
            st.alo = pb.vertex_leaf_lo[vi]; st.ahi = pb.vertex_leaf_hi[vi];
            st.blo = pb.vertex_leaf_lo[ve]; st.bhi = pb.vertex_leaf_hi[ve];
            f.anchors[(size_t)r * (NX + 1) + a] = st;
        }
    for (int v = 0; v < pb.n_vertices; v++) if (pb.vertex_leaf_hi[v] > f.n_leaves) f.n_leaves = pb.vertex_leaf_hi[v];
    f.leaf_node.assign((size_t)f.n_leaves, -1);
    for (int a = 0; a < NX; a++)
        if (pb.node_leaf_pos[a] >= 0 && pb.node_leaf_pos[a] < f.n_leaves) {
            if (f.leaf_node[pb.node_leaf_pos[a]] >= 0) f.leaves_distinct = false;
            f.leaf_node[pb.node_leaf_pos[a]] = a;
        }
    return f;
}

// One rule's tables.  The vectors are filled as far as the analysis got; the driver uploads them only where `ok`
// (cyc, cyc_reg_off, cyc_top_off: only where `cyc_ok`).
struct RuleTables {
    bool ok = false;                  // the rule cuts the leaves into regions (chains)
    int n_regions = 0, max_size = 0;
    int cls_run = 0;                  // S if every exclude class is an aligned run of S = 2^e <= 64 node-carrying leaves, else 0
    int n_stay_wgs = 0;
    std::vector<int32_t> node_region, reg_lo, reg_hi, leaf_cls, cls_size;
    std::vector<int32_t> wg_region, wg_chunk;     // k_stay_by_top: entry b = the tops at leaves reg_lo + 64 chunk .. + 63 of its region
    bool cyc_ok = false;
    std::vector<int32_t> cyc, cyc_reg_off, cyc_top_off;   // [n_alive][kCycWords], [n_regions + 1], [n_leaves + 1]
};

// The regions and the exclude classes of analyse_rule, below.
namespace facts_detail {
using Intervals = std::vector<std::pair<int, int>>;

inline void sort_unique(Intervals& iv) {
    std::sort(iv.begin(), iv.end());
    iv.erase(std::unique(iv.begin(), iv.end()), iv.end());
}
inline bool disjoint(const Intervals& iv) {
    for (size_t i = 1; i < iv.size(); i++) if (iv[i].first < iv[i - 1].second) return false;
    return true;
}

// Does the rule cut the leaves into regions?  Every node whose leaf lies in a region must have exactly that region as
// its include set.
inline bool find_regions(const blance_problem& pb, const AnchorSet* t, RuleTables& rt) {
    const int NX = pb.n_nodes_ext;
    Intervals iv;
    for (int a = 0; a < NX; a++) {
        int lp = pb.node_leaf_pos[a];
        if (lp >= 0 && t[a].alo <= lp && lp < t[a].ahi) iv.emplace_back(t[a].alo, t[a].ahi);
    }
    sort_unique(iv);
    bool ok = iv.size() >= 2 && disjoint(iv);
    rt.node_region.assign((size_t)NX, -1);
    if (ok) {
        for (auto& x : iv) {
            rt.reg_lo.push_back(x.first); rt.reg_hi.push_back(x.second);
            if (x.second - x.first > rt.max_size) rt.max_size = x.second - x.first;
        }
        for (int a = 0; a < NX && ok; a++) {
            int lp = pb.node_leaf_pos[a];
            if (lp < 0) continue;
            size_t j = std::upper_bound(rt.reg_lo.begin(), rt.reg_lo.end(), lp) - rt.reg_lo.begin();
            if (j == 0 || lp >= rt.reg_hi[j - 1]) continue;
            if (t[a].alo != rt.reg_lo[j - 1] || t[a].ahi != rt.reg_hi[j - 1]) ok = false;
            rt.node_region[a] = (int)j - 1;
        }
    }
    if (rt.max_size > kChainMaxLeaves) ok = false;
    return ok;
}

// Exclude classes: inside a region the anchors' exclude intervals must be pairwise disjoint (racks inside a zone), so
// "leaf is excluded by anchor a" is "leaf has a's class".  Intervals that cover the region get class -1.
// cls_run: -1 as long as no class was seen.
inline bool find_classes(const AnchorSet* t, const LeafTables& leaf, int g, RuleTables& rt, int& cls_run) {
    const std::vector<int32_t>& leaf_node = leaf.leaf_node;
    const int lo = rt.reg_lo[g], hi = rt.reg_hi[g];
    Intervals cl;
    for (int lp = lo; lp < hi; lp++) {
        int a = leaf_node[lp];
        if (a < 0) continue;
        int bl = t[a].blo, bh = t[a].bhi;
        if (lo <= bl && bh <= hi && bh - bl < hi - lo) cl.emplace_back(bl, bh);
    }
    sort_unique(cl);
    if (!disjoint(cl)) return false;
    for (size_t i = 0; i < cl.size(); i++) {       // equal, aligned, power-of-two runs? (k_pass_chain_planes)
        const int sz = cl[i].second - cl[i].first;
        if (cls_run == -1) cls_run = sz;
        if (sz != cls_run || sz < 1 || sz > 64 || (sz & (sz - 1)) || (cl[i].first - lo) % sz) cls_run = 0;
        for (int lp = cl[i].first; lp < cl[i].second && cls_run > 0; lp++) if (leaf_node[lp] < 0) cls_run = 0;
    }
    for (size_t i = 0; i < cl.size(); i++) rt.cls_size[lo + i] = cl[i].second - cl[i].first;
    bool ok = true;
    for (int lp = lo; lp < hi && ok; lp++) {
        int a = leaf_node[lp];
        if (a < 0) continue;
        // the class whose interval holds this leaf must be the node's own exclude interval
        size_t j = std::upper_bound(cl.begin(), cl.end(), std::make_pair(lp, INT_MAX)) - cl.begin();
        if (j > 0 && lp < cl[j - 1].second) {
            if (t[a].blo != cl[j - 1].first || t[a].bhi != cl[j - 1].second) ok = false;
            rt.leaf_cls[lp] = (int)j - 1;
        }
    }
    return ok;
}

// The tables of k_cycle.h.  Step j = s A + a of a round robin has top priority node alive_ids[a]: region r_a, rank q_a
// among the region's nodes of nodesNext, c_r of them in the region.  A region's chain has a step per full cycle and
// node, and one more for every node the last, partial cycle still reaches.  Built when no two nodes share a leaf and
// every node of nodesNext lies in a region.
inline void cycle_tables(const blance_problem& pb, const LeafTables& leaf, const NodeFacts& nodes, RuleTables& rt) {
    if (!leaf.leaves_distinct || nodes.n_alive < 1) return;
    const int P = pb.n_parts, n_leaves = leaf.n_leaves;
    const int A = nodes.n_alive, B = (int)rt.reg_lo.size(), full = P / A, part = P % A;
    const std::vector<int32_t>& alive_ids = nodes.alive_ids;
    for (int a = 0; a < A; a++) if (rt.node_region[alive_ids[a]] < 0) return;
    std::vector<int32_t> count((size_t)B, 0), last((size_t)B, 0), leaf_steps((size_t)n_leaves, 0);
    std::vector<int32_t>& cyc = rt.cyc;
    cyc.assign((size_t)A * kCycWords, 0);
    for (int a = 0; a < A; a++) {
        const int n = alive_ids[a], g = rt.node_region[n];
        cyc[(size_t)a * kCycWords + kCycRegion] = g;
        cyc[(size_t)a * kCycWords + kCycRank] = count[g]++;
        cyc[(size_t)a * kCycWords + kCycLeaf] = pb.node_leaf_pos[n];
        if (a < part) last[g]++;
        leaf_steps[pb.node_leaf_pos[n]] = full + (a < part ? 1 : 0);
    }
    for (int a = 0; a < A; a++) cyc[(size_t)a * kCycWords + kCycCount] = count[cyc[(size_t)a * kCycWords + kCycRegion]];
    rt.cyc_reg_off.assign((size_t)B + 1, 0);
    for (int g = 0; g < B; g++) rt.cyc_reg_off[g + 1] = rt.cyc_reg_off[g] + full * count[g] + last[g];
    rt.cyc_top_off.assign((size_t)n_leaves + 1, 0);
    for (int lp = 0; lp < n_leaves; lp++) rt.cyc_top_off[lp + 1] = rt.cyc_top_off[lp] + leaf_steps[lp];
    rt.cyc_ok = true;
}
}  // namespace facts_detail

inline RuleTables analyse_rule(const blance_problem& pb, const LeafTables& leaf, const NodeFacts& nodes, int r) {
    const AnchorSet* t = &leaf.anchors[(size_t)r * (pb.n_nodes_ext + 1)];
    RuleTables rt;
    bool ok = facts_detail::find_regions(pb, t, rt);
    rt.leaf_cls.assign((size_t)leaf.n_leaves, -1);
    rt.cls_size.assign((size_t)leaf.n_leaves, 0);
    int cls_run = -1;
    for (size_t g = 0; g < rt.reg_lo.size() && ok; g++) ok = facts_detail::find_classes(t, leaf, (int)g, rt, cls_run);
    rt.ok = ok;
    rt.n_regions = ok ? (int)rt.reg_lo.size() : 0;
    rt.cls_run = ok && cls_run > 0 ? cls_run : 0;
    if (!ok) return rt;
    for (size_t g = 0; g < rt.reg_lo.size(); g++)
        for (int ch = 0; ch * 64 < rt.reg_hi[g] - rt.reg_lo[g]; ch++) { rt.wg_region.push_back((int32_t)g); rt.wg_chunk.push_back(ch); }
    rt.n_stay_wgs = (int)rt.wg_region.size();
    facts_detail::cycle_tables(pb, leaf, nodes, rt);
    return rt;
}

}  // namespace blance
