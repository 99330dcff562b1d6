// The chain pass behind a round robin, grouped without a sort (DESIGN.md 4.1b "Known from the upload").
//
// A plan from nothing commits its top-state pass as a round robin over nodesNext: step j of the pass order takes
// alive_ids[j % A].  The region and the leaf of a step's top priority node are then functions of a = j % A, and the two
// stable counting sorts of the pass that follows (by region: chain_order / chain_oi / chain_inv / reg_off; by leaf:
// top_off / top_order) are closed forms over tables the upload builds once per rule:
//     step j = s A + a   ->   chain index  i = reg_off[r_a] + s c_r + q_a
// with r_a the region of alive_ids[a], q_a its rank among the region's nodes of nodesNext in alive_ids order and c_r the
// region's count of them.  In the last, partial cycle every a' < a is present too, so the form holds to the last step.
#pragma once

namespace blance {

// (blance_kernels.h has the layout of the per-node table `cyc`: kCycWords, kCycRegion .. kCycCount.)

// k_chain_classify + the grouping by region + k_invert in one launch, one thread per step of the pass order (and one more
// for n_ev[P]).  The classification is k_chain_classify's, from the lists; the chain index comes from the EXPECTED node
// alive_ids[oi % A] and is therefore a permutation position whatever the lists hold.  A step whose top priority node is
// not the expected one raises flags[kFlagNotLocal]: the host sends the pass the in-order way and drops the grouping.
// refute (a test knob): step 0 expects alive_ids[1 % A] instead.
// reg_off_out[0 .. B] = reg_off_tab[0 .. B] (the driver's chain offsets are the upload's).
__global__ void k_cycle_group(DevProblem d, int m, int top_state, const int32_t* order, const int32_t* node_region, int A,
                              int B, const int32_t* alive_ids, const int32_t* cyc /* [A][kCycWords] */,
                              const int32_t* reg_off_tab, int refute, int32_t* regid, int32_t* n_ev, int32_t* chain_order,
                              int32_t* chain_oi, int32_t* chain_inv, int32_t* reg_off_out, int32_t* flags, Gate gate) {
    if (gate_closed(gate)) return;                 // (the host runs the sweep again from its first pass)
    const int oi = blockIdx.x * blockDim.x + threadIdx.x;
    for (int j = oi; j <= B; j += gridDim.x * blockDim.x) reg_off_out[j] = reg_off_tab[j];
    if (oi > d.P) return;
    if (oi == d.P) { n_ev[oi] = 0; return; }
    const int p = order[oi];
    const int idxT = p * d.M + top_state;
    const int top = (d.live_kind[idxT] != kListAbsent && d.live_len[idxT] > 0) ? d.live[(size_t)idxT * d.L] : -1;
    int rg = top >= 0 ? node_region[top] : -1;
    int ne = 0;
    if (rg >= 0) {
        const int idx = p * d.M + m;
        if (d.live_kind[idx] != kListAbsent)
            for (int i = 0; i < d.live_len[idx]; i++) {
                const int r2 = node_region[d.live[(size_t)idx * d.L + i]];
                if (r2 == rg) continue;
                if (r2 >= 0) ne++; else flags[kFlagOrphans] = 1;
                flags[kFlagEvents] = 1;
            }
    }
    if (rg < 0) { flags[kFlagNotLocal] = 1; rg = 0; }
    regid[oi] = rg;
    n_ev[oi] = ne;
    const int s = oi / A, a = oi - s * A;
    const int expect = alive_ids[refute && oi == 0 ? (oi + 1) % A : a];
    if (top != expect) flags[kFlagNotLocal] = 1;
    const int32_t* t = cyc + (size_t)a * kCycWords;
    const int i = reg_off_tab[t[kCycRegion]] + s * t[kCycCount] + t[kCycRank];
    chain_order[i] = p;
    chain_oi[i] = oi;
    chain_inv[p] = i;
}

// k_stay_by_top's work list (the chain indices grouped by the leaf of their top priority node, chain order inside a
// group) from the same tables: the list of alive_ids[a] is reg_off[r_a] + s c_r + q_a for s = 0, 1, ...  A wave takes 64
// consecutive s of one a and stores them side by side (a thread per step would store at stride count_a).
// waves_per_a = cdiv(cdiv(P, A), 64); the grid is A * waves_per_a waves.  top_off_out[0 .. n_leaves] = top_off_tab.
__global__ void k_cycle_top(int P, int A, int waves_per_a, int n_leaves, const int32_t* cyc, const int32_t* reg_off_tab,
                            const int32_t* top_off_tab, int32_t* top_off_out, int32_t* top_order, Gate gate) {
    if (gate_closed(gate)) return;
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;
    for (int j = tid; j <= n_leaves; j += gridDim.x * blockDim.x) top_off_out[j] = top_off_tab[j];
    const int w = tid >> 6, lane = tid & 63;
    const int a = w / waves_per_a;
    if (a >= A) return;
    const int s = (w - a * waves_per_a) * 64 + lane;
    const int count = P / A + (a < P % A ? 1 : 0);
    if (s >= count) return;
    const int32_t* t = cyc + (size_t)a * kCycWords;
    top_order[top_off_tab[t[kCycLeaf]] + s] = reg_off_tab[t[kCycRegion]] + s * t[kCycCount] + t[kCycRank];
}

}  // namespace blance
