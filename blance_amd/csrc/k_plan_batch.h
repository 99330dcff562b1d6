// k_plan_batch: the whole of planNextMapEx (plan.go:23-58) for many small problems in one launch, one workgroup per
// problem, no host round trip between sweeps.  The line-by-line specification is oracle/blance_oracle.c (sweep,
// state_pass, find_best_nodes, remove_from_all_states); this is its workgroup-parallel restatement.  DESIGN.md §4.8.
#pragma once

namespace blance {

// Thread n owns node n (T >= NX): its weight, its alive bit, its leaf position and its total count
// (nodePartitionCounts, plan.go:118-124) sit in registers; its stateNodeCounts column cnt[t * NX + n] in LDS and its
// nodeToNodeCounts column in the problem's HBM scratch are touched by no other thread between two counting phases.
// A step is: the partition's lists into LDS, one score per node, one workgroup argmin per pick (block_argmin, the
// (score, position) order of better()), then every thread commits its own node and threads t < M their state's list.
template <int T>
__global__ __launch_bounds__(T) void k_plan_batch(BatchParams bp) {
    constexpr int W = T / 64;
    const BatchDesc& D = bp.desc[bp.first + blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = D.N, NX = D.NX, M = D.M, P = D.P, L = D.L, PM = D.P * D.M;
    const int32_t* in = bp.in + D.in_base;
    int32_t* sc = bp.sc + D.sc_base;
    int32_t* out = bp.out + D.out_base;
    if (D.skip) {                                  // blance_plan_batch_docs: its document was refused or goes the single path
        if (tid == 0) { out[kBoError] = 0; out[kBoDone] = 0; }  // (not done: the kernels behind this one leave it alone; uniform exit)
        return;
    }
    const int32_t* st = in + D.i_state;
    const int32_t* rule_off = in + D.i_rule_off;
    const int32_t* node = in + D.i_node;
    const int32_t* part = in + D.i_part;
    const AnchorSet* anch = (const AnchorSet*)(in + D.i_anch);
    int32_t* live = sc + D.s_live;
    int32_t* lhdr_g = sc + D.s_lhdr;
    int32_t* prv = sc + D.s_prv;
    int32_t* phdr = sc + D.s_phdr;
    int32_t* pflag = sc + D.s_pflag;
    int32_t* ord = sc + D.s_order;
    int32_t* catpos = sc + D.s_cat;

    BLANCE_DYN_LDS(lds);
    RedSlot* red = (RedSlot*)lds;                  // [2 W] block_argmin
    int* shw = (int*)(red + 2 * W);                // [32] flags and the stable partition's per-wave counts
    int* lst = shw + 32;                           // [kMaxStates][kBatchMaxL] the step's partition lists
    int* lhdr = lst + kMaxStates * kBatchMaxL;     // [kMaxStates] their headers (length | kind << 16)
    int* cnt = lhdr + kMaxStates;                  // [max((M + 1) * NX, T)] stateNodeCounts; at the end the scan's sums
    int round = 0;

    const int n = tid;
    int w_n = 0, nf = 0, leaf_n = -1;
    if (n < NX) { w_n = node[n * 4]; nf = node[n * 4 + 1]; leaf_n = node[n * 4 + 2]; }
    const int hasw = (nf >> 2) & 1;
    const bool alive = n < N && !(nf & 1);         // nodesNext, plan.go:77
    int32_t* ntn_col = sc + D.s_ntn + (n < N ? n : 0);   // column n of nodeToNodeCounts: ntn_col[row * N]

    // prevMap as the call passes it (it is overwritten by every sweep's write-back, plan.go:49-52)
    for (int idx = tid; idx < PM; idx += T) {
        const int h = in[D.i_phdr + idx];
        phdr[idx] = h;
        for (int j = 0; j < (h & 0xffff); j++) prv[idx * L + j] = in[D.i_plist + idx * L + j];
    }
    for (int p = tid; p < P; p += T) pflag[p] = (part[p * 2 + 1] >> 1) & 3;
    __syncthreads();

    int iterations = 0, converged = 0, n_warn = 0, err = 0;
    long long steps = 0;
    for (int it = 0; it < D.max_iterations; it++) {                  // plan.go:32
        const bool first = it == 0;
        const int NP = first ? D.n_prev : D.n_prev + D.fresh;        // plan.go:50, :161
        const int add_nil = first ? D.add_nil : 0;                   // plan.go:53-55
        const int any_removed = first ? D.any_removed : 0;
        n_warn = 0;
        // nextPartitions: partitionsToAssign minus nodesToRemove (plan.go:83-88); later sweeps keep the last result, every
        // present key a non-nil slice again
        for (int idx = tid; idx < PM; idx += T) {
            if (first) {
                const int h = in[D.i_ahdr + idx];
                int len = 0;
                for (int j = 0; j < (h & 0xffff); j++) {
                    const int x = in[D.i_alist + idx * L + j];
                    if (!(node[x * 4 + 1] & 1)) live[idx * L + len++] = x;
                }
                lhdr_g[idx] = len | (((h >> 16) == kListAbsent ? kListAbsent : kListSet) << 16);
            } else {
                const int h = lhdr_g[idx];
                if ((h >> 16) != kListAbsent) lhdr_g[idx] = (h & 0xffff) | (kListSet << 16);
            }
        }
        // stateNodeCounts = countStateNodes(prevMap), plan.go:94, :374-399 (integer sums: any order gives the same counts)
        for (int i = tid; i < (M + 1) * NX; i += T) cnt[i] = 0;
        __syncthreads();
        {
            const int32_t* ld = in + D.i_loads;
            for (int i = tid; i < D.n_loads; i += T)
                if (first || !ld[i * 4 + 3]) atomicAdd(&cnt[ld[i * 4] * NX + ld[i * 4 + 1]], ld[i * 4 + 2]);
            for (int p = tid; p < P; p += T) {
                if (!(pflag[p] & 1)) continue;
                const int w = (!D.weights_nil && (part[p * 2 + 1] & 1)) ? part[p * 2] : 1;
                for (int m = 0; m < M; m++) {
                    const int idx = p * M + m, len = phdr[idx] & 0xffff;
                    for (int j = 0; j < len; j++) atomicAdd(&cnt[m * NX + prv[idx * L + j]], w);
                }
            }
        }
        __syncthreads();
        int tot = 0;
        if (n < NX)
            for (int t = 0; t <= M; t++) tot += cnt[t * NX + n];

        for (int m = 0; m < M; m++) {                                // plan.go:307-324
            const int k = st[m * 4 + 1];
            if (k <= 0) continue;
            int higher_mask = 0;                                     // plan.go:146-154
            for (int t = 0; t < M; t++)
                if (st[t * 4] < st[m * 4]) higher_mask |= 1 << t;
            const int r0 = rule_off[m], r1 = rule_off[m + 1];
            const bool rules = !D.hier_nil && r1 > r0;
            const int32_t* order = in + D.i_order;
            __syncthreads();                                         // the last pass's list writes are seen
            // partitionSorter's category (plan.go:542-561) as a stable 3-way partition of the static order.  In later sweeps
            // and when nothing is removed and nodesToAdd is nil every partition has the same category: the static order.
            if (first && (any_removed || !add_nil)) {
                for (int i = tid; i < P; i += T) {
                    const int p = order[i];
                    bool is0 = false;
                    if (any_removed && (pflag[p] & 1)) {
                        const int h = phdr[p * M + m];
                        if ((h >> 16) == kListSet)
                            for (int j = 0; j < (h & 0xffff); j++)
                                if (node[prv[(p * M + m) * L + j] * 4 + 1] & 1) { is0 = true; break; }
                    }
                    int cv = 2;
                    if (is0) cv = 0;
                    else if (!add_nil) {
                        bool hit = false;
                        for (int t = 0; t < M && !hit; t++) {
                            const int h = lhdr_g[p * M + t];
                            if ((h >> 16) == kListAbsent) continue;
                            for (int j = 0; j < (h & 0xffff); j++)
                                if ((node[live[(p * M + t) * L + j] * 4 + 1] >> 1) & 1) { hit = true; break; }
                        }
                        if (!hit) cv = 1;
                    }
                    catpos[i] = cv;
                }
                if (tid < 3) shw[tid] = 0;
                __syncthreads();
                {
                    int c0 = 0, c1 = 0;
                    for (int i = tid; i < P; i += T) { c0 += catpos[i] == 0; c1 += catpos[i] == 1; }
                    if (c0) atomicAdd(&shw[0], c0);
                    if (c1) atomicAdd(&shw[1], c1);
                }
                __syncthreads();
                int base[3] = {0, shw[0], shw[0] + shw[1]};
                const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
                for (int s0 = 0; s0 < P; s0 += T) {                  // (bounds uniform: every lane takes the ballots)
                    const int i = s0 + tid;
                    const int cv = i < P ? catpos[i] : 3;
                    const unsigned long long b0 = __ballot(cv == 0), b1 = __ballot(cv == 1), b2 = __ballot(cv == 2);
                    if (lane == 0) { shw[4 + wave * 3] = __popcll(b0); shw[5 + wave * 3] = __popcll(b1); shw[6 + wave * 3] = __popcll(b2); }
                    __syncthreads();
                    if (i < P) {
                        const unsigned long long mine = cv == 0 ? b0 : cv == 1 ? b1 : b2;
                        int at = base[cv] + __popcll(mine & below);
                        for (int v = 0; v < wave; v++) at += shw[4 + v * 3 + cv];
                        ord[at] = order[i];
                    }
                    for (int v = 0; v < W; v++)
                        for (int c = 0; c < 3; c++) base[c] += shw[4 + v * 3 + c];
                    __syncthreads();
                }
                order = ord;
            }
            // nodeToNodeCounts := fresh (plan.go:266); only read and bumped while NumPartitions > 0
            if (NP > 0 && n < N)
                for (int r = 0; r <= NX; r++) ntn_col[r * N] = 0;

            for (int oi = 0; oi < P; oi++) {                         // assignStateToPartitions, plan.go:253-303
                const int p = order[oi];
                __syncthreads();                                     // the last step's readers of lst are done
                if (tid < M) {
                    const int h = lhdr_g[p * M + tid];
                    lhdr[tid] = h;
                    for (int j = 0; j < (h & 0xffff); j++) lst[tid * kBatchMaxL + j] = live[(p * M + tid) * L + j];
                }
                __syncthreads();
                const int pf = part[p * 2 + 1];
                const int w = (!D.weights_nil && (pf & 1)) ? part[p * 2] : 1;          // plan.go:269-275
                double stick = 1.5;                                                     // plan.go:104-115
                if (!D.weights_nil) {
                    if (pf & 1) stick = (double)part[p * 2];
                    else if (st[m * 4 + 3]) stick = (double)st[m * 4 + 2];
                }
                int top = -1;                                                           // plan.go:134-138
                {
                    const int h = lhdr[D.top_state];
                    if ((h >> 16) != kListAbsent && (h & 0xffff) > 0) top = lst[D.top_state * kBatchMaxL];
                }
                const int row = top < 0 ? NX : top;
                // my node in the partition's lists: higher priority (excluded), this state's (currentFactor)
                int any_higher_key = 0;
                unsigned held = 0;                                   // bit t: my node is in state t's (present) list
                for (int t = 0; t < M; t++) {
                    const int h = lhdr[t];
                    if ((h >> 16) == kListAbsent) continue;
                    if ((higher_mask >> t) & 1) any_higher_key = 1;
                    for (int j = 0; j < (h & 0xffff); j++)
                        if (lst[t * kBatchMaxL + j] == n) held |= 1u << t;
                }
                const bool own = (held >> m) & 1;
                const bool elig = alive && !(held & (unsigned)higher_mask);
                double sc_n = pos_inf();
                if (elig)
                    sc_n = node_score(cnt[m * NX + n], NP > 0 ? ntn_col[row * N] : 0, tot, hasw, w_n, NP, own ? stick : 0.0,
                                      D.booster_kind);

                int chosen[kMaxK];
#pragma unroll
                for (int c = 0; c < kMaxK; c++) chosen[c] = -1;
                int n_out = 0;
                bool emitted = false;
                if (rules) {                                          // plan.go:174-226
                    int hn[kMaxAnchors];
#pragma unroll
                    for (int j = 0; j < kMaxAnchors; j++) hn[j] = -1;
                    int n_hn = 0, cand0 = -2;
                    auto anchor = [&](const AnchorSet* tab, int a) {
                        AnchorSet s = tab[a];
                        s.alo = uni(s.alo); s.ahi = uni(s.ahi); s.blo = uni(s.blo); s.bhi = uni(s.bhi);
                        return s;
                    };
                    for (int r = r0; r < r1; r++) {
                        const AnchorSet* tab = anch + (size_t)r * (NX + 1);
                        int h = top < 0 ? NX : top;                  // anchor NX: the "" vertex
                        if (top < 0 && n_hn > 0) h = hn[0];
                        Fold f;
                        fold_reset(f);
                        fold_step(f, anchor(tab, h), &err);
#pragma unroll
                        for (int j = 0; j < kMaxAnchors; j++)
                            if (j < n_hn) fold_step(f, anchor(tab, hn[j]), &err);
                        for (int i = 0; i < k; i++) {
                            const bool in_set = elig && leaf_n >= 0 && fold_contains(f, leaf_n);
                            int pick = uni(block_argmin<T>(in_set ? sc_n : pos_inf(), in_set ? n : INT_MAX, red, round));
                            if (pick == INT_MAX) {                   // plan.go:216-218
                                if (cand0 == -2) {
                                    cand0 = uni(block_argmin<T>(sc_n, elig ? n : INT_MAX, red, round));
                                    if (cand0 == INT_MAX) cand0 = -1;
                                }
                                pick = cand0;
                            }
                            if (pick >= 0) {
                                if (n_hn >= kMaxAnchors - 1) {
                                    err = 1;
                                } else {
#pragma unroll
                                    for (int j = 0; j < kMaxAnchors; j++) if (j == n_hn) hn[j] = pick;
                                    n_hn++;
                                    fold_step(f, anchor(tab, pick), &err);
                                }
                            }
                        }
                    }
                    // candidateNodes = dedupe(hierarchyNodes ++ candidateNodes), plan.go:224-225
#pragma unroll
                    for (int j = 0; j < kMaxAnchors; j++) {
                        if (j < n_hn && n_out < k) {
                            const int x = hn[j];
                            bool dup = false;
#pragma unroll
                            for (int c = 0; c < kMaxK; c++) if (c < n_out && chosen[c] == x) dup = true;
                            if (!dup) {
#pragma unroll
                                for (int c = 0; c < kMaxK; c++) if (c == n_out) chosen[c] = x;
                                n_out++;
                                if (x == n) emitted = true;
                            }
                        }
                    }
                }
                while (n_out < k) {                                   // the sorted candidates, consumed lazily (plan.go:228-235)
                    const bool cand = elig && !emitted;
                    const int best = uni(block_argmin<T>(cand ? sc_n : pos_inf(), cand ? n : INT_MAX, red, round));
                    if (best == INT_MAX) break;
#pragma unroll
                    for (int c = 0; c < kMaxK; c++) if (c == n_out) chosen[c] = best;
                    n_out++;
                    if (best == n) emitted = true;
                }
                steps++;
                if (n_out < k) {                                      // plan.go:230-235
                    if (tid == 0 && n_warn < D.wcap) {
                        out[D.o_wp + n_warn] = p;
                        out[D.o_ws + n_warn] = m;
                    }
                    n_warn++;
                }
                const bool is_nil = n_out == 0 && D.n_alive == 0 && !any_higher_key && D.hier_nil;
                // commit.  Counters: a node of this state's old list, or a chosen one, leaves every state list of the
                // partition that holds it (plan.go:290-297, once per list however often it is there), a chosen one enters
                // this state's (:301); nodeToNodeCounts (:238-245)
                if (NP > 0 && emitted) ntn_col[row * N] += 1;
                if (n < NX && (own || emitted)) {
                    for (int t = 0; t < M; t++)
                        if ((held >> t) & 1) { cnt[t * NX + n] -= w; tot -= w; }
                }
                if (emitted) { cnt[m * NX + n] += w; tot += w; }
                // lists: thread t < M rewrites state t's list (removal of old and chosen nodes, every present key non-nil),
                // state m's is the chosen list (:299)
                if (tid < M) {
                    const int t = tid, h = lhdr[t];
                    int32_t* dst = live + (p * M + t) * L;
                    if (t == m) {
#pragma unroll
                        for (int c = 0; c < kMaxK; c++) if (c < n_out) dst[c] = chosen[c];
                        lhdr_g[p * M + t] = n_out | ((is_nil ? kListNil : kListSet) << 16);
                    } else if ((h >> 16) != kListAbsent) {
                        const int hm = lhdr[m];
                        const int n_old = (hm >> 16) == kListAbsent ? 0 : (hm & 0xffff);
                        int o = 0;
                        for (int j = 0; j < (h & 0xffff); j++) {
                            const int x = lst[t * kBatchMaxL + j];
                            bool rm = false;
                            for (int i = 0; i < n_old; i++) if (lst[m * kBatchMaxL + i] == x) rm = true;
#pragma unroll
                            for (int c = 0; c < kMaxK; c++) if (c < n_out && chosen[c] == x) rm = true;
                            if (!rm) dst[o++] = x;
                        }
                        lhdr_g[p * M + t] = o | (kListSet << 16);
                    }
                }
            }
        }
        iterations++;
        // convergence: every result partition DeepEquals prevMap[name], plan.go:36-45
        if (tid == 0) shw[0] = 0;
        __syncthreads();
        for (int p = tid; p < P; p += T) {
            bool diff = (pflag[p] & 1) == 0 || (pflag[p] & 2) != 0;
            for (int m = 0; m < M && !diff; m++) {
                const int idx = p * M + m, h = lhdr_g[idx];
                if (h != phdr[idx]) { diff = true; break; }
                for (int j = 0; j < (h & 0xffff); j++)
                    if (live[idx * L + j] != prv[idx * L + j]) { diff = true; break; }
            }
            if (diff) shw[0] = 1;
        }
        __syncthreads();
        const int not_match = shw[0];
        if (!not_match) { converged = 1; break; }
        // prevMap[name] = partitionsToAssign[name] = result, plan.go:49-52
        for (int idx = tid; idx < PM; idx += T) {
            const int h = lhdr_g[idx];
            phdr[idx] = h;
            for (int j = 0; j < (h & 0xffff); j++) prv[idx * L + j] = live[idx * L + j];
        }
        for (int p = tid; p < P; p += T) pflag[p] = 1;
        __syncthreads();
    }

    // the result as CSR over (p * M + state): the lengths of a chunk per thread, an exclusive scan over the threads
    __syncthreads();
    if (iterations == 0) n_warn = 0;                                  // MaxIterationsPerPlan <= 0: (nil, nil)
    const int C = (PM + T - 1) / T;
    const int lo = tid * C < PM ? tid * C : PM, hi = lo + C < PM ? lo + C : PM;
    int s = 0;
    if (iterations > 0)
        for (int idx = lo; idx < hi; idx++) s += lhdr_g[idx] & 0xffff;
    cnt[tid] = s;
    __syncthreads();
    int at = 0, total = 0;
    for (int t = 0; t < T; t++) {
        if (t < tid) at += cnt[t];
        total += cnt[t];
    }
    if (total > D.cap) err = 2;                                       // (cannot happen: lists never outgrow the capacity)
    for (int idx = lo; idx < hi; idx++) {
        const int h = iterations > 0 ? lhdr_g[idx] : 0, len = h & 0xffff;
        out[D.o_off + idx] = at;
        out[D.o_kind + idx] = h >> 16;
        if (at + len <= D.cap)
            for (int j = 0; j < len; j++) out[D.o_nodes + at + j] = live[idx * L + j];
        at += len;
    }
    if (tid == 0) {
        out[D.o_off + PM] = total;
        out[kBoIterations] = iterations;
        out[kBoConverged] = converged;
        out[kBoWarnings] = n_warn;
        out[kBoEntries] = total;
        out[kBoError] = err;
        out[kBoDone] = 1;
        out[kBoSteps] = (int)(steps & 0x7fffffff);
    }
}

}  // namespace blance
