// k_batch_moves: CalcPartitionMoves (moves.go:41-136) for every partition of every batched problem that asks for them, one
// workgroup per problem, launched after k_plan_batch on the same stream.  The begin map is the problem's prevMap as the
// call passed it: the packed input lists (the input slice is const, k_plan_batch's write-back of plan.go:49-52 goes to its
// scratch copy) and the beg_other CSR behind the input slice; the end map is the result CSR k_plan_batch wrote.  The moves
// land in the problem's output slice, so the batch's one download brings them back.  DESIGN.md §4.9.
#pragma once

namespace blance {

__global__ __launch_bounds__(kBatchMovesThreads) void k_batch_moves(BatchMovesParams bp) {
    constexpr int T = kBatchMovesThreads;
    const BatchMovesDesc& V = bp.mdesc[blockIdx.x];
    const BatchDesc& D = bp.desc[V.desc];
    const int32_t* in = bp.in + D.in_base;
    int32_t* sc = bp.sc + D.sc_base;
    int32_t* out = bp.out + D.out_base;
    if (!batch_planned(out)) return;              // not planned exactly here: the host takes the single path (uniform exit)
    const int tid = threadIdx.x, M = D.M, P = D.P, L = D.L, S = V.stride;
    const int32_t* phdr = in + D.i_phdr;          // prevMap lists [P*M][L], lengths in the low half of the header
    const int32_t* plist = in + D.i_plist;
    const int32_t* ooff = in + V.i_ooff;          // keys outside the model: CSR over partitions
    const int32_t* onod = in + V.i_onodes;
    const int32_t* eoff = out + D.o_off;          // result: CSR over p * M + state
    const int32_t* enod = out + D.o_nodes;
    int32_t* cnt = sc + V.s_cnt;
    int32_t* mv = sc + V.s_mv;

    // phase 1: each thread a stride of partitions, its moves into the partition's scratch slice (stride >= the distinct
    // nodes of begin and end, which bounds the moves: addMoves keeps a node once, moves.go:49-58)
    for (int p = tid; p < P; p += T) {
        int32_t* slot = mv + (int64_t)p * S;
        int n = 0;
        auto in_beg = [&](int t, int x) {                                    // t == M: the keys outside the model
            const int32_t* a = t < M ? plist + (int64_t)(p * M + t) * L : onod + ooff[p];
            const int len = t < M ? (phdr[p * M + t] & 0xffff) : ooff[p + 1] - ooff[p];
            for (int j = 0; j < len; j++) if (a[j] == x) return true;
            return false;
        };
        auto in_end = [&](int t, int x) {
            for (int j = eoff[p * M + t]; j < eoff[p * M + t + 1]; j++) if (enod[j] == x) return true;
            return false;
        };
        auto add_move = [&](int x, int state, int kind) {                   // addMoves + seen, moves.go:49-58
            for (int j = 0; j < n; j++) if ((slot[j] & 0xffff) == x) return;
            if (n == S) return;                                             // (never: S bounds the distinct nodes)
            slot[n++] = x | ((state + 1) << 16) | (kind << 24);
        };
        auto state_changes = [&](int si, int lo, int hi, int kind) {        // findStateChanges, moves.go:121-136
            for (int e = eoff[p * M + si]; e < eoff[p * M + si + 1]; e++) {
                const int x = enod[e];
                for (int t = lo; t < hi; t++) if (in_beg(t, x)) add_move(x, si, kind);
            }
        };
        auto adds = [&](int si) {                 // end[si] - beg[si], intersected with end nodes in no begin list (:77-82)
            for (int e = eoff[p * M + si]; e < eoff[p * M + si + 1]; e++) {
                const int x = enod[e];
                bool any = false;
                for (int t = 0; t <= M && !any; t++) any = in_beg(t, x);
                if (!any) add_move(x, si, BLANCE_OP_ADD);
            }
        };
        auto dels = [&](int si) {                 // beg[si] - end[si], intersected with begin nodes in no end list (:84-89)
            const int len = phdr[p * M + si] & 0xffff;
            for (int j = 0; j < len; j++) {
                const int x = plist[(int64_t)(p * M + si) * L + j];
                bool any = false;
                for (int t = 0; t < M && !any; t++) any = in_end(t, x);
                if (!any) add_move(x, -1, BLANCE_OP_DEL);
            }
        };
        if (!V.favor_min_nodes) {                                           // moves.go:66-91
            for (int si = 0; si < M; si++) {
                state_changes(si, si + 1, M, BLANCE_OP_PROMOTE);
                state_changes(si, 0, si, BLANCE_OP_DEMOTE);
                adds(si);
                dels(si);
            }
        } else {                                                            // moves.go:92-116
            for (int si = M - 1; si >= 0; si--) {
                dels(si);
                state_changes(si, 0, si, BLANCE_OP_DEMOTE);
                state_changes(si, si + 1, M, BLANCE_OP_PROMOTE);
                adds(si);
            }
        }
        cnt[p] = n;
    }
    __syncthreads();

    // phase 2: exclusive scan of the counts in partition order (a chunk per thread, as k_plan_batch's CSR tail);
    // phase 3: each thread compacts its chunk into the output slice
    BLANCE_DYN_LDS(lds);
    int* sums = (int*)lds;                        // [T]
    const int C = (P + T - 1) / T;
    const int lo = tid * C < P ? tid * C : P, hi = lo + C < P ? lo + C : P;
    int s = 0;
    for (int p = lo; p < hi; p++) s += cnt[p];
    sums[tid] = s;
    __syncthreads();
    int at = 0, total = 0;
    for (int t = 0; t < T; t++) {
        if (t < tid) at += sums[t];
        total += sums[t];
    }
    int32_t* moff = out + V.o_moff;
    int32_t* mops = out + V.o_mops;
    for (int p = lo; p < hi; p++) {
        const int n = cnt[p];
        const int32_t* slot = mv + (int64_t)p * S;
        moff[p] = at;
        if (at + n <= V.cap)                      // (always: the capacity counts every begin and end entry)
            for (int j = 0; j < n; j++) mops[at + j] = slot[j];
        at += n;
    }
    if (tid == 0) moff[P] = total;
}

}  // namespace blance
