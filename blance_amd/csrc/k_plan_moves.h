// k_plan_moves: CalcPartitionMoves (moves.go:41-136) for every partition of the plan the context holds
// (blance_plan_moves_get), one thread per partition, read where the two maps already lie: the begin map is prevMap as it
// was uploaded (the CSR p_off / p_nodes, M lists per partition, plus the caller's beg_other CSR as pseudo state M), the
// end map the planned lists at stride L (result_problem).  Part of blance_hip.hip; DESIGN.md §4.11.
//
// Two passes of the same walk instead of per-partition scratch slices and a compaction: k_plan_moves<false> counts the
// moves of every partition (and the call's six counters), the host scans the counts, k_plan_moves<true> writes every move
// once, at its final place.  The counters of the call (all moves, moves per kind, partitions with a move) come out of the
// counting pass.
//
// `seen` (addMoves keeps a node once, moves.go:49-58) is kept nowhere.  Whether a node moves, and in which phase of the
// walk first, follows from two bit masks alone -- B(x): the begin states that hold x (bit M: a key outside the model),
// E(x): the end states that hold x:
//   promote(s): s in E and B has a model state behind s      demote(s): s in E and B has a model state before s
//   add(s):     s in E and B is empty                          del(s):    s in B (model) and E is empty
// so x is a candidate in state s exactly when
//   B == 0:            s in E                   (an add)
//   B != 0, E != 0:    s in E and B has a model state other than s   (promote / demote, whichever phase comes first)
//   E == 0:            s in B (model)           (a del)
// and the move it gets is the one of the FIRST such s in walk order (ascending, or descending with favorMinNodes).  An
// element of a list emits its move when the list's state is that first state and no earlier element of the same list is
// the same node; within a phase the moves keep list order, as findStateChanges / StringsIntersectStrings do.  Nothing
// depends on what the thread emitted before, so the counting pass needs no storage at all and both passes agree by
// construction.
#pragma once

namespace blance {

struct PlanMovesParams {
    int32_t P, M, L, favor_min_nodes;
    const int32_t* beg_off; const int32_t* beg_nodes;   // prevMap as uploaded: CSR over p * M + state
    const uint8_t* in_prev;                             // [P] 0: the partition's begin map is empty
    const int32_t* other_off; const int32_t* other_nodes;   // keys outside the model: CSR over partitions, or both null
    const int32_t* end; const int32_t* end_len; const uint8_t* end_kind;   // the planned lists [P*M][L]
    int32_t* n_moves;                // [P + 1]: pass 1 writes the counts (and 0 behind them), pass 2 reads the offsets
    unsigned long long* counters;    // zeroed, word i at counters[i * kPlanMovesCounterStride]: all moves, moves per
                                     // BLANCE_OP_*, partitions with a move (pass 1)
    int32_t* op_node; int32_t* op_state; int32_t* op_kind;     // pass 2
};

// The counting pass runs on at most kPlanMovesMaxWgs workgroups that stride over the partitions: a workgroup folds its
// four waves in LDS and makes one atomic per counter, each counter on a cache line of its own.  (One atomic per wave and
// word, 16 K waves at the full size on six words of one line, took 0.81 ms of which the walk is 0.08: k_validate_parts
// met the same wall.)
constexpr int kPlanMovesMaxWgs = 2048, kPlanMovesCounterStride = 16;

template <bool WRITE>
__global__ __launch_bounds__(256) void k_plan_moves(PlanMovesParams q) {
    int n_add = 0, n_del = 0, n_pro = 0, n_dem = 0, moved = 0;
    const int stride = (int)(gridDim.x * blockDim.x), p_end = WRITE ? q.P : q.P + 1;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < p_end; p += stride) {
    int n = 0;
    if (p < q.P) {
        const int M = q.M, L = q.L, base = p * M;
        const bool favor = q.favor_min_nodes != 0, has_beg = q.in_prev[p] != 0;
        const unsigned model = (1u << M) - 1u;                               // (M <= kMaxStates = 16)
        const int o0 = q.other_off ? q.other_off[p] : 0, o1 = q.other_off ? q.other_off[p + 1] : 0;
        const int out0 = WRITE ? q.n_moves[p] : 0, out1 = WRITE ? q.n_moves[p + 1] : 0;
        auto end_list = [&](int t) { return q.end + (size_t)(base + t) * L; };
        auto end_count = [&](int t) { return q.end_kind[base + t] == kListAbsent ? 0 : q.end_len[base + t]; };
        auto beg_mask = [&](int x) {
            unsigned b = 0;
            if (has_beg)
                for (int t = 0; t < M; t++)
                    for (int j = q.beg_off[base + t]; j < q.beg_off[base + t + 1]; j++) if (q.beg_nodes[j] == x) b |= 1u << t;
            for (int j = o0; j < o1; j++) if (q.other_nodes[j] == x) b |= 1u << M;
            return b;
        };
        auto end_mask = [&](int x) {
            unsigned e = 0;
            for (int t = 0; t < M; t++) {
                const int32_t* l = end_list(t);
                const int len = end_count(t);
                for (int j = 0; j < len; j++) if (l[j] == x) e |= 1u << t;
            }
            return e;
        };
        auto first_of = [&](unsigned m) { return favor ? 31 - __builtin_clz(m) : __builtin_ctz(m); };   // (m != 0)
        auto emit = [&](int at, int x, int state, int kind) {
            if (WRITE && out0 + at < out1) {                                 // (always: both passes count the same moves)
                q.op_node[out0 + at] = x; q.op_state[out0 + at] = state; q.op_kind[out0 + at] = kind;
            }
        };
        // the move of end[si]'s element e (findStateChanges, moves.go:121-136; the clean adds, :77-82), or -1
        auto end_move = [&](int si, const int32_t* l, int e) {
            const int x = l[e];
            for (int j = 0; j < e; j++) if (l[j] == x) return -1;
            const unsigned B = beg_mask(x), Bm = B & model;
            if (B == 0) return first_of(end_mask(x)) == si ? BLANCE_OP_ADD : -1;
            if ((Bm & ~(1u << si)) == 0) return -1;                          // begin holds it here only, or outside the model only
            const unsigned cand = end_mask(x) & ~((Bm & (Bm - 1)) ? 0u : Bm);     // one begin state: that state moves nothing
            if (first_of(cand) != si) return -1;
            if (favor) return (Bm & ((1u << si) - 1u)) ? BLANCE_OP_DEMOTE : BLANCE_OP_PROMOTE;
            return (Bm >> (si + 1)) ? BLANCE_OP_PROMOTE : BLANCE_OP_DEMOTE;
        };
        auto tally = [&](int kind) {
            n_add += kind == BLANCE_OP_ADD; n_del += kind == BLANCE_OP_DEL;
            n_pro += kind == BLANCE_OP_PROMOTE; n_dem += kind == BLANCE_OP_DEMOTE;
        };
        // promote, demote, add in the order of the walk (moves.go:68-82; :100-115 with favorMinNodes: demote first)
        auto state_moves = [&](int si) {
            const int32_t* l = end_list(si);
            const int len = end_count(si);
            const int k0 = favor ? BLANCE_OP_DEMOTE : BLANCE_OP_PROMOTE;
            int c0 = 0, c1 = 0, c2 = 0;
            for (int e = 0; e < len; e++) {
                const int kind = end_move(si, l, e);
                if (kind < 0) continue;
                if (!WRITE) tally(kind);
                if (kind == BLANCE_OP_ADD) c2++; else if (kind == k0) c0++; else c1++;
            }
            if (WRITE && c0 + c1 + c2 > 0) {
                int a0 = n, a1 = n + c0, a2 = n + c0 + c1;
                for (int e = 0; e < len; e++) {
                    const int kind = end_move(si, l, e);
                    if (kind < 0) continue;
                    emit(kind == BLANCE_OP_ADD ? a2++ : kind == k0 ? a0++ : a1++, l[e], si, kind);
                }
            }
            n += c0 + c1 + c2;
        };
        auto clean_dels = [&](int si) {                                      // moves.go:84-89
            if (!has_beg) return;
            const int b0 = q.beg_off[base + si], b1 = q.beg_off[base + si + 1];
            for (int e = b0; e < b1; e++) {
                const int x = q.beg_nodes[e];
                bool dup = false;
                for (int j = b0; j < e; j++) dup |= q.beg_nodes[j] == x;
                if (dup || end_mask(x) != 0 || first_of(beg_mask(x) & model) != si) continue;
                if (!WRITE) tally(BLANCE_OP_DEL);
                emit(n, x, -1, BLANCE_OP_DEL);
                n++;
            }
        };
        if (!favor) {
            for (int si = 0; si < M; si++) { state_moves(si); clean_dels(si); }
        } else {
            for (int si = M - 1; si >= 0; si--) { clean_dels(si); state_moves(si); }
        }
    }
    if (!WRITE) {
        q.n_moves[p] = n;                                                    // (p == P: the 0 the scan turns into the total)
        moved += n > 0;
    }
    }
    if (!WRITE) {
        // the call's counters: wave sums, the workgroup's waves through LDS, one 64-bit atomic per word (every thread of the
        // workgroup is here; a sum of one kind fits 32 bits: adds, promotes and demotes are end entries, dels begin entries)
        BLANCE_DYN_LDS(lds);
        int (*red)[5] = (int (*)[5])lds;                                     // [waves][5]
        for (int o = 32; o; o >>= 1) {
            n_add += __shfl_xor(n_add, o, 64); n_del += __shfl_xor(n_del, o, 64);
            n_pro += __shfl_xor(n_pro, o, 64); n_dem += __shfl_xor(n_dem, o, 64);
            moved += __shfl_xor(moved, o, 64);
        }
        const int wv = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) {
            red[wv][BLANCE_OP_ADD] = n_add; red[wv][BLANCE_OP_DEL] = n_del; red[wv][BLANCE_OP_PROMOTE] = n_pro;
            red[wv][BLANCE_OP_DEMOTE] = n_dem; red[wv][4] = moved;
        }
        __syncthreads();
        if (threadIdx.x < 5) {                                               // thread k: counter 1 + k
            unsigned long long sum = 0;
            for (int w = 0; w < (int)(blockDim.x >> 6); w++) sum += (unsigned long long)red[w][threadIdx.x];
            if (sum) atomicAdd(q.counters + (1 + threadIdx.x) * kPlanMovesCounterStride, sum);
        }
        if (threadIdx.x == 5) {                                              // all moves
            unsigned long long sum = 0;
            for (int w = 0; w < (int)(blockDim.x >> 6); w++)
                for (int k = 0; k < 4; k++) sum += (unsigned long long)red[w][k];
            if (sum) atomicAdd(q.counters, sum);
        }
    }
}

}  // namespace blance
