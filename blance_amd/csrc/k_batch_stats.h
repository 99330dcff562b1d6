// k_batch_stats: the plan statistics of blance_plan_stats_get for every batched problem that asks for them, one workgroup
// per problem, launched after k_plan_batch on the same stream (before or after k_batch_moves: neither reads the other's
// words).  It restates k_stats_load, k_stats_rules and k_stats_reduce (k_sweep.h) for one problem: the map is the result
// CSR k_plan_batch wrote into the problem's output slice, everything else comes from the packed input slice.  The numbers
// land in the problem's output slice as int64, so the batch's one download brings them back.  DESIGN.md §4.10.
#pragma once

namespace blance {

// a 64-bit value from lane ^ mask (two 32-bit cross-lane moves)
__device__ __forceinline__ long long shfl_xor_i64(long long v, int mask) {
    const int lo = __shfl_xor((int)(unsigned)((unsigned long long)v & 0xffffffffull), mask);
    const int hi = __shfl_xor((int)((unsigned long long)v >> 32), mask);
    return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo);
}

__global__ __launch_bounds__(kBatchStatsThreads) void k_batch_stats(BatchStatsParams bp) {
    constexpr int T = kBatchStatsThreads, W = T / 64;
    const BatchStatsDesc& V = bp.sdesc[blockIdx.x];
    const BatchDesc& D = bp.desc[V.desc];
    const int32_t* in = bp.in + D.in_base;
    int32_t* out = bp.out + D.out_base;
    if (!batch_planned(out)) return;              // not planned exactly here: the host takes the single path (uniform exit)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = D.N, NX = D.NX, M = D.M, P = D.P;
    long long* res = (long long*)(out + V.o_stats);                 // [1 + 7 M]
    if (out[kBoIterations] == 0) {                // MaxIterationsPerPlan <= 0: no map, every number 0
        for (int i = tid; i < 1 + kBatchStatsArrays * M; i += T) res[i] = 0;
        return;
    }
    const int32_t* st = in + D.i_state;
    const int32_t* rule_off = in + D.i_rule_off;
    const int32_t* node = in + D.i_node;
    const int32_t* part = in + D.i_part;
    const AnchorSet* anch = (const AnchorSet*)(in + D.i_anch);      // [R][NX + 1], entry NX the anchor ""
    const int32_t* eoff = out + D.o_off;          // result: CSR over p * M + state
    const int32_t* ekind = out + D.o_kind;
    const int32_t* enod = out + D.o_nodes;

    BLANCE_DYN_LDS(lds);
    unsigned long long* acc = (unsigned long long*)lds;             // [2][M] unmet slots, rule violations
    long long* wred = (long long*)(acc + 2 * M);                    // [M][5][W] the waves' partial reductions
    int* load = (int*)(wred + M * 5 * W);                           // [M][NX] countStateNodes of the result
    for (int i = tid; i < 2 * M; i += T) acc[i] = 0;
    for (int i = tid; i < M * NX; i += T) load[i] = 0;
    __syncthreads();

    // k_stats_load and k_stats_rules: thread tid keeps state tid % M and strides over the partitions, T / M at a time, so
    // its two counters belong to one state
    const int G = M > 0 ? T / M : 0;
    if (tid < G * M) {
        const int m = tid % M;
        const int k = st[m * 4 + 1] > 0 ? st[m * 4 + 1] : 0;
        const int r0 = rule_off[m], r1 = rule_off[m + 1];
        unsigned long long unmet = 0, viol = 0;
        for (int p = tid / M; p < P; p += G) {
            const int idx = p * M + m;
            const int beg = eoff[idx], len = ekind[idx] == kListAbsent ? 0 : eoff[idx + 1] - beg;
            const int w = (!D.weights_nil && (part[p * 2 + 1] & 1)) ? part[p * 2] : 1;          // plan.go:387-394
            for (int i = 0; i < len; i++) atomicAdd(&load[m * NX + enod[beg + i]], w);
            if (len < k) unmet += (unsigned long long)(k - len);
            if (r1 <= r0) continue;
            const int ti = p * M + D.top_state;
            const int top = (ekind[ti] != kListAbsent && eoff[ti + 1] > eoff[ti]) ? enod[eoff[ti]] : NX;
            for (int i = 0; i < len; i++) {
                const int lp = node[enod[beg + i] * 4 + 2];
                bool v = false;
                for (int r = r0; r < r1 && !v; r++)
                    for (int j = -1; j < i && !v; j++) {
                        const AnchorSet a = anch[(size_t)r * (NX + 1) + (j < 0 ? top : enod[beg + j])];
                        v = lp < a.alo || lp >= a.ahi || (lp >= a.blo && lp < a.bhi);
                    }
                viol += v;
            }
        }
        if (unmet) atomicAdd(&acc[m], unmet);
        if (viol) atomicAdd(&acc[M + m], viol);
    }
    __syncthreads();

    // k_stats_reduce: per state min / max / sum / sum of squares / nodes in use over nodesNext (plan.go:77), in int64:
    // across the lanes of each wave, then across the waves through LDS
    for (int m = 0; m < M; m++) {
        long long mn = LLONG_MAX, mx = LLONG_MIN, sum = 0, sq = 0, used = 0;
        for (int n = tid; n < N; n += T) {
            if (node[n * 4 + 1] & 1) continue;
            const long long v = load[m * NX + n];
            mn = v < mn ? v : mn;
            mx = v > mx ? v : mx;
            sum += v;
            sq += v * v;
            used += v > 0;
        }
        for (int off = 32; off >= 1; off >>= 1) {
            const long long omn = shfl_xor_i64(mn, off), omx = shfl_xor_i64(mx, off);
            mn = omn < mn ? omn : mn;
            mx = omx > mx ? omx : mx;
            sum += shfl_xor_i64(sum, off);
            sq += shfl_xor_i64(sq, off);
            used += shfl_xor_i64(used, off);
        }
        if (lane == 0) {
            long long* s = wred + (m * 5) * W + wave;
            s[0] = mn; s[W] = mx; s[2 * W] = sum; s[3 * W] = sq; s[4 * W] = used;
        }
    }
    __syncthreads();
    if (tid < M) {
        const int m = tid;
        const long long* s = wred + (m * 5) * W;
        long long mn = s[0], mx = s[W], sum = s[2 * W], sq = s[3 * W], used = s[4 * W];
        for (int v = 1; v < W; v++) {
            mn = s[v] < mn ? s[v] : mn;
            mx = s[W + v] > mx ? s[W + v] : mx;
            sum += s[2 * W + v];
            sq += s[3 * W + v];
            used += s[4 * W + v];
        }
        const bool any = D.n_alive > 0;
        res[1 + m] = any ? mn : 0;
        res[1 + M + m] = any ? mx : 0;
        res[1 + 2 * M + m] = any ? sum : 0;
        res[1 + 3 * M + m] = any ? sq : 0;
        res[1 + 4 * M + m] = any ? used : 0;
        res[1 + 5 * M + m] = (long long)acc[m];
        res[1 + 6 * M + m] = (long long)acc[M + m];
    }
    if (tid == 0) res[0] = D.n_alive;
}

}  // namespace blance
