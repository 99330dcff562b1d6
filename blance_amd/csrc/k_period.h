// k_period: an all-blank chain pass (k_pass_chain_planes) whose step records repeat with a period T.
// Part of blance_hip.hip (one translation unit); DESIGN.md section 4.1c.  On by default (options.reserved[2] & 256 or
// BLANCE_PERIODIC=0 turn it off).
#pragma once

namespace blance {

// ============================================================================
// The all-blank pass of a region is a deterministic automaton: its state is the
// region's load counters (NumPartitions == 0, no node weights: a leaf's score is
// its counter, plan.go:634-689), its input per step the words 1..23 of the step's
// compact record (weight, top priority node's exclude class, higher priority
// leaves: plan.go:146-154, :185-212) -- word 0, the step's index in pass order,
// is not read by the chain.  Scores are compared inside the region only, so a
// state is the same state after every live leaf's counter grew by the same d.
//
// If the records repeat with period T from the chain's first step up to step
// `limit`, and the counters after 2T steps are the counters after T steps plus a
// uniform d, then by induction step t >= 2T (t < limit) picks what step t - T
// picked: the chain is walked for 2T steps, the rest of the periodic stretch is
// copied data-parallel, its counters follow in closed form, and the chain kernel
// walks whatever lies behind `limit`.  BASELINE config 3: T = 128 (the primaries
// cycle through a zone), 32,768 steps per region -> 256 walked, 32,512 copied.
// Nothing is assumed: both conditions are checked on the device for every region,
// and a region that fails either is walked in full by the same kernel.  (The first
// is not SEARCHED for where the driver holds it from the upload: k_period_find's
// known mode.)
// ============================================================================
constexpr int kPeriodCap = 4096;                 // longest period looked for
constexpr int kPeriodMinRounds = 4;              // a region joins if its periodic stretch is at least this many periods

// per region arrays of the period buffer, B ints each
enum { kPT = 0, kPLimit, kPOk, kPD, kPBeg1, kPEnd1, kPBeg2, kPEnd2, kPBeg3, kPEnd3, kPWords };

__device__ __forceinline__ bool period_same_input(const int32_t* a, const int32_t* b) {
    bool same = true;
#pragma unroll
    for (int j = 1; j < kCW; j++) same = same && a[j] == b[j];
    return same;
}

// One workgroup per region: T[rg] = smallest t > 0 (t <= kPeriodCap) whose record equals the first step's, INT_MAX if
// none.  The workgroup looks at blockDim.x candidates per trip in rising order and stops after the first trip with a
// match (config 3: T = 128, one trip); then it sets up the region's other words, which once took a launch of their own:
// limit = the chain's length (k_period_verify narrows it behind the kernel boundary), not ok, no d yet.
//
// known != 0: THE PERIOD WITHOUT THE SEARCH.  The driver holds that the pass before this one was committed as a round robin
// over nodesNext (k_fresh_cycle_commit: step j of the pass order took alive_ids[j % A]), that this pass runs in the same
// order, and that words 1..23 of a record are a function of the step's top priority node alone (run_state_pass lists
// the conditions).  The grouping by region is stable, so the chain of region rg has the region's nodes of nodesNext as
// its tops, in id order, again and again from its first step to its last; distinct nodes lie on distinct leaves, so the
// smallest t whose record equals the first step's is their number, and no step breaks the repetition -- what the search and
// k_period_verify would find: T = the region's count of alive leaves (k_period_judge's test of a leaf) if a candidate,
// limit = the chain's length.  No record is read, and k_period_verify is not launched.
__global__ __launch_bounds__(1024) void k_period_find(int B, int known, int N, const int32_t* reg_off, const int32_t* reg_lo,
                                                      const int32_t* reg_hi, const int32_t* leaf_node, const uint8_t* alive,
                                                      const int32_t* crec, int32_t* pb) {
    BLANCE_DYN_LDS(lds);
    int* best = (int*)lds;
    const int rg = blockIdx.x, tid = threadIdx.x;
    const int cbeg = reg_off[rg], len = reg_off[rg + 1] - cbeg;
    const int last = len - 1 < kPeriodCap ? len - 1 : kPeriodCap;       // candidates: t in [1, last]
    if (known) {
        if (tid == 0) *best = 0;
        __syncthreads();
        int mine = 0;
        for (int pos = reg_lo[rg] + tid; pos < reg_hi[rg]; pos += (int)blockDim.x) {
            const int n = leaf_node[pos];
            if (n >= 0 && n < N && alive[n]) mine++;
        }
        if (mine) atomicAdd(best, mine);
        __syncthreads();
        if (tid == 0) {
            const int count = *best;
            pb[kPT * B + rg] = (count >= 1 && count <= last) ? count : INT_MAX;
            pb[kPLimit * B + rg] = len;
            pb[kPOk * B + rg] = 0;
            pb[kPD * B + rg] = INT_MIN;
        }
        return;
    }
    if (tid == 0) *best = INT_MAX;
    __syncthreads();
    int found = INT_MAX;
    for (int base = 1; base <= last && found == INT_MAX; base += (int)blockDim.x) {
        const int t = base + tid;
        if (t <= last && period_same_input(crec + (size_t)cbeg * kCW, crec + (size_t)(cbeg + t) * kCW)) atomicMin(best, t);
        __syncthreads();
        found = *best;
        __syncthreads();                            // (everyone has read it before the next trip's matches land)
    }
    if (tid == 0) {
        pb[kPT * B + rg] = found;
        pb[kPLimit * B + rg] = len;
        pb[kPOk * B + rg] = 0;
        pb[kPD * B + rg] = INT_MIN;
    }
}

// limit[rg] = first step t >= T whose record differs from step t - T's (the chain's length if none).  One thread per 16 bytes
// of the region's records (a record is kCW / 4 = 6 of them; word 0 of a record, the step's pass index, does not count): the
// loads of a wave are one contiguous 1 KB, and the piece T records back is in the L2 (12 KB behind at T = 128) -- the 100 MB
// of config 3's records cross the HBM interface once.  (One thread per RECORD, each reading its 96 bytes, ran at 0.5 TB/s.)
__global__ void k_period_verify(int B, int gx, const int32_t* reg_off, const int32_t* crec, int32_t* pb) {
    static_assert(kCW % 4 == 0, "records are whole 16-byte pieces");
    constexpr int per = kCW / 4;
    const int rg = blockIdx.x / gx;
    const int cbeg = reg_off[rg], len = reg_off[rg + 1] - cbeg;
    const int T = pb[kPT * B + rg];
    const long long qi = (long long)(blockIdx.x % gx) * blockDim.x + threadIdx.x;
    const long long t = qi / per;
    if (T < 1 || T > kPeriodCap || t < T || t >= len) return;
    const int4* r4 = (const int4*)(crec + (size_t)cbeg * kCW);
    const int4 a = r4[qi], b = r4[qi - (long long)per * T];
    const bool same = a.y == b.y && a.z == b.z && a.w == b.w && (qi % per == 0 || a.x == b.x);
    if (!same) atomicMin(pb + kPLimit * B + rg, (int)t);
}

// the first two segments: [0, T) and [T, 2T) of a region that joins, the whole chain and nothing of one that does not
// cut > 0, a test knob (BLANCE_PERIODIC_CUT=n): the periodic stretch ends after n steps at the latest -- any prefix of a
// periodic stretch is one; what lies behind is walked by the chain kernel (the path a chain with a non-periodic tail takes)
__global__ void k_period_segments(int B, int cut, const int32_t* reg_off, int32_t* pb) {
    const int rg = blockIdx.x * blockDim.x + threadIdx.x;
    if (rg >= B) return;
    const int cbeg = reg_off[rg], cend = reg_off[rg + 1];
    int limit = pb[kPLimit * B + rg];
    if (cut > 0 && limit > cut) pb[kPLimit * B + rg] = limit = cut;
    const int T = pb[kPT * B + rg];
    const bool joins = T >= 1 && T <= kPeriodCap && (long long)limit >= (long long)kPeriodMinRounds * T;
    pb[kPOk * B + rg] = joins ? 1 : 0;
    pb[kPBeg1 * B + rg] = cbeg;
    pb[kPEnd1 * B + rg] = joins ? cbeg + T : cend;
    pb[kPBeg2 * B + rg] = joins ? cbeg + T : cend;
    pb[kPEnd2 * B + rg] = joins ? cbeg + 2 * T : cend;
    pb[kPBeg3 * B + rg] = cend;
    pb[kPEnd3 * B + rg] = cend;
}

// One workgroup per region, behind the second walk: are the counters after 2T steps (cnt) those after T steps (cnt1) plus
// the same d on every live leaf?  The largest difference over the region's live leaves, every difference against it, the
// verdict with the third segment -- behind `limit` if so, behind 2T if not -- and, if so, the counters behind the copied
// stretch: d per full period on every live leaf, and the picks of the stretch's last, partial period one by one.  Those
// are read from `out` of steps [T, 2T), which the second walk wrote and k_period_replicate leaves alone: this kernel may
// run before it, each with the weight of its own record (word 1 of step T + j, which is step 2T + full * T + j's: the records
// repeat) -- weights may differ inside a period while d is uniform (64 leaves taken in turn, 64 steps of weight 1 and 64 of
// weight 2: d = 3), and the count does not rest on the pass order keeping a chain to one weight: k_pass_chain_blank takes the
// weight per batch of steps, and the sort by weight is the caller's, not this kernel's.  Everything here belongs to the region -- its leaves' counters, its chain's outputs, its words of pb --
// and the workgroup is the only one that touches it.  The workgroup loops over the leaves when there are more than threads.
// (A leaf that is no candidate never moves: one that did refutes the region.  flags[kFlagEscaped]: a chain of the walks so
// far had to escape -- it published nothing, the host will redo the whole pass with k_pass_chain from the saved counters:
// then nothing is copied either.  Without this a walk that escaped in its second period left the counters where the first
// period had put them, "the same d = 0 on every leaf" passed for a verdict, and the outputs of steps nobody had written
// were replicated and counted -- node ids out of whatever the buffer held.)
__global__ void k_period_judge(int B, int s, int N, int NX, int OW, const int32_t* reg_off, const int32_t* reg_lo,
                               const int32_t* reg_hi, const int32_t* leaf_node, const uint8_t* alive, const int32_t* crec,
                               const int32_t* out, const int32_t* flags, const int32_t* cnt1, int32_t* cnt, int32_t* pb) {
    BLANCE_DYN_LDS(lds);
    int* red = (int*)lds;                            // [0] the largest difference, [1] refuted
    const int rg = blockIdx.x, tid = threadIdx.x;
    const int cbeg = reg_off[rg], cend = reg_off[rg + 1];
    const int T = pb[kPT * B + rg], limit = pb[kPLimit * B + rg];
    // (k_period_segments left ok = joins; of a region that does not join segment 1 was the whole chain, 2 and 3 are empty)
    if (!(T >= 1 && T <= kPeriodCap && (long long)limit >= (long long)kPeriodMinRounds * T)) return;
    const int lo = reg_lo[rg], hi = reg_hi[rg];
    if (tid == 0) { red[0] = INT_MIN; red[1] = 0; }
    __syncthreads();
    for (int pos = lo + tid; pos < hi; pos += (int)blockDim.x) {
        const int n = leaf_node[pos];
        if (n < 0) continue;
        const int diff = cnt[s * NX + n] - cnt1[s * NX + n];
        if (n < N && alive[n]) atomicMax(&red[0], diff);
        else if (diff != 0) atomicOr(&red[1], 1);
    }
    __syncthreads();
    const int d = red[0];
    for (int pos = lo + tid; pos < hi; pos += (int)blockDim.x) {
        const int n = leaf_node[pos];
        if (n >= 0 && n < N && alive[n] && cnt[s * NX + n] - cnt1[s * NX + n] != d) atomicOr(&red[1], 1);
    }
    __syncthreads();
    const bool ok = red[1] == 0 && d != INT_MIN && d >= 0 && flags[kFlagEscaped] == 0;
    if (tid == 0) {
        pb[kPD * B + rg] = d;
        pb[kPOk * B + rg] = ok ? 1 : 0;
        pb[kPBeg3 * B + rg] = ok ? cbeg + limit : cbeg + 2 * T;
        pb[kPEnd3 * B + rg] = cend;
    }
    if (!ok) return;
    const int copied = limit - 2 * T, full = copied / T, rest = copied % T;
    for (int pos = lo + tid; pos < hi; pos += (int)blockDim.x) {
        const int n = leaf_node[pos];
        if (n >= 0 && n < N && alive[n]) cnt[s * NX + n] += d * full;
    }
    __syncthreads();
    for (int j = tid; j < rest; j += (int)blockDim.x) {
        const int32_t* o = out + (size_t)(cbeg + T + j) * OW;
        const int w = crec[(size_t)(cbeg + T + j) * kCW + 1];      // the step's own weight
        const int n_out = o[0] & 0xffff;
        for (int c = 0; c < n_out; c++) {
            const int n = o[1 + c];
            if (n >= 0 && n < NX) atomicAdd(cnt + s * NX + n, w);
        }
    }
}

// grid: gx workgroups per region over its steps: step t in [2T, limit) emits what step T + (t - T) % T emitted
__global__ void k_period_replicate(int B, int gx, int OW, const int32_t* reg_off, const int32_t* pb, int32_t* out) {
    const int rg = blockIdx.x / gx;
    if (!pb[kPOk * B + rg]) return;
    const int cbeg = reg_off[rg];
    const int T = pb[kPT * B + rg], limit = pb[kPLimit * B + rg];
    const int t = 2 * T + (blockIdx.x % gx) * blockDim.x + threadIdx.x;
    if (t >= limit) return;
    const int32_t* src = out + (size_t)(cbeg + T + (t - T) % T) * OW;
    int32_t* dst = out + (size_t)(cbeg + t) * OW;
    for (int j = 0; j < OW; j++) dst[j] = src[j];
}

}  // namespace blance
