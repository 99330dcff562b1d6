// blance_plan_adopt: the planned map becomes the next call's prevMap and partitionsToAssign where it lies.
// Two kernels around launch_scan_excl: k_adopt_len measures the planned lists (lengths for the scan, and the summary a fresh
// upload's k_validate_parts would have made of them), k_adopt_write streams them out of the working state's strided rows
// into the problem's two CSRs.  Part of blance_hip.hip (one translation unit).
#pragma once

namespace blance {

constexpr int kAdoptMaxWgs = 2048;     // k_adopt_len's grid: a workgroup folds its waves in LDS and makes one atomic per word
constexpr int kAdoptLists = 256;       // (partition, state) lists per workgroup of k_adopt_write
// Summary block of k_adopt_len, zeroed by the caller: the words of k_validate_parts' result block that depend on the lists
// ([1] longest list, [10] the kinds of the lists to assign, 64-bit words from byte 16: [0] result capacity, [2] |weight| *
// prev entries), and 64-bit word [4]: the entries of all lists.
constexpr int kAdoptResWords = 16;
constexpr int kAdoptResLongest = 1, kAdoptResKinds = 10, kAdoptRes64Cap = 0, kAdoptRes64Prev = 2, kAdoptRes64Total = 4;

struct AdoptParams {
    int32_t P, M, L, weights_nil;
    int32_t k[kMaxStates];
    // the planned map (result_problem: prevMap as the last sweep wrote it back), rows of L words
    const int32_t* prv; const int32_t* prv_len; const uint8_t* prv_kind;
    const int32_t* part_weight; const uint8_t* part_has_weight;
    int32_t* len;                  // [P*M + 1] k_adopt_len: list lengths, [P*M] = 0; exclusive offsets after the scan
    int32_t* res;                  // [kAdoptResWords]
    // k_adopt_write's outputs: both CSRs ([P*M + 1], [len[P*M]], [P*M]) and the two per-partition flags [P]
    int32_t* a_off; int32_t* a_nodes; uint8_t* a_kind;
    int32_t* p_off; int32_t* p_nodes; uint8_t* p_kind;
    uint8_t* part_in_prev; uint8_t* part_never_equal;
};

// An absent list has length 0; a length outside [0, L] cannot come from a plan and is cut to the row, so that whatever
// the scan yields fits the stage of k_adopt_write.
__device__ __forceinline__ int adopt_list_len(const AdoptParams& q, long long idx) {
    if (q.prv_kind[idx] == kListAbsent) return 0;
    const int n = q.prv_len[idx];
    return n < 0 ? 0 : n > q.L ? q.L : n;
}

__global__ __launch_bounds__(256) void k_adopt_len(AdoptParams q) {
    BLANCE_DYN_LDS(lds);
    unsigned long long (*red)[5] = (unsigned long long (*)[5])lds;      // [4 waves][5]
    const long long PM = (long long)q.P * q.M, stride = (long long)gridDim.x * blockDim.x;
    int longest = 0, kinds = 0;
    unsigned long long cap = 0, aprev = 0, total = 0;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx <= PM; idx += stride) {
        if (idx == PM) { q.len[idx] = 0; continue; }
        const int n = adopt_list_len(q, idx), m = (int)(idx % q.M), p = (int)(idx / q.M);
        q.len[idx] = n;
        longest = n > longest ? n : longest;
        kinds |= 1 << (m + (q.prv_kind[idx] == kListAbsent ? 0 : 16));
        const int k = q.k[m];
        cap += (unsigned long long)(n > k ? n : k);
        long long w = (!q.weights_nil && q.part_has_weight[p]) ? (long long)q.part_weight[p] : 1;
        if (w < 0) w = -w;
        aprev += (unsigned long long)(w * n);
        total += (unsigned long long)n;
    }
    // wave totals, the workgroup's four waves through LDS, then one atomic per word
    for (int o = 32; o; o >>= 1) {
        const int l2 = __shfl_xor(longest, o, 64);
        longest = l2 > longest ? l2 : longest;
        kinds |= __shfl_xor(kinds, o, 64);
        cap += ((unsigned long long)(unsigned)__shfl_xor((int)(unsigned)(cap >> 32), o, 64) << 32) | (unsigned)__shfl_xor((int)(unsigned)cap, o, 64);
        aprev += ((unsigned long long)(unsigned)__shfl_xor((int)(unsigned)(aprev >> 32), o, 64) << 32) | (unsigned)__shfl_xor((int)(unsigned)aprev, o, 64);
        total += ((unsigned long long)(unsigned)__shfl_xor((int)(unsigned)(total >> 32), o, 64) << 32) | (unsigned)__shfl_xor((int)(unsigned)total, o, 64);
    }
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[wv][0] = (unsigned long long)(unsigned)longest; red[wv][1] = (unsigned long long)(unsigned)kinds;
        red[wv][2] = cap; red[wv][3] = aprev; red[wv][4] = total;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int nw = (int)(blockDim.x >> 6);
        for (int w2 = 1; w2 < nw; w2++) {
            longest = (int)red[w2][0] > longest ? (int)red[w2][0] : longest;
            kinds |= (int)red[w2][1];
            cap += red[w2][2]; aprev += red[w2][3]; total += red[w2][4];
        }
        unsigned long long* r64 = (unsigned long long*)(q.res + 4);
        if (longest) atomicMax(q.res + kAdoptResLongest, longest);
        if (kinds) atomicOr(q.res + kAdoptResKinds, kinds);
        if (cap) atomicAdd(r64 + kAdoptRes64Cap, cap);
        if (aprev) atomicAdd(r64 + kAdoptRes64Prev, aprev);
        if (total) atomicAdd(r64 + kAdoptRes64Total, total);
    }
}

// dynamic LDS of one k_adopt_write workgroup: the lists' offsets and their entries (L <= 59 -- blance_validate's bound on
// the step record --, so at most 61 KB)
inline size_t adopt_write_lds(int L) { return sizeof(int32_t) * ((size_t)kAdoptLists + 1 + (size_t)kAdoptLists * L); }

// A workgroup takes kAdoptLists consecutive lists: their rows are one contiguous stretch of prv, read in order; the entries
// are staged in LDS at their places in the CSR and leave as one contiguous stretch of a_nodes and of p_nodes (per-thread
// rows written straight to HBM cost 3.6 times their bytes in write traffic, k_gather).  q.len holds the exclusive offsets.
// The workgroup whose lists end the map writes the last offset.
__global__ __launch_bounds__(kAdoptLists) void k_adopt_write(AdoptParams q) {
    BLANCE_DYN_LDS(lds);
    int32_t* s_off = (int32_t*)lds;                     // [kAdoptLists + 1]
    int32_t* stage = s_off + kAdoptLists + 1;           // [kAdoptLists * L]
    const long long PM = (long long)q.P * q.M, base = (long long)blockIdx.x * kAdoptLists;
    const int tid = threadIdx.x;
    const long long idx = base + tid;
    const int lists = (int)(PM - base < kAdoptLists ? PM - base : kAdoptLists);      // of this workgroup: 1 .. kAdoptLists
    if (tid < lists) s_off[tid] = q.len[idx];
    if (tid == 0) s_off[lists] = q.len[base + lists];
    __syncthreads();
    const int o0 = s_off[0], words = lists * q.L;
    for (int j = tid; j < words; j += kAdoptLists) {
        const int li = j / q.L, i = j % q.L;
        if (i < s_off[li + 1] - s_off[li]) stage[s_off[li] - o0 + i] = q.prv[base * q.L + j];
    }
    __syncthreads();
    const int n = s_off[lists] - o0;
    for (int j = tid; j < n; j += kAdoptLists) {
        const int32_t v = stage[j];
        q.a_nodes[(long long)o0 + j] = v;
        q.p_nodes[(long long)o0 + j] = v;
    }
    if (tid == 0 && base + lists == PM) { q.a_off[PM] = s_off[lists]; q.p_off[PM] = s_off[lists]; }
    if (tid < lists) {
        q.a_off[idx] = s_off[tid];
        q.p_off[idx] = s_off[tid];
        const uint8_t kind = q.prv_kind[idx];
        q.a_kind[idx] = kind;
        q.p_kind[idx] = kind;
        if (idx % q.M == 0) { q.part_in_prev[idx / q.M] = 1; q.part_never_equal[idx / q.M] = 0; }
    }
}

}  // namespace blance
