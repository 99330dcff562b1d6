// blance_wire_adopt: a decoded PartitionMap document becomes prevMap -- and, with assign_too, the partitions
// to assign -- of the problem the context holds, where the decoder left it.  Two kernels behind the decoder's device part:
// k_wire_adopt_sum makes the summary a fresh upload's k_validate_parts would have made of the lists and finds what the
// interners refuse on the host; k_wire_adopt_write streams the decoded CSR into the problem's.  The source is a contiguous
// CSR already (k_adopt_write gathers strided rows through LDS; nothing here needs that).  Part of blance_hip.hip.
#pragma once

namespace blance {

constexpr int kWireAdoptMaxWgs = 2048; // both grids: a grid-stride loop takes the rest
// Summary block of k_wire_adopt_sum.  The caller zeroes it and sets the three "first offender" words to INT_MAX (none).
// 32-bit words: [0] first list longer than L, [1] longest list, [2] partitions the document does not have (`fresh`),
// [3] first such partition, [10] the kinds of the lists to assign (k_validate_parts' word), [11] first list to assign with
// a node twice; 64-bit words from byte 16: [0] result capacity, [2] |weight| * entries of the partitions the document
// has, [4] the entries of the lists to assign.
constexpr int kWireAdoptResWords = 16;
constexpr int kWaResFirstLong = 0, kWaResLongest = 1, kWaResFresh = 2, kWaResFirstMissing = 3, kWaResKinds = 10, kWaResFirstDup = 11;
constexpr int kWaRes64Cap = 0, kWaRes64Prev = 2, kWaRes64Total = 4;

struct WireAdoptParams {
    int32_t P, M, L, weights_nil, assign_too;
    int32_t k[kMaxStates];
    // the decoded document (blance_wire_lists' arrays on the device): [P], [P*M + 1], [P*M], [off[P*M]]
    const uint8_t* part_kind; const int32_t* off; const uint8_t* kind; const int32_t* nodes;
    // !assign_too: the lists to assign the context holds ([P*M + 1], [P*M]); they stay
    const int32_t* cur_a_off; const uint8_t* cur_a_kind;
    const int32_t* part_weight; const uint8_t* part_has_weight;
    int32_t* res;                  // [kWireAdoptResWords]
    // k_wire_adopt_write's outputs: prev's CSR, with assign_too assign's too, and the two per-partition flags [P]; these and
    // the four decoded arrays are 16-byte aligned
    int32_t* a_off; int32_t* a_nodes; uint8_t* a_kind;
    int32_t* p_off; int32_t* p_nodes; uint8_t* p_kind;
    uint8_t* part_in_prev; uint8_t* part_never_equal;
};

__device__ __forceinline__ unsigned long long wa_shfl_xor64(unsigned long long v, int o) {
    return ((unsigned long long)(unsigned)__shfl_xor((int)(unsigned)(v >> 32), o, 64) << 32) | (unsigned)__shfl_xor((int)(unsigned)v, o, 64);
}

// One thread per decoded list and per partition, grid-stride.  The duplicate test is quadratic in a list of at most L <= 59
// entries; a list over L is reported as such and not searched.
__global__ __launch_bounds__(256) void k_wire_adopt_sum(WireAdoptParams q) {
    BLANCE_DYN_LDS(lds);
    unsigned long long (*red)[9] = (unsigned long long (*)[9])lds;      // [4 waves][9]
    const long long PM = (long long)q.P * q.M;
    const long long n = PM > q.P ? PM : q.P, stride = (long long)gridDim.x * blockDim.x;
    int longest = 0, kinds = 0, fresh = 0, first_long = INT_MAX, first_missing = INT_MAX, first_dup = INT_MAX;
    unsigned long long cap = 0, aprev = 0, total = 0;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += stride) {
        if (idx < PM) {
            const int m = (int)(idx % q.M);
            const int beg = q.off[idx], len = q.off[idx + 1] - beg;
            int alen = len, akind = q.kind[idx];
            if (!q.assign_too) { alen = q.cur_a_off[idx + 1] - q.cur_a_off[idx]; akind = q.cur_a_kind[idx]; }
            longest = len > longest ? len : longest;
            longest = alen > longest ? alen : longest;
            kinds |= 1 << (m + (akind == kListAbsent ? 0 : 16));
            const int k = q.k[m];
            cap += (unsigned long long)(alen > k ? alen : k);
            total += (unsigned long long)alen;
            if (len > q.L) first_long = idx < first_long ? (int)idx : first_long;
            else if (q.assign_too && len >= 2) {
                bool dup = false;
                for (int i = 1; i < len && !dup; i++) {
                    const int32_t v = q.nodes[beg + i];
                    for (int j = 0; j < i; j++) dup |= q.nodes[beg + j] == v;
                }
                if (dup) first_dup = idx < first_dup ? (int)idx : first_dup;
            }
        }
        if (idx < q.P) {
            const int p = (int)idx;
            if (q.part_kind[p] == kListAbsent) {
                fresh++;
                first_missing = p < first_missing ? p : first_missing;
            } else {
                long long w = (!q.weights_nil && q.part_has_weight[p]) ? (long long)q.part_weight[p] : 1;
                if (w < 0) w = -w;
                aprev += (unsigned long long)(w * ((long long)q.off[(long long)(p + 1) * q.M] - q.off[(long long)p * q.M]));
            }
        }
    }
    // wave totals, the workgroup's four waves through LDS, then one atomic per word
    for (int o = 32; o; o >>= 1) {
        int t = __shfl_xor(longest, o, 64);
        longest = t > longest ? t : longest;
        kinds |= __shfl_xor(kinds, o, 64);
        fresh += __shfl_xor(fresh, o, 64);
        t = __shfl_xor(first_long, o, 64);
        first_long = t < first_long ? t : first_long;
        t = __shfl_xor(first_missing, o, 64);
        first_missing = t < first_missing ? t : first_missing;
        t = __shfl_xor(first_dup, o, 64);
        first_dup = t < first_dup ? t : first_dup;
        cap += wa_shfl_xor64(cap, o);
        aprev += wa_shfl_xor64(aprev, o);
        total += wa_shfl_xor64(total, o);
    }
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[wv][0] = (unsigned long long)(unsigned)longest; red[wv][1] = (unsigned long long)(unsigned)kinds;
        red[wv][2] = (unsigned long long)(unsigned)fresh; red[wv][3] = (unsigned long long)(unsigned)first_long;
        red[wv][4] = (unsigned long long)(unsigned)first_missing; red[wv][5] = (unsigned long long)(unsigned)first_dup;
        red[wv][6] = cap; red[wv][7] = aprev; red[wv][8] = total;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int nw = (int)(blockDim.x >> 6);
        for (int w2 = 1; w2 < nw; w2++) {
            longest = (int)red[w2][0] > longest ? (int)red[w2][0] : longest;
            kinds |= (int)red[w2][1];
            fresh += (int)red[w2][2];
            first_long = (int)red[w2][3] < first_long ? (int)red[w2][3] : first_long;
            first_missing = (int)red[w2][4] < first_missing ? (int)red[w2][4] : first_missing;
            first_dup = (int)red[w2][5] < first_dup ? (int)red[w2][5] : first_dup;
            cap += red[w2][6]; aprev += red[w2][7]; total += red[w2][8];
        }
        unsigned long long* r64 = (unsigned long long*)(q.res + 4);
        if (longest) atomicMax(q.res + kWaResLongest, longest);
        if (kinds) atomicOr(q.res + kWaResKinds, kinds);
        if (fresh) atomicAdd(q.res + kWaResFresh, fresh);
        if (first_long != INT_MAX) atomicMin(q.res + kWaResFirstLong, first_long);
        if (first_missing != INT_MAX) atomicMin(q.res + kWaResFirstMissing, first_missing);
        if (first_dup != INT_MAX) atomicMin(q.res + kWaResFirstDup, first_dup);
        if (cap) atomicAdd(r64 + kWaRes64Cap, cap);
        if (aprev) atomicAdd(r64 + kWaRes64Prev, aprev);
        if (total) atomicAdd(r64 + kWaRes64Total, total);
    }
}

// The four streams of k_wire_adopt_write in 16-byte chunks: the offsets (P*M + 1 words), the node ids (off[P*M] words), the
// kinds (P*M bytes), the partitions' kinds (P bytes).  A chunk is read once and written once per destination; a stream's
// last, partial chunk goes element by element.  Every array is 16-byte aligned: each starts an allocation.
__device__ __forceinline__ void wa_copy_words(const int32_t* src, int32_t* d0, int32_t* d1, long long chunk, long long n) {
    const long long at = chunk * 4;
    if (at + 4 <= n) {
        const int4 v = *(const int4*)(src + at);
        *(int4*)(d0 + at) = v;
        if (d1) *(int4*)(d1 + at) = v;
        return;
    }
    for (long long i = at; i < at + 4 && i < n; i++) {
        const int32_t v = src[i];
        d0[i] = v;
        if (d1) d1[i] = v;
    }
}
__device__ __forceinline__ void wa_copy_bytes(const uint8_t* src, uint8_t* d0, uint8_t* d1, long long chunk, long long n) {
    const long long at = chunk * 16;
    if (at + 16 <= n) {
        const int4 v = *(const int4*)(src + at);
        *(int4*)(d0 + at) = v;
        if (d1) *(int4*)(d1 + at) = v;
        return;
    }
    for (long long i = at; i < at + 16 && i < n; i++) {
        const uint8_t v = src[i];
        d0[i] = v;
        if (d1) d1[i] = v;
    }
}
// part_in_prev = (kind != absent), part_never_equal = (kind == nil), sixteen partitions at a time
__device__ __forceinline__ unsigned wa_flags4(unsigned w, bool never) {
    unsigned out = 0;
    for (int b = 0; b < 4; b++) {
        const unsigned kd = (w >> (8 * b)) & 255u;
        out |= (unsigned)(never ? kd == kListNil : kd != kListAbsent) << (8 * b);
    }
    return out;
}
__device__ __forceinline__ void wa_part_flags(const WireAdoptParams& q, long long chunk) {
    const long long at = chunk * 16;
    if (at + 16 <= q.P) {
        const int4 v = *(const int4*)(q.part_kind + at);
        int4 a, b;
        a.x = (int)wa_flags4((unsigned)v.x, false); a.y = (int)wa_flags4((unsigned)v.y, false);
        a.z = (int)wa_flags4((unsigned)v.z, false); a.w = (int)wa_flags4((unsigned)v.w, false);
        b.x = (int)wa_flags4((unsigned)v.x, true); b.y = (int)wa_flags4((unsigned)v.y, true);
        b.z = (int)wa_flags4((unsigned)v.z, true); b.w = (int)wa_flags4((unsigned)v.w, true);
        *(int4*)(q.part_in_prev + at) = a;
        *(int4*)(q.part_never_equal + at) = b;
        return;
    }
    for (long long p = at; p < at + 16 && p < q.P; p++) {
        const uint8_t kd = q.part_kind[p];
        q.part_in_prev[p] = kd != kListAbsent;
        q.part_never_equal[p] = kd == kListNil;
    }
}

__global__ __launch_bounds__(256) void k_wire_adopt_write(WireAdoptParams q) {
    const long long PM = (long long)q.P * q.M, n_off = PM + 1, n_nodes = q.off[PM];
    const long long c_off = (n_off + 3) / 4, c_nodes = (n_nodes + 3) / 4, c_kind = (PM + 15) / 16, c_part = ((long long)q.P + 15) / 16;
    const long long chunks = c_off + c_nodes + c_kind + c_part, stride = (long long)gridDim.x * blockDim.x;
    int32_t* a_off = q.assign_too ? q.a_off : nullptr;
    int32_t* a_nodes = q.assign_too ? q.a_nodes : nullptr;
    uint8_t* a_kind = q.assign_too ? q.a_kind : nullptr;
    for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < chunks; c += stride) {
        if (c < c_off) wa_copy_words(q.off, q.p_off, a_off, c, n_off);
        else if (c < c_off + c_nodes) wa_copy_words(q.nodes, q.p_nodes, a_nodes, c - c_off, n_nodes);
        else if (c < c_off + c_nodes + c_kind) wa_copy_bytes(q.kind, q.p_kind, a_kind, c - c_off - c_nodes, PM);
        else wa_part_flags(q, c - c_off - c_nodes - c_kind);
    }
}

// workgroups of k_wire_adopt_write for a document of `total` entries
inline int wire_adopt_write_wgs(long long P, long long M, long long total) {
    const long long chunks = (P * M + 1 + 3) / 4 + (total + 3) / 4 + (P * M + 15) / 16 + (P + 15) / 16;
    const long long wgs = (chunks + 255) / 256;
    return (int)(wgs < 1 ? 1 : wgs > kWireAdoptMaxWgs ? kWireAdoptMaxWgs : wgs);
}

}  // namespace blance
