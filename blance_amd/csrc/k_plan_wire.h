// k_wire_size / k_wire_write: json.Marshal(PartitionMap) (api.go:24-36) of the plan the context holds, composed on the
// device (blance_plan_wire_get), byte for byte what the host encoder (host/blance_wire.cpp) makes of a downloaded result.
// Part of blance_hip.hip; DESIGN.md §4.12.
//
// What depends on the names alone was prepared by blance_plan_wire_names: every string in its escaped form (quotes included,
// a state's with the colon behind it), the partitions' strings laid out in the order of the document (byte order of the
// names: rank r is partition order[r]), the states in the order of their names.  What is left is the shape k_plan_moves
// established -- size, scan, write -- with no per-partition scratch: one walk over a partition's planned lists
// (wire_partition) feeds a sink, and the sink is all that differs between the passes.
//   k_wire_size    one thread per rank counts its bytes (the nodes' escaped lengths from a table in LDS);
//   (scan)         the counts become the byte offsets of the ranks;
//   k_wire_write   a workgroup owns 256 consecutive ranks = one contiguous byte range of the document.  It cuts the range into
//                  sub-runs that fit its LDS stage, one thread per rank writes its partition's bytes into the stage, then the
//                  workgroup streams the stage out with aligned 16-byte stores per lane (byte stores for the unaligned head
//                  and tail only).  The stage starts at (document offset mod 16), so both sides of a 16-byte store are
//                  aligned.  A partition that alone is larger than the stage (names have no length bound) is copied to the
//                  document directly by the workgroup's first wave, lanes striding over the bytes of each piece.
// Composition is a thread per partition, not a wave per partition copying (source, length, destination) pieces: a
// partition is a dozen pieces of 1 to 17 bytes (about 100 bytes at the benchmark's shape), so a wave per partition would
// run every piece with 50 or more of its 64 lanes idle and walk the lists of one partition at a time; a thread per partition
// keeps 64 walks per wave in flight, and the byte traffic it makes is LDS traffic.  No workgroup waits for another.
#pragma once

namespace blance {

struct PlanWireParams {
    int32_t P, M, L, NX;
    const int32_t* order;                                   // [P] rank -> partition id
    const char* part_esc; const int32_t* part_off;          // [P + 1] by RANK: "name" escaped, quotes included
    const char* node_esc; const int32_t* node_off;          // [NX + 1] by node id, likewise
    const char* state_esc; const int32_t* state_off;        // [M + 1] by place in the sorted state names: "name":
    const int32_t* state_id;                                // [M] the state at that place
    const int32_t* lists; const int32_t* list_len; const uint8_t* list_kind;   // the planned lists [P*M][L]
    int32_t* len;                    // [P + 1]: k_wire_size writes the lengths (0 behind them), k_wire_write reads the offsets
    unsigned long long* total;       // zeroed, on a cache line of its own: all bytes (k_wire_size)
    char* doc;                       // the document, 16-byte aligned (k_wire_write)
    int32_t stage;                   // bytes of k_wire_write's LDS stage
};

// the sizing pass runs on at most kWireMaxWgs workgroups that stride over the ranks, one atomic per workgroup
// (k_plan_moves.h: kPlanMovesMaxWgs has the measurement); k_wire_write's workgroup takes kWireRun ranks
constexpr int kWireMaxWgs = 2048, kWireRun = 256, kWireStageDefault = 32 * 1024, kWireStageMin = 64, kWireStageMax = 64 * 1024;

// The document's bytes of rank r, in order, to a sink: lit(text, n) punctuation, put(src, n) an escaped string, node(x).
template <class Sink>
__device__ inline void wire_partition(const PlanWireParams& q, int r, Sink& o) {
    const int p = q.order[r], M = q.M, L = q.L;
    const char* name = q.part_esc + q.part_off[r];
    const int name_n = q.part_off[r + 1] - q.part_off[r];
    o.lit(r ? "," : "{", 1);
    o.put(name, name_n);                                     // the key ...
    o.lit(":{\"name\":", 9);
    o.put(name, name_n);                                     // ... is the partition's name
    o.lit(",\"nodesByState\":{", 17);
    bool first = true;
    for (int j = 0; j < M; j++) {
        const int idx = p * M + q.state_id[j];
        const int kind = q.list_kind[idx];
        if (kind == kListAbsent) continue;
        if (!first) o.lit(",", 1);
        first = false;
        o.put(q.state_esc + q.state_off[j], q.state_off[j + 1] - q.state_off[j]);
        if (kind != kListSet) { o.lit("null", 4); continue; }
        o.lit("[", 1);
        int n = q.list_len[idx];
        n = n < 0 ? 0 : (n > L ? L : n);
        const int32_t* l = q.lists + (size_t)idx * L;
        for (int e = 0; e < n; e++) {
            if (e) o.lit(",", 1);
            const int x = l[e];
            if ((unsigned)x < (unsigned)q.NX) o.node(x);     // (always: the lists hold ids of the problem)
        }
        o.lit("]", 1);
    }
    if (r == q.P - 1) o.lit("}}}", 3); else o.lit("}}", 2);
}

struct WireCount {                                           // k_wire_size: bytes only
    const int32_t* node_len;                                 // [NX] in LDS
    long long n;
    __device__ void lit(const char*, int k) { n += k; }
    __device__ void put(const char*, int k) { n += k; }
    __device__ void node(int x) { n += node_len[x]; }
};
struct WireToStage {                                         // k_wire_write: one thread writes its partition into LDS
    const PlanWireParams* q;
    unsigned char* at;
    __device__ void lit(const char* s, int k) { for (int i = 0; i < k; i++) at[i] = (unsigned char)s[i]; at += k; }
    __device__ void put(const char* s, int k) { for (int i = 0; i < k; i++) at[i] = (unsigned char)s[i]; at += k; }
    __device__ void node(int x) { put(q->node_esc + q->node_off[x], q->node_off[x + 1] - q->node_off[x]); }
};
struct WireByWave {                                          // k_wire_write: a wave copies one partition to the document
    const PlanWireParams* q;
    char* at;
    int lane;
    __device__ void lit(const char* s, int k) { put(s, k); }
    __device__ void put(const char* s, int k) { for (int i = lane; i < k; i += 64) at[i] = s[i]; at += k; }
    __device__ void node(int x) { put(q->node_esc + q->node_off[x], q->node_off[x + 1] - q->node_off[x]); }
};

__global__ __launch_bounds__(256) void k_wire_size(PlanWireParams q) {
    BLANCE_DYN_LDS(lds);
    int32_t* node_len = (int32_t*)lds;                                                         // [NX]
    unsigned long long* red = (unsigned long long*)(lds + (((size_t)q.NX * 4 + 15) & ~(size_t)15));   // [256]
    const int tid = threadIdx.x;
    for (int x = tid; x < q.NX; x += (int)blockDim.x) node_len[x] = q.node_off[x + 1] - q.node_off[x];
    __syncthreads();
    unsigned long long sum = 0;
    const int stride = (int)(gridDim.x * blockDim.x);
    for (int r = blockIdx.x * blockDim.x + tid; r <= q.P; r += stride) {
        long long n = 0;
        if (r < q.P) {
            WireCount o{node_len, 0};
            wire_partition(q, r, o);
            n = o.n;
        }
        q.len[r] = n > (long long)INT32_MAX ? INT32_MAX : (int32_t)n;   // (a document of 2^31 bytes is refused by the total)
        sum += (unsigned long long)n;
    }
    red[tid] = sum;
    __syncthreads();
    for (int s = (int)blockDim.x >> 1; s; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0 && red[0]) atomicAdd(q.total, red[0]);
}

__global__ __launch_bounds__(256) void k_wire_write(PlanWireParams q) {
    BLANCE_DYN_LDS(lds);
    const int tid = threadIdx.x;
    const int r0 = blockIdx.x * kWireRun, r1 = r0 + kWireRun < q.P ? r0 + kWireRun : q.P;
    const int budget = q.stage - 16;                         // bytes of a sub-run; 16: the stage starts at (offset mod 16)
    int a = r0;
    while (a < r1) {                                         // (a and b are the same in every thread: the barriers are uniform)
        const int g0 = q.len[a];
        int b = a, hi = r1;                                  // the sub-run [a, b): the most ranks whose bytes fit the budget
        while (b < hi) {
            const int mid = (b + hi + 1) >> 1;
            if (q.len[mid] - g0 <= budget) b = mid; else hi = mid - 1;
        }
        if (b == a) {                                        // one partition larger than the stage: straight to the document
            if (tid < 64) {
                WireByWave o{&q, q.doc + g0, tid};
                wire_partition(q, a, o);
            }
            a++;
            continue;
        }
        const int n = q.len[b] - g0, skew = g0 & 15;
        if (a + tid < b) {
            WireToStage o{&q, lds + skew + (q.len[a + tid] - g0)};
            wire_partition(q, a + tid, o);
        }
        __syncthreads();
        const int to_line = (16 - skew) & 15;
        const int head = n < to_line ? n : to_line, body_end = head + ((n - head) & ~15);
        if (tid < head) q.doc[g0 + tid] = (char)lds[skew + tid];
        for (int i = head + tid * 16; i < body_end; i += kWireRun * 16)
            *(int4*)(q.doc + g0 + i) = *(const int4*)(lds + skew + i);
        if (body_end + tid < n) q.doc[g0 + body_end + tid] = (char)lds[skew + body_end + tid];   // (fewer than 16 bytes)
        __syncthreads();
        a = b;
    }
}

}  // namespace blance
