// k_batch_wire_size / k_batch_wire_write: json.Marshal(PartitionMap) of every batched problem that asks for it, one
// workgroup of 256 threads per problem, launched after k_plan_batch on the same stream (before or after k_batch_moves and
// k_batch_stats: they read and write disjoint words).  It restates k_plan_wire.h for one problem per workgroup: the lists
// are the result CSR k_plan_batch wrote into the problem's output slice (a list's length is off[idx + 1] - off[idx]), the
// prepared names (a blance_batch_names' block) lie behind the problem's packed input slice.  DESIGN.md §4.16.
//   k_batch_wire_size    thread t counts the bytes of ranks t, t + 256, ... (the nodes' escaped lengths from a table in
//                        LDS), then the workgroup scans the P lengths in rank order, a chunk per thread, into the byte
//                        offsets of the ranks.  The document's length goes to the output slice (the batch's one download
//                        brings it back) and, rounded up to 16, to wire_total[workgroup].
//   k_batch_wire_write   workgroup j finds its document's base in the one compact buffer as the sum of wire_total[0 .. j)
//                        (a block reduction: no third launch, no workgroup waits for another, every base 16-byte aligned)
//                        and writes the document as k_wire_write does: sub-runs of at most 256 consecutive ranks that fit
//                        the LDS stage, one thread per rank composing into the stage at (offset mod 16), aligned 16-byte
//                        vector stores out (byte stores for the head and the tail only); a partition larger than the stage
//                        goes straight to the document on the first wave.
// A thread's bytes in the stage are contiguous and about 100 at the consumer's shape, so the byte stores of a wave's lanes
// spread over the banks as their partitions' offsets do; the stores out read the stage with aligned 16-byte LDS loads (the
// stage starts 16-byte aligned behind the reduction words).
#pragma once

namespace blance {

struct BatchWireView {                                       // what the walk over one partition reads
    int P, M, NX;
    const int32_t* order;                                    // [P] rank -> partition id
    const int32_t* part_off; const char* part_esc;           // [P + 1] by RANK: "name" escaped, quotes included
    const int32_t* node_off; const char* node_esc;           // [NX + 1] by node id, likewise
    const int32_t* state_off; const char* state_esc;         // [M + 1] by place in the sorted state names: "name":
    const int32_t* state_id;                                 // [M] the state at that place
    const int32_t* off; const int32_t* kind; const int32_t* nodes;   // the result CSR over p * M + state
};

__device__ inline BatchWireView batch_wire_view(const BatchDesc& D, const BatchWireDesc& V, const int32_t* in, const int32_t* out) {
    const int32_t* nm = in + V.i_names;                      // header: the word offsets of the eight tables
    BatchWireView q;
    q.P = D.P; q.M = D.M; q.NX = D.NX;
    q.order = nm + nm[kNamesOrder];
    q.part_off = nm + nm[kNamesPartOff]; q.part_esc = (const char*)(nm + nm[kNamesPartEsc]);
    q.node_off = nm + nm[kNamesNodeOff]; q.node_esc = (const char*)(nm + nm[kNamesNodeEsc]);
    q.state_off = nm + nm[kNamesStateOff]; q.state_esc = (const char*)(nm + nm[kNamesStateEsc]);
    q.state_id = nm + nm[kNamesStateId];
    q.off = out + D.o_off; q.kind = out + D.o_kind; q.nodes = out + D.o_nodes;
    return q;
}

// The document's bytes of rank r, in order, to a sink (wire_partition of k_plan_wire.h over the result CSR).
template <class Sink>
__device__ inline void batch_wire_partition(const BatchWireView& q, int r, Sink& o) {
    const int p = q.order[r], M = q.M;
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
        const int kind = q.kind[idx];
        if (kind == kListAbsent) continue;
        if (!first) o.lit(",", 1);
        first = false;
        o.put(q.state_esc + q.state_off[j], q.state_off[j + 1] - q.state_off[j]);
        if (kind != kListSet) { o.lit("null", 4); continue; }
        o.lit("[", 1);
        const int beg = q.off[idx], n = q.off[idx + 1] - beg;
        for (int e = 0; e < n; e++) {
            if (e) o.lit(",", 1);
            const int x = q.nodes[beg + e];
            if ((unsigned)x < (unsigned)q.NX) o.node(x);     // (always: the lists hold ids of the problem)
        }
        o.lit("]", 1);
    }
    if (r == q.P - 1) o.lit("}}}", 3); else o.lit("}}", 2);
}

struct BatchWireCount {                                      // k_batch_wire_size: bytes only
    const int32_t* node_len;                                 // [NX] in LDS
    int n;
    __device__ void lit(const char*, int k) { n += k; }
    __device__ void put(const char*, int k) { n += k; }
    __device__ void node(int x) { n += node_len[x]; }
};
struct BatchWireToStage {                                    // k_batch_wire_write: one thread writes its partition into LDS
    const BatchWireView* q;
    unsigned char* at;
    __device__ void lit(const char* s, int k) { for (int i = 0; i < k; i++) at[i] = (unsigned char)s[i]; at += k; }
    __device__ void put(const char* s, int k) { for (int i = 0; i < k; i++) at[i] = (unsigned char)s[i]; at += k; }
    __device__ void node(int x) { put(q->node_esc + q->node_off[x], q->node_off[x + 1] - q->node_off[x]); }
};
struct BatchWireByWave {                                     // k_batch_wire_write: a wave copies one partition to the document
    const BatchWireView* q;
    char* at;
    int lane;
    __device__ void lit(const char* s, int k) { put(s, k); }
    __device__ void put(const char* s, int k) { for (int i = lane; i < k; i += 64) at[i] = s[i]; at += k; }
    __device__ void node(int x) { put(q->node_esc + q->node_off[x], q->node_off[x + 1] - q->node_off[x]); }
};

// LDS of the two kernels: the node lengths [256] and the scan's partial sums [256]; the reduction words [256] and the stage
constexpr size_t kBatchWireSizeLds = sizeof(int32_t) * (kBatchMaxNX + kBatchWireThreads);
constexpr size_t kBatchWireRedLds = sizeof(unsigned long long) * kBatchWireThreads;

__global__ __launch_bounds__(kBatchWireThreads) void k_batch_wire_size(BatchWireParams bp) {
    constexpr int T = kBatchWireThreads;
    const BatchWireDesc& V = bp.wdesc[blockIdx.x];
    const BatchDesc& D = bp.desc[V.desc];
    const int32_t* in = bp.in + D.in_base;
    int32_t* out = bp.out + D.out_base;
    const int tid = threadIdx.x;
    // not planned exactly here, or no map: no document (uniform exit).  !batch_planned(out), spelled out: through the inlined
    // predicate the compiler shapes this kernel's entry branches differently, and a refactor keeps the code object as it was
    if (out[kBoDone] != 1 || out[kBoError] != 0 || out[kBoIterations] == 0) {
        if (tid == 0) { bp.wire_total[blockIdx.x] = 0; out[V.o_total] = 0; }
        return;
    }
    const BatchWireView q = batch_wire_view(D, V, in, out);
    int32_t* len = bp.sc + D.sc_base + V.s_len;              // [P + 1]
    BLANCE_DYN_LDS(lds);
    int32_t* node_len = (int32_t*)lds;                       // [kBatchMaxNX]
    int32_t* part = node_len + kBatchMaxNX;                  // [T]
    const int P = q.P;
    for (int x = tid; x < q.NX; x += T) node_len[x] = q.node_off[x + 1] - q.node_off[x];
    __syncthreads();
    for (int r = tid; r < P; r += T) {
        BatchWireCount o{node_len, 0};
        batch_wire_partition(q, r, o);
        len[r] = o.n;
    }
    __syncthreads();
    // the lengths become the offsets of the ranks: a chunk per thread, an exclusive scan over the threads
    const int C = (P + T - 1) / T;
    const int lo = tid * C < P ? tid * C : P, hi = lo + C < P ? lo + C : P;
    int s = 0;
    for (int r = lo; r < hi; r++) s += len[r];
    part[tid] = s;
    __syncthreads();
    int at = 0, total = 0;
    for (int t = 0; t < T; t++) {
        if (t < tid) at += part[t];
        total += part[t];
    }
    for (int r = lo; r < hi; r++) {
        const int n = len[r];
        len[r] = at;
        at += n;
    }
    if (tid == 0) {
        len[P] = total;
        out[V.o_total] = total;
        bp.wire_total[blockIdx.x] = (total + 15) & ~15;
    }
}

__global__ __launch_bounds__(kBatchWireThreads) void k_batch_wire_write(BatchWireParams bp) {
    constexpr int T = kBatchWireThreads;
    const BatchWireDesc& V = bp.wdesc[blockIdx.x];
    const BatchDesc& D = bp.desc[V.desc];
    const int32_t* in = bp.in + D.in_base;
    const int32_t* out = bp.out + D.out_base;
    if (!batch_planned(out) || out[kBoIterations] == 0) return;   // as k_batch_wire_size (uniform exit)
    const BatchWireView q = batch_wire_view(D, V, in, out);
    const int32_t* len = bp.sc + D.sc_base + V.s_len;        // [P + 1] the offsets of the ranks
    BLANCE_DYN_LDS(lds);
    unsigned long long* red = (unsigned long long*)lds;      // [T]
    unsigned char* stage = lds + kBatchWireRedLds;
    const int tid = threadIdx.x;
    // the document's base: the 16-rounded lengths of the documents in front of it
    unsigned long long sum = 0;
    for (int i = tid; i < (int)blockIdx.x; i += T) sum += (unsigned long long)(unsigned)bp.wire_total[i];
    red[tid] = sum;
    __syncthreads();
    for (int s = T >> 1; s; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    char* doc = bp.doc + red[0];
    const int P = q.P, budget = bp.stage - 16;               // bytes of a sub-run; 16: the stage starts at (offset mod 16)
    int a = 0;
    while (a < P) {                                          // (a and b are the same in every thread: the barriers are uniform)
        const int g0 = len[a];
        int b = a, hi = a + T < P ? a + T : P;               // the sub-run [a, b): the most ranks, at most T, whose bytes fit
        while (b < hi) {
            const int mid = (b + hi + 1) >> 1;
            if (len[mid] - g0 <= budget) b = mid; else hi = mid - 1;
        }
        if (b == a) {                                        // one partition larger than the stage: straight to the document
            if (tid < 64) {
                BatchWireByWave o{&q, doc + g0, tid};
                batch_wire_partition(q, a, o);
            }
            a++;
            continue;
        }
        const int n = len[b] - g0, skew = g0 & 15;
        if (a + tid < b) {
            BatchWireToStage o{&q, stage + skew + (len[a + tid] - g0)};
            batch_wire_partition(q, a + tid, o);
        }
        __syncthreads();
        const int to_line = (16 - skew) & 15;
        const int head = n < to_line ? n : to_line, body_end = head + ((n - head) & ~15);
        if (tid < head) doc[g0 + tid] = (char)stage[skew + tid];
        for (int i = head + tid * 16; i < body_end; i += T * 16)
            *(int4*)(doc + g0 + i) = *(const int4*)(stage + skew + i);
        if (body_end + tid < n) doc[g0 + body_end + tid] = (char)stage[skew + body_end + tid];   // (fewer than 16 bytes)
        __syncthreads();
        a = b;
    }
}

}  // namespace blance
