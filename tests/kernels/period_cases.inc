// TEST INFRASTRUCTURE ONLY: the five kernels of blance_amd/csrc/k_period.h one at a time, on hand-made region tables, records,
// counters and outputs: k_period_find in its searched and its known mode, k_period_verify, k_period_segments, k_period_judge
// and k_period_replicate.  Included behind the product's headers by two wrappers: tests/kernels/period_cases.hip (hipcc,
// gfx950) and tests/simt/emu_period_cases.cpp (the SIMT emulator, g++).  tests/period_case_tables.py has the cases of
// k_period_find, tests/period_kernel_cases.py those of the other four and of the form as a whole.
#include <algorithm>
#include <vector>

namespace {
constexpr int kPeriodCaseBadArg = -100;
}  // namespace

extern "C" int blance_case_period_words(void) { return blance::kPWords; }

// pb[kPWords][B] comes in as the caller filled it and goes back as one launch of k_period_find left it.  Every index the
// kernel can form is checked first -- the chain offsets against n_steps, the leaf ranges against n_leaves, the nodes against
// NX -- and a table that fails is refused without a launch (kPeriodCaseBadArg); else the launch's own status (0: it ran).
extern "C" int blance_case_period_find(int B, int known, int threads, int N, int NX, int n_steps, int n_leaves, const int32_t* reg_off,
                                       const int32_t* reg_lo, const int32_t* reg_hi, const int32_t* leaf_node, const uint8_t* alive,
                                       const int32_t* crec, int32_t* pb) {
    if (B < 1 || B > 4096 || N < 0 || N > NX || NX < 1 || n_steps < 0 || n_leaves < 0 || !reg_off || !reg_lo || !reg_hi || !leaf_node ||
        !alive || !crec || !pb)
        return kPeriodCaseBadArg;
    if (threads != 64 && threads != 128 && threads != 256 && threads != 512 && threads != 1024) return kPeriodCaseBadArg;
    if (reg_off[0] < 0 || reg_off[B] > n_steps) return kPeriodCaseBadArg;
    for (int r = 0; r < B; r++) {
        if (reg_off[r + 1] < reg_off[r]) return kPeriodCaseBadArg;
        if (reg_lo[r] < 0 || reg_hi[r] < reg_lo[r] || reg_hi[r] > n_leaves) return kPeriodCaseBadArg;
    }
    for (int i = 0; i < n_leaves; i++)
        if (leaf_node[i] < -1 || leaf_node[i] >= NX) return kPeriodCaseBadArg;
    const size_t n_pb = (size_t)blance::kPWords * B, n_rec = (size_t)n_steps * blance::kCW;
    int32_t *d_off = nullptr, *d_lo = nullptr, *d_hi = nullptr, *d_leaf = nullptr, *d_rec = nullptr, *d_pb = nullptr;
    uint8_t* d_alive = nullptr;
    int st = (int)hipMalloc((void**)&d_off, sizeof(int32_t) * ((size_t)B + 1));
    if (!st) st = (int)hipMalloc((void**)&d_lo, sizeof(int32_t) * (size_t)B);
    if (!st) st = (int)hipMalloc((void**)&d_hi, sizeof(int32_t) * (size_t)B);
    if (!st) st = (int)hipMalloc((void**)&d_leaf, sizeof(int32_t) * ((size_t)n_leaves + 1));
    if (!st) st = (int)hipMalloc((void**)&d_alive, (size_t)NX);
    if (!st) st = (int)hipMalloc((void**)&d_rec, sizeof(int32_t) * (n_rec + 1));
    if (!st) st = (int)hipMalloc((void**)&d_pb, sizeof(int32_t) * n_pb);
    if (!st) st = (int)hipMemcpy(d_off, reg_off, sizeof(int32_t) * ((size_t)B + 1), hipMemcpyHostToDevice);
    if (!st) st = (int)hipMemcpy(d_lo, reg_lo, sizeof(int32_t) * (size_t)B, hipMemcpyHostToDevice);
    if (!st) st = (int)hipMemcpy(d_hi, reg_hi, sizeof(int32_t) * (size_t)B, hipMemcpyHostToDevice);
    if (!st && n_leaves > 0) st = (int)hipMemcpy(d_leaf, leaf_node, sizeof(int32_t) * (size_t)n_leaves, hipMemcpyHostToDevice);
    if (!st) st = (int)hipMemcpy(d_alive, alive, (size_t)NX, hipMemcpyHostToDevice);
    if (!st && n_rec > 0) st = (int)hipMemcpy(d_rec, crec, sizeof(int32_t) * n_rec, hipMemcpyHostToDevice);
    if (!st) st = (int)hipMemcpy(d_pb, pb, sizeof(int32_t) * n_pb, hipMemcpyHostToDevice);
    if (!st) {
        hipStream_t sm = nullptr;
        BLANCE_LAUNCH(blance::k_period_find, B, threads, 64, sm, B, known ? 1 : 0, N, d_off, d_lo, d_hi, d_leaf, d_alive, d_rec, d_pb);
        st = (int)hipGetLastError();
        if (!st) st = (int)hipStreamSynchronize(nullptr);
    }
    if (!st) st = (int)hipMemcpy(pb, d_pb, sizeof(int32_t) * n_pb, hipMemcpyDeviceToHost);
    for (void* p : {(void*)d_off, (void*)d_lo, (void*)d_hi, (void*)d_leaf, (void*)d_alive, (void*)d_rec, (void*)d_pb})
        if (p) (void)hipFree(p);
    return st;
}

// ---- the other four kernels ------------------------------------------------------------------------------------------------
// Every buffer a kernel writes (pb, cnt, out) or that shares a caller's poison (cnt1, flags) carries ONE GUARD WORD behind its
// last: the caller passes n + 1 words, n + 1 go up and n + 1 come back, so a store one word past the end shows in the caller's
// array (a store further out is the sanitizer's to see: the buffers are of exactly this size).
namespace {
bool period_case_chains_ok(int B, int threads, int n_steps, const int32_t* reg_off) {
    if (B < 1 || B > 4096 || n_steps < 0 || !reg_off) return false;
    if (threads != 64 && threads != 128 && threads != 256 && threads != 512 && threads != 1024) return false;
    if (reg_off[0] < 0 || reg_off[B] > n_steps) return false;
    for (int r = 0; r < B; r++)
        if (reg_off[r + 1] < reg_off[r]) return false;
    return true;
}
int period_case_longest(int B, const int32_t* reg_off) {
    int max_len = 0;
    for (int r = 0; r < B; r++) max_len = std::max(max_len, (int)(reg_off[r + 1] - reg_off[r]));
    return max_len;
}
bool period_case_joins(int T, int limit) {
    return T >= 1 && T <= blance::kPeriodCap && (long long)limit >= (long long)blance::kPeriodMinRounds * T;
}
// device copies of the caller's arrays: up() allocates exactly n elements and fills them, down() brings them back
struct PeriodCaseArrays {
    std::vector<void*> all;
    int st = 0;
    template <class T> T* up(const T* host, size_t n) {
        void* p = nullptr;
        if (!st) st = (int)hipMalloc(&p, sizeof(T) * (n ? n : 1));
        if (!st) all.push_back(p);
        if (!st && n) st = (int)hipMemcpy(p, host, sizeof(T) * n, hipMemcpyHostToDevice);
        return (T*)p;
    }
    template <class T> void down(T* host, const T* dev, size_t n) {
        if (!st && n) st = (int)hipMemcpy(host, dev, sizeof(T) * n, hipMemcpyDeviceToHost);
    }
    void ran() {
        if (!st) st = (int)hipGetLastError();
        if (!st) st = (int)hipStreamSynchronize(nullptr);
    }
    ~PeriodCaseArrays() {
        for (void* p : all) (void)hipFree(p);
    }
};
}  // namespace

// One launch of k_period_verify, `threads` wide (the driver's 256), gv workgroups per region as ChainPass::periodic_walk sizes
// them from the longest chain.  pb: kPWords * B + 1 words.  The kernel reads 16-byte pieces of steps [0, len) of a chain that
// lies inside the records, whatever T is: the chains are all there is to check.
extern "C" int blance_case_period_verify(int B, int threads, int n_steps, const int32_t* reg_off, const int32_t* crec, int32_t* pb) {
    if (!period_case_chains_ok(B, threads, n_steps, reg_off) || !crec || !pb) return kPeriodCaseBadArg;
    const size_t n_pb = (size_t)blance::kPWords * B + 1;
    const long long pieces = (long long)period_case_longest(B, reg_off) * (blance::kCW / 4);
    const int gv = std::max(1, (int)((pieces + threads - 1) / threads));
    PeriodCaseArrays a;
    int32_t* d_off = a.up(reg_off, (size_t)B + 1);
    int32_t* d_rec = a.up(crec, (size_t)n_steps * blance::kCW);
    int32_t* d_pb = a.up(pb, n_pb);
    if (!a.st) {
        hipStream_t sm = nullptr;
        BLANCE_LAUNCH_NOSYNC(blance::k_period_verify, gv * B, threads, 0, sm, B, gv, d_off, d_rec, d_pb);
        a.ran();
    }
    a.down(pb, d_pb, n_pb);
    return a.st;
}

// One launch of k_period_segments, `threads` wide (the driver's 64).  pb: kPWords * B + 1 words.  It forms no index but rg.
extern "C" int blance_case_period_segments(int B, int threads, int cut, int n_steps, const int32_t* reg_off, int32_t* pb) {
    if (!period_case_chains_ok(B, threads, n_steps, reg_off) || !pb) return kPeriodCaseBadArg;
    const size_t n_pb = (size_t)blance::kPWords * B + 1;
    PeriodCaseArrays a;
    int32_t* d_off = a.up(reg_off, (size_t)B + 1);
    int32_t* d_pb = a.up(pb, n_pb);
    if (!a.st) {
        hipStream_t sm = nullptr;
        BLANCE_LAUNCH_NOSYNC(blance::k_period_segments, (B + threads - 1) / threads, threads, 0, sm, B, cut, d_off, d_pb);
        a.ran();
    }
    a.down(pb, d_pb, n_pb);
    return a.st;
}

// One launch of k_period_judge for state s of n_states, `threads` wide (the driver's 128).  cnt1, cnt: n_states * NX + 1 words;
// out: n_steps * OW + 1; flags: kChainFlags + 1; pb: kPWords * B + 1.  Checked: s, the leaf ranges, the nodes against NX, and of
// every region that joins (the others return at once) that two periods lie inside its chain -- the kernel counts steps of
// [T, 2T) -- and that each of those steps' records lists no more picks than a record of OW words holds.
extern "C" int blance_case_period_judge(int B, int threads, int s, int n_states, int N, int NX, int OW, int n_steps, int n_leaves,
                                        const int32_t* reg_off, const int32_t* reg_lo, const int32_t* reg_hi, const int32_t* leaf_node,
                                        const uint8_t* alive, const int32_t* crec, int32_t* out, int32_t* flags, int32_t* cnt1,
                                        int32_t* cnt, int32_t* pb) {
    if (!period_case_chains_ok(B, threads, n_steps, reg_off) || !reg_lo || !reg_hi || !leaf_node || !alive || !crec || !out || !flags ||
        !cnt1 || !cnt || !pb)
        return kPeriodCaseBadArg;
    if (n_states < 1 || n_states > 64 || s < 0 || s >= n_states || NX < 1 || N < 0 || N > NX || OW < 2 || OW > 5 || n_leaves < 0)
        return kPeriodCaseBadArg;
    for (int r = 0; r < B; r++) {
        if (reg_lo[r] < 0 || reg_hi[r] < reg_lo[r] || reg_hi[r] > n_leaves) return kPeriodCaseBadArg;
        const int T = pb[blance::kPT * B + r], limit = pb[blance::kPLimit * B + r];
        if (!period_case_joins(T, limit)) continue;
        if (limit > reg_off[r + 1] - reg_off[r]) return kPeriodCaseBadArg;
        for (int t = reg_off[r] + T; t < reg_off[r] + 2 * T; t++)
            if ((out[(size_t)t * OW] & 0xffff) > OW - 1) return kPeriodCaseBadArg;
    }
    for (int i = 0; i < n_leaves; i++)
        if (leaf_node[i] < -1 || leaf_node[i] >= NX) return kPeriodCaseBadArg;
    const size_t n_pb = (size_t)blance::kPWords * B + 1, n_cnt = (size_t)n_states * NX + 1, n_out = (size_t)n_steps * OW + 1;
    const size_t n_flags = (size_t)blance::kChainFlags + 1;
    PeriodCaseArrays a;
    int32_t* d_off = a.up(reg_off, (size_t)B + 1);
    int32_t* d_lo = a.up(reg_lo, (size_t)B);
    int32_t* d_hi = a.up(reg_hi, (size_t)B);
    int32_t* d_leaf = a.up(leaf_node, (size_t)n_leaves);
    uint8_t* d_alive = a.up(alive, (size_t)NX);
    int32_t* d_rec = a.up(crec, (size_t)n_steps * blance::kCW);
    int32_t* d_out = a.up(out, n_out);
    int32_t* d_flags = a.up(flags, n_flags);
    int32_t* d_cnt1 = a.up(cnt1, n_cnt);
    int32_t* d_cnt = a.up(cnt, n_cnt);
    int32_t* d_pb = a.up(pb, n_pb);
    if (!a.st) {
        hipStream_t sm = nullptr;
        BLANCE_LAUNCH(blance::k_period_judge, B, threads, 64, sm, B, s, N, NX, OW, d_off, d_lo, d_hi, d_leaf, d_alive, d_rec, d_out, d_flags,
                      d_cnt1, d_cnt, d_pb);
        a.ran();
    }
    a.down(out, d_out, n_out);
    a.down(flags, d_flags, n_flags);
    a.down(cnt1, d_cnt1, n_cnt);
    a.down(cnt, d_cnt, n_cnt);
    a.down(pb, d_pb, n_pb);
    return a.st;
}

// One launch of k_period_replicate, `threads` wide (the driver's 256), gx workgroups per region as ChainPass::periodic_walk sizes
// them from the longest chain.  out: n_steps * OW + 1 words; pb: kPWords * B + 1.  Checked of every region that is ok (the
// others return at once): a period of at least one step, two of them in front of `limit`, `limit` inside the chain.
extern "C" int blance_case_period_replicate(int B, int threads, int OW, int n_steps, const int32_t* reg_off, int32_t* pb, int32_t* out) {
    if (!period_case_chains_ok(B, threads, n_steps, reg_off) || !pb || !out || OW < 2 || OW > 5) return kPeriodCaseBadArg;
    for (int r = 0; r < B; r++) {
        if (!pb[blance::kPOk * B + r]) continue;
        const int T = pb[blance::kPT * B + r], limit = pb[blance::kPLimit * B + r];
        if (T < 1 || T > blance::kPeriodCap || limit < 2 * T || limit > reg_off[r + 1] - reg_off[r]) return kPeriodCaseBadArg;
    }
    const size_t n_pb = (size_t)blance::kPWords * B + 1, n_out = (size_t)n_steps * OW + 1;
    const int gx = std::max(1, (period_case_longest(B, reg_off) + threads - 1) / threads);
    PeriodCaseArrays a;
    int32_t* d_off = a.up(reg_off, (size_t)B + 1);
    int32_t* d_pb = a.up(pb, n_pb);
    int32_t* d_out = a.up(out, n_out);
    if (!a.st) {
        hipStream_t sm = nullptr;
        BLANCE_LAUNCH_NOSYNC(blance::k_period_replicate, gx * B, threads, 0, sm, B, gx, OW, d_off, d_pb, d_out);
        a.ran();
    }
    a.down(pb, d_pb, n_pb);
    a.down(out, d_out, n_out);
    return a.st;
}
