// TEST INFRASTRUCTURE ONLY: the data-parallel building blocks of the planner, one at a time, on inputs a test makes by hand.
// Included behind blance_hip.hip by two wrappers: tests/simt/emu_kernel_cases.cpp (the SIMT emulator, g++) and
// tests/kernels/kernel_cases.hip (hipcc, gfx950) -- the translation unit's static host helpers and blance_ctx are visible
// here, so an entry runs launch_scan_excl_on, group_by_key, radix_sort_pairs, the fresh-run helpers of run_flat_pass and the
// launch_flat_* helpers of its stay side themselves, with the launch shapes the driver uses.
//
// Conventions: plain host arrays in and out; every device buffer is sized from the entry's own arguments; whatever a kernel
// would index with (keys < B, node ids < N, list lengths) is checked first and a bad value returns kCaseBadArg WITHOUT a
// launch; the work runs on a fresh context's stream, which is synchronised before anything is copied back; outputs are
// filled with 0x5a first and have a guard word behind them.
// (tests/kernel_case_tables.py has the cases and the references.)
#include <vector>

namespace {
constexpr int kCaseBadArg = -100;

struct CaseCtx {
    blance_ctx* c = nullptr;
    ~CaseCtx() { if (c) blance_ctx_destroy(c); }
    int open() { return blance_ctx_create(nullptr, &c); }
};
#define CASETRY(expr) do { const int ce__ = (expr); if (ce__) return ce__; } while (0)

// `extra` elements of T behind the n copied ones (guards, a kernel's one-past word), filled with `fill` bytes
template <class T>
int case_up(DevBuf& b, const T* src, size_t n, size_t extra = 0, int fill = 0) {
    if (b.reserve(sizeof(T) * (n + extra))) return fail(BLANCE_ERR_DEVICE, "hipMalloc failed");
    HIPTRY(hipMemsetAsync(b.p, fill, b.cap, nullptr));
    HIPTRY(hipStreamSynchronize(nullptr));
    if (n && src) HIPTRY(hipMemcpy(b.p, src, sizeof(T) * n, hipMemcpyHostToDevice));
    return 0;
}
template <class T>
int case_down(T* dst, const void* dev, size_t n) {
    if (n) HIPTRY(hipMemcpy(dst, dev, sizeof(T) * n, hipMemcpyDeviceToHost));
    return 0;
}
int case_sync(blance_ctx* c) {
    HIPTRY(stream_sync(c));
    return 0;
}

// What radix_sort_pairs works in, for n pairs (blance_upload sizes them from P)
int case_sort_buffers(blance_ctx* c, size_t n) {
    RESERVE(f_keys_a, sizeof(unsigned long long) * (n + 1));
    RESERVE(f_keys_b, sizeof(unsigned long long) * (n + 1));
    RESERVE(f_vals_a, sizeof(int32_t) * (n + 1));
    RESERVE(f_vals_b, sizeof(int32_t) * (n + 1));
    RESERVE(f_hist, sizeof(int32_t) * 256 * ((size_t)cdiv((int64_t)n, kSortTile) + 1));
    RESERVE(scalars, sizeof(int32_t) * kScalWords);
    HIPTRY(hipMemsetAsync(c->scalars.p, 0, sizeof(int32_t) * kScalWords, c->stream));
    HIPTRY(hipMemsetAsync(c->f_vals_b.p, 0x5a, sizeof(int32_t) * (n + 1), c->stream));
    HIPTRY(hipMemsetAsync(c->f_keys_b.p, 0x5a, sizeof(unsigned long long) * (n + 1), c->stream));
    return 0;
}

// Step records as k_gather lays them out (L = 1): partition, weight, stickiness (fp64), then per state a header
// (kind << 16 | length) and one node.  State 0's list holds the step's excluded node (excl[t] >= 0) or is absent.
std::vector<int32_t> case_records(int R, int M, int w, const int32_t* excl) {
    const int RW = kRecHead + M * 2;
    std::vector<int32_t> rec((size_t)R * RW, 0);
    for (int t = 0; t < R; t++) {
        int32_t* r = &rec[(size_t)t * RW];
        r[0] = t; r[1] = w;
        const double stick = 1.5;
        memcpy(&r[2], &stick, 8);
        if (excl && excl[t] >= 0) { r[kRecHead] = (kListSet << 16) | 1; r[kRecHead + 1] = excl[t]; }
    }
    return rec;
}

// The sibling for arbitrary steps: lists[P M L], len[P M], kind[P M] (kListAbsent / kListNil / kListSet), the step's weight and
// its stickiness -- a partition's live lists as k_gather copies them into a record (unused slots -1).
std::vector<int32_t> case_records_lists(int P, int M, int L, const int32_t* lists, const int32_t* len, const uint8_t* kind,
                                        const int32_t* w, const double* stick) {
    const int SW = 1 + L, RW = kRecHead + M * SW;
    std::vector<int32_t> rec((size_t)P * RW, 0);
    for (int i = 0; i < P; i++) {
        int32_t* r = &rec[(size_t)i * RW];
        r[0] = i; r[1] = w[i];
        memcpy(&r[2], &stick[i], 8);
        for (int t = 0; t < M; t++) {
            const size_t idx = (size_t)i * M + t;
            const int n = kind[idx] == kListAbsent ? 0 : len[idx];
            int32_t* rs = r + kRecHead + t * SW;
            rs[0] = n | ((int)kind[idx] << 16);
            for (int j = 0; j < L; j++) rs[1 + j] = j < n ? lists[idx * L + j] : -1;
        }
    }
    return rec;
}
// every list of the steps is something a kernel may read: a known kind, at most L nodes, node ids in [0, NX)
bool case_lists_ok(int P, int M, int L, int NX, const int32_t* lists, const int32_t* len, const uint8_t* kind) {
    if (!lists || !len || !kind) return false;
    for (size_t idx = 0; idx < (size_t)P * M; idx++) {
        if (kind[idx] > kListSet || len[idx] < 0 || len[idx] > L) return false;
        for (int j = 0; j < len[idx]; j++) if (lists[idx * L + j] < 0 || lists[idx * L + j] >= NX) return false;
    }
    return true;
}

constexpr int kCaseMaxNX = 8192 + 64, kCaseMaxP = 1 << 16, kCaseMaxL = 64;

// The node tables of a flat pass and what k_flat_prepare leaves for the stay test, on the device: cnt[(M + 1) NX], alive[N],
// node_w[NX], node_has_w[NX]; tot[NX], g[NX], top_g[kTopList], top_n[kTopList] with one guard word behind each; row_count[NX + 1]
// zeroed, one guard word behind it.
struct FlatCase {
    DevBuf cnt, alive, node_w, node_has_w, tot, g, top_g, top_n, row_count;
};
bool case_flat_args_ok(int N, int NX, int M, const int32_t* cnt, const uint8_t* alive, const int32_t* node_w, const uint8_t* node_has_w,
                       int NP, int s) {
    return N >= 1 && NX >= N && NX <= kCaseMaxNX && M >= 1 && M <= kMaxStates && s >= 0 && s < M && NP >= 0 && cnt && alive && node_w &&
           node_has_w;
}
int case_flat_tables(FlatCase& f, FlatParams& fq, int N, int NX, int M, const int32_t* cnt, const uint8_t* alive, const int32_t* node_w,
                     const uint8_t* node_has_w, int NP, int booster_kind, int s) {
    CASETRY(case_up(f.cnt, cnt, (size_t)(M + 1) * NX));
    CASETRY(case_up(f.alive, alive, (size_t)N));
    CASETRY(case_up(f.node_w, node_w, (size_t)NX));
    CASETRY(case_up(f.node_has_w, node_has_w, (size_t)NX));
    CASETRY(case_up<int32_t>(f.tot, nullptr, 0, (size_t)NX + 1, 0x5a));
    CASETRY(case_up<double>(f.g, nullptr, 0, (size_t)NX + 1, 0x5a));
    CASETRY(case_up<double>(f.top_g, nullptr, 0, (size_t)kTopList + 1, 0x5a));
    CASETRY(case_up<int32_t>(f.top_n, nullptr, 0, (size_t)kTopList + 1, 0x5a));
    std::vector<int32_t> rows((size_t)NX + 2, 0);
    rows[(size_t)NX + 1] = 0x5a5a5a5a;
    CASETRY(case_up(f.row_count, rows.data(), rows.size()));
    fq.N = N; fq.NX = NX; fq.M = M; fq.s = s; fq.NP = NP; fq.booster_kind = booster_kind;
    fq.alive = f.alive.as<uint8_t>(); fq.node_weight = f.node_w.as<int32_t>(); fq.node_has_weight = f.node_has_w.as<uint8_t>();
    fq.cnt = f.cnt.as<int32_t>(); fq.tot = f.tot.as<int32_t>(); fq.g = f.g.as<double>();
    fq.top_g = f.top_g.as<double>(); fq.top_n = f.top_n.as<int32_t>(); fq.row_count = f.row_count.as<int32_t>();
    return 0;
}
}  // namespace

extern "C" {

// launch_scan_excl_on over data[0, n); data[n] is a guard word the scan must leave alone (copied in and out with the rest)
int kcase_scan_excl(int n, int32_t* data /* [n + 1] */) {
    if (n < 1 || !data) return kCaseBadArg;
    CaseCtx cx;
    CASETRY(cx.open());
    blance_ctx* c = cx.c;
    DevBuf d;
    CASETRY(case_up(d, data, (size_t)n + 1));
    CASETRY(launch_scan_excl_on(c, c->stream, c->scan_sums, n, d.as<int32_t>()));
    CASETRY(case_sync(c));
    return case_down(data, d.p, (size_t)n + 1);
}

// group_by_key: offs[B + 1], out[n] (src[i] or i), out_oi[n] (null: not asked for).  One guard word behind each output.
int kcase_group_by_key(int n, const int32_t* key, const int32_t* src /* or null */, int B, int32_t* offs /* [B + 2] */,
                       int32_t* out /* [n + 1] */, int32_t* out_oi /* [n + 1] or null */) {
    if (n < 1 || B < 1 || B > 4096 || !key || !offs || !out) return kCaseBadArg;
    for (int i = 0; i < n; i++) if (key[i] < 0 || key[i] >= B) return kCaseBadArg;
    CaseCtx cx;
    CASETRY(cx.open());
    blance_ctx* c = cx.c;
    DevBuf dkey, dsrc, dcounts, doffs, dout, doi;
    CASETRY(case_up(dkey, key, (size_t)n));
    if (src) CASETRY(case_up(dsrc, src, (size_t)n));
    CASETRY(case_up<int32_t>(dcounts, nullptr, (size_t)B * cdiv(n, kPartChunk) + 1));
    CASETRY(case_up<int32_t>(doffs, nullptr, 0, (size_t)B + 2, 0x5a));
    CASETRY(case_up<int32_t>(dout, nullptr, 0, (size_t)n + 1, 0x5a));
    if (out_oi) CASETRY(case_up<int32_t>(doi, nullptr, 0, (size_t)n + 1, 0x5a));
    CASETRY(group_by_key(c, c->stream, c->scan_sums, n, dkey.as<int32_t>(), src ? dsrc.as<int32_t>() : nullptr, B,
                         dcounts.as<int32_t>(), doffs.as<int32_t>(), dout.as<int32_t>(), out_oi ? doi.as<int32_t>() : nullptr));
    CASETRY(case_sync(c));
    CASETRY(case_down(offs, doffs.p, (size_t)B + 2));
    CASETRY(case_down(out, dout.p, (size_t)n + 1));
    if (out_oi) CASETRY(case_down(out_oi, doi.p, (size_t)n + 1));
    return 0;
}

// The sweep driver's category partition (pass_order): item i has category cat[index[i]] < kCatBuckets; out[] = index[] in
// category order, stable.
int kcase_partition_category(int n, const uint8_t* cat /* [n] */, const int32_t* index /* [n] */, int32_t* out /* [n + 1] */) {
    if (n < 1 || !cat || !index || !out) return kCaseBadArg;
    for (int i = 0; i < n; i++) if (index[i] < 0 || index[i] >= n || cat[i] >= kCatBuckets) return kCaseBadArg;
    CaseCtx cx;
    CASETRY(cx.open());
    blance_ctx* c = cx.c;
    DevBuf dcat, dindex, dcounts, dout;
    CASETRY(case_up(dcat, cat, (size_t)n));
    CASETRY(case_up(dindex, index, (size_t)n));
    CASETRY(case_up<int32_t>(dcounts, nullptr, (size_t)kCatBuckets * (cdiv(n, kPartChunk) + 1)));
    CASETRY(case_up<int32_t>(dout, nullptr, 0, (size_t)n + 1, 0x5a));
    CASETRY(partition_by_category(c, n, dcat.as<uint8_t>(), dindex.as<int32_t>(), dcounts.as<int32_t>(), dout.as<int32_t>()));
    CASETRY(case_sync(c));
    return case_down(out, dout.p, (size_t)n + 1);
}
int kcase_category_buckets(void) { return kCatBuckets; }

// radix_sort_pairs over n (key, value) pairs.  known: 0 = the k_sort_varbits round trip, 1 = *known_varying as given.
// vals_out[n] = the sorted values; *in_a = 1 if they ended in buffer a (no pass, or an even number); *launches as counted.
int kcase_radix_sort(int n, const unsigned long long* keys, const int32_t* vals, int known, unsigned long long known_varying,
                     int32_t* vals_out, int32_t* in_a, int64_t* launches) {
    if (n < 1 || !keys || !vals || !vals_out || !in_a || !launches) return kCaseBadArg;
    CaseCtx cx;
    CASETRY(cx.open());
    blance_ctx* c = cx.c;
    CASETRY(case_sort_buffers(c, (size_t)n));
    CASETRY(case_sync(c));
    HIPTRY(hipMemcpy(c->f_keys_a.p, keys, sizeof(unsigned long long) * n, hipMemcpyHostToDevice));
    HIPTRY(hipMemcpy(c->f_vals_a.p, vals, sizeof(int32_t) * n, hipMemcpyHostToDevice));
    int32_t *sorted = nullptr, *other = nullptr;
    *launches = 0;
    CASETRY(radix_sort_pairs(c, n, launches, &sorted, &other, known ? &known_varying : nullptr));
    CASETRY(case_sync(c));
    *in_a = sorted == c->f_vals_a.as<int32_t>() ? 1 : 0;
    return case_down(vals_out, sorted, (size_t)n);
}

// k_sort_varbits alone, as radix_sort_pairs launches it: *out = the bits in which some key differs from keys[0]
int kcase_sort_varbits(int n, const unsigned long long* keys, unsigned long long* out) {
    if (n < 1 || !keys || !out) return kCaseBadArg;
    CaseCtx cx;
    CASETRY(cx.open());
    blance_ctx* c = cx.c;
    DevBuf dkeys, dout;
    CASETRY(case_up(dkeys, keys, (size_t)n));
    CASETRY(case_up<unsigned long long>(dout, nullptr, 1));
    launch_sort_varbits(c->stream, n, dkeys.as<unsigned long long>(), dout.as<unsigned long long>());
    CASETRY(case_sync(c));
    return case_down(out, dout.p, 1);
}

// k_flat_scan_min over part[2][n_waves]; scan_out[2] / not_whole_out[1] keep what the caller put there if the kernel is
// given a null pointer for them (with_scan / with_not_whole = 0)
int kcase_flat_scan_min(int n_waves, const int32_t* part, int with_scan, int with_not_whole, int end, int32_t* scan_out,
                        int32_t* not_whole_out) {
    if (n_waves < 1 || !part || !scan_out || !not_whole_out) return kCaseBadArg;
    CaseCtx cx;
    CASETRY(cx.open());
    blance_ctx* c = cx.c;
    DevBuf dpart, dscan, dnw;
    CASETRY(case_up(dpart, part, (size_t)2 * n_waves));
    CASETRY(case_up(dscan, scan_out, 2));
    CASETRY(case_up(dnw, not_whole_out, 1));
    launch_flat_scan_min(c->stream, n_waves, dpart.as<int32_t>(), with_scan ? dscan.as<int32_t>() : nullptr,
                         with_not_whole ? dnw.as<int32_t>() : nullptr, end);
    CASETRY(case_sync(c));
    CASETRY(case_down(scan_out, dscan.p, 2));
    return case_down(not_whole_out, dnw.p, 1);
}

// k_flat_row_count over P steps: top[oi] = the step's top priority node, -1 = no list for the top state, -2 = an empty one.
// row_count[N + 1]: steps per node, then the "" row.
int kcase_flat_row_count(int P, int N, const int32_t* top, int32_t* row_count) {
    if (P < 1 || N < 1 || !top || !row_count) return kCaseBadArg;
    for (int i = 0; i < P; i++) if (top[i] < -2 || top[i] >= N) return kCaseBadArg;
    CaseCtx cx;
    CASETRY(cx.open());
    blance_ctx* c = cx.c;
    FlatParams fq{};
    fq.N = N; fq.NX = N; fq.M = 1; fq.L = 1; fq.P = P; fq.top_state = 0; fq.RW = kRecHead + 2; fq.k = 1; fq.OW = 2;
    std::vector<int32_t> rec((size_t)P * fq.RW, 0);
    for (int i = 0; i < P; i++) {
        int32_t* r = &rec[(size_t)i * fq.RW];
        r[0] = i; r[1] = 1;
        if (top[i] >= 0) { r[kRecHead] = (kListSet << 16) | 1; r[kRecHead + 1] = top[i]; }
        else if (top[i] == -2) { r[kRecHead] = kListNil << 16; r[kRecHead + 1] = 0; }
    }
    DevBuf drec, drow;
    CASETRY(case_up(drec, rec.data(), rec.size()));
    CASETRY(case_up<int32_t>(drow, nullptr, (size_t)N + 2));
    fq.rec = drec.as<int32_t>();
    launch_flat_row_count(c->stream, fq, drow.as<int32_t>());
    CASETRY(case_sync(c));
    return case_down(row_count, drow.p, (size_t)N + 1);
}

// The first R picks of a fresh run (k = 1, every step alike), as run_flat_pass makes them: k_fresh_threshold ->
// k_fresh_emit -> radix_sort_pairs (cycle = 0), or k_fresh_cycle's closed form (cycle = 1: counters zero, w = 1, integer
// keys; m_off is not made then).  cnt_s[N]: the state's counters, tot[N]: the nodes' load totals, ntn_row[N]: the "" row
// of nodeToNodeCounts (read when NP > 0).  Out: m[N] picks per node, m_off[N + 1], seq[R] the picks in order.
int kcase_fresh_select(int N, const uint8_t* alive, const int32_t* cnt_s, const int32_t* tot, const int32_t* ntn_row,
                       const int32_t* node_w, const uint8_t* node_has_w, int NP, int booster_kind, int w, int R, int int_keys,
                       int cycle, int32_t* m, int32_t* m_off, int32_t* seq) {
    if (N < 1 || N > 8192 || R < 1 || w < 1 || NP < 0 || !alive || !cnt_s || !tot || !node_w || !node_has_w || !m || !m_off || !seq)
        return kCaseBadArg;
    if (NP > 0 && (N > 2048 || !ntn_row)) return kCaseBadArg;             // (the matrix is (N + 1) N words)
    int A = 0;
    bool any_w = false;
    for (int n = 0; n < N; n++) {
        A += alive[n] ? 1 : 0;
        any_w |= node_has_w[n] != 0;
        // validate_tail_b's guarantee to the kernels: no counter passes INT32_MAX however the R picks fall
        if (cnt_s[n] < 0 || tot[n] < cnt_s[n] || (int64_t)tot[n] + (int64_t)R * w >= INT32_MAX) return kCaseBadArg;
        if (NP > 0 && (ntn_row[n] < 0 || (int64_t)ntn_row[n] + R >= INT32_MAX)) return kCaseBadArg;
    }
    if (A < 1) return kCaseBadArg;
    if (int_keys && (NP > 0 || any_w)) return kCaseBadArg;
    if (cycle) {
        if (!int_keys || w != 1) return kCaseBadArg;
        for (int n = 0; n < N; n++) if (cnt_s[n] != 0 || tot[n] != 0) return kCaseBadArg;
    }
    CaseCtx cx;
    CASETRY(cx.open());
    blance_ctx* c = cx.c;
    FlatParams fq{};
    fq.N = N; fq.NX = N; fq.M = 1; fq.L = 1; fq.P = R; fq.s = 0; fq.k = 1; fq.top_state = 0; fq.NP = NP; fq.RW = kRecHead + 2;
    fq.OW = 2; fq.higher_mask = 0; fq.booster_kind = booster_kind; fq.int_keys = int_keys;
    const std::vector<int32_t> rec = case_records(1, 1, w, nullptr);
    std::vector<int32_t> cnt((size_t)2 * N, 0);                           // [(M + 1) NX]: the state's row, the extra loads' row
    for (int n = 0; n < N; n++) { cnt[n] = cnt_s[n]; cnt[(size_t)N + n] = tot[n] - cnt_s[n]; }
    DevBuf drec, dcnt, dntn;
    CASETRY(case_up(drec, rec.data(), rec.size()));
    CASETRY(case_up(dcnt, cnt.data(), cnt.size()));
    CASETRY(case_up(c->alive, alive, (size_t)N));
    CASETRY(case_up(c->node_weight, node_w, (size_t)N));
    CASETRY(case_up(c->node_has_weight, node_has_w, (size_t)N));
    CASETRY(case_up(c->f_tot, tot, (size_t)N, 1));
    CASETRY(case_up<int32_t>(c->f_m, nullptr, 0, (size_t)N + 2, 0x5a));
    CASETRY(case_up<int32_t>(c->f_moff, nullptr, 0, (size_t)N + 2, 0x5a));
    if (NP > 0) {
        CASETRY(case_up<int32_t>(dntn, nullptr, (size_t)(N + 1) * N));
        HIPTRY(hipMemcpy(dntn.as<int32_t>() + (size_t)N * N, ntn_row, sizeof(int32_t) * N, hipMemcpyHostToDevice));
    }
    CASETRY(case_sort_buffers(c, (size_t)R));
    fq.alive = c->alive.as<uint8_t>(); fq.node_weight = c->node_weight.as<int32_t>();
    fq.node_has_weight = c->node_has_weight.as<uint8_t>();
    fq.cnt = dcnt.as<int32_t>(); fq.tot = c->f_tot.as<int32_t>(); fq.ntn = NP > 0 ? dntn.as<int32_t>() : nullptr;
    fq.rec = drec.as<int32_t>();
    int32_t *sorted = nullptr, *other = nullptr;
    int64_t launches = 0;
    if (cycle) {
        std::vector<int32_t> ids, rank(N, -1);
        for (int n = 0; n < N; n++) if (alive[n]) { rank[n] = (int32_t)ids.size(); ids.push_back(n); }
        CASETRY(case_up(c->alive_ids, ids.data(), ids.size()));
        CASETRY(case_up(c->alive_rank, rank.data(), rank.size()));
        c->n_alive = A;
        fresh_cycle_sorted(c, N, R, &sorted, &other);
    } else {
        CASETRY(fresh_run_sorted(c, fq, 0, R, &launches, &sorted, &other));
    }
    CASETRY(case_sync(c));
    CASETRY(case_down(m, c->f_m.p, (size_t)N));
    CASETRY(case_down(m_off, c->f_moff.p, (size_t)N + 1));
    return case_down(seq, sorted, (size_t)R);
}

// The exclusion automaton over R steps of k picks: S[k R + k] the exclusion-free sequence, excl[t] the node step t may not
// take (-1: none).  Out: picks[k R] and *first_bad (INT_MAX: none), as run_flat_pass reads them.
int kcase_fresh_excl(int N, int k, int R, const int32_t* S, const int32_t* excl, int32_t* picks, int32_t* first_bad) {
    if (N < 1 || k < 1 || k > 2 || R < 1 || (int64_t)k * R + k > (1 << 24) || !S || !excl || !picks || !first_bad) return kCaseBadArg;
    for (int64_t i = 0; i < (int64_t)k * R + k; i++) if (S[i] < 0 || S[i] >= N) return kCaseBadArg;
    for (int t = 0; t < R; t++) if (excl[t] < -1 || excl[t] >= N) return kCaseBadArg;
    CaseCtx cx;
    CASETRY(cx.open());
    blance_ctx* c = cx.c;
    FlatParams fq{};
    fq.N = N; fq.NX = N; fq.M = 2; fq.L = 1; fq.P = R; fq.s = 1; fq.k = k; fq.top_state = 0; fq.NP = 0; fq.RW = kRecHead + 4;
    fq.OW = 1 + k; fq.higher_mask = 1;
    const std::vector<int32_t> rec = case_records(R, 2, 1, excl);
    DevBuf drec, dS, dpicks;
    const size_t ns = (size_t)k * R + k;
    CASETRY(case_up(drec, rec.data(), rec.size()));
    CASETRY(case_up(dS, S, ns));
    CASETRY(case_up<int32_t>(dpicks, nullptr, 0, ns, 0x5a));
    RESERVE(scalars, sizeof(int32_t) * kScalWords);
    HIPTRY(hipMemsetAsync(c->scalars.p, 0, sizeof(int32_t) * kScalWords, c->stream));
    fq.rec = drec.as<int32_t>();
    int32_t bad = 0;
    CASETRY(fresh_excl_resolve(c, fq, 0, R, dS.as<int32_t>(), dpicks.as<int32_t>(), c->scalars.as<int32_t>() + kScalFlatBad, &bad));
    *first_bad = bad;
    return case_down(picks, dpicks.p, (size_t)k * R);
}
// workgroups and steps per thread of the exclusion scan for a run of R steps (the tests place their seams by these)
int kcase_fresh_excl_shape(int R, int32_t* G, int32_t* per) {
    if (R < 1 || !G || !per) return kCaseBadArg;
    *G = fresh_excl_groups(R);
    *per = (R + *G * 1024 - 1) / (*G * 1024);
    return 0;
}


// k_flat_prepare alone.  Out: tot[NX + 1], g[NX + 1] and top_g[kTopList + 1] as raw 64-bit words, top_n[kTopList + 1] -- the
// last element of each is its guard.  Nodes [N, NX) are the removed ones: they get tot and g, never a place in the top list.
int kcase_flat_prepare(int N, int NX, int M, const int32_t* cnt, const uint8_t* alive, const int32_t* node_w, const uint8_t* node_has_w,
                       int NP, int booster_kind, int s, int32_t* tot, unsigned long long* g, unsigned long long* top_g, int32_t* top_n) {
    if (!case_flat_args_ok(N, NX, M, cnt, alive, node_w, node_has_w, NP, s) || !tot || !g || !top_g || !top_n) return kCaseBadArg;
    CaseCtx cx;
    CASETRY(cx.open());
    blance_ctx* c = cx.c;
    FlatCase f;
    FlatParams fq{};
    CASETRY(case_flat_tables(f, fq, N, NX, M, cnt, alive, node_w, node_has_w, NP, booster_kind, s));
    launch_flat_prepare(c->stream, fq, f.tot.as<int32_t>(), f.g.as<double>(), f.top_g.as<double>(), f.top_n.as<int32_t>());
    CASETRY(case_sync(c));
    CASETRY(case_down(tot, f.tot.p, (size_t)NX + 1));
    CASETRY(case_down(g, f.g.p, (size_t)NX + 1));
    CASETRY(case_down(top_g, f.top_g.p, (size_t)kTopList + 1));
    return case_down(top_n, f.top_n.p, (size_t)kTopList + 1);
}

// k_flat_prepare -> k_flat_scan over the steps [beg, end) -> k_flat_scan_min, as run_flat_pass's loop launches them.  The steps
// are given as lists (case_records_lists); row_count[NX + 1] is the caller's.  Out: scan[2 + 1] and part[2 * waves + 1], the
// last word of each its guard; part_words = 2 * waves + 1 is checked, waves as kcase_flat_scan_waves(beg, end) gives them.
int kcase_flat_scan(int N, int NX, int M, const int32_t* cnt, const uint8_t* alive, const int32_t* node_w, const uint8_t* node_has_w,
                    int NP, int booster_kind, int s, int P, int L, const int32_t* lists, const int32_t* len, const uint8_t* kind,
                    const int32_t* w, const double* stick, const int32_t* row_count, int k, int top_state, int higher_mask, int beg,
                    int end, int32_t* scan, int32_t* part, int part_words) {
    if (!case_flat_args_ok(N, NX, M, cnt, alive, node_w, node_has_w, NP, s) || P < 1 || P > kCaseMaxP || L < 1 || L > kCaseMaxL ||
        !w || !stick || !row_count || k < 1 || top_state < 0 || top_state >= M || beg < 0 || beg >= end || end > P || !scan || !part)
        return kCaseBadArg;
    if (!case_lists_ok(P, M, L, NX, lists, len, kind)) return kCaseBadArg;
    const int waves = flat_scan_waves(beg, end);
    if (part_words != 2 * waves + 1) return kCaseBadArg;
    CaseCtx cx;
    CASETRY(cx.open());
    blance_ctx* c = cx.c;
    FlatCase f;
    FlatParams fq{};
    CASETRY(case_flat_tables(f, fq, N, NX, M, cnt, alive, node_w, node_has_w, NP, booster_kind, s));
    const std::vector<int32_t> rec = case_records_lists(P, M, L, lists, len, kind, w, stick);
    DevBuf drec, dscan, dpart;
    CASETRY(case_up(drec, rec.data(), rec.size()));
    CASETRY(case_up<int32_t>(dscan, nullptr, 0, 3, 0x5a));
    CASETRY(case_up<int32_t>(dpart, nullptr, 0, (size_t)2 * waves + 1, 0x5a));
    HIPTRY(hipMemcpy(f.row_count.p, row_count, sizeof(int32_t) * ((size_t)NX + 1), hipMemcpyHostToDevice));
    fq.L = L; fq.P = P; fq.k = k; fq.top_state = top_state; fq.higher_mask = higher_mask; fq.RW = kRecHead + M * (1 + L); fq.OW = 1 + k;
    fq.rec = drec.as<int32_t>(); fq.scan = dscan.as<int32_t>(); fq.scan_part = dpart.as<int32_t>(); fq.scan_waves = waves;
    launch_flat_prepare(c->stream, fq, f.tot.as<int32_t>(), f.g.as<double>(), f.top_g.as<double>(), f.top_n.as<int32_t>());
    launch_flat_scan(c->stream, fq, beg, end);
    launch_flat_scan_min(c->stream, waves, fq.scan_part, fq.scan, nullptr, end);
    CASETRY(case_sync(c));
    CASETRY(case_down(scan, dscan.p, 3));
    return case_down(part, dpart.p, (size_t)2 * waves + 1);
}
int kcase_flat_scan_waves(int beg, int end) { return beg < 0 || beg >= end ? kCaseBadArg : flat_scan_waves(beg, end); }

// The stay test of a whole pass on the live lists, as run_flat_pass launches it under assume_stays: k_flat_prepare_count_live
// (NP > 0) or k_flat_prepare, then k_flat_stay_live.  The partitions are a hand-made DevProblem: live[P M L], live_len[P M],
// live_kind[P M], weights_nil, part_has_weight[P], part_weight[P]; order[P] a permutation; the states' stickiness.
// words[3]: copied in and out, the kernel's verdict word is words[1].  row_count[NX + 2]: the counted rows, the "" row, a guard.
int kcase_flat_stay_live(int N, int NX, int M, const int32_t* cnt, const uint8_t* alive, const int32_t* node_w,
                         const uint8_t* node_has_w, int NP, int booster_kind, int s, int P, int L, const int32_t* live,
                         const int32_t* live_len, const uint8_t* live_kind, const int32_t* order, int weights_nil,
                         const uint8_t* part_has_weight, const int32_t* part_weight, const int32_t* state_stick,
                         const uint8_t* state_has_stick, int k, int top_state, int higher_mask, int32_t* words, int32_t* row_count) {
    if (!case_flat_args_ok(N, NX, M, cnt, alive, node_w, node_has_w, NP, s) || P < 1 || P > kCaseMaxP || L < 1 || L > kCaseMaxL ||
        !order || !part_has_weight || !part_weight || !state_stick || !state_has_stick || k < 1 || top_state < 0 || top_state >= M ||
        !words || !row_count)
        return kCaseBadArg;
    if (!case_lists_ok(P, M, L, NX, live, live_len, live_kind)) return kCaseBadArg;
    for (int i = 0; i < P; i++) if (order[i] < 0 || order[i] >= P) return kCaseBadArg;
    CaseCtx cx;
    CASETRY(cx.open());
    blance_ctx* c = cx.c;
    FlatCase f;
    FlatParams fq{};
    CASETRY(case_flat_tables(f, fq, N, NX, M, cnt, alive, node_w, node_has_w, NP, booster_kind, s));
    DevBuf dlive, dlen, dkind, dorder, dphw, dpw, dss, dhs, dwords;
    CASETRY(case_up(dlive, live, (size_t)P * M * L));
    CASETRY(case_up(dlen, live_len, (size_t)P * M));
    CASETRY(case_up(dkind, live_kind, (size_t)P * M));
    CASETRY(case_up(dorder, order, (size_t)P));
    CASETRY(case_up(dphw, part_has_weight, (size_t)P));
    CASETRY(case_up(dpw, part_weight, (size_t)P));
    CASETRY(case_up(dss, state_stick, (size_t)M));
    CASETRY(case_up(dhs, state_has_stick, (size_t)M));
    CASETRY(case_up(dwords, words, 3));
    DevProblem d{};
    d.N = N; d.NX = NX; d.M = M; d.L = L; d.P = P; d.weights_nil = weights_nil ? 1 : 0;
    d.part_weight = dpw.as<int32_t>(); d.part_has_weight = dphw.as<uint8_t>();
    d.live = dlive.as<int32_t>(); d.live_len = dlen.as<int32_t>(); d.live_kind = dkind.as<uint8_t>();
    fq.L = L; fq.P = P; fq.k = k; fq.top_state = top_state; fq.higher_mask = higher_mask; fq.RW = kRecHead + M * (1 + L); fq.OW = 1 + k;
    if (NP > 0)
        launch_flat_prepare_count_live(c->stream, fq, f.tot.as<int32_t>(), f.g.as<double>(), f.top_g.as<double>(), f.top_n.as<int32_t>(), d,
                                       f.row_count.as<int32_t>());
    else
        launch_flat_prepare(c->stream, fq, f.tot.as<int32_t>(), f.g.as<double>(), f.top_g.as<double>(), f.top_n.as<int32_t>());
    launch_flat_stay_live(c->stream, fq, d, dorder.as<int32_t>(), dss.as<int32_t>(), dhs.as<uint8_t>(), dwords.as<int32_t>() + 1);
    CASETRY(case_sync(c));
    CASETRY(case_down(words, dwords.p, 3));
    return case_down(row_count, f.row_count.p, (size_t)NX + 2);
}

// k_flat_commit_stay over the steps [beg, end) of P (k = 1: two output words a step).  Every step of the range holds ONE node
// o < N in state s -- what a certain stay guarantees the kernel.  ntn[(NX + 1) N + 1]: copied in and out, the last word a guard
// of the caller's; out[2 P + 1]: filled with the guard, then written by the kernel.
int kcase_flat_commit_stay(int N, int NX, int M, int P, int L, const int32_t* lists, const int32_t* len, const uint8_t* kind,
                           const int32_t* w, const double* stick, int s, int top_state, int NP, int beg, int end, int bump,
                           int32_t* ntn, int32_t* out) {
    if (N < 1 || NX < N || NX > kCaseMaxNX || (int64_t)(NX + 1) * N > (1 << 24) || M < 1 || M > kMaxStates || s < 0 || s >= M ||
        top_state < 0 || top_state >= M || NP < 0 || P < 1 || P > kCaseMaxP || L < 1 || L > kCaseMaxL || !w || !stick || beg < 0 ||
        beg >= end || end > P || !ntn || !out)
        return kCaseBadArg;
    if (!case_lists_ok(P, M, L, NX, lists, len, kind)) return kCaseBadArg;
    for (int i = beg; i < end; i++) {
        const size_t idx = (size_t)i * M + s;
        if (kind[idx] == kListAbsent || len[idx] != 1 || lists[idx * L] >= N) return kCaseBadArg;
    }
    CaseCtx cx;
    CASETRY(cx.open());
    blance_ctx* c = cx.c;
    const std::vector<int32_t> rec = case_records_lists(P, M, L, lists, len, kind, w, stick);
    const size_t n_ntn = (size_t)(NX + 1) * N + 1;
    DevBuf drec, dntn, dout;
    CASETRY(case_up(drec, rec.data(), rec.size()));
    CASETRY(case_up(dntn, ntn, n_ntn));
    CASETRY(case_up<int32_t>(dout, nullptr, 0, (size_t)2 * P + 1, 0x5a));
    FlatParams fq{};
    fq.N = N; fq.NX = NX; fq.M = M; fq.L = L; fq.P = P; fq.s = s; fq.k = 1; fq.top_state = top_state; fq.NP = NP;
    fq.RW = kRecHead + M * (1 + L); fq.OW = 2;
    fq.rec = drec.as<int32_t>(); fq.ntn = dntn.as<int32_t>(); fq.out = dout.as<int32_t>();
    launch_flat_commit_stay(c->stream, fq, beg, end, bump);
    CASETRY(case_sync(c));
    CASETRY(case_down(ntn, dntn.p, n_ntn));
    return case_down(out, dout.p, (size_t)2 * P + 1);
}

}  // extern "C"
