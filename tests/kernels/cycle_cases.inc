// TEST INFRASTRUCTURE ONLY: k_cycle_group and k_cycle_top (blance_amd/csrc/k_cycle.h) alone, against the launches they stand
// for -- k_chain_classify + the stable counting sort by region + k_invert, and k_gather_chain's top priority keys + the
// stable counting sort by leaf -- on a hand-made world.  Included behind the product's headers by two wrappers:
// tests/kernels/cycle_cases.hip (hipcc, gfx950) and tests/simt/emu_cycle_cases.cpp (the SIMT emulator, g++).
// tests/cycle_case_tables.py has the worlds.
#include <algorithm>
#include <vector>

namespace {
constexpr int kCycleCaseBadArg = -100;

struct CycleDev {                        // device copies, freed together
    std::vector<void*> all;
    int st = 0;
    template <class T>
    T* make(const T* src, size_t n) {
        T* p = nullptr;
        if (!st) st = (int)hipMalloc((void**)&p, sizeof(T) * (n + 1));
        if (!st && p) all.push_back(p);
        if (!st && src && n) st = (int)hipMemcpy(p, src, sizeof(T) * n, hipMemcpyHostToDevice);
        return p;
    }
    template <class T>
    void back(T* dst, const T* src, size_t n) {
        if (!st && n) st = (int)hipMemcpy(dst, src, sizeof(T) * n, hipMemcpyDeviceToHost);
    }
    ~CycleDev() { for (void* p : all) (void)hipFree(p); }
};

// the stable counting sort of blance_hip.hip's group_by_key, for B * chunks small enough for one k_scan_excl launch
void cycle_case_sort(int n, const int32_t* key, const int32_t* src, int B, int32_t* counts, int32_t* offs, int32_t* out, int32_t* out_oi) {
    using namespace blance;
    hipStream_t st = nullptr;
    const int nch = (n + kPartChunk - 1) / kPartChunk;
    int bits = 1;
    while ((1 << bits) < B) bits++;
    BLANCE_LAUNCH(k_part_count, nch, 64, sizeof(int32_t) * B + 64, st, n, key, (const uint8_t*)nullptr, (const int32_t*)nullptr, nch, B, counts);
    BLANCE_LAUNCH(k_scan_excl, 1, 1024, 256, st, B * nch, counts);
    BLANCE_LAUNCH_NOSYNC(k_region_offsets, (B + 1 + 63) / 64, 64, 0, st, B, nch, n, counts, offs);
    BLANCE_LAUNCH(k_part_scatter, nch, 64, sizeof(int32_t) * B + 64, st, n, key, (const uint8_t*)nullptr, (const int32_t*)nullptr, src, nch, B, bits,
                  counts, out, out_oi);
}
}  // namespace

extern "C" int blance_case_cycle_words(void) { return blance::kCycWords; }
extern "C" int blance_case_cycle_flags(void) { return blance::kChainFlags; }

// which = 0: the parent's launches; 1: k_cycle_group, then k_cycle_top.  State 0 is the top state, state 1 the pass's.
// The arrays that go back come in as the caller filled them (a poison pattern) and return as the launches left them:
// chain_order, chain_oi, chain_inv, regid [P]; n_ev [P + 1]; reg_off [B + 1]; top_off [n_leaves + 1]; top_order [P];
// flags [kChainFlags].  closed: every launch behind a closed Gate.  with_top = 0: the grouping by region alone.
// Every index a kernel can form is checked first; a world that fails is refused without a launch (kCycleCaseBadArg).
extern "C" int blance_case_cycle(int which, int P, int L, int NX, int A, int B, int n_leaves, int refute, int closed, int with_top,
                                 const int32_t* order, const int32_t* live, const int32_t* live_len, const uint8_t* live_kind,
                                 const int32_t* node_region, const int32_t* node_leaf_pos, const int32_t* reg_lo,
                                 const int32_t* alive_ids, const int32_t* cyc, const int32_t* reg_off_tab, const int32_t* top_off_tab,
                                 int32_t* chain_order, int32_t* chain_oi, int32_t* chain_inv, int32_t* regid, int32_t* n_ev,
                                 int32_t* reg_off, int32_t* top_off, int32_t* top_order, int32_t* flags) {
    using namespace blance;
    const int M = 2, top_state = 0, m = 1;
    if (P < 1 || P > 8192 || L < 1 || L > 4 || NX < 1 || A < 1 || A > NX || B < 1 || B > 1024 || n_leaves < 1 || n_leaves > 4096) return kCycleCaseBadArg;
    const int nch = (P + kPartChunk - 1) / kPartChunk;
    if ((int64_t)B * nch > 4 * kScanTile || (int64_t)n_leaves * nch > 4 * kScanTile) return kCycleCaseBadArg;
    std::vector<char> seen((size_t)P, 0);
    for (int i = 0; i < P; i++) {
        if (order[i] < 0 || order[i] >= P || seen[order[i]]) return kCycleCaseBadArg;
        seen[order[i]] = 1;
    }
    for (int i = 0; i < P * M; i++) {
        if (live_len[i] < 0 || live_len[i] > L || live_kind[i] > kListSet) return kCycleCaseBadArg;
        for (int j = 0; j < live_len[i]; j++) if (live[(size_t)i * L + j] < 0 || live[(size_t)i * L + j] >= NX) return kCycleCaseBadArg;
    }
    for (int n = 0; n < NX; n++) {
        if (node_region[n] < -1 || node_region[n] >= B) return kCycleCaseBadArg;
        if (node_region[n] >= 0 && (node_leaf_pos[n] < 0 || node_leaf_pos[n] >= n_leaves || node_leaf_pos[n] < reg_lo[node_region[n]])) return kCycleCaseBadArg;
    }
    for (int a = 0; a < A; a++) {
        const int32_t* t = cyc + (size_t)a * kCycWords;
        if (alive_ids[a] < 0 || alive_ids[a] >= NX || t[kCycRegion] < 0 || t[kCycRegion] >= B || t[kCycLeaf] < 0 || t[kCycLeaf] >= n_leaves)
            return kCycleCaseBadArg;
        const int count = P / A + (a < P % A ? 1 : 0);
        for (int s = 0; s < count; s++) {
            const int64_t i = (int64_t)reg_off_tab[t[kCycRegion]] + (int64_t)s * t[kCycCount] + t[kCycRank];
            const int64_t j = (int64_t)top_off_tab[t[kCycLeaf]] + s;
            if (i < 0 || i >= P || j < 0 || j >= P) return kCycleCaseBadArg;
        }
    }
    CycleDev dv;
    DevProblem d{};
    d.N = NX; d.NX = NX; d.M = M; d.L = L; d.P = P; d.weights_nil = 1;
    d.live = dv.make(live, (size_t)P * M * L); d.live_len = dv.make(live_len, (size_t)P * M); d.live_kind = dv.make(live_kind, (size_t)P * M);
    const int32_t* d_order = dv.make(order, P);
    const int32_t* d_nreg = dv.make(node_region, NX);
    const int32_t* d_leafpos = dv.make(node_leaf_pos, NX);
    const int32_t* d_reglo = dv.make(reg_lo, B);
    const int32_t* d_alive = dv.make(alive_ids, A);
    const int32_t* d_cyc = dv.make(cyc, (size_t)A * kCycWords);
    const int32_t* d_rot = dv.make(reg_off_tab, (size_t)B + 1);
    const int32_t* d_tot = dv.make(top_off_tab, (size_t)n_leaves + 1);
    int32_t* d_co = dv.make(chain_order, P); int32_t* d_oi = dv.make(chain_oi, P); int32_t* d_inv = dv.make(chain_inv, P);
    int32_t* d_regid = dv.make(regid, P); int32_t* d_nev = dv.make(n_ev, (size_t)P + 1); int32_t* d_ro = dv.make(reg_off, (size_t)B + 1);
    int32_t* d_to = dv.make(top_off, (size_t)n_leaves + 1); int32_t* d_tord = dv.make(top_order, P);
    std::vector<int32_t> fl0(32, 0), minus((size_t)n_leaves, -1), zeros((size_t)n_leaves, 0), stick(M, 0);
    std::vector<uint8_t> has_stick(M, 0);
    if (closed) fl0[kFlagForced] = 1;
    int32_t* d_flags = dv.make(fl0.data(), fl0.size());
    const Gate gate = closed ? Gate{d_flags, 1u << kFlagForced} : kNoGate;
    int32_t* d_counts = dv.make((const int32_t*)nullptr, (size_t)std::max(B, n_leaves) * nch + 1);
    int32_t* d_topkey = dv.make((const int32_t*)nullptr, (size_t)P + 1);
    int32_t* d_crec = dv.make((const int32_t*)nullptr, (size_t)P * kCW + 64);
    const int32_t* d_cls = dv.make(minus.data(), minus.size());
    const int32_t* d_clsz = dv.make(zeros.data(), zeros.size());
    const int32_t* d_stick = dv.make(stick.data(), stick.size());
    const uint8_t* d_hstick = dv.make(has_stick.data(), has_stick.size());
    if (dv.st) return dv.st;
    hipStream_t sm = nullptr;
    if (which == 0) {
        BLANCE_LAUNCH_NOSYNC(k_chain_classify, (P + 1 + 255) / 256, 256, 0, sm, d, m, top_state, d_order, d_nreg, d_regid, d_nev, d_flags, gate);
        if (!closed) {                   // (the driver never sorts behind a closed gate: no region ids were written)
            cycle_case_sort(P, d_regid, d_order, B, d_counts, d_ro, d_co, d_oi);
            BLANCE_LAUNCH_NOSYNC(k_invert, (P + 255) / 256, 256, 0, sm, P, d_co, d_inv);
            if (with_top) {
                BLANCE_LAUNCH(k_gather_chain, (P + 255) / 256, 256, sizeof(int32_t) * 256 * (kCW + 1) + 64, sm, d, m, top_state, 1, d_co, d_oi,
                              d_stick, d_hstick, d_leafpos, d_nreg, d_reglo, d_cls, d_clsz, 0, 0, d_crec, d_flags, d_topkey, gate);
                cycle_case_sort(P, d_topkey, nullptr, n_leaves, d_counts, d_to, d_tord, nullptr);
            }
        }
    } else {
        BLANCE_LAUNCH_NOSYNC(k_cycle_group, (P + 1 + 255) / 256, 256, 0, sm, d, m, top_state, d_order, d_nreg, A, B, d_alive, d_cyc, d_rot,
                             refute, d_regid, d_nev, d_co, d_oi, d_inv, d_ro, d_flags, gate);
        if (with_top) {
            const int wpa = std::max(1, ((P + A - 1) / A + 63) / 64);
            BLANCE_LAUNCH_NOSYNC(k_cycle_top, (int)(((int64_t)A * wpa + 3) / 4), 256, 0, sm, P, A, wpa, n_leaves, d_cyc, d_rot, d_tot, d_to, d_tord, gate);
        }
    }
    dv.st = (int)hipGetLastError();
    if (!dv.st) dv.st = (int)hipStreamSynchronize(nullptr);
    dv.back(chain_order, d_co, P); dv.back(chain_oi, d_oi, P); dv.back(chain_inv, d_inv, P); dv.back(regid, d_regid, P);
    dv.back(n_ev, d_nev, (size_t)P + 1); dv.back(reg_off, d_ro, (size_t)B + 1); dv.back(top_off, d_to, (size_t)n_leaves + 1);
    dv.back(top_order, d_tord, P); dv.back(flags, d_flags, (size_t)kChainFlags);
    return dv.st;
}
