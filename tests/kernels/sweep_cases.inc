// TEST INFRASTRUCTURE ONLY: the kernels of k_sweep.h that stand between the live lists and a pass -- step records, the pass
// order's category, k_pass_queue's bit maps, the region chains' classification, events and compact records, a pass's list edits and the sweep's end -- one at a time, on a DevProblem a test
// makes by hand.  Included behind kernel_cases.inc by the same two wrappers (tests/simt/emu_kernel_cases.cpp,
// tests/kernels/kernel_cases.hip) and built into the same libraries; kernel_cases.inc has the conventions and the helpers.
// Every launch goes through the shape_* helper the driver uses, and an entry returns the launch's own status after it has
// synchronised: a launch the runtime refuses shows as an error code, not as untouched output.
// (tests/sweep_case_tables.py has the cases and the references.)

extern "C" {
// A DevProblem in host arrays: lists [P M L] with lengths [P M] and kinds [P M], flags [P], node tables [NX], weights [P].
// An entry copies ALL of them back, so a test sees every array a kernel may have written.
struct KSweepProblem {
    int32_t N, NX, M, L, P, weights_nil;
    int32_t* live; int32_t* live_len; uint8_t* live_kind;
    int32_t* prv; int32_t* prv_len; uint8_t* prv_kind;
    uint8_t* in_prev; uint8_t* never_equal;
    uint8_t* node_removed; uint8_t* node_added;
    int32_t* part_weight; uint8_t* part_has_weight;
};
}

namespace {
constexpr int kCaseGuard = -101;                     // a kernel wrote the guard behind one of the problem's arrays

bool case_problem_ok(const KSweepProblem* h) {
    if (!h || h->N < 1 || h->NX < h->N || h->NX > kCaseMaxNX || h->M < 1 || h->M > kMaxStates || h->L < 1 || h->L > kCaseMaxL ||
        h->P < 1 || h->P > kCaseMaxP)
        return false;
    if (!h->in_prev || !h->never_equal || !h->node_removed || !h->node_added || !h->part_weight || !h->part_has_weight) return false;
    return case_lists_ok(h->P, h->M, h->L, h->NX, h->live, h->live_len, h->live_kind) &&
           case_lists_ok(h->P, h->M, h->L, h->NX, h->prv, h->prv_len, h->prv_kind);
}
bool case_perm_ok(int n, const int32_t* perm) {      // a permutation of 0 .. n - 1 (k_invert, k_sweep_tail's inverse)
    if (!perm) return false;
    std::vector<char> seen((size_t)n, 0);
    for (int i = 0; i < n; i++) {
        if (perm[i] < 0 || perm[i] >= n || seen[perm[i]]) return false;
        seen[perm[i]] = 1;
    }
    return true;
}
bool case_state_ok(const KSweepProblem* h, int m) { return m >= 0 && m < h->M; }

template <class T>
int case_down_guarded(T* dst, const DevBuf& b, size_t n) {
    std::vector<T> tmp(n + 1);
    CASETRY(case_down(tmp.data(), b.p, n + 1));
    T g;
    memset(&g, 0x5a, sizeof g);
    if (memcmp(&tmp[n], &g, sizeof g)) return kCaseGuard;
    memcpy(dst, tmp.data(), sizeof(T) * n);
    return 0;
}

// the hand-made problem on the device (one guard element behind every array) and back
struct SweepCase {
    DevBuf live, live_len, live_kind, prv, prv_len, prv_kind, in_prev, never_equal, node_removed, node_added, part_weight, part_has_weight;
    DevProblem d{};
    int up(const KSweepProblem& h) {
        const size_t PM = (size_t)h.P * h.M, P = (size_t)h.P, NX = (size_t)h.NX;
        CASETRY(case_up(live, h.live, PM * h.L, 1, 0x5a));
        CASETRY(case_up(live_len, h.live_len, PM, 1, 0x5a));
        CASETRY(case_up(live_kind, h.live_kind, PM, 1, 0x5a));
        CASETRY(case_up(prv, h.prv, PM * h.L, 1, 0x5a));
        CASETRY(case_up(prv_len, h.prv_len, PM, 1, 0x5a));
        CASETRY(case_up(prv_kind, h.prv_kind, PM, 1, 0x5a));
        CASETRY(case_up(in_prev, h.in_prev, P, 1, 0x5a));
        CASETRY(case_up(never_equal, h.never_equal, P, 1, 0x5a));
        CASETRY(case_up(node_removed, h.node_removed, NX, 1, 0x5a));
        CASETRY(case_up(node_added, h.node_added, NX, 1, 0x5a));
        CASETRY(case_up(part_weight, h.part_weight, P, 1, 0x5a));
        CASETRY(case_up(part_has_weight, h.part_has_weight, P, 1, 0x5a));
        d.N = h.N; d.NX = h.NX; d.M = h.M; d.L = h.L; d.P = h.P; d.weights_nil = h.weights_nil ? 1 : 0;
        d.node_removed = node_removed.as<uint8_t>(); d.node_added = node_added.as<uint8_t>();
        d.part_weight = part_weight.as<int32_t>(); d.part_has_weight = part_has_weight.as<uint8_t>();
        d.live = live.as<int32_t>(); d.live_len = live_len.as<int32_t>(); d.live_kind = live_kind.as<uint8_t>();
        d.prv = prv.as<int32_t>(); d.prv_len = prv_len.as<int32_t>(); d.prv_kind = prv_kind.as<uint8_t>();
        d.in_prev = in_prev.as<uint8_t>(); d.never_equal = never_equal.as<uint8_t>();
        return 0;
    }
    int down(const KSweepProblem& h) {
        const size_t PM = (size_t)h.P * h.M, P = (size_t)h.P, NX = (size_t)h.NX;
        CASETRY(case_down_guarded(h.live, live, PM * h.L));
        CASETRY(case_down_guarded(h.live_len, live_len, PM));
        CASETRY(case_down_guarded(h.live_kind, live_kind, PM));
        CASETRY(case_down_guarded(h.prv, prv, PM * h.L));
        CASETRY(case_down_guarded(h.prv_len, prv_len, PM));
        CASETRY(case_down_guarded(h.prv_kind, prv_kind, PM));
        CASETRY(case_down_guarded(h.in_prev, in_prev, P));
        CASETRY(case_down_guarded(h.never_equal, never_equal, P));
        CASETRY(case_down_guarded(h.node_removed, node_removed, NX));
        CASETRY(case_down_guarded(h.node_added, node_added, NX));
        CASETRY(case_down_guarded(h.part_weight, part_weight, P));
        return case_down_guarded(h.part_has_weight, part_has_weight, P);
    }
};

// the stream is drained, then the launches' own status: what a refused launch leaves behind
int case_sync_launched(blance_ctx* c) {
    CASETRY(case_sync(c));
    HIPTRY(hipGetLastError());
    return 0;
}
// The region tables a chain pass reads: node_region[NX] in [-1, B), node_leaf_pos[NX] a leaf of [0, n_leaves) not below its
// region's first, reg_lo[B]; with_cls: leaf_cls[n_leaves] >= -1 and, for a class c of a leaf of region r, reg_lo[r] + c a
// leaf too (cls_size is read there).
bool case_regions_ok(int NX, int B, int n_leaves, const int32_t* node_region, const int32_t* node_leaf_pos, const int32_t* reg_lo,
                     const int32_t* leaf_cls, const int32_t* cls_size, bool with_cls) {
    if (B < 1 || B > 4096 || n_leaves < 1 || n_leaves > kCaseMaxNX || !node_region || !node_leaf_pos || !reg_lo) return false;
    if (with_cls && (!leaf_cls || !cls_size)) return false;
    for (int b = 0; b < B; b++) if (reg_lo[b] < 0 || reg_lo[b] >= n_leaves) return false;
    for (int x = 0; x < NX; x++) {
        const int r = node_region[x], lp = node_leaf_pos[x];
        if (r < -1 || r >= B || lp < 0 || lp >= n_leaves) return false;
        if (r >= 0 && lp < reg_lo[r]) return false;
        if (with_cls && r >= 0) {
            const int cl = leaf_cls[lp];
            if (cl < -1 || (cl >= 0 && reg_lo[r] + cl >= n_leaves)) return false;
        }
    }
    return true;
}
bool case_gate_closed(const int32_t* words, unsigned mask) {
    bool closed = false;
    for (int b = 0; b < kGateWords; b++) closed |= ((mask >> b) & 1) && words[b] != 0;
    return closed;
}
}  // namespace

extern "C" {

// k_category: cat[P + 1], the last byte its guard
int kcase_category(const KSweepProblem* h, int m, int any_removed, int add_nil, uint8_t* cat) {
    if (!case_problem_ok(h) || !case_state_ok(h, m) || !cat) return kCaseBadArg;
    CaseCtx cx;
    CASETRY(cx.open());
    blance_ctx* c = cx.c;
    SweepCase s;
    CASETRY(s.up(*h));
    DevBuf dcat;
    CASETRY(case_up<uint8_t>(dcat, nullptr, 0, (size_t)h->P + 1, 0x5a));
    BLANCE_LAUNCH_NOSYNC(k_category, cdiv(h->P, 256), 256, 0, c->stream, s.d, m, any_removed ? 1 : 0, add_nil ? 1 : 0, dcat.as<uint8_t>());
    CASETRY(case_sync_launched(c));
    CASETRY(s.down(*h));
    return case_down(cat, dcat.p, (size_t)h->P + 1);
}

// k_gather in pass order `order` (partition ids, each < P).  rec[P RW + 1]: the records and a guard; row_count[NX + 2]: zeroed,
// counted when with_rows (the "" row is row NX), the last word a guard -- left as zeroed when with_rows = 0.
int kcase_gather(const KSweepProblem* h, int m, int top_state, const int32_t* order, const int32_t* state_stick,
                 const uint8_t* state_has_stick, int with_rows, int32_t* rec, int32_t* row_count) {
    if (!case_problem_ok(h) || !case_state_ok(h, m) || !case_state_ok(h, top_state) || !order || !state_stick || !state_has_stick ||
        !rec || !row_count)
        return kCaseBadArg;
    const int RW = kRecHead + h->M * (1 + h->L);
    if (RW > 64) return kCaseBadArg;                 // (what blance_validate admits)
    for (int i = 0; i < h->P; i++) if (order[i] < 0 || order[i] >= h->P) return kCaseBadArg;
    CaseCtx cx;
    CASETRY(cx.open());
    blance_ctx* c = cx.c;
    SweepCase s;
    CASETRY(s.up(*h));
    const size_t n_rec = (size_t)h->P * RW;
    DevBuf dorder, dss, dhs, drec, drow;
    CASETRY(case_up(dorder, order, (size_t)h->P));
    CASETRY(case_up(dss, state_stick, (size_t)h->M));
    CASETRY(case_up(dhs, state_has_stick, (size_t)h->M));
    CASETRY(case_up<int32_t>(drec, nullptr, 0, n_rec + 1, 0x5a));
    std::vector<int32_t> rows((size_t)h->NX + 2, 0);
    rows[(size_t)h->NX + 1] = 0x5a5a5a5a;
    CASETRY(case_up(drow, rows.data(), rows.size()));
    const LaunchShape gs = shape_gather(h->P, RW);
    BLANCE_LAUNCH(k_gather, gs.grid, gs.block, gs.lds, c->stream, s.d, m, top_state, RW, dorder.as<int32_t>(), dss.as<int32_t>(),
                  dhs.as<uint8_t>(), drec.as<int32_t>(), with_rows ? drow.as<int32_t>() : (int32_t*)nullptr, h->NX);
    CASETRY(case_sync_launched(c));
    CASETRY(s.down(*h));
    CASETRY(case_down(rec, drec.p, n_rec + 1));
    return case_down(row_count, drow.p, (size_t)h->NX + 2);
}

// k_ntn_bits over ntn[rows N] (the driver: rows = NX + 1).  BW as the driver computes it; bits[rows BW + 1], the last word a guard.
int kcase_ntn_bits_words(int NX) { return NX < 1 || NX > 4096 ? kCaseBadArg : (int)(queue_bits_words(NX) / ((size_t)NX + 1)); }
int kcase_ntn_bits(int N, int NX, int rows, const int32_t* ntn, uint32_t* bits) {
    if (N < 1 || NX < N || NX > 4096 || rows < 1 || rows > NX + 1 || !ntn || !bits) return kCaseBadArg;
    const int BW = (int)(queue_bits_words(NX) / ((size_t)NX + 1));
    if ((long long)BW * 32 < N) return kCaseBadArg;
    CaseCtx cx;
    CASETRY(cx.open());
    blance_ctx* c = cx.c;
    DevBuf dntn, dbits;
    const size_t n_bits = (size_t)rows * BW;
    CASETRY(case_up(dntn, ntn, (size_t)rows * N));
    CASETRY(case_up<uint32_t>(dbits, nullptr, 0, n_bits + 1, 0x5a));
    const LaunchShape bs = shape_ntn_bits(rows);
    BLANCE_LAUNCH(k_ntn_bits, bs.grid, bs.block, bs.lds, c->stream, N, rows, BW, dntn.as<int32_t>(), dbits.as<uint32_t>());
    CASETRY(case_sync_launched(c));
    return case_down(bits, dbits.p, n_bits + 1);
}

// k_invert: inv[n + 1], the last word its guard
int kcase_invert(int n, const int32_t* perm, int32_t* inv) {
    if (n < 1 || n > kCaseMaxP || !inv || !case_perm_ok(n, perm)) return kCaseBadArg;
    CaseCtx cx;
    CASETRY(cx.open());
    blance_ctx* c = cx.c;
    DevBuf dperm, dinv;
    CASETRY(case_up(dperm, perm, (size_t)n));
    CASETRY(case_up<int32_t>(dinv, nullptr, 0, (size_t)n + 1, 0x5a));
    BLANCE_LAUNCH_NOSYNC(k_invert, cdiv(n, 256), 256, 0, c->stream, n, dperm.as<int32_t>(), dinv.as<int32_t>());
    CASETRY(case_sync_launched(c));
    return case_down(inv, dinv.p, (size_t)n + 1);
}

// The sweep's end after state m's pass, whose choices are out[P OW] in pass order `order` (a permutation): per step
// n_out | nil << 16, then n_out node ids.
//   mode 0, fused: k_invert, then k_sweep_tail (with_out = 0: out is null; with_cnt = 0: cnt_next is null)
//   mode 1, unfused: k_scatter (when with_out), k_converge, k_count_prev into the zeroed cnt_next (when with_cnt), k_live_refresh
//   mode 2: k_scatter alone;  mode 3: k_scatter (when with_out), then k_converge
// words[3]: a sentinel, the not_match word, a sentinel -- copied in and out.  gate_words[kGateWords] with gate_mask (0: no
// Gate) stand for the scalar block a Gate looks at.  cnt_next[M NX + 1]: zeroed, the last word a guard.
int kcase_sweep_end(const KSweepProblem* h, int mode, int m, int OW, const int32_t* order, const int32_t* out, int with_out, int with_cnt,
                    int32_t* words, const int32_t* gate_words, unsigned gate_mask, int32_t* cnt_next) {
    if (!case_problem_ok(h) || !case_state_ok(h, m) || mode < 0 || mode > 3 || OW < 1 || OW > 1 + h->L || !out || !words || !gate_words ||
        !cnt_next || !case_perm_ok(h->P, order))
        return kCaseBadArg;
    for (int i = 0; i < h->P; i++) {
        const int32_t* o = out + (size_t)i * OW;
        const int n_out = o[0] & 0xffff;
        if (o[0] < 0 || (o[0] >> 16) > 1 || n_out > OW - 1) return kCaseBadArg;
        for (int j = 0; j < n_out; j++) if (o[1 + j] < 0 || o[1 + j] >= h->NX) return kCaseBadArg;
    }
    CaseCtx cx;
    CASETRY(cx.open());
    blance_ctx* c = cx.c;
    SweepCase s;
    CASETRY(s.up(*h));
    const int P = h->P;
    const size_t n_cnt = (size_t)h->M * h->NX;
    DevBuf dorder, dinv, dout, dwords, dgate, dcnt;
    CASETRY(case_up(dorder, order, (size_t)P));
    CASETRY(case_up<int32_t>(dinv, nullptr, 0, (size_t)P + 1, 0x5a));
    CASETRY(case_up(dout, out, (size_t)P * OW));
    CASETRY(case_up(dwords, words, 3));
    CASETRY(case_up(dgate, gate_words, (size_t)kGateWords));
    std::vector<int32_t> cnt0(n_cnt + 1, 0);
    cnt0[n_cnt] = 0x5a5a5a5a;
    CASETRY(case_up(dcnt, cnt0.data(), cnt0.size()));
    const Gate gate = gate_mask ? Gate{dgate.as<int32_t>(), gate_mask} : kNoGate;
    int32_t* not_match = dwords.as<int32_t>() + 1;
    hipStream_t sm = c->stream;
    if (mode == 0) {
        BLANCE_LAUNCH_NOSYNC(k_invert, cdiv(P, 256), 256, 0, sm, P, dorder.as<int32_t>(), dinv.as<int32_t>());
        const LaunchShape ts = shape_sweep_tail(P);
        BLANCE_LAUNCH(k_sweep_tail, ts.grid, ts.block, ts.lds, sm, s.d, m, OW, with_out ? dinv.as<int32_t>() : (const int32_t*)nullptr,
                      with_out ? dout.as<int32_t>() : (const int32_t*)nullptr, not_match, with_cnt ? dcnt.as<int32_t>() : (int32_t*)nullptr, gate);
    } else {
        if (with_out || mode == 2) {
            const LaunchShape ss = shape_scatter(P);
            BLANCE_LAUNCH_NOSYNC(k_scatter, ss.grid, ss.block, ss.lds, sm, s.d, m, OW, dorder.as<int32_t>(), dout.as<int32_t>(), gate);
        }
        if (mode != 2) {
            const LaunchShape cs = shape_converge(P);
            BLANCE_LAUNCH(k_converge, cs.grid, cs.block, cs.lds, sm, s.d, not_match, gate);
        }
        if (mode == 1) {
            // (the driver opens the next sweep only after it has read the sweep's words: these two have no Gate, and do not run behind a closed one)
            const int PM = P * h->M;
            if (case_gate_closed(gate_words, gate_mask)) { /* the host comes back: no opening */ } else {
            if (with_cnt) BLANCE_LAUNCH_NOSYNC(k_count_prev, cdiv(PM, 256), 256, 0, sm, s.d, dcnt.as<int32_t>());
            BLANCE_LAUNCH_NOSYNC(k_live_refresh, cdiv(PM, 256), 256, 0, sm, s.d);
            }
        }
    }
    CASETRY(case_sync_launched(c));
    CASETRY(s.down(*h));
    CASETRY(case_down(words, dwords.p, 3));
    return case_down(cnt_next, dcnt.p, n_cnt + 1);
}

// k_chain_classify over the pass order `order` (a permutation), then -- stage 1 -- what ChainPass::events launches: the scan of
// n_ev and k_chain_ev_fill, when no step was NotLocal and the Events word is up; cnt[(M + 1) NX + 1] (or null; the last word a
// guard of the caller's): k_chain_orphans on it.  flags[kGateWords + 1]: the caller's starting words and a guard, copied in and
// out; the Gate looks at the same block (gate_mask 0: no Gate) -- behind a closed one only the classification is launched.
// Out: regid[P + 1], n_ev[P + 2] (the counts, before the scan), *n_events, ev_key / ev_oi / ev_leaf / ev_w[ev_cap + 1], each
// with its guard.  More events than ev_cap: kCaseBadArg before k_chain_ev_fill is launched.
int kcase_chain_events(const KSweepProblem* h, int m, int top_state, const int32_t* order, const int32_t* node_region,
                       const int32_t* node_leaf_pos, const int32_t* reg_lo, int B, int n_leaves, int32_t* flags, unsigned gate_mask,
                       int stage, int32_t* regid, int32_t* n_ev, int ev_cap, int32_t* n_events, int32_t* ev_key, int32_t* ev_oi,
                       int32_t* ev_leaf, int32_t* ev_w, int32_t* cnt) {
    if (!case_problem_ok(h) || !case_state_ok(h, m) || !case_state_ok(h, top_state) || !case_perm_ok(h->P, order) || !flags ||
        stage < 0 || stage > 1 || !regid || !n_ev || ev_cap < 0 || ev_cap > (1 << 20) || !n_events || !ev_key || !ev_oi || !ev_leaf || !ev_w)
        return kCaseBadArg;
    if (!case_regions_ok(h->NX, B, n_leaves, node_region, node_leaf_pos, reg_lo, nullptr, nullptr, false)) return kCaseBadArg;
    CaseCtx cx;
    CASETRY(cx.open());
    blance_ctx* c = cx.c;
    SweepCase s;
    CASETRY(s.up(*h));
    const int P = h->P;
    const size_t n_cnt = (size_t)(h->M + 1) * h->NX;
    DevBuf dorder, dreg, dleaf, dlo, dflags, dregid, dnev, dkey, doi, dlf, dw, dcnt;
    CASETRY(case_up(dorder, order, (size_t)P));
    CASETRY(case_up(dreg, node_region, (size_t)h->NX));
    CASETRY(case_up(dleaf, node_leaf_pos, (size_t)h->NX));
    CASETRY(case_up(dlo, reg_lo, (size_t)B));
    CASETRY(case_up(dflags, flags, (size_t)kGateWords + 1));
    CASETRY(case_up<int32_t>(dregid, nullptr, 0, (size_t)P + 1, 0x5a));
    CASETRY(case_up<int32_t>(dnev, nullptr, 0, (size_t)P + 2, 0x5a));
    CASETRY(case_up<int32_t>(dkey, nullptr, 0, (size_t)ev_cap + 1, 0x5a));
    CASETRY(case_up<int32_t>(doi, nullptr, 0, (size_t)ev_cap + 1, 0x5a));
    CASETRY(case_up<int32_t>(dlf, nullptr, 0, (size_t)ev_cap + 1, 0x5a));
    CASETRY(case_up<int32_t>(dw, nullptr, 0, (size_t)ev_cap + 1, 0x5a));
    if (cnt) CASETRY(case_up(dcnt, cnt, n_cnt + 1));
    const bool closed = case_gate_closed(flags, gate_mask);
    const Gate gate = gate_mask ? Gate{dflags.as<int32_t>(), gate_mask} : kNoGate;
    hipStream_t sm = c->stream;
    const LaunchShape cs = shape_chain_classify(P);
    BLANCE_LAUNCH_NOSYNC(k_chain_classify, cs.grid, cs.block, cs.lds, sm, s.d, m, top_state, dorder.as<int32_t>(), dreg.as<int32_t>(),
                         dregid.as<int32_t>(), dnev.as<int32_t>(), dflags.as<int32_t>(), gate);
    CASETRY(case_sync_launched(c));
    CASETRY(case_down(flags, dflags.p, (size_t)kGateWords + 1));
    CASETRY(case_down(regid, dregid.p, (size_t)P + 1));
    CASETRY(case_down(n_ev, dnev.p, (size_t)P + 2));
    *n_events = 0;
    if (!closed && stage == 1 && !flags[kFlagNotLocal] && flags[kFlagEvents]) {
        CASETRY(launch_scan_excl_on(c, sm, c->scan_sums, P + 1, dnev.as<int32_t>()));
        CASETRY(case_sync_launched(c));
        CASETRY(case_down(n_events, dnev.as<int32_t>() + P, 1));
        if (*n_events < 0 || *n_events > ev_cap) return kCaseBadArg;
        if (*n_events > 0)
            BLANCE_LAUNCH_NOSYNC(k_chain_ev_fill, cdiv(P, 256), 256, 0, sm, s.d, m, top_state, dorder.as<int32_t>(), dreg.as<int32_t>(),
                                 dlo.as<int32_t>(), dleaf.as<int32_t>(), dregid.as<int32_t>(), dnev.as<int32_t>(), dkey.as<int32_t>(),
                                 doi.as<int32_t>(), dlf.as<int32_t>(), dw.as<int32_t>());
    }
    if (!closed && cnt)
        BLANCE_LAUNCH_NOSYNC(k_chain_orphans, cdiv(P, 256), 256, 0, sm, s.d, m, top_state, dorder.as<int32_t>(), dreg.as<int32_t>(),
                             dcnt.as<int32_t>());
    CASETRY(case_sync_launched(c));
    CASETRY(s.down(*h));
    CASETRY(case_down(ev_key, dkey.p, (size_t)ev_cap + 1));
    CASETRY(case_down(ev_oi, doi.p, (size_t)ev_cap + 1));
    CASETRY(case_down(ev_leaf, dlf.p, (size_t)ev_cap + 1));
    CASETRY(case_down(ev_w, dw.p, (size_t)ev_cap + 1));
    if (cnt) CASETRY(case_down(cnt, dcnt.p, n_cnt + 1));
    return 0;
}

// k_gather_chain over chain_order (a permutation), chain_oi[P] or null.  flags as in kcase_chain_events.  Out: crec[P kCW + 1]
// and its guard; topkey[P + 1] and its guard when with_topkey (the kernel gets null otherwise and topkey comes back zeroed).
int kcase_gather_chain(const KSweepProblem* h, int m, int top_state, int higher_mask, const int32_t* chain_order, const int32_t* chain_oi,
                       const int32_t* state_stick, const uint8_t* state_has_stick, const int32_t* node_region,
                       const int32_t* node_leaf_pos, const int32_t* reg_lo, const int32_t* leaf_cls, const int32_t* cls_size, int B,
                       int n_leaves, int flat, int classify, int32_t* flags, unsigned gate_mask, int with_topkey, int32_t* crec,
                       int32_t* topkey) {
    if (!case_problem_ok(h) || !case_state_ok(h, m) || !case_state_ok(h, top_state) || !case_perm_ok(h->P, chain_order) || !state_stick ||
        !state_has_stick || !flags || !crec || !topkey || higher_mask < 0 || higher_mask >= (1 << h->M))
        return kCaseBadArg;
    if (!case_regions_ok(h->NX, B, n_leaves, node_region, node_leaf_pos, reg_lo, leaf_cls, cls_size, true)) return kCaseBadArg;
    if (flat) for (int x = 0; x < h->NX; x++) if (node_region[x] != 0) return kCaseBadArg;      // (the flat chain's one region)
    CaseCtx cx;
    CASETRY(cx.open());
    blance_ctx* c = cx.c;
    SweepCase s;
    CASETRY(s.up(*h));
    const int P = h->P;
    DevBuf dorder, doi, dss, dhs, dreg, dleaf, dlo, dcls, dsz, dflags, dcrec, dtop;
    CASETRY(case_up(dorder, chain_order, (size_t)P));
    if (chain_oi) CASETRY(case_up(doi, chain_oi, (size_t)P));
    CASETRY(case_up(dss, state_stick, (size_t)h->M));
    CASETRY(case_up(dhs, state_has_stick, (size_t)h->M));
    CASETRY(case_up(dreg, node_region, (size_t)h->NX));
    CASETRY(case_up(dleaf, node_leaf_pos, (size_t)h->NX));
    CASETRY(case_up(dlo, reg_lo, (size_t)B));
    CASETRY(case_up(dcls, leaf_cls, (size_t)n_leaves));
    CASETRY(case_up(dsz, cls_size, (size_t)n_leaves));
    CASETRY(case_up(dflags, flags, (size_t)kGateWords + 1));
    CASETRY(case_up<int32_t>(dcrec, nullptr, 0, (size_t)P * kCW + 1, 0x5a));
    if (with_topkey) CASETRY(case_up<int32_t>(dtop, nullptr, 0, (size_t)P + 1, 0x5a));
    const Gate gate = gate_mask ? Gate{dflags.as<int32_t>(), gate_mask} : kNoGate;
    const LaunchShape gs = shape_gather_chain(P);
    BLANCE_LAUNCH(k_gather_chain, gs.grid, gs.block, gs.lds, c->stream, s.d, m, top_state, higher_mask, dorder.as<int32_t>(),
                  chain_oi ? doi.as<int32_t>() : (const int32_t*)nullptr, dss.as<int32_t>(), dhs.as<uint8_t>(), dleaf.as<int32_t>(),
                  dreg.as<int32_t>(), dlo.as<int32_t>(), dcls.as<int32_t>(), dsz.as<int32_t>(), flat ? 1 : 0, classify ? 1 : 0,
                  dcrec.as<int32_t>(), dflags.as<int32_t>(), with_topkey ? dtop.as<int32_t>() : (int32_t*)nullptr, gate);
    CASETRY(case_sync_launched(c));
    CASETRY(s.down(*h));
    CASETRY(case_down(flags, dflags.p, (size_t)kGateWords + 1));
    CASETRY(case_down(crec, dcrec.p, (size_t)P * kCW + 1));
    if (with_topkey) CASETRY(case_down(topkey, dtop.p, (size_t)P + 1));
    else memset(topkey, 0, sizeof(int32_t) * ((size_t)P + 1));
    return 0;
}

}  // extern "C"
