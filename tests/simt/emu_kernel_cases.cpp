// TEST INFRASTRUCTURE ONLY: single product kernels under the SIMT emulator on inputs a test makes by hand -- for branches
// that no plan reaches (see tests/test_fewer_launches_kernels_emulated.py).  The library is emu_lib.cpp's plus these entries.
#include "emu_lib.cpp"
#include <vector>

extern "C" {

// The flag words of k_chain_classify (into flags_classify) and of k_gather_chain (classify as given, into flags_gather)
// over the same live lists: kChainFlags words each, zeroed by the caller.  No partition weights; every leaf has no exclude class.
void emu_case_classify_words(int P, int M, int L, int N, int m, int top_state, int32_t* live, int32_t* live_len,
                             uint8_t* live_kind, const int32_t* order, const int32_t* node_region, const int32_t* node_leaf_pos,
                             const int32_t* reg_lo, int n_leaves, int classify, int32_t* flags_classify, int32_t* flags_gather) {
    DevProblem d{};
    d.N = N; d.NX = N; d.M = M; d.L = L; d.P = P; d.weights_nil = 1;
    d.live = live; d.live_len = live_len; d.live_kind = live_kind;
    std::vector<int32_t> regid(P + 1), n_ev(P + 2), crec((size_t)(P + 1) * kCW), leaf_cls(n_leaves + 1, -1), cls_size(n_leaves + 1, 0);
    std::vector<int32_t> stick(M + 1, 0);
    std::vector<uint8_t> has_stick(M + 1, 0);
    hipStream_t sm = nullptr;
    BLANCE_LAUNCH_NOSYNC(k_chain_classify, cdiv(P + 1, 256), 256, 0, sm, d, m, top_state, order, node_region, regid.data(),
                         n_ev.data(), flags_classify, kNoGate);
    BLANCE_LAUNCH(k_gather_chain, cdiv(P, 256), 256, sizeof(int32_t) * 256 * (kCW + 1) + 64, sm, d, m, top_state, 1 << top_state,
                  order, (const int32_t*)nullptr, stick.data(), has_stick.data(), node_leaf_pos, node_region, reg_lo,
                  leaf_cls.data(), cls_size.data(), 0, classify, crec.data(), flags_gather, (int32_t*)nullptr, kNoGate);
}

// k_period_judge as ChainPass::periodic_walk launches it, `threads` wide
void emu_case_period_judge(int B, int s, int N, int NX, int OW, const int32_t* reg_off, const int32_t* reg_lo,
                           const int32_t* reg_hi, const int32_t* leaf_node, const uint8_t* alive, const int32_t* crec,
                           const int32_t* out, const int32_t* flags, const int32_t* cnt1, int32_t* cnt, int32_t* pb, int threads) {
    hipStream_t sm = nullptr;
    BLANCE_LAUNCH(k_period_judge, B, threads, 64, sm, B, s, N, NX, OW, reg_off, reg_lo, reg_hi, leaf_node, alive, crec, out, flags,
                  cnt1, cnt, pb);
}

// k_flat_stay_live over P partitions of one state (k = 1, NumPartitions == 0, no other candidate listed: a partition that
// holds exactly one live node is a certain stay, any other is not), as run_flat_pass launches it; the verdict goes to *moved
void emu_case_stay_live(int P, int N, int32_t* live, int32_t* live_len, uint8_t* live_kind, const int32_t* order, int32_t* moved) {
    DevProblem d{};
    d.N = N; d.NX = N; d.M = 1; d.L = 1; d.P = P; d.weights_nil = 1;
    d.live = live; d.live_len = live_len; d.live_kind = live_kind;
    std::vector<uint8_t> alive(N + 1, 1), has_w(N + 1, 0), has_stick(2, 0);
    std::vector<int32_t> node_w(N + 1, 0), cnt((size_t)2 * (N + 1), 0), tot(N + 1, 0), row_count(N + 2, 0), top_n(kTopList, INT_MAX), stick(2, 0);
    std::vector<double> g(N + 1, 0.0), top_g(kTopList, 0.0);
    FlatParams q{};
    q.N = N; q.NX = N; q.M = 1; q.L = 1; q.P = P; q.s = 0; q.k = 1; q.top_state = 0; q.NP = 0;
    q.alive = alive.data(); q.node_weight = node_w.data(); q.node_has_weight = has_w.data(); q.cnt = cnt.data(); q.tot = tot.data();
    q.g = g.data(); q.top_g = top_g.data(); q.top_n = top_n.data(); q.row_count = row_count.data();
    hipStream_t sm = nullptr;
    BLANCE_LAUNCH(k_flat_stay_live, cdiv(P, 256), 256, 0, sm, q, d, order, stick.data(), has_stick.data(), moved);
}

}  // extern "C"

// the bulk primitives one at a time (tests/test_kernel_cases_emulated.py): the same entries the device build runs
#include "../kernels/kernel_cases.inc"
// the sweep's record, list-edit and tail kernels (tests/test_sweep_cases_emulated.py)
#include "../kernels/sweep_cases.inc"
