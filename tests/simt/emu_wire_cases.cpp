// TEST INFRASTRUCTURE ONLY: k_wire_size and k_wire_write under the SIMT emulator on lists a test makes by hand -- for the
// nil list (`null`), which no plan was found to produce (see tests/test_plan_wire_kernels_emulated.py).  The library is
// emu_lib.cpp's plus this entry.
#include "emu_lib.cpp"
#include <vector>

extern "C" {

// The document of P partitions whose names are already in byte order (rank = partition id), states in name order (place =
// state id); every string comes escaped (quotes included, a state's with its colon), as blance_plan_wire_names leaves them.
// Sizing pass, an exclusive scan on the host, writing pass with an LDS stage of `stage` bytes.  Returns the length;
// doc (16-byte aligned, `cap` bytes) is written when the length fits.
long long emu_case_wire(int P, int M, int L, int NX, const char* part_esc, const int32_t* part_off, const char* node_esc,
                        const int32_t* node_off, const char* state_esc, const int32_t* state_off, const int32_t* lists,
                        const int32_t* list_len, const uint8_t* list_kind, int stage, char* doc, long long cap) {
    std::vector<int32_t> order(P + 1), state_id(M + 1), len(P + 2, 0);
    for (int p = 0; p < P; p++) order[p] = p;
    for (int m = 0; m < M; m++) state_id[m] = m;
    unsigned long long total = 0;
    PlanWireParams q{};
    q.P = P; q.M = M; q.L = L; q.NX = NX;
    q.order = order.data();
    q.part_esc = part_esc; q.part_off = part_off;
    q.node_esc = node_esc; q.node_off = node_off;
    q.state_esc = state_esc; q.state_off = state_off; q.state_id = state_id.data();
    q.lists = lists; q.list_len = list_len; q.list_kind = list_kind;
    q.len = len.data(); q.total = &total; q.doc = doc; q.stage = stage;
    hipStream_t sm = nullptr;
    const size_t lds1 = (((size_t)NX * 4 + 15) & ~(size_t)15) + sizeof(unsigned long long) * 256;
    BLANCE_LAUNCH(k_wire_size, cdiv((int64_t)P + 1, 256), 256, lds1, sm, q);
    int32_t at = 0;
    for (int r = 0; r <= P; r++) { const int32_t n = len[r]; len[r] = at; at += n; }
    if ((unsigned long long)at != total) return -1;
    if ((long long)total <= cap) BLANCE_LAUNCH(k_wire_write, cdiv(P, kWireRun), kWireRun, (size_t)stage, sm, q);
    return (long long)total;
}

}  // extern "C"
