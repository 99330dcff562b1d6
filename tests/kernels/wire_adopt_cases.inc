// TEST INFRASTRUCTURE ONLY: the two kernels of blance_wire_adopt alone (blance_amd/csrc/k_wire_adopt.h: k_wire_adopt_sum,
// k_wire_adopt_write) on a decoded document a test makes by hand.  Included behind the product's headers by two wrappers:
// tests/kernels/wire_adopt_cases.hip (hipcc, gfx950) and tests/simt/emu_wire_adopt_cases.cpp (the SIMT emulator, g++); the
// stand-alone sanitizer program tests/simt/wire_adopt_asan_main.cpp includes it too.  tests/wire_adopt_cases.py has the
// documents and the definition the results are compared with.
namespace {
constexpr int kWireAdoptCaseBadArg = -100, kWireAdoptCaseDevice = -101;
struct WireAdoptCaseBufs {                                   // device memory of one call, freed on every way out
    std::vector<void*> all;
    ~WireAdoptCaseBufs() { for (void* p : all) (void)hipFree(p); }
    // n elements on the device holding the host's n elements (the caller's poison included); exactly n, not one more
    template <class T> T* up(const T* host, size_t n) {
        void* p = nullptr;
        if (hipMalloc(&p, (n ? n : 1) * sizeof(T)) != hipSuccess) return nullptr;
        all.push_back(p);
        if (n && hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
        return (T*)p;
    }
};
template <class T> bool wire_adopt_case_down(T* host, const T* dev, size_t n) {
    return !n || hipMemcpy(host, dev, n * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess;
}
}  // namespace

// The decoded document: part_kind [P], off [P*M + 1], kind [P*M], nodes [off[P*M]]; the lists to assign the context holds:
// cur_a_off [P*M + 1], cur_a_kind [P*M]; k [M]; part_weight / part_has_weight [P].  Every output array comes in filled by the
// caller (poison) and goes back whole: res_io [16] (the caller presets it as the driver does), a_off / p_off [off_words >=
// P*M + 1], a_nodes / p_nodes [nodes_words >= the entries], a_kind / p_kind [kind_bytes >= P*M], in_prev / never
// [part_bytes >= P].  grid_sum / grid_write: workgroups (0: as the driver chooses).  Returns 0, or a negative code.
extern "C" int blance_case_wire_adopt(int P, int M, int L, int weights_nil, int assign_too, const int32_t* k, const uint8_t* part_kind,
                                      const int32_t* off, const uint8_t* kind, const int32_t* nodes, const int32_t* cur_a_off,
                                      const uint8_t* cur_a_kind, const int32_t* part_weight, const uint8_t* part_has_weight,
                                      int grid_sum, int grid_write, int32_t* res_io, int32_t* a_off, int32_t* p_off, int off_words,
                                      int32_t* a_nodes, int32_t* p_nodes, int nodes_words, uint8_t* a_kind, uint8_t* p_kind,
                                      int kind_bytes, uint8_t* in_prev, uint8_t* never, int part_bytes) {
    using namespace blance;
    if (P < 1 || M < 1 || M > kMaxStates || L < 1 || L > 59 || grid_sum < 0 || grid_sum > kWireAdoptMaxWgs || grid_write < 0 ||
        grid_write > kWireAdoptMaxWgs)
        return kWireAdoptCaseBadArg;
    const long long PM = (long long)P * M;
    if (!k || !part_kind || !off || !kind || !nodes || !cur_a_off || !cur_a_kind || !part_weight || !part_has_weight || !res_io ||
        !a_off || !p_off || !a_nodes || !p_nodes || !a_kind || !p_kind || !in_prev || !never)
        return kWireAdoptCaseBadArg;
    if (off[0] != 0) return kWireAdoptCaseBadArg;
    for (long long i = 0; i < PM; i++) if (off[i + 1] < off[i]) return kWireAdoptCaseBadArg;
    const long long total = off[PM];
    if (off_words < PM + 1 || kind_bytes < PM || part_bytes < P || nodes_words < total) return kWireAdoptCaseBadArg;
    WireAdoptCaseBufs b;
    WireAdoptParams q;
    memset(&q, 0, sizeof q);
    q.P = P; q.M = M; q.L = L; q.weights_nil = weights_nil; q.assign_too = assign_too;
    for (int m = 0; m < M; m++) q.k[m] = k[m];
    q.part_kind = b.up(part_kind, (size_t)P); q.off = b.up(off, (size_t)PM + 1); q.kind = b.up(kind, (size_t)PM);
    q.nodes = b.up(nodes, (size_t)total);
    q.cur_a_off = b.up(cur_a_off, (size_t)PM + 1); q.cur_a_kind = b.up(cur_a_kind, (size_t)PM);
    q.part_weight = b.up(part_weight, (size_t)P); q.part_has_weight = b.up(part_has_weight, (size_t)P);
    q.res = b.up(res_io, (size_t)kWireAdoptResWords);
    q.a_off = b.up(a_off, (size_t)off_words); q.p_off = b.up(p_off, (size_t)off_words);
    q.a_nodes = b.up(a_nodes, (size_t)nodes_words); q.p_nodes = b.up(p_nodes, (size_t)nodes_words);
    q.a_kind = b.up(a_kind, (size_t)kind_bytes); q.p_kind = b.up(p_kind, (size_t)kind_bytes);
    q.part_in_prev = b.up(in_prev, (size_t)part_bytes); q.part_never_equal = b.up(never, (size_t)part_bytes);
    if (!q.part_kind || !q.off || !q.kind || !q.nodes || !q.cur_a_off || !q.cur_a_kind || !q.part_weight || !q.part_has_weight ||
        !q.res || !q.a_off || !q.p_off || !q.a_nodes || !q.p_nodes || !q.a_kind || !q.p_kind || !q.part_in_prev || !q.part_never_equal)
        return kWireAdoptCaseDevice;
    hipStream_t sm = nullptr;
    const int wgs = (int)(((PM > P ? PM : P) + 255) / 256);
    BLANCE_LAUNCH(k_wire_adopt_sum, grid_sum ? grid_sum : (wgs < kWireAdoptMaxWgs ? wgs : kWireAdoptMaxWgs), 256,
                  4 * 9 * sizeof(unsigned long long), sm, q);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(sm) != hipSuccess) return kWireAdoptCaseDevice;
    BLANCE_LAUNCH_NOSYNC(k_wire_adopt_write, grid_write ? grid_write : wire_adopt_write_wgs(P, M, total), 256, 0, sm, q);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(sm) != hipSuccess) return kWireAdoptCaseDevice;
    if (!wire_adopt_case_down(res_io, q.res, (size_t)kWireAdoptResWords) || !wire_adopt_case_down(a_off, q.a_off, (size_t)off_words) ||
        !wire_adopt_case_down(p_off, q.p_off, (size_t)off_words) || !wire_adopt_case_down(a_nodes, q.a_nodes, (size_t)nodes_words) ||
        !wire_adopt_case_down(p_nodes, q.p_nodes, (size_t)nodes_words) || !wire_adopt_case_down(a_kind, q.a_kind, (size_t)kind_bytes) ||
        !wire_adopt_case_down(p_kind, q.p_kind, (size_t)kind_bytes) || !wire_adopt_case_down(in_prev, q.part_in_prev, (size_t)part_bytes) ||
        !wire_adopt_case_down(never, q.part_never_equal, (size_t)part_bytes))
        return kWireAdoptCaseDevice;
    return 0;
}
