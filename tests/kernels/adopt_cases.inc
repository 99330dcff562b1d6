// TEST INFRASTRUCTURE ONLY: the two kernels of blance_plan_adopt alone (blance_amd/csrc/k_adopt.h: k_adopt_len, k_adopt_write)
// on a planned map a test makes by hand.  Included behind the product's headers by two wrappers:
// tests/kernels/adopt_cases.hip (hipcc, gfx950) and tests/simt/emu_adopt_cases.cpp (the SIMT emulator, g++); the stand-alone
// sanitizer program tests/simt/adopt_asan_main.cpp includes it too.  tests/adopt_cases.py has the maps and the definition
// the results are compared with.
namespace {
constexpr int kAdoptCaseBadArg = -100, kAdoptCaseDevice = -101;
struct AdoptCaseBufs {                                       // device memory of one call, freed on every way out
    std::vector<void*> all;
    ~AdoptCaseBufs() { for (void* p : all) (void)hipFree(p); }
    // n elements on the device holding the host's n elements (the caller's poison included); exactly n, not one more
    template <class T> T* up(const T* host, size_t n) {
        void* p = nullptr;
        if (hipMalloc(&p, (n ? n : 1) * sizeof(T)) != hipSuccess) return nullptr;
        all.push_back(p);
        if (n && hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
        return (T*)p;
    }
};
template <class T> bool adopt_case_down(T* host, const T* dev, size_t n) {
    return !n || hipMemcpy(host, dev, n * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess;
}
}  // namespace

// The planned map: prv [P*M*L], prv_len / prv_kind [P*M]; k [M]; part_weight / part_has_weight [P].  Every output array comes
// in filled by the caller (poison) and goes back whole: len_io [len_words >= P*M + 1] the lengths as k_adopt_len left them
// (len_scanned_io, same size: after the scan, made on the host here), res_io [16], a_off / p_off [off_words >= P*M + 1],
// a_nodes / p_nodes [nodes_words >= the entries], a_kind / p_kind [kind_bytes >= P*M], in_prev / never [part_bytes >= P].
// grid_len: workgroups of k_adopt_len (0: as the driver chooses).  Returns the entries, or a negative code.
extern "C" int blance_case_adopt(int P, int M, int L, int weights_nil, const int32_t* k, const int32_t* prv, const int32_t* prv_len,
                                 const uint8_t* prv_kind, const int32_t* part_weight, const uint8_t* part_has_weight, int grid_len,
                                 int32_t* len_io, int32_t* len_scanned_io, int len_words, int32_t* res_io, int32_t* a_off,
                                 int32_t* p_off, int off_words, int32_t* a_nodes, int32_t* p_nodes, int nodes_words, uint8_t* a_kind,
                                 uint8_t* p_kind, int kind_bytes, uint8_t* in_prev, uint8_t* never, int part_bytes) {
    using namespace blance;
    if (P < 1 || M < 1 || M > kMaxStates || L < 1 || L > 59 || grid_len < 0 || grid_len > kAdoptMaxWgs) return kAdoptCaseBadArg;
    const long long PM = (long long)P * M;
    if (len_words < PM + 1 || off_words < PM + 1 || kind_bytes < PM || part_bytes < P || nodes_words < 0) return kAdoptCaseBadArg;
    if (!k || !prv || !prv_len || !prv_kind || !part_weight || !part_has_weight || !len_io || !len_scanned_io || !res_io || !a_off ||
        !p_off || !a_nodes || !p_nodes || !a_kind || !p_kind || !in_prev || !never)
        return kAdoptCaseBadArg;
    AdoptCaseBufs b;
    AdoptParams q;
    memset(&q, 0, sizeof q);
    q.P = P; q.M = M; q.L = L; q.weights_nil = weights_nil;
    for (int m = 0; m < M; m++) q.k[m] = k[m];
    q.prv = b.up(prv, (size_t)PM * L); q.prv_len = b.up(prv_len, (size_t)PM); q.prv_kind = b.up(prv_kind, (size_t)PM);
    q.part_weight = b.up(part_weight, (size_t)P); q.part_has_weight = b.up(part_has_weight, (size_t)P);
    q.len = b.up(len_io, (size_t)len_words);
    q.res = b.up(res_io, (size_t)kAdoptResWords);
    if (!q.prv || !q.prv_len || !q.prv_kind || !q.part_weight || !q.part_has_weight || !q.len || !q.res) return kAdoptCaseDevice;
    hipStream_t sm = nullptr;
    const int wgs = (int)((PM + 1 + 255) / 256);
    BLANCE_LAUNCH(k_adopt_len, grid_len ? grid_len : (wgs < kAdoptMaxWgs ? wgs : kAdoptMaxWgs), 256, 4 * 5 * sizeof(unsigned long long), sm, q);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(sm) != hipSuccess) return kAdoptCaseDevice;
    if (!adopt_case_down(len_io, q.len, (size_t)len_words) || !adopt_case_down(res_io, q.res, (size_t)kAdoptResWords)) return kAdoptCaseDevice;
    // the exclusive scan of launch_scan_excl, on the host: len[i] for i <= P*M, the rest as it came
    for (int i = 0; i < len_words; i++) len_scanned_io[i] = len_io[i];
    long long at = 0;
    for (long long i = 0; i <= PM; i++) { const int32_t v = len_io[i]; len_scanned_io[i] = (int32_t)at; at += v; }
    if (at > nodes_words) return kAdoptCaseBadArg;
    if (hipMemcpy(q.len, len_scanned_io, sizeof(int32_t) * (size_t)len_words, hipMemcpyHostToDevice) != hipSuccess) return kAdoptCaseDevice;
    q.a_off = b.up(a_off, (size_t)off_words); q.p_off = b.up(p_off, (size_t)off_words);
    q.a_nodes = b.up(a_nodes, (size_t)nodes_words); q.p_nodes = b.up(p_nodes, (size_t)nodes_words);
    q.a_kind = b.up(a_kind, (size_t)kind_bytes); q.p_kind = b.up(p_kind, (size_t)kind_bytes);
    q.part_in_prev = b.up(in_prev, (size_t)part_bytes); q.part_never_equal = b.up(never, (size_t)part_bytes);
    if (!q.a_off || !q.p_off || !q.a_nodes || !q.p_nodes || !q.a_kind || !q.p_kind || !q.part_in_prev || !q.part_never_equal)
        return kAdoptCaseDevice;
    BLANCE_LAUNCH(k_adopt_write, (int)((PM + kAdoptLists - 1) / kAdoptLists), kAdoptLists, adopt_write_lds(L), sm, q);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(sm) != hipSuccess) return kAdoptCaseDevice;
    if (!adopt_case_down(len_scanned_io, q.len, (size_t)len_words) || !adopt_case_down(a_off, q.a_off, (size_t)off_words) ||
        !adopt_case_down(p_off, q.p_off, (size_t)off_words) || !adopt_case_down(a_nodes, q.a_nodes, (size_t)nodes_words) ||
        !adopt_case_down(p_nodes, q.p_nodes, (size_t)nodes_words) || !adopt_case_down(a_kind, q.a_kind, (size_t)kind_bytes) ||
        !adopt_case_down(p_kind, q.p_kind, (size_t)kind_bytes) || !adopt_case_down(in_prev, q.part_in_prev, (size_t)part_bytes) ||
        !adopt_case_down(never, q.part_never_equal, (size_t)part_bytes))
        return kAdoptCaseDevice;
    return (int)at;
}
