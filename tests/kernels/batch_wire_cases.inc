// TEST INFRASTRUCTURE ONLY: the two kernels of blance_plan_batch_wire alone (blance_amd/csrc/k_batch_wire.h: k_batch_wire_size,
// k_batch_wire_write) on result CSRs and names blocks a test makes by hand.  Included behind the product's headers by two
// wrappers: tests/kernels/batch_wire_cases.hip (hipcc, gfx950) and tests/simt/emu_batch_wire_cases.cpp (the SIMT emulator,
// g++); the stand-alone sanitizer program tests/simt/batch_wire_asan_main.cpp includes it too.  tests/batch_wire_cases.py has
// the cases and the definition the results are compared with.
namespace {
constexpr int kBatchWireCaseBadArg = -100, kBatchWireCaseDevice = -101;
constexpr int kBatchWireCaseShape = 9;                       // ints of one problem: see blance_case_batch_wire
struct BatchWireCaseBufs {                                   // device memory of one call, freed on every way out
    std::vector<void*> all;
    ~BatchWireCaseBufs() { for (void* p : all) (void)hipFree(p); }
    // n elements on the device holding the host's n elements (the caller's poison included); exactly n, not one more
    template <class T> T* up(const T* host, size_t n) {
        void* p = nullptr;
        if (hipMalloc(&p, (n ? n : 1) * sizeof(T)) != hipSuccess) return nullptr;
        all.push_back(p);
        if (n && hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
        return (T*)p;
    }
};
template <class T> bool batch_wire_case_down(T* host, const T* dev, size_t n) {
    return !n || hipMemcpy(host, dev, n * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess;
}
}  // namespace

// nb problems, shape [nb][9] = P, M, NX, in_base, sc_base, out_base, o_off, o_kind, o_nodes (the words of BatchDesc the two
// kernels read); nw requests, wdesc [nw][4] = desc, i_names, s_len, o_total (BatchWireDesc).  in [in_words]: the names blocks
// at in_base + i_names; out_io [out_words]: every problem's header and result CSR; sc_io [sc_words], total_io [nw], doc_io
// [doc_bytes]: whatever the caller filled them with.  which: 1 = k_batch_wire_size, 2 = k_batch_wire_write (on the sc_io /
// total_io / out_io the caller gives), 3 = both.  Every _io array goes back whole.  Returns 0, or a negative code.
extern "C" int blance_case_batch_wire(int nb, const int32_t* shape, int nw, const int32_t* wdesc, const int32_t* in, long long in_words,
                                      int32_t* sc_io, long long sc_words, int32_t* out_io, long long out_words, int32_t* total_io,
                                      char* doc_io, long long doc_bytes, int stage, int which) {
    using namespace blance;
    if (nb < 1 || nw < 1 || !shape || !wdesc || !in || !sc_io || !out_io || !total_io || !doc_io || in_words < 0 || sc_words < 0 ||
        out_words < 0 || doc_bytes < 0 || stage < 64 || (size_t)stage > 64 * 1024 - kBatchWireRedLds || which < 1 || which > 3)
        return kBatchWireCaseBadArg;
    std::vector<BatchDesc> descs((size_t)nb);
    for (int i = 0; i < nb; i++) {
        const int32_t* s = shape + (size_t)i * kBatchWireCaseShape;
        BatchDesc& d = descs[(size_t)i];
        memset(&d, 0, sizeof d);
        d.P = s[0]; d.M = s[1]; d.NX = s[2];
        d.in_base = s[3]; d.sc_base = s[4]; d.out_base = s[5];
        d.o_off = s[6]; d.o_kind = s[7]; d.o_nodes = s[8];
        if (d.P < 1 || d.P > kBatchMaxP || d.M < 1 || d.M > kMaxStates || d.NX < 1 || d.NX > kBatchMaxNX) return kBatchWireCaseBadArg;
        if (s[3] < 0 || s[4] < 0 || s[5] < 0 || s[6] < kBatchHdr || s[7] < kBatchHdr || s[8] < kBatchHdr) return kBatchWireCaseBadArg;
        const long long PM = (long long)d.P * d.M;
        if (s[5] + s[6] + PM + 1 > out_words || s[5] + s[7] + PM > out_words) return kBatchWireCaseBadArg;
        const int32_t* off = out_io + s[5] + s[6];
        for (long long k = 0; k < PM; k++) if (off[k] < 0 || off[k + 1] < off[k]) return kBatchWireCaseBadArg;
        if (s[5] + s[8] + (long long)off[PM] > out_words) return kBatchWireCaseBadArg;
        const int32_t* nodes = out_io + s[5] + s[8];
        for (long long k = 0; k < off[PM]; k++) if (nodes[k] < 0 || nodes[k] >= d.NX) return kBatchWireCaseBadArg;
    }
    std::vector<BatchWireDesc> wds((size_t)nw);
    for (int j = 0; j < nw; j++) {
        const int32_t* w = wdesc + (size_t)j * 4;
        BatchWireDesc& v = wds[(size_t)j];
        v.desc = w[0]; v.i_names = w[1]; v.s_len = w[2]; v.o_total = w[3];
        if (v.desc < 0 || v.desc >= nb || v.i_names < 0 || v.s_len < 0 || v.o_total < kBatchHdr) return kBatchWireCaseBadArg;
        const BatchDesc& d = descs[(size_t)v.desc];
        if (d.in_base + v.i_names + kBatchNamesHdr > in_words || d.sc_base + v.s_len + d.P + 1 > sc_words ||
            d.out_base + v.o_total + 1 > out_words)
            return kBatchWireCaseBadArg;
        const int32_t* hdr = in + d.in_base + v.i_names;     // the eight tables begin inside the block
        for (int k = 0; k < kBatchNamesHdr; k++)
            if (hdr[k] < kBatchNamesHdr || d.in_base + v.i_names + hdr[k] > in_words) return kBatchWireCaseBadArg;
    }
    BatchWireCaseBufs b;
    BatchWireParams q;
    memset(&q, 0, sizeof q);
    q.desc = b.up(descs.data(), (size_t)nb);
    q.wdesc = b.up(wds.data(), (size_t)nw);
    q.in = b.up(in, (size_t)in_words);
    q.sc = b.up(sc_io, (size_t)sc_words);
    q.out = b.up(out_io, (size_t)out_words);
    q.wire_total = b.up(total_io, (size_t)nw);
    q.doc = b.up(doc_io, (size_t)doc_bytes);
    q.stage = stage;
    if (!q.desc || !q.wdesc || !q.in || !q.sc || !q.out || !q.wire_total || !q.doc) return kBatchWireCaseDevice;
    hipStream_t sm = nullptr;
    if (which & 1) {
        BLANCE_LAUNCH(k_batch_wire_size, nw, kBatchWireThreads, kBatchWireSizeLds, sm, q);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(sm) != hipSuccess) return kBatchWireCaseDevice;
    }
    if (which & 2) {                                         // (never a write outside doc: the bases are the sums of these words)
        std::vector<int32_t> tot((size_t)nw);
        if (!batch_wire_case_down(tot.data(), q.wire_total, (size_t)nw)) return kBatchWireCaseDevice;
        long long sum = 0;
        for (int j = 0; j < nw; j++) {
            if (tot[(size_t)j] < 0 || (tot[(size_t)j] & 15)) return kBatchWireCaseBadArg;
            sum += tot[(size_t)j];
        }
        if (sum > doc_bytes) return kBatchWireCaseBadArg;
        BLANCE_LAUNCH(k_batch_wire_write, nw, kBatchWireThreads, kBatchWireRedLds + (size_t)stage, sm, q);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(sm) != hipSuccess) return kBatchWireCaseDevice;
    }
    if (!batch_wire_case_down(sc_io, q.sc, (size_t)sc_words) || !batch_wire_case_down(out_io, q.out, (size_t)out_words) ||
        !batch_wire_case_down(total_io, q.wire_total, (size_t)nw) || !batch_wire_case_down(doc_io, q.doc, (size_t)doc_bytes))
        return kBatchWireCaseDevice;
    return 0;
}
