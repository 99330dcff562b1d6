// TEST INFRASTRUCTURE ONLY: the kernel of blance_plan_batch_docs alone (blance_amd/csrc/k_batch_decode.h: k_batch_decode) on
// documents, dictionary blocks and packed input slices a test makes by hand.  Included behind the product's headers by two
// wrappers: tests/kernels/batch_decode_cases.hip (hipcc, gfx950) and tests/simt/emu_batch_decode_cases.cpp (the SIMT
// emulator, g++); the stand-alone sanitizer program tests/simt/batch_decode_asan_main.cpp includes it too.
// tests/batch_decode_cases.py has the cases and the definition the results are compared with.
namespace {
constexpr int kBatchDecodeCaseBadArg = -100, kBatchDecodeCaseDevice = -101;
constexpr int kBatchDecodeCaseShape = 12, kBatchDecodeCaseDoc = 11;
struct BatchDecodeCaseBufs {                                 // device memory of one call, freed on every way out
    std::vector<void*> all;
    ~BatchDecodeCaseBufs() { for (void* p : all) (void)hipFree(p); }
    // n elements on the device holding the host's n elements (the caller's poison included); exactly n, not one more
    template <class T> T* up(const T* host, size_t n) {
        void* p = nullptr;
        if (hipMalloc(&p, (n ? n : 1) * sizeof(T)) != hipSuccess) return nullptr;
        all.push_back(p);
        if (n && hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
        return (T*)p;
    }
};
template <class T> bool batch_decode_case_down(T* host, const T* dev, size_t n) {
    return !n || hipMemcpy(host, dev, n * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess;
}
}  // namespace

// nb problems, shape [nb][12] = P, M, NX, weights_nil, in_base, sc_base, i_state, i_part, i_alist, i_ahdr, i_plist, i_phdr
// (the words of BatchDesc the kernel reads; the row stride is kBatchMaxL); nd documents, ddesc [nd][11] = desc, len,
// doc_base, i_dict, assign_too, s_claim, s_pkind, s_kind, s_len, s_rec, rec_cap (BatchDocDesc).  in_io [in_words]: the state
// and partition words and the dictionary blocks at in_base + i_dict; sc_io [sc_words], sum_io [nd * 16]: whatever the caller
// filled them with; docs [doc_bytes]: every document at its base, padded to 16.  Every _io array goes back whole.  Every
// offset, the dictionary blocks' headers, offsets and ids are checked before anything is launched.  Returns 0, or a
// negative code.
extern "C" int blance_case_batch_decode(int nb, const int32_t* shape, int nd, const int32_t* ddesc, int32_t* in_io, long long in_words,
                                        int32_t* sc_io, long long sc_words, const unsigned char* docs, long long doc_bytes,
                                        int32_t* sum_io, int tile, int stage) {
    using namespace blance;
    if (nb < 1 || nd < 1 || !shape || !ddesc || !in_io || !sc_io || !docs || !sum_io || in_words < 0 || sc_words < 0 || doc_bytes < 0 ||
        tile < kWdTileMin || tile > kWdTileMax || (tile & 63) || stage < kWdStageMin || (stage & 15) ||
        (size_t)stage > 64 * 1024 - (size_t)kBatchDecodeLdsHead)
        return kBatchDecodeCaseBadArg;
    std::vector<BatchDesc> descs((size_t)nb);
    for (int i = 0; i < nb; i++) {
        const int32_t* s = shape + (size_t)i * kBatchDecodeCaseShape;
        BatchDesc& d = descs[(size_t)i];
        memset(&d, 0, sizeof d);
        d.P = s[0]; d.M = s[1]; d.NX = s[2]; d.weights_nil = s[3]; d.L = kBatchMaxL;
        d.in_base = s[4]; d.sc_base = s[5];
        d.i_state = s[6]; d.i_part = s[7]; d.i_alist = s[8]; d.i_ahdr = s[9]; d.i_plist = s[10]; d.i_phdr = s[11];
        if (d.P < 0 || d.P > kBatchMaxP || d.M < 0 || d.M > kMaxStates || d.NX < 0 || d.NX > kBatchMaxNX) return kBatchDecodeCaseBadArg;
        const long long PM = (long long)d.P * d.M;
        for (int k = 4; k < kBatchDecodeCaseShape; k++) if (s[k] < 0) return kBatchDecodeCaseBadArg;
        if (d.in_base + d.i_state + 4ll * d.M > in_words || d.in_base + d.i_part + 2ll * d.P > in_words ||
            d.in_base + d.i_alist + PM * kBatchMaxL > in_words || d.in_base + d.i_ahdr + PM > in_words ||
            d.in_base + d.i_plist + PM * kBatchMaxL > in_words || d.in_base + d.i_phdr + PM > in_words)
            return kBatchDecodeCaseBadArg;
    }
    std::vector<BatchDocDesc> dds((size_t)nd);
    for (int j = 0; j < nd; j++) {
        const int32_t* w = ddesc + (size_t)j * kBatchDecodeCaseDoc;
        BatchDocDesc& v = dds[(size_t)j];
        memset(&v, 0, sizeof v);
        v.desc = w[0]; v.len = w[1]; v.doc_base = w[2]; v.i_dict = w[3]; v.assign_too = w[4];
        v.s_claim = w[5]; v.s_pkind = w[6]; v.s_kind = w[7]; v.s_len = w[8]; v.s_rec = w[9]; v.rec_cap = w[10];
        if (v.desc < 0 || v.desc >= nb || v.len < 0 || v.doc_base < 0 || (v.doc_base & 15) || v.i_dict < 0) return kBatchDecodeCaseBadArg;
        if (v.doc_base + (((long long)v.len + 15) & ~15ll) > doc_bytes) return kBatchDecodeCaseBadArg;
        const BatchDesc& d = descs[(size_t)v.desc];
        const long long P = d.P, PM = (long long)d.P * d.M;
        if (v.s_claim < 0 || v.s_pkind < v.s_claim + P || v.s_kind < v.s_pkind + (P + 3) / 4 || v.s_len < v.s_kind + (PM + 3) / 4 ||
            v.s_rec < v.s_len + PM + 1 || v.rec_cap < (v.len + 1) / 2 + 1 || d.sc_base + v.s_rec + (long long)v.rec_cap > sc_words)
            return kBatchDecodeCaseBadArg;
        // the dictionary block: its header, the tables inside the slice, every id and offset inside its table
        const long long at = d.in_base + v.i_dict;
        if (at + kBatchDictHdr > in_words) return kBatchDecodeCaseBadArg;
        const int32_t* blk = in_io + at;
        const int want[3] = {d.P, d.NX, d.M};
        for (int k = 0; k < 3; k++) {
            const long long slots = blk[4 * k], mask = (uint32_t)blk[4 * k + 1], bytes = blk[4 * k + 2], off = blk[4 * k + 3];
            if (slots < kBatchDictHdr || bytes < kBatchDictHdr || off < kBatchDictHdr || (mask & (mask + 1)) || mask + 1 < 2ll * want[k] ||
                mask + 1 < 2 || at + slots + 2 * (mask + 1) > in_words || at + off + want[k] + 1 > in_words)
                return kBatchDecodeCaseBadArg;
            const int32_t* o = blk + off;
            if (o[0] != 0) return kBatchDecodeCaseBadArg;
            for (int x = 0; x < want[k]; x++) if (o[x + 1] < o[x]) return kBatchDecodeCaseBadArg;
            if (at + bytes + ((long long)o[want[k]] + 3) / 4 > in_words) return kBatchDecodeCaseBadArg;
            bool empty = false;
            for (long long x = 0; x <= mask; x++) {
                const int32_t id = blk[slots + 2 * x];
                if (id < -1 || id >= want[k]) return kBatchDecodeCaseBadArg;
                empty |= id < 0;
            }
            if (!empty) return kBatchDecodeCaseBadArg;       // (an empty slot ends every probe)
        }
    }
    BatchDecodeCaseBufs b;
    BatchDecodeParams q;
    memset(&q, 0, sizeof q);
    q.desc = b.up(descs.data(), (size_t)nb);
    q.ddesc = b.up(dds.data(), (size_t)nd);
    q.in = b.up(in_io, (size_t)in_words);
    q.sc = b.up(sc_io, (size_t)sc_words);
    q.docs = b.up(docs, (size_t)doc_bytes);
    q.sum = b.up(sum_io, (size_t)nd * kBdSumWords);
    q.tile = tile; q.stage = stage;
    if (!q.desc || !q.ddesc || !q.in || !q.sc || !q.docs || !q.sum) return kBatchDecodeCaseDevice;
    hipStream_t sm = nullptr;
    BLANCE_LAUNCH(k_batch_decode, nd, kBatchDecodeThreads, (size_t)kBatchDecodeLdsHead + (size_t)stage, sm, q);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(sm) != hipSuccess) return kBatchDecodeCaseDevice;
    if (!batch_decode_case_down(in_io, q.in, (size_t)in_words) || !batch_decode_case_down(sc_io, q.sc, (size_t)sc_words) ||
        !batch_decode_case_down(sum_io, q.sum, (size_t)nd * kBdSumWords))
        return kBatchDecodeCaseDevice;
    return 0;
}
