// TEST INFRASTRUCTURE ONLY: stage 1 of the device decoder alone (blance_amd/csrc/k_wire_decode.h: k_wd_tail, k_wd_quotes,
// k_wd_walk) on a document a test makes by hand.  Included behind the product's headers by two wrappers:
// tests/kernels/wire_decode_cases.hip (hipcc, gfx950) and tests/simt/emu_wire_decode_cases.cpp (the SIMT emulator, g++); the
// stand-alone sanitizer program tests/simt/wire_decode_asan_main.cpp includes it too.  tests/wire_decode_cases.py has the
// documents and the definition the results are compared with.
namespace {
constexpr int kWdCaseBadArg = -100, kWdCaseDevice = -101;
struct WdCaseBufs {                                          // device memory of one call, freed on every way out
    std::vector<void*> all;
    ~WdCaseBufs() { for (void* p : all) (void)hipFree(p); }
    template <class T> T* get(size_t n) {
        void* p = nullptr;
        if (hipMalloc(&p, (n ? n : 1) * sizeof(T)) != hipSuccess) return nullptr;
        all.push_back(p);
        return (T*)p;
    }
};
// arr[0 .. n] on the device: the exclusive scan of its first n entries (made on the host), the total behind them (a depth's
// total may be negative); false: a copy failed
bool wd_case_scan(int32_t* arr, int n, int32_t* counts_out, int32_t* total = nullptr) {
    std::vector<int32_t> h((size_t)n + 1);
    if (hipMemcpy(h.data(), arr, sizeof(int32_t) * ((size_t)n + 1), hipMemcpyDeviceToHost) != hipSuccess) return false;
    int32_t at = 0;
    for (int i = 0; i <= n; i++) {
        const int32_t v = h[(size_t)i];
        if (counts_out && i < n) counts_out[i] = v;
        h[(size_t)i] = at;
        at += v;
    }
    if (hipMemcpy(arr, h.data(), sizeof(int32_t) * ((size_t)n + 1), hipMemcpyHostToDevice) != hipSuccess) return false;
    if (total) *total = h[(size_t)n];
    return true;
}
}  // namespace

// The document's copy is len rounded up to 16 bytes and no more (k_wire_decode.h: kWdPad): under a sanitizer a read past it
// is reported.  qbits_out [n_tiles * tile / 32]: bit i & 31 of word i >> 5 -- byte i is an unescaped quote; quotes_out /
// depth_out [n_tiles]: the tile's unescaped quotes / its change of bracket depth outside strings; rec_out [rec_cap]: the record
// starts.  Returns their number (rec_out is written when they fit), or a negative code.
extern "C" int blance_case_wd_split(const unsigned char* doc, int len, int tile, uint32_t* qbits_out, int32_t* quotes_out,
                                    int32_t* depth_out, int32_t* rec_out, int rec_cap) {
    using namespace blance;
    if (len < 0 || (len && !doc) || tile < kWdTileMin || tile > kWdTileMax || (tile & 63) || rec_cap < 0) return kWdCaseBadArg;
    if (!qbits_out || !quotes_out || !depth_out || (rec_cap && !rec_out)) return kWdCaseBadArg;
    WireDecodeParams q;
    memset(&q, 0, sizeof q);
    q.len = len; q.tile = tile;
    q.n_tiles = (int)(((long long)len + tile - 1) / tile);
    if (q.n_tiles == 0) return 0;
    const size_t nt = (size_t)q.n_tiles, words = nt * (size_t)tile / 32;
    WdCaseBufs b;
    unsigned char* d_doc = b.get<unsigned char>(((size_t)len + kWdPad - 1) & ~(size_t)(kWdPad - 1));
    q.tb = b.get<int32_t>(nt); q.qbits = b.get<uint32_t>(words);
    q.quotes = b.get<int32_t>(nt + 1); q.depth = b.get<int32_t>(nt + 1); q.count = b.get<int32_t>(nt + 1);
    if (!d_doc || !q.tb || !q.qbits || !q.quotes || !q.depth || !q.count) return kWdCaseDevice;
    q.doc = d_doc;
    if (hipMemcpy(d_doc, doc, (size_t)len, hipMemcpyHostToDevice) != hipSuccess) return kWdCaseDevice;
    hipStream_t sm = nullptr;
    const int wgs = (q.n_tiles + 255) / 256;
    BLANCE_LAUNCH_NOSYNC(k_wd_tail, wgs, 256, 0, sm, q);
    BLANCE_LAUNCH_NOSYNC(k_wd_quotes, wgs, 256, 0, sm, q);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(sm) != hipSuccess) return kWdCaseDevice;
    if (hipMemcpy(qbits_out, q.qbits, sizeof(uint32_t) * words, hipMemcpyDeviceToHost) != hipSuccess) return kWdCaseDevice;
    if (!wd_case_scan(q.quotes, q.n_tiles, quotes_out)) return kWdCaseDevice;
    BLANCE_LAUNCH_NOSYNC(k_wd_walk<0>, wgs, 256, 0, sm, q);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(sm) != hipSuccess) return kWdCaseDevice;
    if (!wd_case_scan(q.depth, q.n_tiles, depth_out)) return kWdCaseDevice;
    BLANCE_LAUNCH_NOSYNC(k_wd_walk<1>, wgs, 256, 0, sm, q);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(sm) != hipSuccess) return kWdCaseDevice;
    int32_t R = 0;
    if (!wd_case_scan(q.count, q.n_tiles, nullptr, &R) || R < 0 || R > len) return kWdCaseDevice;
    if (R == 0 || R > rec_cap) return R;
    q.rec = b.get<int32_t>((size_t)R);
    if (!q.rec) return kWdCaseDevice;
    BLANCE_LAUNCH_NOSYNC(k_wd_walk<2>, wgs, 256, 0, sm, q);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(sm) != hipSuccess) return kWdCaseDevice;
    if (hipMemcpy(rec_out, q.rec, sizeof(int32_t) * (size_t)R, hipMemcpyDeviceToHost) != hipSuccess) return kWdCaseDevice;
    return R;
}
