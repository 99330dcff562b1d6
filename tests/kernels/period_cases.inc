// TEST INFRASTRUCTURE ONLY: k_period_find (blance_amd/csrc/k_period.h) alone, on hand-made region tables and records, in its
// searched and its known mode.  Included behind the product's headers by two wrappers: tests/kernels/period_cases.hip (hipcc,
// gfx950) and tests/simt/emu_period_cases.cpp (the SIMT emulator, g++).  tests/period_case_tables.py has the cases.
namespace {
constexpr int kPeriodCaseBadArg = -100;
}  // namespace

extern "C" int blance_case_period_words(void) { return blance::kPWords; }

// pb[kPWords][B] comes in as the caller filled it and goes back as one launch of k_period_find left it.  Every index the
// kernel can form is checked first -- the chain offsets against n_steps, the leaf ranges against n_leaves, the nodes against
// NX -- and a table that fails is refused without a launch (kPeriodCaseBadArg); else the launch's own status (0: it ran).
extern "C" int blance_case_period_find(int B, int known, int threads, int N, int NX, int n_steps, int n_leaves, const int32_t* reg_off,
                                       const int32_t* reg_lo, const int32_t* reg_hi, const int32_t* leaf_node, const uint8_t* alive,
                                       const int32_t* crec, int32_t* pb) {
    if (B < 1 || B > 4096 || N < 0 || N > NX || NX < 1 || n_steps < 0 || n_leaves < 0 || !reg_off || !reg_lo || !reg_hi || !leaf_node ||
        !alive || !crec || !pb)
        return kPeriodCaseBadArg;
    if (threads != 64 && threads != 128 && threads != 256 && threads != 512 && threads != 1024) return kPeriodCaseBadArg;
    if (reg_off[0] < 0 || reg_off[B] > n_steps) return kPeriodCaseBadArg;
    for (int r = 0; r < B; r++) {
        if (reg_off[r + 1] < reg_off[r]) return kPeriodCaseBadArg;
        if (reg_lo[r] < 0 || reg_hi[r] < reg_lo[r] || reg_hi[r] > n_leaves) return kPeriodCaseBadArg;
    }
    for (int i = 0; i < n_leaves; i++)
        if (leaf_node[i] < -1 || leaf_node[i] >= NX) return kPeriodCaseBadArg;
    const size_t n_pb = (size_t)blance::kPWords * B, n_rec = (size_t)n_steps * blance::kCW;
    int32_t *d_off = nullptr, *d_lo = nullptr, *d_hi = nullptr, *d_leaf = nullptr, *d_rec = nullptr, *d_pb = nullptr;
    uint8_t* d_alive = nullptr;
    int st = (int)hipMalloc((void**)&d_off, sizeof(int32_t) * ((size_t)B + 1));
    if (!st) st = (int)hipMalloc((void**)&d_lo, sizeof(int32_t) * (size_t)B);
    if (!st) st = (int)hipMalloc((void**)&d_hi, sizeof(int32_t) * (size_t)B);
    if (!st) st = (int)hipMalloc((void**)&d_leaf, sizeof(int32_t) * ((size_t)n_leaves + 1));
    if (!st) st = (int)hipMalloc((void**)&d_alive, (size_t)NX);
    if (!st) st = (int)hipMalloc((void**)&d_rec, sizeof(int32_t) * (n_rec + 1));
    if (!st) st = (int)hipMalloc((void**)&d_pb, sizeof(int32_t) * n_pb);
    if (!st) st = (int)hipMemcpy(d_off, reg_off, sizeof(int32_t) * ((size_t)B + 1), hipMemcpyHostToDevice);
    if (!st) st = (int)hipMemcpy(d_lo, reg_lo, sizeof(int32_t) * (size_t)B, hipMemcpyHostToDevice);
    if (!st) st = (int)hipMemcpy(d_hi, reg_hi, sizeof(int32_t) * (size_t)B, hipMemcpyHostToDevice);
    if (!st && n_leaves > 0) st = (int)hipMemcpy(d_leaf, leaf_node, sizeof(int32_t) * (size_t)n_leaves, hipMemcpyHostToDevice);
    if (!st) st = (int)hipMemcpy(d_alive, alive, (size_t)NX, hipMemcpyHostToDevice);
    if (!st && n_rec > 0) st = (int)hipMemcpy(d_rec, crec, sizeof(int32_t) * n_rec, hipMemcpyHostToDevice);
    if (!st) st = (int)hipMemcpy(d_pb, pb, sizeof(int32_t) * n_pb, hipMemcpyHostToDevice);
    if (!st) {
        hipStream_t sm = nullptr;
        BLANCE_LAUNCH(blance::k_period_find, B, threads, 64, sm, B, known ? 1 : 0, N, d_off, d_lo, d_hi, d_leaf, d_alive, d_rec, d_pb);
        st = (int)hipGetLastError();
        if (!st) st = (int)hipStreamSynchronize(nullptr);
    }
    if (!st) st = (int)hipMemcpy(pb, d_pb, sizeof(int32_t) * n_pb, hipMemcpyDeviceToHost);
    for (void* p : {(void*)d_off, (void*)d_lo, (void*)d_hi, (void*)d_leaf, (void*)d_alive, (void*)d_rec, (void*)d_pb})
        if (p) (void)hipFree(p);
    return st;
}
