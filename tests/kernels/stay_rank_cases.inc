// TEST INFRASTRUCTURE ONLY: k_stay_by_top's rank function (stay_round_ranks, blance_amd/csrc/k_stay.h) alone, on one wave.
// Included behind the product's headers by two wrappers: tests/kernels/stay_rank_cases.hip (hipcc, gfx950) and
// tests/simt/emu_stay_rank_cases.cpp (the SIMT emulator, g++).  tests/stay_rank_tables.py has the cases and the reference.
namespace {
constexpr int kRankCaseBadArg = -100;
constexpr int kRankCaseMaxRounds = 4096;

// One wave, a round after the other: lane l of round r holds leaves[(r * 64 + l) * KM ..] (-1: no such node) and writes its
// ranks to the same place of `ranks`.  Every lane stays to the end (the function's ballots).
template <int KM>
__global__ __launch_bounds__(64) void k_case_stay_ranks(const int32_t* leaves, int32_t* ranks, int size, int rounds) {
    const int lane = threadIdx.x & 63;
    const int nbits = blance::stay_leaf_bits(size);
    for (int r = 0; r < rounds; r++) {
        int oi[KM], rk[KM];
#pragma unroll
        for (int j = 0; j < KM; j++) oi[j] = leaves[((size_t)r * 64 + lane) * KM + j];
        blance::stay_round_ranks<KM>(oi, nbits, rk);
#pragma unroll
        for (int j = 0; j < KM; j++) ranks[((size_t)r * 64 + lane) * KM + j] = rk[j];
    }
}
}  // namespace

// ranks[rounds][64][km] of leaves[rounds][64][km] in a region of `size` leaves.  A leaf outside [-1, size) is refused
// without a launch (kRankCaseBadArg); else the launch's own status (0: it ran).
extern "C" int blance_case_stay_ranks(int km, int size, int rounds, const int32_t* leaves, int32_t* ranks) {
    if ((km != 2 && km != 4) || size < 1 || size > blance::kStayMaxLeaves || rounds < 1 || rounds > kRankCaseMaxRounds || !leaves || !ranks)
        return kRankCaseBadArg;
    const size_t n = (size_t)rounds * 64 * km;
    for (size_t i = 0; i < n; i++)
        if (leaves[i] < -1 || leaves[i] >= size) return kRankCaseBadArg;
    int32_t *d_in = nullptr, *d_out = nullptr;
    int st = (int)hipMalloc((void**)&d_in, sizeof(int32_t) * n);
    if (!st) st = (int)hipMalloc((void**)&d_out, sizeof(int32_t) * n);
    if (!st) st = (int)hipMemcpy(d_in, leaves, sizeof(int32_t) * n, hipMemcpyHostToDevice);
    if (!st) st = (int)hipMemsetAsync(d_out, 0x5a, sizeof(int32_t) * n, nullptr);
    if (!st) {
        hipStream_t sm = nullptr;
        if (km == 2) { auto kern = k_case_stay_ranks<2>; BLANCE_LAUNCH(kern, 1, 64, 0, sm, d_in, d_out, size, rounds); }
        else { auto kern = k_case_stay_ranks<4>; BLANCE_LAUNCH(kern, 1, 64, 0, sm, d_in, d_out, size, rounds); }
        st = (int)hipGetLastError();
        if (!st) st = (int)hipStreamSynchronize(nullptr);
    }
    if (!st) st = (int)hipMemcpy(ranks, d_out, sizeof(int32_t) * n, hipMemcpyDeviceToHost);
    if (d_in) (void)hipFree(d_in);
    if (d_out) (void)hipFree(d_out);
    return st;
}
