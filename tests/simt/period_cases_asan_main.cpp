// TEST INFRASTRUCTURE ONLY: k_period_judge and k_period_replicate (blance_amd/csrc/k_period.h) under the SIMT emulator as a
// stand-alone program for AddressSanitizer and UBSan -- CPU only, nothing is loaded into another process:
//     g++ -std=c++17 -O1 -g1 -fsanitize=address,undefined -fno-omit-frame-pointer -x c++ period_cases_asan_main.cpp -o prog
//     prog <input>          (the file tests/period_kernel_cases.py: write_program_input makes)
// A case is a line of numbers and a line per array.  The arrays go through the entries of tests/kernels/period_cases.inc, which
// copy each into a heap block of exactly its size ("device" memory is the heap here): a read or a write outside is reported.
// One line per case: its letter, the entry's status, and every array that came back.  tests/test_period_cases_emulated.py
// builds and runs the program and compares the lines with the references.
#include "emu_lib.cpp"
#include "../kernels/period_cases.inc"

#include <fstream>
#include <iostream>

namespace {
template <class T> std::vector<T> numbers(std::istream& in, size_t n) {
    std::vector<T> v(n);
    for (size_t i = 0; i < n; i++) {
        long long x = 0;
        if (!(in >> x)) { fprintf(stderr, "the input ends inside an array\n"); exit(2); }
        v[i] = (T)x;
    }
    return v;
}
void print(const std::vector<int32_t>& v) {
    for (int32_t x : v) printf(" %d", x);
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s <input>\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::string kind;
    int cases = 0;
    while (in >> kind) {
        if (kind == "J") {
            int B, threads, s, n_states, N, NX, OW, n_steps, n_leaves;
            in >> B >> threads >> s >> n_states >> N >> NX >> OW >> n_steps >> n_leaves;
            if (!in || B < 1 || NX < 1 || n_states < 1 || OW < 1 || n_steps < 0 || n_leaves < 0) { fprintf(stderr, "a bad case line\n"); return 2; }
            auto reg_off = numbers<int32_t>(in, (size_t)B + 1), reg_lo = numbers<int32_t>(in, (size_t)B), reg_hi = numbers<int32_t>(in, (size_t)B);
            auto leaf_node = numbers<int32_t>(in, (size_t)n_leaves);
            auto alive = numbers<uint8_t>(in, (size_t)NX);
            auto crec = numbers<int32_t>(in, (size_t)n_steps * blance::kCW), out = numbers<int32_t>(in, (size_t)n_steps * OW + 1);
            auto flags = numbers<int32_t>(in, (size_t)blance::kChainFlags + 1);
            auto cnt1 = numbers<int32_t>(in, (size_t)n_states * NX + 1), cnt = numbers<int32_t>(in, (size_t)n_states * NX + 1);
            auto pb = numbers<int32_t>(in, (size_t)blance::kPWords * B + 1);
            leaf_node.reserve(1);
            crec.reserve(1);
            const int st = blance_case_period_judge(B, threads, s, n_states, N, NX, OW, n_steps, n_leaves, reg_off.data(), reg_lo.data(),
                                                    reg_hi.data(), leaf_node.data(), alive.data(), crec.data(), out.data(), flags.data(),
                                                    cnt1.data(), cnt.data(), pb.data());
            printf("J %d", st);
            print(cnt); print(pb); print(out); print(flags); print(cnt1);
            printf("\n");
        } else if (kind == "R") {
            int B, threads, OW, n_steps;
            in >> B >> threads >> OW >> n_steps;
            if (!in || B < 1 || OW < 1 || n_steps < 0) { fprintf(stderr, "a bad case line\n"); return 2; }
            auto reg_off = numbers<int32_t>(in, (size_t)B + 1), pb = numbers<int32_t>(in, (size_t)blance::kPWords * B + 1);
            auto out = numbers<int32_t>(in, (size_t)n_steps * OW + 1);
            const int st = blance_case_period_replicate(B, threads, OW, n_steps, reg_off.data(), pb.data(), out.data());
            printf("R %d", st);
            print(pb); print(out);
            printf("\n");
        } else {
            fprintf(stderr, "no such case: %s\n", kind.c_str());
            return 2;
        }
        cases++;
    }
    printf("ran %d cases\n", cases);
    return 0;
}
