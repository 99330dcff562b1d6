// TEST INFRASTRUCTURE ONLY: the two kernels of blance_plan_adopt (blance_amd/csrc/k_adopt.h) under the SIMT emulator as a
// stand-alone program for AddressSanitizer and UBSan -- CPU only, nothing is loaded into another process:
//     g++ -std=c++17 -O1 -g1 -fsanitize=address,undefined -fno-omit-frame-pointer -x c++ adopt_asan_main.cpp -o prog
//     prog <input>          (the file tests/adopt_cases.py: write_program_input makes)
// Every case runs through blance_case_adopt with every buffer of exactly the size AdoptParams documents -- "device" memory
// is the heap here, so a read or a write one word outside is reported -- and is compared with the numbers the definition
// gave (tests/adopt_cases.py: kernel_reference).  tests/test_adopt_emulated.py builds and runs it.
#include "emu_lib.cpp"
#include "../kernels/adopt_cases.inc"

#include <fstream>
#include <iostream>
#include <sstream>

namespace {
struct Case {
    int P = 0, M = 0, L = 0, weights_nil = 0;
    long long total = 0;
    std::vector<long long> k, prv, prv_len, prv_kind, part_weight, part_has_weight, want, off, nodes;
};
template <class T> std::vector<T> as(const std::vector<long long>& v) {
    std::vector<T> out(v.size());
    for (size_t i = 0; i < v.size(); i++) out[i] = (T)v[i];
    return out;
}
bool run(const Case& c) {
    const size_t PM = (size_t)c.P * c.M, total = (size_t)c.total;
    const auto k = as<int32_t>(c.k), prv = as<int32_t>(c.prv), prv_len = as<int32_t>(c.prv_len), pw = as<int32_t>(c.part_weight);
    const auto kind = as<uint8_t>(c.prv_kind), has = as<uint8_t>(c.part_has_weight);
    // exact sizes: P*M + 1 offsets, `total` entries (one word where there are none: the entry never writes it), P*M kinds, P flags
    std::vector<int32_t> len(PM + 1, -1), scanned(PM + 1, -1), res(16, 0), a_off(PM + 1, -1), p_off(PM + 1, -1);
    std::vector<int32_t> a_nodes(total ? total : 1, -1), p_nodes(total ? total : 1, -1);
    std::vector<uint8_t> a_kind(PM, 9), p_kind(PM, 9), in_prev((size_t)c.P, 9), never((size_t)c.P, 9);
    const int st = blance_case_adopt(c.P, c.M, c.L, c.weights_nil, k.data(), prv.data(), prv_len.data(), kind.data(), pw.data(), has.data(),
                                     0, len.data(), scanned.data(), (int)PM + 1, res.data(), a_off.data(), p_off.data(), (int)PM + 1,
                                     a_nodes.data(), p_nodes.data(), (int)total, a_kind.data(), p_kind.data(), (int)PM, in_prev.data(),
                                     never.data(), c.P);
    if (st != (int)c.total) return false;
    long long r64[5];
    memcpy(r64, res.data() + 4, sizeof r64);
    bool ok = res[1] == (int32_t)c.want[0] && (uint32_t)res[10] == (uint32_t)c.want[1] && r64[0] == c.want[2] && r64[2] == c.want[3] &&
              r64[4] == c.total;
    for (size_t i = 0; i <= PM; i++) ok = ok && a_off[i] == (int32_t)c.off[i] && p_off[i] == (int32_t)c.off[i];
    for (size_t i = 0; i < total; i++) ok = ok && a_nodes[i] == (int32_t)c.nodes[i] && p_nodes[i] == (int32_t)c.nodes[i];
    for (size_t i = 0; i < PM; i++) ok = ok && a_kind[i] == kind[i] && p_kind[i] == kind[i];
    for (int p = 0; p < c.P; p++) ok = ok && in_prev[(size_t)p] == 1 && never[(size_t)p] == 0;
    return ok;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s <input>\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::vector<Case> cases;
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string tag;
        ss >> tag;
        if (tag == "C") {
            Case c;
            ss >> c.P >> c.M >> c.L >> c.weights_nil >> c.total;
            cases.push_back(c);
            continue;
        }
        if (cases.empty()) continue;
        Case& c = cases.back();
        std::vector<long long>* dst = tag == "k" ? &c.k : tag == "prv" ? &c.prv : tag == "prv_len" ? &c.prv_len : tag == "prv_kind" ? &c.prv_kind :
                                      tag == "part_weight" ? &c.part_weight : tag == "part_has_weight" ? &c.part_has_weight :
                                      tag == "want" ? &c.want : tag == "off" ? &c.off : tag == "nodes" ? &c.nodes : nullptr;
        long long v;
        while (dst && ss >> v) dst->push_back(v);
    }
    int wrong = 0;
    for (size_t i = 0; i < cases.size(); i++) {
        const Case& c = cases[i];
        const size_t PM = (size_t)c.P * c.M;
        if (c.k.size() != (size_t)c.M || c.prv.size() != PM * c.L || c.prv_len.size() != PM || c.prv_kind.size() != PM ||
            c.part_weight.size() != (size_t)c.P || c.part_has_weight.size() != (size_t)c.P || c.want.size() != 4 || c.off.size() != PM + 1 ||
            c.nodes.size() != (size_t)c.total) {
            fprintf(stderr, "case %zu: malformed input\n", i);
            return 2;
        }
        if (!run(c)) { wrong++; fprintf(stderr, "case %zu (P %d, M %d, L %d): differs from the definition\n", i, c.P, c.M, c.L); }
    }
    printf("ran %zu cases, %d wrong\n", cases.size(), wrong);
    return wrong ? 1 : 0;
}
