// TEST INFRASTRUCTURE ONLY: the two kernels of blance_wire_adopt (blance_amd/csrc/k_wire_adopt.h) under the SIMT emulator as a
// stand-alone program for AddressSanitizer and UBSan -- CPU only, nothing is loaded into another process:
//     g++ -std=c++17 -O1 -g1 -fsanitize=address,undefined -fno-omit-frame-pointer -x c++ wire_adopt_asan_main.cpp -o prog
//     prog <input>          (the file tests/wire_adopt_cases.py: write_program_input makes)
// Every case runs through blance_case_wire_adopt with every buffer of exactly the size WireAdoptParams documents -- "device"
// memory is the heap here, so a read or a write one byte outside is reported -- and is compared with the numbers the
// definition gave (tests/wire_adopt_cases.py: kernel_reference).  tests/test_wire_adopt_emulated.py builds and runs it.
#include "emu_lib.cpp"
#include "../kernels/wire_adopt_cases.inc"

#include <fstream>
#include <iostream>
#include <sstream>

namespace {
struct Case {
    int P = 0, M = 0, L = 0, weights_nil = 0, assign_too = 0;
    std::vector<long long> k, part_kind, off, kind, nodes, cur_a_off, cur_a_kind, part_weight, part_has_weight, want;
};
template <class T> std::vector<T> as(const std::vector<long long>& v, size_t at_least = 0) {
    std::vector<T> out(v.size() > at_least ? v.size() : at_least);
    for (size_t i = 0; i < v.size(); i++) out[i] = (T)v[i];
    return out;
}
bool run(const Case& c) {
    const size_t PM = (size_t)c.P * c.M, total = (size_t)c.off[PM];
    const auto k = as<int32_t>(c.k), off = as<int32_t>(c.off), nodes = as<int32_t>(c.nodes, 1), cur_off = as<int32_t>(c.cur_a_off),
               pw = as<int32_t>(c.part_weight);
    const auto part_kind = as<uint8_t>(c.part_kind), kind = as<uint8_t>(c.kind), cur_kind = as<uint8_t>(c.cur_a_kind),
               has = as<uint8_t>(c.part_has_weight);
    // exact sizes: P*M + 1 offsets, `total` entries (one word where there are none: never written), P*M kinds, P flags
    std::vector<int32_t> res(16, 0), a_off(PM + 1, -1), p_off(PM + 1, -1), a_nodes(total ? total : 1, -1), p_nodes(total ? total : 1, -1);
    std::vector<uint8_t> a_kind(PM, 9), p_kind(PM, 9), in_prev((size_t)c.P, 9), never((size_t)c.P, 9);
    res[0] = res[3] = res[11] = INT_MAX;
    const int st = blance_case_wire_adopt(c.P, c.M, c.L, c.weights_nil, c.assign_too, k.data(), part_kind.data(), off.data(), kind.data(),
                                          nodes.data(), cur_off.data(), cur_kind.data(), pw.data(), has.data(), 0, 0, res.data(),
                                          a_off.data(), p_off.data(), (int)PM + 1, a_nodes.data(), p_nodes.data(), (int)total,
                                          a_kind.data(), p_kind.data(), (int)PM, in_prev.data(), never.data(), c.P);
    if (st != 0) return false;
    long long r64[5];
    memcpy(r64, res.data() + 4, sizeof r64);
    // want: first_long longest fresh first_missing kinds first_dup cap aprev total
    bool ok = res[0] == (int32_t)c.want[0] && res[1] == (int32_t)c.want[1] && res[2] == (int32_t)c.want[2] && res[3] == (int32_t)c.want[3] &&
              (uint32_t)res[10] == (uint32_t)c.want[4] && res[11] == (int32_t)c.want[5] && r64[0] == c.want[6] && r64[2] == c.want[7] &&
              r64[4] == c.want[8];
    for (size_t i = 0; i <= PM; i++) ok = ok && p_off[i] == off[i] && a_off[i] == (c.assign_too ? off[i] : -1);
    for (size_t i = 0; i < total; i++) ok = ok && p_nodes[i] == nodes[i] && a_nodes[i] == (c.assign_too ? nodes[i] : -1);
    for (size_t i = 0; i < PM; i++) ok = ok && p_kind[i] == kind[i] && a_kind[i] == (c.assign_too ? kind[i] : 9);
    for (size_t p = 0; p < (size_t)c.P; p++) ok = ok && in_prev[p] == (part_kind[p] != 0) && never[p] == (part_kind[p] == 1);
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
            ss >> c.P >> c.M >> c.L >> c.weights_nil >> c.assign_too;
            cases.push_back(c);
            continue;
        }
        if (cases.empty()) continue;
        Case& c = cases.back();
        std::vector<long long>* dst = tag == "k" ? &c.k : tag == "part_kind" ? &c.part_kind : tag == "off" ? &c.off : tag == "kind" ? &c.kind :
                                      tag == "nodes" ? &c.nodes : tag == "cur_a_off" ? &c.cur_a_off : tag == "cur_a_kind" ? &c.cur_a_kind :
                                      tag == "part_weight" ? &c.part_weight : tag == "part_has_weight" ? &c.part_has_weight :
                                      tag == "want" ? &c.want : nullptr;
        long long v;
        while (dst && ss >> v) dst->push_back(v);
    }
    int wrong = 0;
    for (size_t i = 0; i < cases.size(); i++) {
        const Case& c = cases[i];
        const size_t PM = (size_t)c.P * c.M;
        if (c.k.size() != (size_t)c.M || c.part_kind.size() != (size_t)c.P || c.off.size() != PM + 1 || c.kind.size() != PM ||
            c.nodes.size() != (size_t)c.off[PM] || c.cur_a_off.size() != PM + 1 || c.cur_a_kind.size() != PM ||
            c.part_weight.size() != (size_t)c.P || c.part_has_weight.size() != (size_t)c.P || c.want.size() != 9) {
            fprintf(stderr, "case %zu: malformed input\n", i);
            return 2;
        }
        if (!run(c)) { wrong++; fprintf(stderr, "case %zu (P %d, M %d, L %d, assign_too %d): differs from the definition\n", i, c.P, c.M, c.L, c.assign_too); }
    }
    printf("ran %zu cases, %d wrong\n", cases.size(), wrong);
    return wrong ? 1 : 0;
}
