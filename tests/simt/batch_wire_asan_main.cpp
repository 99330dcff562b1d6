// TEST INFRASTRUCTURE ONLY: the two kernels of blance_plan_batch_wire (blance_amd/csrc/k_batch_wire.h) under the SIMT emulator as
// a stand-alone program for AddressSanitizer and UBSan -- CPU only, nothing is loaded into another process:
//     g++ -std=c++17 -O1 -g1 -fsanitize=address,undefined -fno-omit-frame-pointer -x c++ batch_wire_asan_main.cpp -o prog
//     prog <input>          (the file tests/batch_wire_cases.py: write_program_input makes)
// Every case runs through blance_case_batch_wire with every block of exactly the size the case gives -- "device" memory is
// the heap here, so a read or a write one byte outside is reported -- and every block is compared whole with what the
// definition says it must be afterwards (tests/batch_wire_cases.py: World).  tests/test_plan_batch_wire_kernels_emulated.py builds
// and runs it.
#include "emu_lib.cpp"
#include "../kernels/batch_wire_cases.inc"

#include <fstream>
#include <iostream>
#include <map>
#include <sstream>

namespace {
struct Case {
    int nb = 0, nw = 0, stage = 0, which = 0;
    std::map<std::string, std::vector<long long>> a;
};
template <class T> std::vector<T> as(const std::vector<long long>& v) {
    std::vector<T> out(v.size());
    for (size_t i = 0; i < v.size(); i++) out[i] = (T)v[i];
    return out;
}
template <class T> bool same(const std::vector<T>& got, const std::vector<long long>& want) {
    if (got.size() != want.size()) return false;
    for (size_t i = 0; i < got.size(); i++) if ((long long)got[i] != want[i]) return false;
    return true;
}
bool run(Case& c) {
    const auto shape = as<int32_t>(c.a["shape"]), wdesc = as<int32_t>(c.a["wdesc"]), in = as<int32_t>(c.a["in"]);
    auto sc = as<int32_t>(c.a["sc"]), out = as<int32_t>(c.a["out"]), total = as<int32_t>(c.a["total"]);
    auto doc = as<unsigned char>(c.a["doc"]);
    const int st = blance_case_batch_wire(c.nb, shape.data(), c.nw, wdesc.data(), in.data(), (long long)in.size(), sc.data(),
                                          (long long)sc.size(), out.data(), (long long)out.size(), total.data(), (char*)doc.data(),
                                          (long long)doc.size(), c.stage, c.which);
    if (st != 0) return false;
    return same(sc, c.a["want_sc"]) && same(out, c.a["want_out"]) && same(total, c.a["want_total"]) && same(doc, c.a["want_doc"]);
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
            ss >> c.nb >> c.nw >> c.stage >> c.which;
            cases.push_back(c);
            continue;
        }
        if (cases.empty() || tag.empty()) continue;
        std::vector<long long>& dst = cases.back().a[tag];
        long long v;
        while (ss >> v) dst.push_back(v);
    }
    int wrong = 0;
    for (size_t i = 0; i < cases.size(); i++) {
        Case& c = cases[i];
        if (c.a["shape"].size() != (size_t)c.nb * 9 || c.a["wdesc"].size() != (size_t)c.nw * 4 || c.a["total"].size() != (size_t)c.nw) {
            fprintf(stderr, "case %zu: malformed input\n", i);
            return 2;
        }
        if (!run(c)) { wrong++; fprintf(stderr, "case %zu (%d problems, %d requests, stage %d, which %d): differs from the definition\n", i, c.nb, c.nw, c.stage, c.which); }
    }
    printf("ran %zu cases, %d wrong\n", cases.size(), wrong);
    return wrong ? 1 : 0;
}
