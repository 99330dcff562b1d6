// TEST INFRASTRUCTURE ONLY: the kernel of blance_plan_batch_docs (blance_amd/csrc/k_batch_decode.h) under the SIMT emulator as a
// stand-alone program for AddressSanitizer and UBSan -- CPU only, nothing is loaded into another process:
//     g++ -std=c++17 -O1 -g1 -fsanitize=address,undefined -fno-omit-frame-pointer -x c++ batch_decode_asan_main.cpp -o prog
//     prog <input>          (the file tests/batch_decode_cases.py: write_program_input makes)
// Every world runs through blance_case_batch_decode with every block of exactly the size the case gives -- "device" memory
// is the heap here, so a read or a write one byte outside is reported -- and every block is compared with what the
// definition fixes of it (the words whose mask is 1).  tests/test_plan_batch_docs_kernels_emulated.py builds and runs it.
#include "emu_lib.cpp"
#include "../kernels/batch_decode_cases.inc"

#include <fstream>
#include <iostream>
#include <map>
#include <sstream>

namespace {
struct World {
    int nb = 0, tile = 0, stage = 0;
    std::map<std::string, std::vector<long long>> a;
};
template <class T> std::vector<T> as(const std::vector<long long>& v) {
    std::vector<T> out(v.size());
    for (size_t i = 0; i < v.size(); i++) out[i] = (T)v[i];
    return out;
}
bool same(const std::vector<int32_t>& got, const std::vector<long long>& want, const std::vector<long long>& mask) {
    if (got.size() != want.size() || got.size() != mask.size()) return false;
    for (size_t i = 0; i < got.size(); i++) if (mask[i] && (long long)got[i] != want[i]) return false;
    return true;
}
bool run(World& w) {
    const auto shape = as<int32_t>(w.a["shape"]), ddesc = as<int32_t>(w.a["ddesc"]);
    auto in = as<int32_t>(w.a["in"]), sc = as<int32_t>(w.a["sc"]);
    const auto docs = as<unsigned char>(w.a["docs"]);
    std::vector<int32_t> sum((size_t)w.nb * 16, (int32_t)0xCACACACA);
    if (docs.size() < 16) return false;
    const int st = blance_case_batch_decode(w.nb, shape.data(), w.nb, ddesc.data(), in.data(), (long long)in.size(), sc.data(),
                                            (long long)sc.size(), docs.data(), (long long)docs.size() - 16, sum.data(), w.tile, w.stage);
    if (st != 0) return false;
    return same(in, w.a["want_in"], w.a["mask_in"]) && same(sc, w.a["want_sc"], w.a["mask_sc"]) && same(sum, w.a["want_sum"], w.a["mask_sum"]);
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s <input>\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::vector<World> worlds;
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string tag;
        ss >> tag;
        if (tag == "W") {
            World w;
            ss >> w.nb >> w.tile >> w.stage;
            worlds.push_back(w);
            continue;
        }
        if (worlds.empty() || tag.empty()) continue;
        std::vector<long long>& dst = worlds.back().a[tag];
        long long v;
        while (ss >> v) dst.push_back(v);
    }
    int wrong = 0;
    for (size_t i = 0; i < worlds.size(); i++) {
        World& w = worlds[i];
        if (w.a["shape"].size() != (size_t)w.nb * 12 || w.a["ddesc"].size() != (size_t)w.nb * 11) {
            fprintf(stderr, "world %zu: malformed input\n", i);
            return 2;
        }
        if (!run(w)) { wrong++; fprintf(stderr, "world %zu (%d problems, tile %d, stage %d): differs from the definition\n", i, w.nb, w.tile, w.stage); }
    }
    printf("ran %zu cases, %d wrong\n", worlds.size(), wrong);
    return wrong ? 1 : 0;
}
