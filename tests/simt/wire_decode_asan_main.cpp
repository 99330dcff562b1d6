// TEST INFRASTRUCTURE ONLY: the device decoder (blance_amd/csrc/k_wire_decode.h) under the SIMT emulator as a stand-alone
// program for AddressSanitizer and UBSan -- CPU only, nothing is loaded into another process:
//     g++ -std=c++17 -O1 -g1 -fsanitize=address,undefined -fno-omit-frame-pointer -x c++ wire_decode_asan_main.cpp -o prog
//     prog <input>          (the file tests/wire_decode_cases.py: write_program_input makes)
// Every document is decoded twice: through blance_wire_decode_device, and by the kernels driven from here with the document in
// a heap block of exactly len bytes rounded up to 16 (kWdPad, the padding the driver documents) and every other buffer of
// exactly the size its comment in WireDecodeParams gives -- "device" memory is the heap here, so a read or a write one byte
// outside is reported.  Both answers must agree.  One line per document: index, reason, offset, node references.
// tests/test_wire_decode_emulated.py builds and runs it and compares the lines with what the emulator library answered.
#include "emu_lib.cpp"
#include "../kernels/wire_decode_cases.inc"

#include <fstream>
#include <iostream>

namespace {
std::string unhex(const std::string& h) {
    std::string out;
    for (size_t i = 0; i + 1 < h.size(); i += 2) out.push_back((char)std::stoi(h.substr(i, 2), nullptr, 16));
    return out;
}
struct Names {
    std::string bytes;
    std::vector<int64_t> off{0};
    void add(const std::string& s) { bytes += s; off.push_back((int64_t)bytes.size()); }
};
template <class T> T* exact(std::vector<void*>& all, size_t n) {
    void* p = malloc((n ? n : 1) * sizeof(T));
    if (!p) abort();
    memset(p, 0, (n ? n : 1) * sizeof(T));
    all.push_back(p);
    return (T*)p;
}
int scan_host(int32_t* a, int n) {                           // exclusive, in place; a[n] = the total
    int32_t at = 0;
    for (int i = 0; i <= n; i++) { const int32_t v = i < n ? a[i] : 0; a[i] = at; at += v; }
    return a[n];
}

// the kernel sequence of wire_decode_locked on buffers of exact size
void decode_exact(const blance_wire_dict* d, const std::string& doc, int tile, int stage, int* reason, long long* at, long long* refs) {
    std::vector<void*> all;
    WireDecodeParams q;
    memset(&q, 0, sizeof q);
    const int len = (int)doc.size(), P = d->n[0], NX = d->n[1], M = d->n[2];
    const long long PM = (long long)P * M;
    q.len = len; q.tile = tile; q.n_tiles = (len + tile - 1) / tile;
    q.P = P; q.NX = NX; q.M = M; q.stage = stage;
    const size_t nt = (size_t)q.n_tiles, padded = ((size_t)len + kWdPad - 1) & ~(size_t)(kWdPad - 1);
    unsigned char* block = (unsigned char*)aligned_alloc(16, padded ? padded : 16);
    if (!block) abort();
    all.push_back(block);
    memcpy(block, doc.data(), (size_t)len);
    q.doc = block;
    q.tb = exact<int32_t>(all, nt); q.qbits = exact<uint32_t>(all, nt * (size_t)tile / 32);
    q.quotes = exact<int32_t>(all, nt + 1); q.depth = exact<int32_t>(all, nt + 1); q.count = exact<int32_t>(all, nt + 1);
    q.claim = exact<int32_t>(all, (size_t)P); q.part_kind = exact<uint8_t>(all, (size_t)P);
    q.kind = exact<uint8_t>(all, (size_t)PM); q.off = exact<int32_t>(all, (size_t)PM + 1);
    q.refusal = exact<unsigned long long>(all, 1);
    *q.refusal = ~0ull;
    WdTable* tabs[3] = {&q.part, &q.node, &q.state};
    for (int k = 0; k < 3; k++)
        *tabs[k] = WdTable{d->slots[k].as<int32_t>(), d->mask[k], d->bytes[k].as<unsigned char>(), d->off[k].as<int32_t>()};
    hipStream_t sm = nullptr;
    int R = 0;
    if (q.n_tiles > 0) {
        const int wgs = (q.n_tiles + 255) / 256;
        BLANCE_LAUNCH_NOSYNC(k_wd_tail, wgs, 256, 0, sm, q);
        BLANCE_LAUNCH_NOSYNC(k_wd_quotes, wgs, 256, 0, sm, q);
        scan_host(q.quotes, q.n_tiles);
        BLANCE_LAUNCH_NOSYNC(k_wd_walk<0>, wgs, 256, 0, sm, q);
        scan_host(q.depth, q.n_tiles);
        BLANCE_LAUNCH_NOSYNC(k_wd_walk<1>, wgs, 256, 0, sm, q);
        R = scan_host(q.count, q.n_tiles);
        q.rec = exact<int32_t>(all, (size_t)R);
        if (R > 0) BLANCE_LAUNCH_NOSYNC(k_wd_walk<2>, wgs, 256, 0, sm, q);
    }
    q.R = R;
    const int wgs2 = R > 0 ? (R + kWdRun - 1) / kWdRun : 1;
    BLANCE_LAUNCH(k_wd_parse<false>, wgs2, kWdRun, (size_t)stage, sm, q);
    *reason = 0; *at = -1; *refs = 0;
    if (*q.refusal != ~0ull) {
        *reason = (int)(*q.refusal & 255u);
        *at = (long long)(*q.refusal >> 8);
    } else {
        const int total = scan_host(q.off, (int)PM);
        *refs = total;
        q.nodes = exact<int32_t>(all, (size_t)total);
        if (total > 0) BLANCE_LAUNCH(k_wd_parse<true>, wgs2, kWdRun, (size_t)stage, sm, q);
        if (*q.refusal != ~0ull) { *reason = -1; }           // the two passes disagree
    }
    for (void* p : all) free(p);
}
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s <input>\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    Names part, node, state;
    std::vector<std::string> docs;
    int tile = kWdTileDefault, stage = kWdStageDefault;
    std::string tag, hex, line;
    while (std::getline(in, line)) {
        const size_t sp = line.find(' ');
        tag = line.substr(0, sp);
        hex = sp == std::string::npos ? "" : line.substr(sp + 1);
        if (tag == "T") { sscanf(hex.c_str(), "%d %d", &tile, &stage); }
        else if (tag == "P") part.add(unhex(hex));
        else if (tag == "N") node.add(unhex(hex));
        else if (tag == "S") state.add(unhex(hex));
        else if (tag == "D") docs.push_back(unhex(hex));
    }
    setenv("BLANCE_WIRE_IN_TILE", std::to_string(tile).c_str(), 1);
    setenv("BLANCE_WIRE_IN_STAGE", std::to_string(stage).c_str(), 1);
    blance_ctx* ctx = nullptr;
    if (blance_ctx_create(nullptr, &ctx) != BLANCE_OK) { fprintf(stderr, "no context: %s\n", blance_last_error()); return 2; }
    blance_wire_names nm{part.bytes.data(), part.off.data(), node.bytes.data(), node.off.data(), state.bytes.data(), state.off.data()};
    blance_wire_dict* d = nullptr;
    if (blance_wire_dict_create(ctx, &nm, (int32_t)part.off.size() - 1, (int32_t)node.off.size() - 1, (int32_t)state.off.size() - 1, &d) != BLANCE_OK) {
        fprintf(stderr, "no dictionary: %s\n", blance_last_error());
        return 2;
    }
    const int P = d->n[0], M = d->n[2];
    int bad = 0;
    for (size_t i = 0; i < docs.size(); i++) {
        const std::string& doc = docs[i];
        // exactly len bytes for the API too: it reads the caller's buffer once, to copy it
        char* own = (char*)malloc(doc.size() ? doc.size() : 1);
        memcpy(own, doc.data(), doc.size());
        blance_wire_lists wl;
        memset(&wl, 0, sizeof wl);
        int st = blance_wire_decode_device(ctx, d, own, doc.size(), &wl);          // count only
        std::vector<uint8_t> part_kind((size_t)P + 1), kind((size_t)P * M + 1);
        std::vector<int32_t> off((size_t)P * M + 1), nodes((size_t)wl.n_node_refs + 1);
        if (st == BLANCE_OK) {
            wl.part_kind = part_kind.data(); wl.off = off.data(); wl.kind = kind.data(); wl.nodes = nodes.data();
            wl.capacity = wl.n_node_refs;
            st = blance_wire_decode_device(ctx, d, own, doc.size(), &wl);
        }
        free(own);
        int reason = 0;
        long long at = -1, refs = 0;
        decode_exact(d, doc, ctx->wd_tile, ctx->wd_stage, &reason, &at, &refs);
        std::vector<uint32_t> qb(((doc.size() + (size_t)ctx->wd_tile - 1) / (size_t)ctx->wd_tile) * (size_t)ctx->wd_tile / 32 + 1);
        std::vector<int32_t> qs(doc.size() / (size_t)ctx->wd_tile + 2), dp(qs.size()), rec(doc.size() + 1);
        const int R = blance_case_wd_split((const unsigned char*)doc.data(), (int)doc.size(), ctx->wd_tile, qb.data(), qs.data(), dp.data(),
                                           rec.data(), (int)doc.size());
        const bool agree = reason == wl.refusal && at == wl.refusal_at && refs == wl.n_node_refs &&
                           (st == BLANCE_OK ? reason == 0 : (st == BLANCE_ERR_UNSUPPORTED && reason > 0)) && R >= 0;
        if (!agree) {
            bad++;
            fprintf(stderr, "document %zu: the library says status %d reason %d at %lld refs %lld, the exact buffers reason %d at %lld refs %lld, split %d\n",
                    i, st, wl.refusal, (long long)wl.refusal_at, (long long)wl.n_node_refs, reason, at, refs, R);
        }
        printf("%zu %d %lld %lld\n", i, reason, at, refs);
    }
    blance_wire_dict_destroy(ctx, d);
    blance_ctx_destroy(ctx);
    printf("decoded %zu documents, %d disagreements\n", docs.size(), bad);
    return bad ? 1 : 0;
}
