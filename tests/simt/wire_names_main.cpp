// TEST INFRASTRUCTURE ONLY: the host tables of the wire paths (blance_amd/csrc/host/wire_names.hpp) alone, as a stand-alone
// program for plain g++ -- no HIP, no context.  It reads the commands tests/test_wire_names.py writes (whitespace-separated
// words: a command's name, then integers), calls the header's functions and prints what they return, one "name values..."
// line each.  Every array is a heap block of exactly its size, so that the build under AddressSanitizer sees an access past
// an end.
//
//   wire_names_main <commands> <answers>
//
// A blob is written <has_off> [<n> off[0..n]] <has_bytes> [<n_bytes> bytes...]: the bytes need not be as many as off[n] says.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "../../blance_amd/csrc/host/wire_names.hpp"

using namespace blance;

namespace {
FILE* g_in = nullptr;
FILE* g_out = nullptr;

long long next_int() {
    long long v = 0;
    if (fscanf(g_in, "%lld", &v) != 1) { fprintf(stderr, "command file ends early\n"); exit(2); }
    return v;
}
template <class T>
std::unique_ptr<T[]> next_array(long long n) {                  // exactly n elements (new T[0] is a valid, unreadable block)
    if (n < 0 || n > (1 << 24)) { fprintf(stderr, "bad array length\n"); exit(2); }
    std::unique_ptr<T[]> a(new T[(size_t)n]);
    for (long long i = 0; i < n; i++) a[(size_t)i] = (T)next_int();
    return a;
}
void line(const char* name, std::initializer_list<long long> v) {
    fprintf(g_out, "%s", name);
    for (long long x : v) fprintf(g_out, " %lld", x);
    fprintf(g_out, "\n");
}
template <class T>
void line(const char* name, const T* v, size_t n) {
    fprintf(g_out, "%s", name);
    for (size_t i = 0; i < n; i++) fprintf(g_out, " %lld", (long long)v[i]);
    fprintf(g_out, "\n");
}
void line_bytes(const char* name, const std::string& s) {
    fprintf(g_out, "%s", name);
    for (unsigned char ch : s) fprintf(g_out, " %d", (int)ch);
    fprintf(g_out, "\n");
}

struct Blob {
    std::unique_ptr<int64_t[]> off;
    std::unique_ptr<char[]> bytes;
    long long n = 0;
    void read() {
        if (next_int()) { n = next_int(); off = next_array<int64_t>(n + 1); }
        if (next_int()) bytes = next_array<char>(next_int());
    }
    WireBlob view() const { return WireBlob{bytes.get(), off.get(), n}; }
};

// three blobs and the sizes the call is told (which may be negative, or differ from the blobs')
struct Names {
    Blob b[3];
    int32_t P = 0, NX = 0, M = 0;
    blance_wire_names nm{};
    void read() {
        P = (int32_t)next_int(); NX = (int32_t)next_int(); M = (int32_t)next_int();
        for (Blob& x : b) x.read();
        nm.part_bytes = b[0].bytes.get(); nm.part_off = b[0].off.get();
        nm.node_bytes = b[1].bytes.get(); nm.node_off = b[1].off.get();
        nm.state_bytes = b[2].bytes.get(); nm.state_off = b[2].off.get();
    }
};

void do_sort() {
    Blob b;
    b.read();
    std::vector<int32_t> order;
    const bool ok = wire_sort(b.view(), order);
    line("ok", {ok});
    line("order", order.data(), order.size());
}

// escape <blob> <has_order> [order n] <tail bytes> tail...
void do_escape() {
    Blob b;
    b.read();
    std::unique_ptr<int32_t[]> order;
    if (next_int()) order = next_array<int32_t>(b.n);
    const long long tn = next_int();
    std::unique_ptr<char[]> tail = next_array<char>(tn);
    const std::string t(tail.get(), (size_t)tn);
    std::string out;
    std::vector<int32_t> off;
    const bool ok = wire_escape(b.view(), order.get(), t.c_str(), out, off);
    line("ok", {ok});
    line("off", off.data(), off.size());
    line_bytes("bytes", out);
}

void do_check() {
    Blob b;
    b.read();
    line("err", {(long long)wire_blob_check(b.view())});
}

// table <blob> <the cause of a duplicate>
void do_table() {
    Blob b;
    b.read();
    const WireErr dup = (WireErr)next_int();
    std::vector<int32_t> slots, off32;
    uint32_t mask = 0;
    const WireErr e = wd_build_table(b.view(), dup, slots, mask, off32);
    line("err", {(long long)e});
    if (e != WireErr::kNone) return;
    line("mask", {(long long)mask});
    line("slots", slots.data(), slots.size());
    line("off32", off32.data(), off32.size());
}

void do_names() {
    Names n;
    n.read();
    NamesBlock nb;
    const WireErr e = names_block_build(&n.nm, n.P, n.NX, n.M, nb);
    line("err", {(long long)e});
    if (e != WireErr::kNone) return;
    line("block", nb.block.data(), nb.block.size());
    line("sums", {(long long)nb.part_esc_bytes, (long long)nb.state_esc_bytes, nb.node_esc_max});
    // every table of the single path: its first byte in the block, its bytes -- in the order of WireTables' fields
    const WireTable* t[8] = {&nb.tables.order, &nb.tables.part_esc, &nb.tables.part_off, &nb.tables.node_esc, &nb.tables.node_off,
                             &nb.tables.state_esc, &nb.tables.state_off, &nb.tables.state_id};
    fprintf(g_out, "tables");
    for (const WireTable* x : t)
        fprintf(g_out, " %lld %lld", (long long)((const char*)x->p - (const char*)nb.block.data()), (long long)x->bytes);
    fprintf(g_out, "\n");
}

void do_dict() {
    Names n;
    n.read();
    DictBlock d;
    const WireErr e = dict_block_build(&n.nm, n.P, n.NX, n.M, d);
    line("err", {(long long)e});
    if (e != WireErr::kNone) return;
    line("block", d.block.data(), d.block.size());
    line("n", d.tables.n, 3);
    line("mask", d.tables.mask, 3);
    long long at[3];                                             // where the tables' names lie: bytes from the block's start
    for (int k = 0; k < 3; k++) at[k] = (const char*)d.tables.bytes[k] - (const char*)d.block.data();
    line("bytes_at", at, 3);
    const char* slots_k[3] = {"slots0", "slots1", "slots2"};
    const char* off32_k[3] = {"off32_0", "off32_1", "off32_2"};
    for (int k = 0; k < 3; k++) {
        line(slots_k[k], d.tables.slots[k].data(), d.tables.slots[k].size());
        line(off32_k[k], d.tables.off32[k].data(), d.tables.off32[k].size());
    }
}

// layout <first> <n> words...
void do_layout() {
    const long long first = next_int(), n = next_int();
    std::unique_ptr<size_t[]> words = next_array<size_t>(n);
    std::unique_ptr<size_t[]> at(new size_t[(size_t)n]);
    size_t total = 0;
    const bool ok = wire_block_layout(words.get(), (int)n, (size_t)first, at.get(), total);
    line("ok", {ok});
    line("at", at.get(), (size_t)n);
    line("total", {(long long)total});
}

// bounds <P> <M> k[M] <len> <assign_too> <has_names> <part_esc> <state_esc> <node_max> <skeleton_cap> <result_cap of wire_cap>
void do_bounds() {
    blance_problem pb{};
    pb.n_parts = (int32_t)next_int(); pb.n_states = (int32_t)next_int();
    std::unique_ptr<int32_t[]> k = next_array<int32_t>(pb.n_states);
    pb.state_constraints = k.get();
    const long long len = next_int(), assign_too = next_int(), has_names = next_int();
    NamesBlock nb;
    nb.part_esc_bytes = (size_t)next_int(); nb.state_esc_bytes = (size_t)next_int(); nb.node_esc_max = (int32_t)next_int();
    const long long skeleton = next_int(), result_cap = next_int();
    const DocBounds b = batch_doc_bounds(&pb, (size_t)len, assign_too != 0, has_names ? &nb : nullptr, skeleton);
    line("bounds", {b.result_cap, b.moves_cap, (long long)b.wire_cap});
    line("wire_cap", {(long long)batch_wire_cap_of(&pb, nb, result_cap)});
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: wire_names_main <commands> <answers>\n"); return 2; }
    g_in = fopen(argv[1], "r");
    g_out = fopen(argv[2], "w");
    if (!g_in || !g_out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    char cmd[64];
    int ran = 0;
    while (fscanf(g_in, "%63s", cmd) == 1) {
        const std::string c = cmd;
        fprintf(g_out, "answer\n");
        if (c == "sort") do_sort();
        else if (c == "escape") do_escape();
        else if (c == "check") do_check();
        else if (c == "table") do_table();
        else if (c == "names") do_names();
        else if (c == "dict") do_dict();
        else if (c == "layout") do_layout();
        else if (c == "bounds") do_bounds();
        else { fprintf(stderr, "unknown command %s\n", cmd); return 2; }
        ran++;
    }
    fprintf(g_out, "ran %d commands\n", ran);
    fclose(g_in);
    fclose(g_out);
    return 0;
}
