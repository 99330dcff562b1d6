// The host tables of the wire paths: the partitions' document order, every escaped
// byte, the open-addressing hash tables of the decoder, the word layout of a batch's names block and dictionary block, and
// the capacities of a batch's documents.  Pure functions: no HIP, no context, no error text -- a failure is a WireErr,
// blance_hip.hip's wire_fail() gives it the entry point's status and words; tests/simt/wire_names_main.cpp prints the tables.
// k_wire_*, k_wd_parse, k_batch_wire_* and k_batch_decode follow these ranks and offsets blindly.
#pragma once

#include <limits.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../../include/blance_hip.h"
#include "../../../include/blance_batch.h"
#include "../blance_kernels.h"
#include "json_escape.hpp"

namespace blance {

// one value per cause; what a caller is told of it depends on the entry point (wire_fail)
enum class WireErr {
    kNone = 0,
    kNegativeSize,                                       // a count below zero
    kTooManyLists,                                       // n_parts * n_states of 2^31 - 1 or more (the dictionaries)
    kNullOffsets, kFirstOffset, kNotMonotone, kNullBytes,   // the blob checks
    kDupPartition, kDupNode, kDupState,                  // (the names encoder accepts two nodes with one name)
    kTooLong,                                            // names, escaped names or a block of 2^31 bytes / words or more
};

struct WireBlob { const char* bytes; const int64_t* off; int64_t n; };

// the three blobs of the caller's names: partitions, nodes, states
struct WireBlobs { WireBlob b[3]; };
inline WireBlobs wire_blobs(const blance_wire_names* nm, int64_t P, int64_t NX, int64_t M) {
    return WireBlobs{{{nm->part_bytes, nm->part_off, P}, {nm->node_bytes, nm->node_off, NX}, {nm->state_bytes, nm->state_off, M}}};
}

// n + 1 offsets from 0, not falling; bytes where there are any (off[n] == 0 with null bytes is fine)
inline WireErr wire_blob_check(const WireBlob& b) {
    if (!b.off) return WireErr::kNullOffsets;
    if (b.off[0] != 0) return WireErr::kFirstOffset;
    for (int64_t i = 0; i < b.n; i++)
        if (b.off[i + 1] < b.off[i]) return WireErr::kNotMonotone;
    if (b.off[b.n] > 0 && !b.bytes) return WireErr::kNullBytes;
    return WireErr::kNone;
}
inline WireErr wire_blobs_check(const WireBlobs& w) {
    for (const WireBlob& b : w.b)
        if (const WireErr e = wire_blob_check(b); e != WireErr::kNone) return e;
    return WireErr::kNone;
}

// ---- the names of a document to write (§4.12, 4.16)
inline int wire_cmp(const WireBlob& b, int64_t x, int64_t y) {       // bytewise, as the host encoder orders map keys
    const size_t xn = (size_t)(b.off[x + 1] - b.off[x]), yn = (size_t)(b.off[y + 1] - b.off[y]);
    const size_t m = xn < yn ? xn : yn;
    const int c = m ? memcmp(b.bytes + b.off[x], b.bytes + b.off[y], m) : 0;
    if (c) return c;
    return xn < yn ? -1 : (xn > yn ? 1 : 0);
}
// the ids of a blob's strings in byte order of the strings; false: two strings are equal
inline bool wire_sort(const WireBlob& b, std::vector<int32_t>& order) {
    const int64_t n = b.n;
    order.resize((size_t)n);
    for (int64_t i = 0; i < n; i++) order[(size_t)i] = (int32_t)i;
    bool sorted = true;                                  // already in key order, strictly?  (then there is no duplicate either)
    for (int64_t i = 1; i < n && sorted; i++) sorted = wire_cmp(b, i - 1, i) < 0;
    if (sorted) return true;
    // by the first eight bytes as one big-endian word (a shorter string padded with zeros), the whole strings on a tie
    struct Key { uint64_t pre; int32_t id; };
    std::vector<Key> keys((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        const size_t len = (size_t)(b.off[i + 1] - b.off[i]);
        uint64_t pre = 0;
        for (size_t k = 0; k < 8; k++) pre = (pre << 8) | (k < len ? (unsigned char)b.bytes[b.off[i] + (int64_t)k] : 0u);
        keys[(size_t)i] = Key{pre, (int32_t)i};
    }
    std::sort(keys.begin(), keys.end(), [&](const Key& x, const Key& y) {
        if (x.pre != y.pre) return x.pre < y.pre;
        return wire_cmp(b, x.id, y.id) < 0;
    });
    for (int64_t i = 0; i < n; i++) order[(size_t)i] = keys[(size_t)i].id;
    for (int64_t i = 1; i < n; i++)
        if (wire_cmp(b, order[(size_t)i - 1], order[(size_t)i]) == 0) return false;
    return true;
}
// the escaped forms of a blob's strings in the order `order` gives (null: as they lie), `tail` behind each, with n + 1 offsets;
// false: 2^31 bytes or more
inline bool wire_escape(const WireBlob& b, const int32_t* order, const char* tail, std::string& out, std::vector<int32_t>& off) {
    off.assign((size_t)b.n + 1, 0);
    for (int64_t i = 0; i < b.n; i++) {
        const int64_t id = order ? order[(size_t)i] : i;
        blance_json::put_string(out, b.bytes + b.off[id], (size_t)(b.off[id + 1] - b.off[id]));
        out += tail;
        if (out.size() > (size_t)INT32_MAX) return false;
        off[(size_t)i + 1] = (int32_t)out.size();
    }
    return true;
}

// What the document needs of the names alone: the partitions' order, every string escaped.
struct WirePrepared {
    std::vector<int32_t> order, sorder, poff, noff, soff;
    std::string pesc, nesc, sesc;
};

// the checks of the names and their prepared tables (blance_plan_wire_names and blance_batch_names_create)
inline WireErr wire_prepare(const blance_wire_names* nm, int64_t n_parts, int64_t n_nodes_ext, int64_t n_states, WirePrepared& w) {
    const WireBlobs blobs = wire_blobs(nm, n_parts, n_nodes_ext, n_states);
    if (const WireErr e = wire_blobs_check(blobs); e != WireErr::kNone) return e;
    const WireBlob &part = blobs.b[0], &node = blobs.b[1], &state = blobs.b[2];
    if (!wire_sort(state, w.sorder)) return WireErr::kDupState;
    if (!wire_sort(part, w.order)) return WireErr::kDupPartition;
    if (!wire_escape(part, w.order.data(), "", w.pesc, w.poff) || !wire_escape(node, nullptr, "", w.nesc, w.noff) ||
        !wire_escape(state, w.sorder.data(), ":", w.sesc, w.soff))
        return WireErr::kTooLong;
    return WireErr::kNone;
}

// the eight prepared tables as the context's buffers of the same names want them (PlanWireParams' fields)
struct WireTable { const void* p; size_t bytes; };
struct WireTables { WireTable order, part_esc, part_off, node_esc, node_off, state_esc, state_off, state_id; };

inline WireTables wire_tables_of(const WirePrepared& w) {
    auto words = [](const std::vector<int32_t>& v) { return WireTable{v.data(), sizeof(int32_t) * v.size()}; };
    auto chars = [](const std::string& s) { return WireTable{s.data(), s.size()}; };
    return WireTables{words(w.order), chars(w.pesc), words(w.poff), chars(w.nesc), words(w.noff), chars(w.sesc), words(w.soff),
                      words(w.sorder)};
}

// Tables of words[i] words one behind the other from word `first` on, each at a multiple of 4 words: at[i] and the words of
// the whole; false: more than 2^31 - 1 words
inline bool wire_block_layout(const size_t* words, int n, size_t first, size_t* at, size_t& total) {
    total = first;
    for (int i = 0; i < n; i++) { at[i] = total; total += (words[i] + 3) & ~(size_t)3; }
    return total <= (size_t)INT32_MAX;
}

// The prepared names of one index as one block of int32 words (blance_batch_names): kBatchNamesHdr word offsets, then the
// tables in the order of kNames*.  k_batch_wire.h reads it through its header.
struct NamesBlock {
    std::vector<int32_t> block;
    size_t part_esc_bytes = 0, state_esc_bytes = 0;      // the sums of blance_batch_wire_capacity
    int32_t node_esc_max = 0;                            // the longest escaped node name
    WireTables tables{};                                 // the same tables, in the block (the single path)
};

inline WireErr names_block_pack(const WirePrepared& w, NamesBlock& nb) {
    const WireTables t = wire_tables_of(w);
    WireTable src[kBatchNamesHdr];
    src[kNamesOrder] = t.order; src[kNamesPartOff] = t.part_off; src[kNamesNodeOff] = t.node_off; src[kNamesStateOff] = t.state_off;
    src[kNamesStateId] = t.state_id; src[kNamesPartEsc] = t.part_esc; src[kNamesNodeEsc] = t.node_esc; src[kNamesStateEsc] = t.state_esc;
    size_t words[kBatchNamesHdr], at[kBatchNamesHdr], total;
    for (int i = 0; i < kBatchNamesHdr; i++) words[i] = (src[i].bytes + 3) / 4;
    if (!wire_block_layout(words, kBatchNamesHdr, kBatchNamesHdr, at, total)) return WireErr::kTooLong;
    nb.block.assign(total, 0);
    for (int i = 0; i < kBatchNamesHdr; i++) {
        nb.block[(size_t)i] = (int32_t)at[i];
        if (src[i].bytes) memcpy(nb.block.data() + at[i], src[i].p, src[i].bytes);
    }
    const int32_t* b = nb.block.data();
    auto in_block = [&](int k) { return WireTable{b + at[k], src[k].bytes}; };
    nb.tables = WireTables{in_block(kNamesOrder), in_block(kNamesPartEsc), in_block(kNamesPartOff), in_block(kNamesNodeEsc),
                           in_block(kNamesNodeOff), in_block(kNamesStateEsc), in_block(kNamesStateOff), in_block(kNamesStateId)};
    nb.part_esc_bytes = w.pesc.size();
    nb.state_esc_bytes = w.sesc.size();
    nb.node_esc_max = 0;
    for (size_t x = 0; x + 1 < w.noff.size(); x++) nb.node_esc_max = std::max(nb.node_esc_max, w.noff[x + 1] - w.noff[x]);
    return WireErr::kNone;
}

// blance_batch_names_create but for the object
inline WireErr names_block_build(const blance_wire_names* nm, int32_t n_parts, int32_t n_nodes_ext, int32_t n_states, NamesBlock& nb) {
    if (n_parts < 0 || n_nodes_ext < 0 || n_states < 0) return WireErr::kNegativeSize;
    WirePrepared w;
    if (const WireErr e = wire_prepare(nm, n_parts, n_nodes_ext, n_states, w); e != WireErr::kNone) return e;
    return names_block_pack(w, nb);
}

// blance_batch_wire_capacity's formula (blance_batch.h) for a plan of at most result_cap list entries
inline size_t batch_wire_cap_of(const blance_problem* pb, const NamesBlock& nm, int64_t result_cap) {
    const size_t P = (size_t)pb->n_parts, M = (size_t)pb->n_states;
    return 2 + 29 * P + 2 * nm.part_esc_bytes + P * (nm.state_esc_bytes + 5 * M) + (size_t)result_cap * ((size_t)nm.node_esc_max + 1);
}

// blance_batch_doc_bounds' three bounds for a document of len bytes (blance_batch.h); skeleton_cap: blance_result_capacity(pb)
struct DocBounds { int64_t result_cap, moves_cap; size_t wire_cap; };
inline DocBounds batch_doc_bounds(const blance_problem* pb, size_t len, bool assign_too, const NamesBlock* nm, int64_t skeleton_cap) {
    const int64_t refs = (int64_t)(len / 3);
    int64_t rc = skeleton_cap;
    if (assign_too) {
        int64_t ksum = 0;
        for (int m = 0; m < pb->n_states; m++) ksum += pb->state_constraints[m] > 0 ? pb->state_constraints[m] : 0;
        rc = (int64_t)pb->n_parts * ksum + refs;
    }
    return DocBounds{rc, refs + rc, nm ? batch_wire_cap_of(pb, *nm, rc) : 0};
}

// ---- the names of a document to read (§4.13, 4.17)
// the open-addressing table of a blob's names (k_wire_decode.h: WdTable) at load <= 1/2 and the offsets as int32;
// `dup`: two names are equal (the cause of the blob's kind), kTooLong: 2^31 bytes or more
inline WireErr wd_build_table(const WireBlob& b, WireErr dup, std::vector<int32_t>& slots, uint32_t& mask, std::vector<int32_t>& off32) {
    if (b.off[b.n] > (int64_t)INT32_MAX) return WireErr::kTooLong;
    size_t cap = 2;
    while (cap < 2 * (size_t)b.n) cap <<= 1;
    mask = (uint32_t)(cap - 1);
    slots.assign(2 * cap, -1);
    off32.resize((size_t)b.n + 1);
    for (int64_t i = 0; i <= b.n; i++) off32[(size_t)i] = (int32_t)b.off[i];
    for (int64_t i = 0; i < b.n; i++) {
        const unsigned char* s = (const unsigned char*)b.bytes + b.off[i];
        const int n = (int)(b.off[i + 1] - b.off[i]);
        uint32_t h = wd_hash_init();
        for (int k = 0; k < n; k++) h = wd_hash_step(h, s[k]);
        h = wd_hash_done(h, n);
        uint32_t at = h & mask;
        for (;;) {
            const int32_t id = slots[2 * (size_t)at];
            if (id < 0) break;
            if ((uint32_t)slots[2 * (size_t)at + 1] == h && wire_cmp(b, id, i) == 0) return dup;
            at = (at + 1) & mask;
        }
        slots[2 * (size_t)at] = (int32_t)i;
        slots[2 * (size_t)at + 1] = (int32_t)h;
    }
    return WireErr::kNone;
}

// what a dictionary is made of on the host (blance_wire_dict_create and blance_batch_dict_create share it): per kind of name
// wd_build_table's table and int32 offsets, and where the raw names lie (the caller's blobs, or a batch dictionary's block)
struct WdHostTables {
    int32_t n[3] = {0, 0, 0};
    uint32_t mask[3] = {0, 0, 0};
    std::vector<int32_t> slots[3], off32[3];
    const void* bytes[3] = {nullptr, nullptr, nullptr};
};

// the checks of blance_wire_dict_create and the three tables
inline WireErr wd_host_tables(const blance_wire_names* nm, int32_t P, int32_t NX, int32_t M, WdHostTables& t) {
    if (P < 0 || NX < 0 || M < 0) return WireErr::kNegativeSize;
    if ((int64_t)P * M >= (int64_t)INT32_MAX) return WireErr::kTooManyLists;
    const WireBlobs blobs = wire_blobs(nm, P, NX, M);
    if (const WireErr e = wire_blobs_check(blobs); e != WireErr::kNone) return e;
    const WireErr dup[3] = {WireErr::kDupPartition, WireErr::kDupNode, WireErr::kDupState};
    for (int k = 0; k < 3; k++) {
        t.n[k] = (int32_t)blobs.b[k].n;
        t.bytes[k] = blobs.b[k].bytes;
        if (const WireErr e = wd_build_table(blobs.b[k], dup[k], t.slots[k], t.mask[k], t.off32[k]); e != WireErr::kNone) return e;
    }
    return WireErr::kNone;
}

// The dictionary of one index as one block of int32 words (blance_batch_dict): kBatchDictHdr words -- per kind slots (word
// offset), mask, raw bytes (word offset), int32 offsets (word offset), then the three counts --, then per kind slots, offsets,
// raw bytes.  k_batch_decode.h reads it through its header.  Afterwards t's names lie in the block.
inline WireErr dict_block_pack(WdHostTables& t, std::vector<int32_t>& block) {
    size_t words[9], at[9], total;
    for (int k = 0; k < 3; k++) {
        const size_t nb = (size_t)t.off32[k][(size_t)t.n[k]];
        words[3 * k] = t.slots[k].size(); words[3 * k + 1] = t.off32[k].size(); words[3 * k + 2] = (nb + 3) / 4;
    }
    if (!wire_block_layout(words, 9, kBatchDictHdr, at, total)) return WireErr::kTooLong;
    block.assign(total, 0);
    int32_t* b = block.data();
    for (int k = 0; k < 3; k++) {
        const size_t nb = (size_t)t.off32[k][(size_t)t.n[k]];
        const size_t slots = at[3 * k], off = at[3 * k + 1], bytes = at[3 * k + 2];
        b[4 * k] = (int32_t)slots; b[4 * k + 1] = (int32_t)t.mask[k]; b[4 * k + 2] = (int32_t)bytes; b[4 * k + 3] = (int32_t)off;
        b[12 + k] = t.n[k];
        memcpy(b + slots, t.slots[k].data(), sizeof(int32_t) * t.slots[k].size());
        memcpy(b + off, t.off32[k].data(), sizeof(int32_t) * t.off32[k].size());
        if (nb) memcpy(b + bytes, t.bytes[k], nb);
        t.bytes[k] = b + bytes;                          // (the caller's blobs are gone after the call)
    }
    return WireErr::kNone;
}

struct DictBlock {
    std::vector<int32_t> block;
    WdHostTables tables;                                 // the same as blance_wire_dict_create wants it, its names in the block
};

// blance_batch_dict_create but for the object
inline WireErr dict_block_build(const blance_wire_names* nm, int32_t n_parts, int32_t n_nodes_ext, int32_t n_states, DictBlock& d) {
    if (const WireErr e = wd_host_tables(nm, n_parts, n_nodes_ext, n_states, d.tables); e != WireErr::kNone) return e;
    return dict_block_pack(d.tables, d.block);
}

}  // namespace blance
