// k_wd_*: json.Unmarshal of a PartitionMap document on the device, against a dictionary of names given beforehand
// (blance_wire_decode_device), straight into the id space and the CSR layout of blance_problem's prev_* / assign_* arrays.
// Part of blance_hip.hip; DESIGN.md §4.13.  The mirror image of k_plan_wire.h.
//
// Contract: exact or refused, never guessed.  The kernels accept a document only when it is valid JSON of the shape in
// include/blance_wire.h AND lies inside the subset the header of blance_wire_decode_device lists; everything else ends in a
// reason code and a byte offset, and the caller takes the host decoder.
//
// Stage 1 (a HINT): where the records begin.  A record is one "key": value pair of the top-level object.  One thread per
// tile of the document (q.tile bytes, a multiple of 64):
//   k_wd_tail      the backslashes at the tile's end (a run may cross any number of tiles);
//   k_wd_quotes    the backslash run in front of the tile (summed over the tiles behind it while they are backslashes only)
//                  decides whether the tile's first byte is escaped; then one walk marks the unescaped quotes (one bit per
//                  byte, q.qbits) and counts them;
//   (scan)         the counts in front of every tile: their parity is the in-string state at the tile's first byte;
//   k_wd_walk<0>   the tile's change of bracket depth outside strings;  (scan)  the depth at the tile's first byte;
//   k_wd_walk<1>   counts, k_wd_walk<2> (behind a scan) writes the offsets of the opening quotes at depth 1.
// On a malformed document these offsets may be anything (inside the buffer); nothing below trusts them.
//
// Stage 2 (the DECISION): one thread per record parses strictly, from its key's opening quote through the value, and must
// then find, after whitespace, `,` + whitespace + EXACTLY the start of the next record -- the last record `}` + whitespace
// to the end of the document, record 0 `{` behind whitespace from byte 0.  So the threads' ranges tile the document: it is
// valid and inside the subset if and only if every thread says so, whatever stage 1 made of it.  Names are looked up in
// open-addressing hash tables over the UNESCAPED bytes (built on the host at load <= 1/2); a hit is confirmed by comparing
// every byte with the raw name, so the hash only decides the speed.  Two passes in the shape size -> scan -> write:
//   k_wd_parse<false>   claims the partition (a second claim is a refusal), writes part_kind, kind and the list lengths;
//   (scan)              the lengths become off;
//   k_wd_parse<true>    parses again and writes the node ids.
// The smallest (offset, reason) of all refusals wins (one 64-bit atomic min), so the answer does not depend on the schedule.
// A workgroup takes kWdRun consecutive records = one contiguous byte range, stages it in LDS with aligned 16-byte loads and
// its threads read bytes from LDS; a range longer than the stage is read from global memory.  Every read is bounded by
// q.len (WdSrc::at); the device copy is padded to the next multiple of 16 so that the last aligned load stays inside it.
#pragma once

namespace blance {

// reason codes of a refusal (include/blance_hip.h: BLANCE_WIRE_REFUSED_*)
enum WdReason {
    kWdAccepted = 0, kWdGrammar = 1, kWdType = 2, kWdNullDocument = 3, kWdUnknownPartition = 4, kWdUnknownState = 5,
    kWdUnknownNode = 6, kWdRepeatedPartition = 7, kWdRepeatedState = 8, kWdRepeatedField = 9, kWdUnknownField = 10,
    kWdNullPartition = 11, kWdNameMissing = 12, kWdNameDiffers = 13, kWdNullElement = 14, kWdInvalidUtf8 = 15,
    kWdUnpairedSurrogate = 16, kWdControlCharacter = 17, kWdRecordTooLong = 18, kWdDocumentTooLong = 19
};

constexpr int kWdRun = 256;                                  // records of a workgroup of k_wd_parse
constexpr int kWdTileDefault = 256, kWdTileMin = 64, kWdTileMax = 4096;
constexpr int kWdStageDefault = 32 * 1024, kWdStageMin = 64, kWdStageMax = 64 * 1024;
constexpr int kWdPad = 16;                                   // the device copy of the document holds len rounded up to this
// One thread parses one record: a record of more bytes than this is refused (kWdRecordTooLong), so that no thread walks a
// document of gigabytes alone.  Far above the stage: the path through global memory has room.  The same bound holds for
// the bytes in front of record 0 (counted from byte 0, refused at 0), for the whitespace behind the closing brace (counted
// from the brace, refused at the last record's start) and for k_wd_quotes' walk back over tiles of backslashes.
constexpr long long kWdMaxRecord = 1 << 20;

struct WdTable {                                             // names -> ids
    const int32_t* slots;                                    // [2 * (mask + 1)]: id (-1: empty), hash
    uint32_t mask;
    const unsigned char* bytes; const int32_t* off;          // the raw names, [n + 1] offsets
};

struct WireDecodeParams {
    const unsigned char* doc;                                // 16-byte aligned, (len + 15) & ~15 bytes readable
    int32_t len, tile, n_tiles;
    int32_t* tb;                                             // [n_tiles] backslashes at the tile's end
    uint32_t* qbits;                                         // [n_tiles * tile / 32] bit i & 31 of word i >> 5: byte i is an unescaped quote
    int32_t* quotes;                                         // [n_tiles + 1] unescaped quotes of the tile; scanned
    int32_t* depth;                                          // [n_tiles + 1] change of depth outside strings; scanned
    int32_t* count;                                          // [n_tiles + 1] record starts of the tile; scanned
    int32_t* rec;                                            // [R] byte offsets of the record starts
    int32_t R, P, M, NX, stage;
    WdTable part, node, state;
    int32_t* claim;                                          // [P] zeroed; INT32_MAX - (the first record that claimed the partition)
    uint8_t* part_kind;                                      // [P] zeroed
    uint8_t* kind;                                           // [P * M] zeroed
    int32_t* off;                                            // [P * M + 1] zeroed: lengths, then (scanned) offsets
    int32_t* nodes;                                          // [off[P * M]]; with row > 0: [P * M][row]
    int32_t row;                                             // 0: nodes is the CSR of off.  > 0 (k_batch_decode.h): list idx owns the
                                                             // row nodes[idx * row ..), the FIRST pass writes its first `row` ids
                                                             // beside the lengths, off stays lengths and there is no second pass
    unsigned long long* refusal;                             // all ones: min over the refusals of offset << 8 | reason
};

// (wd_hash_init / wd_hash_step / wd_hash_done: blance_kernels.h, shared with the host that builds the tables)

#ifdef BLANCE_SIMT_EMU
inline unsigned long long wd_atomic_min(unsigned long long* p, unsigned long long v) {
    unsigned long long old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (v < old && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return old;
}
#else
__device__ inline unsigned long long wd_atomic_min(unsigned long long* p, unsigned long long v) { return atomicMin(p, v); }
#endif

// ---- stage 1 --------------------------------------------------------------------------------------------------------------
// (BLANCE_WD_NO_KERNELS: a second translation unit of the device build takes the parser alone; the kernels are this file's
// once per library)

// the 16 bytes at doc + b (b a multiple of 16) as four words; byte k is (w[k >> 2] >> 8 * (k & 3)) & 255
#define WD_LOAD16(w, doc, b) const int4 w##_v = *(const int4*)((doc) + (b)); \
    const uint32_t w[4] = {(uint32_t)w##_v.x, (uint32_t)w##_v.y, (uint32_t)w##_v.z, (uint32_t)w##_v.w}

#ifndef BLANCE_WD_NO_KERNELS
__global__ __launch_bounds__(256) void k_wd_tail(WireDecodeParams q) {
    const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (t >= q.n_tiles) return;
    const long long lo = (long long)t * q.tile;
    const long long hi = lo + q.tile < q.len ? lo + q.tile : q.len;
    int n = 0;
    for (long long i = hi - 1; i >= lo && q.doc[i] == '\\'; i--) n++;
    q.tb[t] = n;
}

__global__ __launch_bounds__(256) void k_wd_quotes(WireDecodeParams q) {
    const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (t >= q.n_tiles) return;
    const long long lo = (long long)t * q.tile;
    const long long hi = lo + q.tile < q.len ? lo + q.tile : q.len;
    long long run = 0;                                       // backslashes in front of the tile (every tile behind it is a full one)
    // The walk back ends after kWdMaxRecord bytes of backslashes: a longer run lies in a record that stage 2 refuses as too
    // long whatever this hint says of the bytes behind it, and no thread walks over a document of backslashes alone.
    const int back = t - 1 - (int)(kWdMaxRecord / q.tile);
    for (int u = t - 1; u >= 0 && u > back; u--) {
        run += q.tb[u];
        if (q.tb[u] < q.tile) break;
    }
    bool esc = run & 1;                                      // the next byte is escaped
    int nq = 0;
    for (long long b = lo; b < hi; b += 16) {
        WD_LOAD16(w, q.doc, b);
        const int n = hi - b < 16 ? (int)(hi - b) : 16;
        uint32_t bits = 0;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const unsigned ch = (w[k >> 2] >> (8 * (k & 3))) & 255u;
            if (k < n) {
                if (esc) esc = false;
                else if (ch == '\\') esc = true;
                else if (ch == '"') { bits |= 1u << k; nq++; }
            }
        }
        uint16_t* half = (uint16_t*)q.qbits + (b >> 4);      // (a tile owns its words: no other thread writes them)
        *half = (uint16_t)bits;
    }
    for (long long b = (hi + 15) & ~15ll; b < lo + q.tile; b += 16) ((uint16_t*)q.qbits)[b >> 4] = 0;   // the last tile's rest
    q.quotes[t] = nq;
    if (t == q.n_tiles - 1) q.quotes[q.n_tiles] = 0;
}

// MODE 0: depth[t] = the tile's change of depth.  1: count[t] = opening quotes at depth 1.  2: their offsets to rec.
template <int MODE>
__global__ __launch_bounds__(256) void k_wd_walk(WireDecodeParams q) {
    const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (t >= q.n_tiles) return;
    const long long lo = (long long)t * q.tile;
    const long long hi = lo + q.tile < q.len ? lo + q.tile : q.len;
    bool in_str = q.quotes[t] & 1;
    int d = MODE == 0 ? 0 : q.depth[t], n = 0;
    const int base = MODE == 2 ? q.count[t] : 0;
    for (long long b = lo; b < hi; b += 16) {
        WD_LOAD16(w, q.doc, b);
        const int m = hi - b < 16 ? (int)(hi - b) : 16;
        const uint32_t bits = ((const uint16_t*)q.qbits)[b >> 4];
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const unsigned ch = (w[k >> 2] >> (8 * (k & 3))) & 255u;
            if (k < m) {
                if ((bits >> k) & 1u) {
                    if (MODE != 0 && !in_str && d == 1) {
                        if (MODE == 2) q.rec[base + n] = (int32_t)(b + k);
                        n++;
                    }
                    in_str = !in_str;
                } else if (!in_str) {
                    if (ch == '{' || ch == '[') d++;
                    else if (ch == '}' || ch == ']') d--;
                }
            }
        }
    }
    if (MODE == 0) {
        q.depth[t] = d;
        if (t == q.n_tiles - 1) q.depth[q.n_tiles] = 0;
    }
    if (MODE == 1) {
        q.count[t] = n;
        if (t == q.n_tiles - 1) q.count[q.n_tiles] = 0;
    }
}

#endif  // BLANCE_WD_NO_KERNELS

// ---- stage 2 --------------------------------------------------------------------------------------------------------------

struct WdSrc {                                               // the document's bytes: the staged range from LDS, the rest from global
    const unsigned char* g; const unsigned char* l;
    long long len, a0, hi;                                   // LDS holds [a0, hi)
    __device__ int at(long long i) const {
        if (i < 0 || i >= len) return -1;
        if (i >= a0 && i < hi) return l[i - a0];
        return g[i];
    }
};

struct WdParse {
    const WireDecodeParams* q;
    WdSrc s;
    long long p, start, limit;                               // the cursor; the record's first byte; no byte at or behind limit is read
    int reason;
    long long where;
    mutable bool hit;                                        // a read met the limit in front of the document's end
    __device__ int get(long long i) const {
        if (i < limit) return s.at(i);
        if (limit < s.len) hit = true;
        return -1;
    }
    // (a token that the limit cuts fails in front of it, `\` + nothing for one: whatever fails behind a read at the limit is
    // a record that is too long)
    __device__ bool fail(int why, long long at) {
        if (!reason) {
            if (hit || (at >= limit && limit < s.len)) { why = kWdRecordTooLong; at = start; }
            reason = why; where = at;
        }
        return false;
    }
    __device__ void ws() {
        for (;;) {
            const int c = get(p);
            if (c == ' ' || c == '\t' || c == '\n' || c == '\r') p++; else return;
        }
    }
    __device__ bool null_at(long long i) const { return get(i) == 'n' && get(i + 1) == 'u' && get(i + 2) == 'l' && get(i + 3) == 'l'; }
    // a byte that cannot stand where it does: the first byte of a value of another JSON type, or no value at all
    __device__ bool wrong(int c, long long at) {
        const bool value = c == '"' || c == '{' || c == '[' || c == '-' || (c >= '0' && c <= '9') || c == 't' || c == 'f' || c == 'n';
        return fail(value ? kWdType : kWdGrammar, at);
    }
};

struct WdStr { long long p; uint32_t pend; int npend, cont; };   // a string being unescaped, byte by byte

__device__ inline int wd_hex4(const WdParse& P, long long i) {
    int v = 0;
    for (int k = 0; k < 4; k++) {
        const int c = P.get(i + k);
        const int d = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1;
        if (d < 0) return -1;
        v = v * 16 + d;
    }
    return v;
}

// bytes of the well-formed UTF-8 sequence at i (its first byte is c >= 0x80), 0 if there is none: Go's utf8.DecodeRune
__device__ inline int wd_utf8_len(const WdParse& P, long long i, int c) {
    if (c < 0xC2) return 0;
    const int c1 = P.get(i + 1);
    if (c < 0xE0) return (c1 & 0xC0) == 0x80 && c1 >= 0 ? 2 : 0;
    const int c2 = P.get(i + 2);
    if (c < 0xF0) {
        if (c1 < 0 || c2 < 0 || (c1 & 0xC0) != 0x80 || (c2 & 0xC0) != 0x80) return 0;
        if (c == 0xE0 && c1 < 0xA0) return 0;
        if (c == 0xED && c1 > 0x9F) return 0;                // surrogates
        return 3;
    }
    if (c < 0xF5) {
        const int c3 = P.get(i + 3);
        if (c1 < 0 || c2 < 0 || c3 < 0 || (c1 & 0xC0) != 0x80 || (c2 & 0xC0) != 0x80 || (c3 & 0xC0) != 0x80) return 0;
        if (c == 0xF0 && c1 < 0x90) return 0;
        if (c == 0xF4 && c1 > 0x8F) return 0;
        return 4;
    }
    return 0;
}

// the next unescaped byte of the string d walks (d.p behind the opening quote at first); -1: the closing quote is passed;
// -2: refused (P.reason is set)
__device__ inline int wd_next(WdParse& P, WdStr& d) {
    if (d.npend) {
        const int b = (int)(d.pend & 255u);
        d.pend >>= 8; d.npend--;
        return b;
    }
    const int c = P.get(d.p);
    if (c < 0) { P.fail(kWdGrammar, d.p); return -2; }       // the document ends inside a string
    if (d.cont) { d.cont--; d.p++; return c; }               // (checked with the sequence's first byte)
    if (c == '"') { d.p++; return -1; }
    if (c < 0x20) { P.fail(kWdControlCharacter, d.p); return -2; }
    if (c == '\\') {
        const int x = P.get(d.p + 1);
        int b;
        switch (x) {
            case '"': case '\\': case '/': b = x; break;
            case 'b': b = 8; break;
            case 'f': b = 12; break;
            case 'n': b = 10; break;
            case 'r': b = 13; break;
            case 't': b = 9; break;
            case 'u': {
                const int v = wd_hex4(P, d.p + 2);
                if (v < 0) { P.fail(kWdGrammar, d.p); return -2; }
                uint32_t cp = (uint32_t)v;
                long long next = d.p + 6;
                if (cp >= 0xD800 && cp < 0xDC00) {           // a high surrogate needs a low one behind it (Go: U+FFFD otherwise)
                    int lo = -1;
                    if (P.get(next) == '\\' && P.get(next + 1) == 'u') lo = wd_hex4(P, next + 2);
                    if (lo < 0xDC00 || lo >= 0xE000) { P.fail(kWdUnpairedSurrogate, d.p); return -2; }
                    cp = 0x10000u + ((cp - 0xD800u) << 10) + ((uint32_t)lo - 0xDC00u);
                    next += 6;
                } else if (cp >= 0xDC00 && cp < 0xE000) {
                    P.fail(kWdUnpairedSurrogate, d.p);
                    return -2;
                }
                d.p = next;
                if (cp < 0x80) return (int)cp;
                if (cp < 0x800) { d.pend = 0x80u | (cp & 0x3Fu); d.npend = 1; return (int)(0xC0u | (cp >> 6)); }
                if (cp < 0x10000) {
                    d.pend = (0x80u | ((cp >> 6) & 0x3Fu)) | ((0x80u | (cp & 0x3Fu)) << 8); d.npend = 2;
                    return (int)(0xE0u | (cp >> 12));
                }
                d.pend = (0x80u | ((cp >> 12) & 0x3Fu)) | ((0x80u | ((cp >> 6) & 0x3Fu)) << 8) | ((0x80u | (cp & 0x3Fu)) << 16);
                d.npend = 3;
                return (int)(0xF0u | (cp >> 18));
            }
            default: P.fail(kWdGrammar, d.p); return -2;
        }
        d.p += 2;
        return b;
    }
    if (c < 0x80) { d.p++; return c; }
    const int l = wd_utf8_len(P, d.p, c);
    if (!l) { P.fail(kWdInvalidUtf8, d.p); return -2; }
    d.cont = l - 1; d.p++;
    return c;
}

// the string whose opening quote is at P.p: checked, hashed and measured (unescaped); P.p ends behind its closing quote
__device__ inline bool wd_string(WdParse& P, uint32_t* hash, int* n_out) {
    if (P.get(P.p) != '"') return P.fail(kWdGrammar, P.p);
    WdStr d{P.p + 1, 0u, 0, 0};
    uint32_t h = wd_hash_init();
    int n = 0;
    for (;;) {
        const int b = wd_next(P, d);
        if (b == -1) break;
        if (b < 0) return false;
        h = wd_hash_step(h, (unsigned)b);
        n++;
    }
    P.p = d.p;
    *hash = wd_hash_done(h, n);
    *n_out = n;
    return true;
}

// is the (checked) string whose opening quote is at p0 the n bytes at name?
__device__ inline bool wd_equals(WdParse& P, long long p0, const unsigned char* name, int n) {
    WdStr d{p0 + 1, 0u, 0, 0};
    for (int i = 0; i < n; i++)
        if (wd_next(P, d) != (int)name[i]) return false;
    return wd_next(P, d) == -1;
}
__device__ inline bool wd_equals_lit(WdParse& P, long long p0, const char* lit, int n) {
    WdStr d{p0 + 1, 0u, 0, 0};
    for (int i = 0; i < n; i++)
        if (wd_next(P, d) != (int)(unsigned char)lit[i]) return false;
    return wd_next(P, d) == -1;
}

__device__ inline int wd_lookup(WdParse& P, const WdTable& t, long long p0, uint32_t h, int n) {
    uint32_t s = h & t.mask;
    for (;;) {                                               // (load <= 1/2: an empty slot ends every probe)
        const int id = t.slots[2 * s];
        if (id < 0) return -1;
        if ((uint32_t)t.slots[2 * s + 1] == h && t.off[id + 1] - t.off[id] == n && wd_equals(P, p0, t.bytes + t.off[id], n)) return id;
        s = (s + 1) & t.mask;
    }
}

// `[ "node", ... ]` or null at P.p; the length to *len_out
template <bool WRITE>
__device__ inline bool wd_list(WdParse& P, long long idx, int* kind_out, int* len_out) {
    const WireDecodeParams& q = *P.q;
    int c = P.get(P.p);
    *len_out = 0;
    if (c == 'n' && P.null_at(P.p)) { P.p += 4; *kind_out = kListNil; return true; }
    if (c != '[') return P.wrong(c, P.p);
    P.p++;
    *kind_out = kListSet;
    P.ws();
    if (P.get(P.p) == ']') { P.p++; return true; }
    const bool rows = q.row > 0;
    const int room = rows ? q.row : WRITE ? q.off[idx + 1] - q.off[idx] : 0;
    int32_t* dst = rows ? q.nodes + idx * q.row : WRITE ? q.nodes + q.off[idx] : nullptr;
    int n = 0;
    for (;;) {
        P.ws();
        const long long e0 = P.p;
        c = P.get(e0);
        if (c == 'n' && P.null_at(e0)) return P.fail(kWdNullElement, e0);
        if (c != '"') return P.wrong(c, e0);
        uint32_t h; int len;
        if (!wd_string(P, &h, &len)) return false;
        const int x = wd_lookup(P, q.node, e0, h, len);
        if (x < 0) return P.fail(kWdUnknownNode, e0);
        if (n < room) dst[n] = x;
        n++;
        P.ws();
        c = P.get(P.p);
        if (c == ',') { P.p++; continue; }
        if (c == ']') { P.p++; break; }
        return P.fail(kWdGrammar, P.p);
    }
    *len_out = n;
    return true;
}

// `{ "state": list, ... }` at P.p (the brace is there)
template <bool WRITE>
__device__ inline bool wd_states(WdParse& P, int pid) {
    const WireDecodeParams& q = *P.q;
    P.p++;
    P.ws();
    if (P.get(P.p) == '}') { P.p++; return true; }
    for (;;) {
        P.ws();
        const long long s0 = P.p;
        uint32_t h; int len;
        if (!wd_string(P, &h, &len)) return false;
        const int sid = wd_lookup(P, q.state, s0, h, len);
        if (sid < 0) return P.fail(kWdUnknownState, s0);
        const long long idx = (long long)pid * q.M + sid;
        if (!WRITE && q.kind[idx]) return P.fail(kWdRepeatedState, s0);   // (only this thread writes the partition's slots)
        P.ws();
        if (P.get(P.p) != ':') return P.fail(kWdGrammar, P.p);
        P.p++;
        P.ws();
        int kind, n;
        if (!wd_list<WRITE>(P, idx, &kind, &n)) return false;
        if (!WRITE) { q.kind[idx] = (uint8_t)kind; q.off[idx] = n; }
        P.ws();
        const int c = P.get(P.p);
        if (c == ',') { P.p++; continue; }
        if (c == '}') { P.p++; return true; }
        return P.fail(kWdGrammar, P.p);
    }
}

// record r, from its key's opening quote to the first byte of the next record (the end of the document)
template <bool WRITE>
__device__ inline bool wd_record(WdParse& P, int r) {
    const WireDecodeParams& q = *P.q;
    if (r == 0) {                                            // `{` behind whitespace from byte 0, whitespace up to the record
        const long long rec0 = P.start, limit0 = P.limit;   // (the bytes in front of record 0 are bounded like a record at byte 0)
        P.start = 0;
        P.limit = P.s.len < kWdMaxRecord ? P.s.len : kWdMaxRecord;
        P.p = 0;
        P.ws();
        const int c = P.get(P.p);
        if (c != '{') return P.wrong(c, P.p);
        P.p++;
        P.ws();
        if (P.p != rec0) return P.fail(kWdGrammar, P.p);
        P.start = rec0;
        P.limit = limit0;
        P.hit = false;                                       // (the whitespace may end exactly at its limit)
    }
    P.p = P.start;
    uint32_t h; int len;
    if (!wd_string(P, &h, &len)) return false;
    const int pid = wd_lookup(P, q.part, P.start, h, len);
    if (pid < 0) return P.fail(kWdUnknownPartition, P.start);
    if (!WRITE) {
        // Of the records that claim one partition all but the first are refused; whoever comes second reports the later of the
        // two it knows, so the smallest offset reported is the second record's whatever the order of the claims.
        const int old = atomicMax(&q.claim[pid], INT32_MAX - r);
        if (old) {
            const int other = INT32_MAX - old;
            return P.fail(kWdRepeatedPartition, q.rec[other > r ? other : r]);
        }
    }
    P.ws();
    if (P.get(P.p) != ':') return P.fail(kWdGrammar, P.p);
    P.p++;
    P.ws();
    int c = P.get(P.p);
    if (c == 'n' && P.null_at(P.p)) return P.fail(kWdNullPartition, P.p);
    if (c != '{') return P.wrong(c, P.p);
    P.p++;
    P.ws();
    bool seen_name = false, seen_map = false;
    int part_kind = kListNil;
    if (P.get(P.p) == '}') {
        P.p++;
    } else {
        for (;;) {
            P.ws();
            const long long f0 = P.p;
            if (!wd_string(P, &h, &len)) return false;
            const bool is_name = len == 4 && wd_equals_lit(P, f0, "name", 4);
            const bool is_map = !is_name && len == 12 && wd_equals_lit(P, f0, "nodesByState", 12);
            if (!is_name && !is_map) return P.fail(kWdUnknownField, f0);
            if (is_name ? seen_name : seen_map) return P.fail(kWdRepeatedField, f0);
            P.ws();
            if (P.get(P.p) != ':') return P.fail(kWdGrammar, P.p);
            P.p++;
            P.ws();
            c = P.get(P.p);
            if (is_name) {
                seen_name = true;
                const long long v0 = P.p;
                if (c == 'n' && P.null_at(v0)) return P.fail(kWdNameDiffers, v0);       // (Go leaves Name "")
                if (c != '"') return P.wrong(c, v0);
                if (!wd_string(P, &h, &len)) return false;
                const int want = q.part.off[pid + 1] - q.part.off[pid];
                if (len != want || !wd_equals(P, v0, q.part.bytes + q.part.off[pid], want)) return P.fail(kWdNameDiffers, v0);
            } else {
                seen_map = true;
                if (c == 'n' && P.null_at(P.p)) {
                    P.p += 4;
                } else if (c == '{') {
                    part_kind = kListSet;
                    if (!wd_states<WRITE>(P, pid)) return false;
                } else {
                    return P.wrong(c, P.p);
                }
            }
            P.ws();
            c = P.get(P.p);
            if (c == ',') { P.p++; continue; }
            if (c == '}') { P.p++; break; }
            return P.fail(kWdGrammar, P.p);
        }
    }
    if (!seen_name) return P.fail(kWdNameMissing, P.start);
    if (!WRITE) q.part_kind[pid] = (uint8_t)part_kind;
    P.ws();
    if (r + 1 < q.R) {
        if (P.get(P.p) != ',') return P.fail(kWdGrammar, P.p);
        P.p++;
        P.ws();
        if (P.p != q.rec[r + 1]) return P.fail(kWdGrammar, P.p);
    } else {
        if (P.get(P.p) != '}') return P.fail(kWdGrammar, P.p);
        P.p++;
        // (whitespace behind the document is not the record's: bounded on its own, refused like a record that is too long)
        P.limit = P.p + kWdMaxRecord < P.s.len ? P.p + kWdMaxRecord : P.s.len;
        P.hit = false;
        P.ws();
        if (P.p != P.s.len) return P.fail(kWdGrammar, P.p);
    }
    return true;
}

// a document without a record: `{}`, or `null` (refused), or no document of this shape
__device__ inline bool wd_empty_document(WdParse& P) {
    P.p = 0;
    P.ws();
    const int c = P.get(P.p);
    if (c == 'n' && P.null_at(P.p)) {
        const long long at = P.p;
        P.p += 4;
        P.ws();
        return P.fail(P.p == P.s.len ? kWdNullDocument : kWdGrammar, P.p == P.s.len ? at : P.p);
    }
    if (c != '{') return P.wrong(c, P.p);
    P.p++;
    P.ws();
    if (P.get(P.p) != '}') return P.fail(kWdGrammar, P.p);
    P.p++;
    P.ws();
    if (P.p != P.s.len) return P.fail(kWdGrammar, P.p);
    return true;
}

#ifndef BLANCE_WD_NO_KERNELS
template <bool WRITE>
__global__ __launch_bounds__(kWdRun) void k_wd_parse(WireDecodeParams q) {
    BLANCE_DYN_LDS(lds);
    const int tid = (int)threadIdx.x;
    const int r0 = (int)blockIdx.x * kWdRun, r1 = r0 + kWdRun < q.R ? r0 + kWdRun : q.R;
    long long a0 = 0, hi = 0;
    if (r0 < r1) {                                           // (the same in every thread: the barrier is uniform)
        long long lo = q.rec[r0], end = r1 < q.R ? q.rec[r1] : q.len;
        if (end > q.len) end = q.len;
        if (lo >= 0 && lo < end && end - (lo & ~15ll) <= (long long)q.stage) {
            a0 = lo & ~15ll;
            hi = end;
            for (long long i = (long long)tid * 16; i < end - a0; i += kWdRun * 16)
                *(int4*)(lds + i) = *(const int4*)(q.doc + a0 + i);       // (the last load may pass `end`: inside the padded copy)
        }
    }
    __syncthreads();
    WdParse P;
    P.q = &q;
    P.s = WdSrc{q.doc, lds, (long long)q.len, a0, hi};
    P.reason = 0; P.where = 0; P.p = 0; P.start = 0; P.limit = q.len; P.hit = false;
    bool ok = true;
    if (q.R == 0) {
        if (blockIdx.x != 0 || tid != 0) return;
        P.limit = q.len < kWdMaxRecord ? q.len : kWdMaxRecord;
        ok = wd_empty_document(P);
    } else {
        const int r = r0 + tid;
        if (r >= r1) return;
        P.start = q.rec[r];
        P.limit = P.start + kWdMaxRecord < q.len ? P.start + kWdMaxRecord : q.len;
        ok = wd_record<WRITE>(P, r);
    }
    if (!ok) wd_atomic_min(q.refusal, ((unsigned long long)P.where << 8) | (unsigned long long)P.reason);
}
#endif  // BLANCE_WD_NO_KERNELS

}  // namespace blance
