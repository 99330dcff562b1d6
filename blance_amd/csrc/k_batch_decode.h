// k_batch_decode (blance_plan_batch_docs): the prevMap documents of a batch, one workgroup of 256 threads
// per document, decoded straight into the packed input slice of the document's problem.  Part of tu_batch.hip.
//
// The parser is k_wire_decode.h's, unchanged: wd_record / wd_empty_document with a WireDecodeParams assembled per document
// whose tables point into the dictionary block behind the problem's input slice and whose `row` sends the node ids of list
// idx to row idx of the problem's prevMap lists (i_plist, stride kBatchMaxL) in the one parse there is.  Three phases:
//   split   (a HINT, stage 1 of k_wire_decode.h inside the workgroup) a thread takes a tile of q.tile bytes, the workgroup
//           walks the document in chunks of 256 tiles and carries four values from chunk to chunk -- the parity of the
//           backslash run, the parity of the quotes, the bracket depth, the record count; the three scans are block scans
//           (wave shuffles, the waves' totals through LDS).  All record starts are stored in the document's scratch region:
//           an opening quote at depth 1 stands at most at every second byte, so (len + 1) / 2 words hold them;
//   parse   (the DECISION) a thread takes a record, in runs of 256 with the run's bytes staged in LDS by aligned 16-byte
//           loads when they fit q.stage; the threads' ranges tile the document, the smallest (offset, reason) wins;
//   place   the lists' headers (and with assign_too the lists to assign), the partitions' `in prevMap | never equal` bits,
//           and the summary words the host needs to finish the BatchDesc and to decide the BLANCE_WIRE_ADOPT_* codes.
// Nothing here uses a global atomic but the parser's own claim of a partition; every summary word is written by one thread
// with a plain store.  Every byte read is bounded by the document's length (WdSrc::at); the 16-byte loads stay inside the
// copy, which is padded to 16.
#pragma once

#ifndef BLANCE_SIMT_EMU
#define BLANCE_WD_NO_KERNELS          /* the decoder's own kernels belong to blance_hip.hip's translation unit */
#endif
#include "k_wire_decode.h"

namespace blance {

__device__ __forceinline__ unsigned long long bd_shfl_xor64(unsigned long long v, int o) {
    return ((unsigned long long)(unsigned)__shfl_xor((int)(unsigned)(v >> 32), o, 64) << 32) | (unsigned)__shfl_xor((int)(unsigned)v, o, 64);
}

// exclusive prefix of v over the workgroup's 256 threads, the sum of all to *total; tmp: 4 words of LDS
__device__ inline int bd_scan(int v, int* tmp, int tid, int* total) {
    int x = v;
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if ((tid & 63) >= o) x += y;
    }
    if ((tid & 63) == 63) tmp[tid >> 6] = x;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < (tid >> 6); w++) base += tmp[w];
    *total = tmp[0] + tmp[1] + tmp[2] + tmp[3];
    __syncthreads();                                         // (tmp is written again by the next scan)
    return base + x - v;
}

// the bytes [lo, hi) of a tile (lo a multiple of 16), `esc`: the first byte is escaped; f(offset, byte, is an unescaped quote)
template <class F>
__device__ inline void bd_walk(const unsigned char* doc, long long lo, long long hi, bool esc, F f) {
    for (long long b = lo; b < hi; b += 16) {
        WD_LOAD16(w, doc, b);
        const int n = hi - b < 16 ? (int)(hi - b) : 16;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const unsigned ch = (w[k >> 2] >> (8 * (k & 3))) & 255u;
            if (k < n) {
                bool quote = false;
                if (esc) esc = false;
                else if (ch == '\\') esc = true;
                else if (ch == '"') quote = true;
                f(b + k, ch, quote);
            }
        }
    }
}

__global__ __launch_bounds__(kBatchDecodeThreads) void k_batch_decode(BatchDecodeParams bp) {
    constexpr int T = kBatchDecodeThreads;
    const BatchDocDesc& E = bp.ddesc[blockIdx.x];
    const BatchDesc& D = bp.desc[E.desc];
    const int tid = (int)threadIdx.x;
    const int P = D.P, M = D.M, PM = D.P * D.M;
    int32_t* in = bp.in + D.in_base;
    int32_t* sc = bp.sc + D.sc_base;
    int32_t* sum = bp.sum + (size_t)blockIdx.x * kBdSumWords;
    const unsigned char* doc = bp.docs + E.doc_base;
    const long long len = E.len;
    int32_t* rec = sc + E.s_rec;

    BLANCE_DYN_LDS(lds);
    int* s_tb = (int*)lds;                                   // [T] backslashes at the tile's end
    int* s_full = s_tb + T;                                  // [T] the tile is backslashes only
    int* s_tmp = s_full + T;                                 // [4] bd_scan; [4..8) the carry of the escape parity
    unsigned long long (*red)[8] = (unsigned long long (*)[8])lds;   // [4 waves][8] the reductions (behind the split)
    unsigned char* stage = lds + kBatchDecodeLdsHead;

    // the document's scratch: claim, kinds and lengths zeroed (one run of words in front of the record starts)
    for (int i = E.s_claim + tid; i < E.s_rec; i += T) sc[i] = 0;

    // ---- split: the record starts (a hint; nothing below trusts them)
    const int tile = bp.tile;
    const long long n_tiles = (len + tile - 1) / tile;
    int c_esc = 0, c_quotes = 0, c_depth = 0, c_count = 0;   // the carry, the same in every thread
    for (long long t0 = 0; t0 < n_tiles; t0 += T) {
        const long long t = t0 + tid;
        const bool have = t < n_tiles;
        const long long lo = have ? t * tile : 0;
        const long long hi = have ? (lo + tile < len ? lo + tile : len) : 0;
        int nb = 0;
        for (long long i = hi - 1; i >= lo && doc[i] == '\\'; i--) nb++;
        s_tb[tid] = nb;
        s_full[tid] = have && nb == (int)(hi - lo);
        __syncthreads();
        int par = 0, u = tid - 1;                            // the parity of the backslash run in front of the tile
        for (; u >= 0; u--) {
            par ^= s_tb[u] & 1;
            if (!s_full[u]) break;
        }
        if (u < 0) par ^= c_esc;
        if (tid == T - 1) s_tmp[4] = (nb & 1) ^ (s_full[tid] ? par : 0);      // ... and behind the chunk
        int nq = 0;
        bd_walk(doc, lo, hi, par != 0, [&](long long, unsigned, bool quote) { nq += quote; });
        int total_q, total_d, total_c;
        bool in_str0 = (c_quotes + bd_scan(nq, s_tmp, tid, &total_q)) & 1;
        const int esc_next = s_tmp[4];                       // (read behind the scan's barriers)
        int dd = 0;
        bool in_str = in_str0;
        bd_walk(doc, lo, hi, par != 0, [&](long long, unsigned ch, bool quote) {
            if (quote) in_str = !in_str;
            else if (!in_str) {
                if (ch == '{' || ch == '[') dd++;
                else if (ch == '}' || ch == ']') dd--;
            }
        });
        const int d0 = c_depth + bd_scan(dd, s_tmp, tid, &total_d);
        int d = d0, n = 0;
        in_str = in_str0;
        bd_walk(doc, lo, hi, par != 0, [&](long long, unsigned ch, bool quote) {
            if (quote) {
                if (!in_str && d == 1) n++;
                in_str = !in_str;
            } else if (!in_str) {
                if (ch == '{' || ch == '[') d++;
                else if (ch == '}' || ch == ']') d--;
            }
        });
        const int base = c_count + bd_scan(n, s_tmp, tid, &total_c);
        d = d0; n = 0;
        in_str = in_str0;
        bd_walk(doc, lo, hi, par != 0, [&](long long at, unsigned ch, bool quote) {
            if (quote) {
                if (!in_str && d == 1) {
                    if (base + n >= 0 && base + n < E.rec_cap) rec[base + n] = (int32_t)at;
                    n++;
                }
                in_str = !in_str;
            } else if (!in_str) {
                if (ch == '{' || ch == '[') d++;
                else if (ch == '}' || ch == ']') d--;
            }
        });
        c_esc = esc_next;
        c_quotes = (c_quotes + total_q) & 1;
        c_depth += total_d;
        c_count += total_c;
        __syncthreads();                                     // (s_tb, s_full and the carry word are written again)
    }
    const int R = c_count < 0 ? 0 : c_count > E.rec_cap ? E.rec_cap : c_count;
    __syncthreads();                                         // the record starts and the zeroed scratch are seen

    // ---- parse: every record strictly, its node ids into its lists' rows
    WireDecodeParams q;
    q.doc = doc; q.len = (int32_t)len; q.tile = tile; q.n_tiles = (int32_t)n_tiles;
    q.tb = nullptr; q.qbits = nullptr; q.quotes = nullptr; q.depth = nullptr; q.count = nullptr;
    q.rec = rec; q.R = R; q.P = P; q.M = M; q.NX = D.NX; q.stage = bp.stage;
    {
        const int32_t* blk = in + E.i_dict;
        WdTable* tabs[3] = {&q.part, &q.node, &q.state};
        for (int k = 0; k < 3; k++)
            *tabs[k] = WdTable{blk + blk[4 * k], (uint32_t)blk[4 * k + 1], (const unsigned char*)(blk + blk[4 * k + 2]), blk + blk[4 * k + 3]};
    }
    q.claim = sc + E.s_claim;
    q.part_kind = (uint8_t*)(sc + E.s_pkind);
    q.kind = (uint8_t*)(sc + E.s_kind);
    q.off = sc + E.s_len;
    q.nodes = in + D.i_plist;
    q.row = kBatchMaxL;
    q.refusal = nullptr;
    unsigned long long refusal = ~0ull;
    for (int r0 = 0; r0 < (R > 0 ? R : 1); r0 += T) {
        const int r1 = r0 + T < R ? r0 + T : R;
        long long a0 = 0, hi = 0;
        if (r0 < r1) {                                       // (the same in every thread: the barriers are uniform)
            long long lo = rec[r0], end = r1 < R ? rec[r1] : len;
            if (end > len) end = len;
            if (lo >= 0 && lo < end && end - (lo & ~15ll) <= (long long)bp.stage) {
                a0 = lo & ~15ll;
                hi = end;
                for (long long i = (long long)tid * 16; i < end - a0; i += T * 16)
                    *(int4*)(stage + i) = *(const int4*)(doc + a0 + i);       // (the last load may pass `end`: inside the padded copy)
            }
        }
        __syncthreads();
        WdParse ps;
        ps.q = &q;
        ps.s = WdSrc{doc, stage, len, a0, hi};
        ps.reason = 0; ps.where = 0; ps.p = 0; ps.start = 0; ps.limit = len; ps.hit = false;
        bool ok = true;
        if (R == 0) {
            if (tid == 0) {
                ps.limit = len < kWdMaxRecord ? len : kWdMaxRecord;
                ok = wd_empty_document(ps);
            }
        } else if (r0 + tid < r1) {
            const int r = r0 + tid;
            ps.start = rec[r];
            ps.limit = ps.start + kWdMaxRecord < len ? ps.start + kWdMaxRecord : len;
            ok = wd_record<false>(ps, r);
        }
        if (!ok) {
            const unsigned long long mine = ((unsigned long long)ps.where << 8) | (unsigned long long)ps.reason;
            refusal = mine < refusal ? mine : refusal;
        }
        __syncthreads();                                     // (the stage is written again; behind the last run: the lists are seen)
    }

    // ---- place and sum
    const int L = D.L;                                       // (kBatchMaxL: a document problem's row stride)
    int longest = 0, fresh = 0, first_missing = INT_MAX, first_dup = INT_MAX, first_long = INT_MAX;
    unsigned long long refs = 0, cap = 0, aprev = 0;
    const int32_t* lens = sc + E.s_len;
    for (int idx = tid; idx < PM; idx += T) {
        const int n = lens[idx], kd = q.kind[idx];
        const int32_t* row = in + D.i_plist + (long long)idx * L;
        const int k = in[D.i_state + 4 * (idx % M) + 1];
        refs += (unsigned long long)n;
        longest = n > longest ? n : longest;
        cap += (unsigned long long)(n > k ? n : k);
        if (n > L) {
            first_long = idx < first_long ? idx : first_long;
            continue;                                        // (not planned here: the single path reads the bytes again)
        }
        in[D.i_phdr + idx] = n | (kd << 16);
        if (E.assign_too) {
            in[D.i_ahdr + idx] = n | (kd << 16);
            bool dup = false;
            for (int i = 0; i < n; i++) {
                const int32_t v = row[i];
                in[D.i_alist + (long long)idx * L + i] = v;
                for (int j = 0; j < i; j++) dup |= row[j] == v;
            }
            if (dup) first_dup = idx < first_dup ? idx : first_dup;
        }
    }
    for (int p = tid; p < P; p += T) {
        const int kd = q.part_kind[p];
        const int w0 = in[D.i_part + 2 * p + 1];
        in[D.i_part + 2 * p + 1] = (w0 & 1) | (kd != kListAbsent ? 2 : 0) | (kd == kListNil ? 4 : 0);
        if (kd == kListAbsent) {
            fresh++;
            first_missing = p < first_missing ? p : first_missing;
        } else {
            long long w = (!D.weights_nil && (w0 & 1)) ? (long long)in[D.i_part + 2 * p] : 1;
            if (w < 0) w = -w;
            long long entries = 0;
            for (int m = 0; m < M; m++) entries += lens[p * M + m];
            aprev += (unsigned long long)(w * entries);
        }
    }
    // wave totals by shuffles, the four waves through LDS, one plain store per word by thread 0
    for (int o = 32; o; o >>= 1) {
        int t = __shfl_xor(longest, o, 64);
        longest = t > longest ? t : longest;
        fresh += __shfl_xor(fresh, o, 64);
        t = __shfl_xor(first_missing, o, 64);
        first_missing = t < first_missing ? t : first_missing;
        t = __shfl_xor(first_dup, o, 64);
        first_dup = t < first_dup ? t : first_dup;
        t = __shfl_xor(first_long, o, 64);
        first_long = t < first_long ? t : first_long;
        const unsigned long long other = bd_shfl_xor64(refusal, o);
        refusal = other < refusal ? other : refusal;
        refs += bd_shfl_xor64(refs, o);
        cap += bd_shfl_xor64(cap, o);
        aprev += bd_shfl_xor64(aprev, o);
    }
    const int wv = tid >> 6;
    if ((tid & 63) == 0) {
        red[wv][0] = refusal; red[wv][1] = refs; red[wv][2] = cap; red[wv][3] = aprev;
        red[wv][4] = ((unsigned long long)(unsigned)longest << 32) | (unsigned)fresh;
        red[wv][5] = (unsigned long long)(unsigned)first_missing;
        red[wv][6] = (unsigned long long)(unsigned)first_dup;
        red[wv][7] = (unsigned long long)(unsigned)first_long;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w2 = 1; w2 < T / 64; w2++) {
            refusal = red[w2][0] < refusal ? red[w2][0] : refusal;
            refs += red[w2][1]; cap += red[w2][2]; aprev += red[w2][3];
            const int lg = (int)(red[w2][4] >> 32);
            longest = lg > longest ? lg : longest;
            fresh += (int)(unsigned)red[w2][4];
            first_missing = (int)red[w2][5] < first_missing ? (int)red[w2][5] : first_missing;
            first_dup = (int)red[w2][6] < first_dup ? (int)red[w2][6] : first_dup;
            first_long = (int)red[w2][7] < first_long ? (int)red[w2][7] : first_long;
        }
        sum[kBdRefusal] = (int32_t)(uint32_t)refusal;
        sum[kBdRefusal + 1] = (int32_t)(uint32_t)(refusal >> 32);
        sum[kBdRecords] = R;
        sum[kBdRefs] = refs > (unsigned long long)INT_MAX ? -1 : (int32_t)refs;
        sum[kBdLongest] = longest;
        sum[kBdFresh] = fresh;
        sum[kBdFirstMissing] = first_missing;
        sum[kBdFirstDup] = first_dup;
        sum[kBdFirstLong] = first_long;
        sum[9] = 0;
        sum[kBdCap] = (int32_t)(uint32_t)cap;
        sum[kBdCap + 1] = (int32_t)(uint32_t)(cap >> 32);
        sum[kBdPrevLoad] = (int32_t)(uint32_t)aprev;
        sum[kBdPrevLoad + 1] = (int32_t)(uint32_t)(aprev >> 32);
        sum[14] = sum[15] = 0;
    }
}

}  // namespace blance
