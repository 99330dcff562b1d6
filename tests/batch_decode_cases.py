"""k_batch_decode alone (blance_amd/csrc/k_batch_decode.h) on documents, dictionary blocks and packed input slices made by hand:
the cases, the definition in numpy and the check, shared by tests/test_plan_batch_docs_kernels_emulated.py (the SIMT emulator),
tests/test_plan_batch_docs_kernels_gpu.py (the device) and the stand-alone sanitizer program
(tests/simt/batch_decode_asan_main.cpp reads what write_program_input writes).

A world is a few problems with one document each, every slice poisoned.  What the kernel owns: in the input slice the prevMap
rows and headers, with assign_too the rows and headers to assign, and the flag word of every partition; in scratch the run
of words from s_claim to s_rec (zeroed, then claim, kinds and lengths) and the first R record starts; the 16 summary words.
Every other word must come back as it went in.  The record starts are compared with the sequential definition
(wire_decode_cases.split_reference) for every document, refused ones included; an accepted document's lists, kinds, headers
and summary words with what json.loads makes of it."""
import ctypes as C
import json
import random

import numpy as np

import wire_decode_cases as WD
from blance_amd import abi

POISON = -0x35353536                                     # 0xCACACACA as int32
INT_MAX = 2 ** 31 - 1
L = 8                                                    # kBatchMaxL
HDR = 16                                                 # kBatchDictHdr
SUM = 16                                                 # kBdSumWords
STATES, NODES = WD.STATES, WD.NODES                      # (the decoder's own documents name these)


def fnv(raw):
    h = 2166136261
    for x in raw:
        h = ((h ^ x) * 16777619) & 0xFFFFFFFF
    h ^= len(raw)
    h ^= h >> 15
    return h


def r4(n):
    return (n + 3) & ~3


def dict_block(parts, nodes, states):
    """The words of a blance_batch_dict (blance_kernels.h: kBatchDictHdr): per kind slots, offsets, raw bytes."""
    words = [0] * HDR
    for k, names in enumerate((parts, nodes, states)):
        raw = [x.encode("utf-8") for x in names]
        cap = 2
        while cap < 2 * len(raw):
            cap <<= 1
        slots = [-1] * (2 * cap)
        for i, b in enumerate(raw):
            h = fnv(b)
            at = h & (cap - 1)
            while slots[2 * at] >= 0:
                at = (at + 1) & (cap - 1)
            slots[2 * at], slots[2 * at + 1] = i, h - (1 << 32) if h >= 1 << 31 else h
        off = [0]
        for b in raw:
            off.append(off[-1] + len(b))
        blob = b"".join(raw)
        blob += b"\0" * (-len(blob) % 4)
        words[4 * k], words[4 * k + 1], words[12 + k] = len(words), cap - 1, len(raw)
        words += slots + [0] * (r4(len(slots)) - len(slots))
        words[4 * k + 3] = len(words)
        words += off + [0] * (r4(len(off)) - len(off))
        words[4 * k + 2] = len(words)
        bw = np.frombuffer(blob, dtype=np.int32).tolist()
        words += bw + [0] * (r4(len(bw)) - len(bw))
    return words


class Problem:
    def __init__(self, rng, parts, doc, assign_too, pmap=None, refusal=None, weights_nil=False):
        self.parts, self.doc, self.assign_too, self.pmap, self.refusal = parts, doc, assign_too, pmap, refusal
        self.P, self.M, self.NX = len(parts), len(STATES), len(NODES)
        self.weights_nil = weights_nil
        self.k = [rng.choice([0, 1, 2, 3, -1]) for _ in range(self.M)]
        self.weight = [rng.randrange(-5, 40) for _ in range(self.P)]
        self.flags = [rng.randrange(8) for _ in range(self.P)]   # has weight | stale in prevMap / never equal bits


class World:
    """nb problems with a document each, laid out as the host lays a batch out, with poisoned gaps between all regions."""

    def __init__(self, problems, tile, stage):
        self.problems, self.tile, self.stage = problems, tile, stage
        self.shape, self.ddesc = [], []
        inw, scw, docs = [], [], b""
        for j, pb in enumerate(problems):
            P, M, PM = pb.P, pb.M, pb.P * pb.M
            in_base = len(inw) + 5                           # (a gap of poison in front of every slice)
            inw += [POISON] * 5
            at = 0

            def take(n, gap=3):
                nonlocal at
                first = at
                at += n + gap
                return first
            i_state, i_part = take(4 * M), take(2 * P)
            i_alist, i_ahdr, i_plist, i_phdr = take(PM * L), take(PM), take(PM * L), take(PM)
            at = r4(at)
            i_dict = at
            sl = [POISON] * at
            for m in range(M):
                sl[i_state + 4 * m:i_state + 4 * m + 4] = [m, pb.k[m], 0, 0]
            for p in range(P):
                sl[i_part + 2 * p], sl[i_part + 2 * p + 1] = pb.weight[p], pb.flags[p]
            sl += dict_block(pb.parts, NODES, STATES)
            inw += sl
            sc_base = len(scw) + 7
            scw += [POISON] * 7
            s_claim = 2
            s_pkind = s_claim + r4(P)
            s_kind = s_pkind + r4((P + 3) // 4)
            s_len = s_kind + r4((PM + 3) // 4)
            s_rec = s_len + r4(PM + 1)
            rec_cap = (len(pb.doc) + 1) // 2 + 1
            scw += [POISON] * (s_rec + rec_cap + 4)
            doc_base = len(docs)
            docs += pb.doc + b"\0" * (-len(pb.doc) % 16)
            self.shape.append([P, M, pb.NX, int(pb.weights_nil), in_base, sc_base, i_state, i_part, i_alist, i_ahdr, i_plist, i_phdr])
            self.ddesc.append([j, len(pb.doc), doc_base, i_dict, int(pb.assign_too), s_claim, s_pkind, s_kind, s_len, s_rec, rec_cap])
        self.inw = np.asarray(inw + [POISON] * 6, dtype=np.int32)
        self.scw = np.asarray(scw + [POISON] * 6, dtype=np.int32)
        self.docs = np.frombuffer(docs + b"\0" * 16, dtype=np.uint8).copy()

    def run(self, lib):
        nb = len(self.problems)
        shape = np.asarray(self.shape, dtype=np.int32)
        ddesc = np.asarray(self.ddesc, dtype=np.int32)
        inw, scw = self.inw.copy(), self.scw.copy()
        summ = np.full(nb * SUM, POISON, dtype=np.int32)
        i32p = C.POINTER(C.c_int32)
        lib.blance_case_batch_decode.restype = C.c_int
        lib.blance_case_batch_decode.argtypes = [C.c_int, i32p, C.c_int, i32p, i32p, C.c_longlong, i32p, C.c_longlong,
                                                 C.POINTER(C.c_ubyte), C.c_longlong, i32p, C.c_int, C.c_int]
        st = lib.blance_case_batch_decode(nb, shape.ctypes.data_as(i32p), nb, ddesc.ctypes.data_as(i32p), inw.ctypes.data_as(i32p),
                                          len(inw), scw.ctypes.data_as(i32p), len(scw), self.docs.ctypes.data_as(C.POINTER(C.c_ubyte)),
                                          len(self.docs) - 16, summ.ctypes.data_as(i32p), self.tile, self.stage)
        assert st == 0, st
        return inw, scw, summ

    def expected(self):
        """(in, in mask, sc, sc mask, sum, sum mask): the words the definition fixes (mask 1) and their values."""
        inw, scw = self.inw.copy(), self.scw.copy()
        in_m, sc_m = np.ones(len(inw), dtype=bool), np.ones(len(scw), dtype=bool)
        nb = len(self.problems)
        summ, sum_m = np.zeros(nb * SUM, dtype=np.int32), np.ones(nb * SUM, dtype=bool)
        for j, pb in enumerate(self.problems):
            P, M, PM = pb.P, pb.M, pb.P * pb.M
            _, _, _, _, in_base, sc_base, i_state, i_part, i_alist, i_ahdr, i_plist, i_phdr = self.shape[j]
            _, _, _, _, _, s_claim, s_pkind, s_kind, s_len, s_rec, rec_cap = self.ddesc[j]
            starts = WD.split_reference(pb.doc, self.tile)[3]
            R = len(starts)
            scw[sc_base + s_rec:sc_base + s_rec + R] = starts
            sc = scw[sc_base:]
            s = summ[j * SUM:(j + 1) * SUM]
            s[2] = R
            if pb.pmap is None:                              # refused: the smallest (offset, reason); the lists are anyone's
                in_m[in_base + i_plist:in_base + i_plist + PM * L] = False
                in_m[in_base + i_phdr:in_base + i_phdr + PM] = False
                in_m[in_base + i_part + 1:in_base + i_part + 2 * P:2] = False
                if pb.assign_too:
                    in_m[in_base + i_alist:in_base + i_alist + PM * L] = False
                    in_m[in_base + i_ahdr:in_base + i_ahdr + PM] = False
                sc_m[sc_base + s_claim:sc_base + s_rec] = False
                sum_m[j * SUM:(j + 1) * SUM] = False
                sum_m[j * SUM + 2] = True
                sum_m[j * SUM + 9], sum_m[j * SUM + 14], sum_m[j * SUM + 15] = True, True, True
                continue
            s[0] = s[1] = -1
            sc[s_claim:s_rec] = 0
            pid = {name: i for i, name in enumerate(pb.parts)}
            nid = {name: i for i, name in enumerate(NODES)}
            order = [pid[json.loads(pb.doc[a:pb.doc.index(b":", _key_end(pb.doc, a))].decode("utf-8", "surrogatepass"))] for a in starts]
            for r, p in enumerate(order):
                sc[s_claim + p] = INT_MAX - r
            pkind = np.zeros(r4((P + 3) // 4) * 4, dtype=np.uint8)
            kind = np.zeros(r4((PM + 3) // 4) * 4, dtype=np.uint8)
            lens = np.zeros(PM + 1, dtype=np.int32)
            ins = inw[in_base:]
            longest = fresh = refs = cap = aprev = 0
            first_missing = first_dup = first_long = INT_MAX
            for p, name in enumerate(pb.parts):
                w0 = pb.flags[p]
                if name not in pb.pmap:
                    fresh += 1
                    first_missing = min(first_missing, p)
                    ins[i_part + 2 * p + 1] = w0 & 1
                else:
                    nbs = pb.pmap[name]["nodesByState"]
                    pkind[p] = 1 if nbs is None else 2
                    ins[i_part + 2 * p + 1] = (w0 & 1) | 2 | (4 if nbs is None else 0)
                    entries = 0
                    for m, sname in enumerate(STATES):
                        if nbs is None or sname not in nbs:
                            continue
                        idx = p * M + m
                        lst = nbs[sname]
                        kind[idx] = 1 if lst is None else 2
                        ids = [nid[x] for x in (lst or [])]
                        lens[idx] = len(ids)
                        entries += len(ids)
                        ins[i_plist + idx * L:i_plist + idx * L + min(len(ids), L)] = ids[:L]
                    w = 1 if pb.weights_nil or not (w0 & 1) else abs(pb.weight[p])
                    aprev += w * entries
            for idx in range(PM):
                n, kd = int(lens[idx]), int(kind[idx])
                refs += n
                longest = max(longest, n)
                cap += max(n, pb.k[idx % M])
                if n > L:
                    first_long = min(first_long, idx)
                    continue
                ins[i_phdr + idx] = n | (kd << 16)
                if pb.assign_too:
                    ins[i_ahdr + idx] = n | (kd << 16)
                    row = ins[i_plist + idx * L:i_plist + idx * L + n].copy()
                    ins[i_alist + idx * L:i_alist + idx * L + n] = row
                    if len(set(row.tolist())) != n:
                        first_dup = min(first_dup, idx)
            sc[s_pkind:s_pkind + len(pkind) // 4] = pkind.view(np.int32)
            sc[s_kind:s_kind + len(kind) // 4] = kind.view(np.int32)
            sc[s_len:s_len + PM + 1] = lens
            s[3:9] = [refs, longest, fresh, first_missing, first_dup, first_long]
            s[10], s[11] = _lo(cap), cap >> 32
            s[12], s[13] = _lo(aprev), aprev >> 32
        return inw, in_m, scw, sc_m, summ, sum_m


def _lo(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= 1 << 31 else v


def _key_end(doc, a):
    """The closing quote of the string that opens at a."""
    i = a + 1
    while doc[i] != 0x22:
        i += 2 if doc[i] == 0x5C else 1
    return i


def random_pmap(rng, parts, share=0.8, long_lists=False, dups=False):
    pmap = {}
    for name in parts:
        if rng.random() > share:
            continue
        nbs = None
        if rng.randrange(6):
            nbs = {}
            for s in rng.sample(STATES, rng.randrange(len(STATES) + 1)):
                k = rng.randrange(6)
                n = 0 if k == 1 else rng.randrange(1, 11 if long_lists else 9)
                nbs[s] = None if k == 0 else (rng.sample(NODES, n) if not dups else [rng.choice(NODES[:6]) for _ in range(n)])
        pmap[name] = {"name": name, "nodesByState": nbs}
    return pmap


def worlds():
    rng = random.Random(11)
    out = {}
    special = WD.SPECIAL[:18]

    def accepted(P, assign_too, **kw):
        parts = ["p%d" % i for i in range(P - min(P, len(special)))] + special[:min(P, len(special))]
        weights_nil = kw.pop("weights_nil", False)
        pmap = random_pmap(rng, parts, **kw)
        return Problem(rng, parts, WD.render(rng, pmap), assign_too, pmap, weights_nil=weights_nil)

    for tile, stage in ((64, 64), (64, 256), (256, 32768)):
        out["sizes_tile%d_stage%d" % (tile, stage)] = World(
            [accepted(P, i % 2 == 0, share=1.0 if i % 3 == 0 else 0.8) for i, P in enumerate((0, 1, 2, 255, 256, 257, 513))], tile, stage)
    out["long_lists_and_duplicates"] = World([accepted(40, True, long_lists=True), accepted(40, True, dups=True),
                                              accepted(40, False, dups=True, long_lists=True), accepted(30, True, weights_nil=True)], 64, 32768)
    out["empty_documents"] = World([Problem(rng, ["p0", "p1"], b"{}", True, {}), Problem(rng, ["p0"], b" \n{\t} ", False, {}),
                                    Problem(rng, [], b"{}", True, {})], 64, 64)
    # the chunk of 256 tiles: a document longer than 256 * 64 bytes, the carry of all four values
    parts = ["p%d" % i for i in range(600)]
    pmap = random_pmap(rng, parts, share=1.0)
    assert len(WD.render(random.Random(3), pmap)) > 3 * 256 * 64
    out["chunks"] = World([Problem(rng, parts, WD.render(random.Random(3), pmap), True, pmap)], 64, 256)
    # a run of 600 backslashes (a name of 300) lying over the chunk seam at 256 * 64 bytes, even and odd (a quote behind it),
    # with the seam at several places inside the run: the carry of the escape parity
    seam = 256 * 64
    carry = []
    for name in ("\\" * 300, "\\" * 300 + '"'):
        for back in (1, 2, 301, 599):
            pm = {name: {"name": name, "nodesByState": {"primary": ["a", "b"]}}, "p1": {"name": "p1", "nodesByState": None}}
            rec = WD.record(name, {"primary": ["a", "b"]})
            lead = seam - 1 - back                           # the key's opening quote; its backslashes begin one byte on
            doc = b"{" + b" " * (lead - 1) + rec + b" , " + WD.record("p1") + b"\n}"
            assert doc[lead:lead + 2] == b'"\\' and doc[seam - 1:seam + 1] == b"\\\\"
            carry.append(Problem(rng, [name, "p1", "p2"], doc, len(carry) % 2 == 0, pm))
    out["escape_carry"] = World(carry, 64, 256)
    # every length residue mod 16
    base_map = random_pmap(rng, ["p%d" % i for i in range(5)], share=1.0)
    base = WD.render(random.Random(4), base_map).rstrip()
    out["residues"] = World([Problem(rng, ["p%d" % i for i in range(5)], base + b" " * k, k % 2 == 0, base_map) for k in range(16)], 64, 64)
    # refused documents: the record starts and the untouched words are still checked
    bad = []
    for tag, doc, reason, lo, hi in WD.refusal_documents(64)[::4]:
        bad.append(Problem(rng, WD.PARTS[:8], doc, len(bad) % 2 == 0, None, refusal=(reason, lo, hi)))
    out["refused"] = World(bad, 64, 256)
    return out


def check(lib, world):
    inw, scw, summ = world.run(lib)
    want_in, in_m, want_sc, sc_m, want_sum, sum_m = world.expected()
    bad = np.flatnonzero((inw != want_in) & in_m)
    assert bad.size == 0, ("input slices", bad[:8], inw[bad[:8]], want_in[bad[:8]])
    bad = np.flatnonzero((scw != want_sc) & sc_m)
    assert bad.size == 0, ("scratch", bad[:8], scw[bad[:8]], want_sc[bad[:8]])
    bad = np.flatnonzero((summ != want_sum) & sum_m)
    assert bad.size == 0, ("summary", bad[:8], summ[bad[:8]], want_sum[bad[:8]])
    for j, pb in enumerate(world.problems):
        if pb.refusal:
            word = (int(summ[j * SUM]) & 0xFFFFFFFF) | (int(summ[j * SUM + 1]) << 32)
            reason, lo, hi = pb.refusal
            assert word & 255 == abi.WIRE_REFUSED[reason] and lo <= word >> 8 < hi, (j, reason, word & 255, word >> 8, lo, hi)


def write_program_input(path, ws):
    """Every world for the stand-alone sanitizer program: `W nb tile stage`, then one line per array (decimal words)."""
    with open(path, "w") as f:
        for name in sorted(ws):
            w = ws[name]
            want_in, in_m, want_sc, sc_m, want_sum, sum_m = w.expected()
            f.write("W %d %d %d\n" % (len(w.problems), w.tile, w.stage))
            for tag, a in (("shape", np.asarray(w.shape).ravel()), ("ddesc", np.asarray(w.ddesc).ravel()), ("in", w.inw), ("sc", w.scw),
                           ("docs", w.docs), ("want_in", want_in), ("mask_in", in_m.astype(np.int32)), ("want_sc", want_sc),
                           ("mask_sc", sc_m.astype(np.int32)), ("want_sum", want_sum), ("mask_sum", sum_m.astype(np.int32))):
                f.write(tag + " " + " ".join(str(int(x)) for x in a) + "\n")
