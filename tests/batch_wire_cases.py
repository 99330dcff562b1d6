"""k_batch_wire_size and k_batch_wire_write alone (blance_amd/csrc/k_batch_wire.h): hand-made result CSRs and names blocks, the
definition the kernels' words are compared with, and the check.  tests/kernels/batch_wire_cases.inc is the entry; the emulator
(tests/test_plan_batch_wire_kernels_emulated.py), its stand-alone sanitizer program and the device
(tests/test_plan_batch_wire_kernels_gpu.py) run the same cases.

A case is a `world`: a few problems with their three slices laid out by hand, poison in every word no table owns.  The
definition of a document is the host encoder's (wire.encode) on the map the CSR spells, nil lists (`null`) among them -- no
plan was found to produce one, so only hand-made lists reach that branch.  What a kernel does not own must come back as it
went in: the scratch outside the [P + 1] offsets of an asking, finished problem; the output slices but for the length word;
the 0 to 15 bytes between two documents and everything behind the last."""
import ctypes

import numpy as np

from blance_amd import wire

ABSENT, NIL, SET = 0, 1, 2
HDR = 8                                  # kBatchHdr, and kBatchNamesHdr
POISON32, POISON8 = -0x5A5A5A5B, 0xAB
SHAPE = 9


def _quoted(strs, tail=b""):
    parts = [b'"' + s.encode() + b'"' + tail for s in strs]
    off = np.zeros(len(parts) + 1, np.int32)
    off[1:] = np.cumsum([len(x) for x in parts])
    return b"".join(parts), off


def names_block(part_names, node_names, state_names):
    """The words of a blance_batch_names for names that need no escape: the header (word offsets of the eight tables), then
    order [P], part_off [P + 1] by rank, node_off [NX + 1], state_off [M + 1], state_id [M], the three blobs of escaped bytes;
    every table at a multiple of 4 words."""
    order = sorted(range(len(part_names)), key=lambda p: part_names[p].encode())
    sorder = sorted(range(len(state_names)), key=lambda m: state_names[m].encode())
    pesc, poff = _quoted([part_names[p] for p in order])
    nesc, noff = _quoted(node_names)
    sesc, soff = _quoted([state_names[m] for m in sorder], b":")
    tables = [np.asarray(order, np.int32), poff, noff, soff, np.asarray(sorder, np.int32)]
    for blob in (pesc, nesc, sesc):
        tables.append(np.frombuffer(blob + b"\0" * (-len(blob) % 4), np.uint8).view(np.int32))
    at, words = [], HDR
    for t in tables:
        at.append(words)
        words += (len(t) + 3) & ~3
    block = np.zeros(words, np.int32)
    block[:HDR] = at
    for a, t in zip(at, tables):
        block[a:a + len(t)] = t
    return block, order


class Problem:
    def __init__(self, P, M, NX, L, seed, part_names=None, node_names=None, state_names=None, done=1, err=0, iterations=1,
                 ask=True):
        rng = np.random.RandomState(seed)
        self.P, self.M, self.NX, self.ask = P, M, NX, ask
        self.header = (iterations, err, done)
        self.part_names = part_names or ["p%d" % ((p * 7919) % 10007) for p in range(P)]    # id order is not byte order
        assert len(set(self.part_names)) == P
        self.node_names = node_names or ["n%d" % i + "w" * (rng.randint(0, 4) * 9) for i in range(NX)]
        self.state_names = state_names or ["replica", "primary", "spare", "dead"][:M]
        self.kind = rng.choice([ABSENT, NIL, SET], size=P * M, p=[0.2, 0.2, 0.6]).astype(np.int32)
        if P * M >= 4:
            self.kind[:M] = NIL                               # a partition of nil lists only
            self.kind[-1] = NIL
        length = np.where(self.kind == SET, rng.randint(0, L + 1, size=P * M), 0)
        self.off = np.zeros(P * M + 1, np.int32)
        self.off[1:] = np.cumsum(length)
        self.nodes = rng.randint(0, NX, size=max(int(self.off[-1]), 1)).astype(np.int32)
        self.skipped = done != 1 or err != 0 or iterations == 0

    def pmap(self):
        out = {}
        for p, name in enumerate(self.part_names):
            nbs = {}
            for m, s in enumerate(self.state_names):
                i = p * self.M + m
                if self.kind[i] != ABSENT:
                    nbs[s] = None if self.kind[i] == NIL else [self.node_names[x] for x in self.nodes[self.off[i]:self.off[i + 1]]]
            out[name] = {"name": name, "nodesByState": nbs}
        return out

    def piece_offsets(self):
        pm = self.pmap()
        keys = sorted(pm, key=lambda k: k.encode())
        lens = [len(wire.encode({k: pm[k]})) - 1 for k in keys]
        lens[-1] += 1
        return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


class World:
    """The blocks of one call and what they must be afterwards."""

    def __init__(self, problems, stage=32768):
        self.problems, self.stage = problems, stage
        shape, wdesc, ins, scs, outs = [], [], [], [], []
        in_at = sc_at = out_at = 0
        self.docs, want_len = [], []
        for i, pb in enumerate(problems):
            PM = pb.P * pb.M
            pad = 4 * (1 + i % 3)                              # (the packed problem stands in front of the names: poison here)
            block, _ = names_block(pb.part_names, pb.node_names, pb.state_names)
            o_off, o_kind = HDR, HDR + ((PM + 1 + 3) & ~3)
            o_nodes = o_kind + ((PM + 3) & ~3)
            o_total = o_nodes + ((len(pb.nodes) + 3) & ~3) + 4 * (i % 2)
            out = np.full(o_total + 4, POISON32, np.int32)
            out[:HDR] = 0
            out[0], out[4], out[5] = pb.header
            out[o_off:o_off + PM + 1] = pb.off
            out[o_kind:o_kind + PM] = pb.kind
            out[o_nodes:o_nodes + len(pb.nodes)] = pb.nodes
            s_len = 4 * (i % 4)
            sc = np.full(s_len + ((pb.P + 1 + 3) & ~3) + 4, POISON32, np.int32)
            shape.append([pb.P, pb.M, pb.NX, in_at, sc_at, out_at, o_off, o_kind, o_nodes])
            if pb.ask:
                wdesc.append([i, pad, s_len, o_total])
                doc = None if pb.skipped else wire.encode(pb.pmap())
                self.docs.append(doc)
                want_len.append((sc_at + s_len, None if pb.skipped else pb.piece_offsets(), out_at + o_total))
            ins.append(np.concatenate([np.full(pad, POISON32, np.int32), block]))
            scs.append(sc)
            outs.append(out)
            in_at += len(ins[-1]); sc_at += len(sc); out_at += len(out)
        self.shape = np.asarray(shape, np.int32).reshape(-1)
        self.wdesc = np.asarray(wdesc, np.int32).reshape(-1)
        self.nb, self.nw = len(problems), len(wdesc)
        self.inp, self.sc, self.out = np.concatenate(ins), np.concatenate(scs), np.concatenate(outs)
        self.total = np.full(self.nw, POISON32, np.int32)
        rounded = [0 if d is None else (len(d) + 15) & ~15 for d in self.docs]
        self.doc = np.full(sum(rounded) + 48, POISON8, np.uint8)
        # afterwards
        self.want_sc, self.want_out = self.sc.copy(), self.out.copy()
        self.want_total = np.asarray(rounded, np.int32)
        self.want_doc = self.doc.copy()
        base = 0
        for (sc_w, offs, tot_w), d, r in zip(want_len, self.docs, rounded):
            self.want_out[tot_w] = 0 if d is None else len(d)
            if d is not None:
                assert offs[-1] == len(d)
                self.want_sc[sc_w:sc_w + len(offs)] = offs
                self.want_doc[base:base + len(d)] = np.frombuffer(d, np.uint8)
            base += r

    def arrays(self, which=3):
        """The _io arrays as the call gets them: poisoned, or (which == 2) with what k_batch_wire_size leaves."""
        first = which & 1
        return ((self.sc if first else self.want_sc).copy(), (self.out if first else self.want_out).copy(),
                (self.total if first else self.want_total).copy(), self.doc.copy())

    def wanted(self, which=3):
        return self.want_sc, self.want_out, self.want_total, (self.want_doc if which & 2 else self.doc)


def _aligned_copy(a):
    """A copy of the bytes at a 16-byte aligned address (the document buffer is 16-byte aligned on the device)."""
    raw = np.empty(a.nbytes + 16, np.uint8)
    skip = (-raw.ctypes.data) % 16
    out = raw[skip:skip + a.nbytes]
    out[:] = a
    return out


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def run(lib, w, which=3):
    sc, out, total, doc = w.arrays(which)
    doc = _aligned_copy(doc)
    lib.blance_case_batch_wire.restype = ctypes.c_int
    st = lib.blance_case_batch_wire(w.nb, _p(w.shape), w.nw, _p(w.wdesc), _p(w.inp), ctypes.c_longlong(len(w.inp)),
                                    _p(sc), ctypes.c_longlong(len(sc)), _p(out), ctypes.c_longlong(len(out)), _p(total),
                                    _p(doc), ctypes.c_longlong(len(doc)), w.stage, which)
    return st, (sc, out, total, doc)


def check(lib, w, which=3):
    st, got = run(lib, w, which)
    assert st == 0, st
    for name, g, want in zip(("scratch", "output", "wire_total", "documents"), got, w.wanted(which)):
        bad = np.nonzero(g != want)[0]
        assert bad.size == 0, (name, which, bad[:8].tolist(), g[bad[:8]].tolist(), want[bad[:8]].tolist())


def long_names(P, at, n):
    names = ["k%03d" % p for p in range(P)]
    names[at] = "L" * n
    return names


def worlds():
    """name -> World.  Both kernels see: one partition and two; the seams of the 256-rank run and of the scan's chunks; nil,
    empty, absent and full lists; a problem that does not ask between two that do; problems the plan kernel did not finish
    (not done, an error, no sweep) between finished ones; 256 nodes with names of very different lengths; small stages with
    a partition larger than the stage; documents whose lengths leave every gap from 0 to 15 bytes."""
    out = {}
    out["mixed"] = World([Problem(1, 1, 1, 2, 1), Problem(2, 2, 3, 3, 2), Problem(40, 3, 5, 2, 3, done=0),
                          Problem(257, 3, 5, 2, 4), Problem(9, 2, 4, 2, 5, ask=False), Problem(30, 2, 7, 2, 6, err=2),
                          Problem(12, 4, 9, 8, 7), Problem(5, 1, 2, 1, 8, iterations=0), Problem(3, 2, 2, 2, 9)])
    out["seams"] = World([Problem(255, 2, 256, 3, 11), Problem(256, 1, 64, 2, 12), Problem(513, 2, 65, 2, 13)])
    out["skipped_first_and_last"] = World([Problem(4, 2, 3, 2, 21, done=0), Problem(6, 2, 3, 2, 22), Problem(4, 2, 3, 2, 23, err=1)])
    for stage in (64, 128, 256):
        out["stage_%d" % stage] = World([Problem(20, 1, 3, 1, 31, part_names=long_names(20, 7, 3)),
                                        Problem(300, 2, 6, 2, 32, part_names=long_names(300, 150, 500)),
                                        Problem(3, 1, 2, 1, 33, part_names=["b", "a" * 1200, "c"])], stage=stage)
    # the same lists under names of 1 to 16 bytes (a name is written twice) and two state names (written once per list kept):
    # one problem for each gap of 0 to 15 bytes behind a document
    by_gap = {}
    for k in range(32):
        pb = Problem(3, 1, 2, 1, 46, part_names=["a", "b", "c" * (1 + k // 2)], state_names=["s" * (1 + k % 2)])
        by_gap.setdefault((-len(wire.encode(pb.pmap()))) % 16, pb)
    out["every_gap"] = World([by_gap[g] for g in sorted(by_gap)])
    return out


def gaps_seen(w):
    return {(-len(d)) % 16 for d in w.docs if d is not None}


def write_program_input(path, runs):
    """The cases as text for the stand-alone program: per run a line `C nb nw stage which`, then one line per array."""
    with open(path, "w") as f:
        for w, which in runs:
            sc, out, total, doc = w.arrays(which)
            wsc, wout, wtotal, wdoc = w.wanted(which)
            f.write("C %d %d %d %d\n" % (w.nb, w.nw, w.stage, which))
            for tag, a in (("shape", w.shape), ("wdesc", w.wdesc), ("in", w.inp), ("sc", sc), ("out", out), ("total", total),
                           ("doc", doc), ("want_sc", wsc), ("want_out", wout), ("want_total", wtotal), ("want_doc", wdoc)):
                f.write(tag + " " + " ".join(map(str, np.asarray(a).astype(np.int64).tolist())) + "\n")
