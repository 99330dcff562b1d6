"""The upload's analysis alone (blance_amd/csrc/host/problem_facts.hpp): node_facts, order_facts, leaf_tables and analyse_rule
through a stand-alone program (tests/simt/problem_facts_main.cpp, plain g++, no HIP), built twice -- plain, and under
AddressSanitizer and UBSan -- and compared with references written here from the definitions, in plain Python.

What these functions decide is which kernels run: a wrong `ok = false`, `cls_run = 0` or `cyc_ok = false` leaves every plan
bit-identical to the oracle on a slower path, so no test of whole plans can see it.  The cases are each the smallest world
where one decision can go wrong.  The k_cycle.h tables are also compared with tests/cycle_case_tables.py::tables, the builder
the single-kernel suites feed their kernels from.

Mutants of problem_facts.hpp applied by hand, and what failed then:
  cls_run without its alignment term `(cl[i].first - lo) % sz`   -> test_regions[class_at_an_odd_offset]
  `>=` for `>` at kChainMaxLeaves                                -> test_regions[region_of_512]
  chunk count size / 64 (for ch * 64 < size)                     -> test_stay_work_table, and every test with a region under 64 leaves
  last[g] counted for a <= part                                  -> test_cycle_tables, and every test whose P is no multiple of n_alive
  uniform_all without all_alive_added                            -> test_order_truth_table
(each in both builds; the other tests passed under each mutant)
"""
import fcntl
import itertools
import os
import subprocess

import numpy as np
import pytest

import cycle_case_tables as CT

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "simt", "problem_facts_main.cpp")
HDRS = [os.path.join(HERE, "..", "blance_amd", "csrc", "host", "problem_facts.hpp"),
        os.path.join(HERE, "..", "blance_amd", "csrc", "blance_kernels.h"), os.path.join(HERE, "..", "include", "blance_hip.h")]
EXE = os.path.join(HERE, "simt", "_build", "problem_facts")
SANITIZE = ["-fsanitize=address,undefined", "-static-libasan", "-static-libubsan"]     # the runtimes inside the program
CHAIN_MAX_LEAVES, CYC_WORDS = 512, 4                                                   # blance_kernels.h


# ---- the two builds ---------------------------------------------------------------------------------------------------------

def build_program(sanitized):
    """The program, or (None, why) when a sanitized program does not link or start here."""
    exe = EXE + ("_asan" if sanitized else "")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    with open(exe + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if os.path.exists(exe) and all(os.path.getmtime(d) <= os.path.getmtime(exe) for d in [SRC] + HDRS):
            return exe, ""
        flags = []
        if sanitized:
            probe = subprocess.run(["g++"] + SANITIZE + ["-x", "c++", "-", "-o", exe + ".probe"], input="int main(){return 0;}\n",
                                   capture_output=True, text=True)
            if probe.returncode != 0:
                return None, probe.stderr[-400:]
            started = subprocess.run([exe + ".probe"], capture_output=True, text=True)
            os.remove(exe + ".probe")
            if started.returncode != 0:
                return None, "the program does not start: " + started.stderr[-400:]
            flags = ["-g1"] + SANITIZE + ["-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
        tmp = "%s.%d.tmp" % (exe, os.getpid())
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", tmp, SRC])
        os.replace(tmp, exe)
    return exe, ""


# ---- worlds -----------------------------------------------------------------------------------------------------------------

class World:
    """A blance_problem's node, hierarchy and rule arrays.  tree: nested lists; an int is the leaf of that node, None a leaf
    without a node, ("at", n, [children...]) an inner vertex that is node n itself.  Vertices 0 .. NX - 1 are the nodes, the
    inner vertices and the other leaves follow, the vertex of "" is last; a root's parent is "" (findAncestor of a missing
    key)."""

    def __init__(self, NX, tree=None, rules=(), N=None, P=100, na=0, removed=(), added=(), add_nil=0, weights=(),
                 prio=(0, 1), top=0):
        self.NX, self.N, self.P, self.na, self.add_nil = NX, NX if N is None else N, P, na, add_nil
        self.prio, self.top, self.rules = list(prio), top, list(rules)
        self.removed = np.zeros(NX, np.uint8); self.removed[list(removed)] = 1
        self.added = np.zeros(NX, np.uint8); self.added[list(added)] = 1
        self.has_weight = np.zeros(NX, np.uint8); self.has_weight[list(weights)] = 1
        self.leaf_pos = np.full(NX, -1, np.int32)
        self.parent, self.lo, self.hi = {}, {}, {}
        self.n_vertices = NX
        self.pos = 0
        if tree is not None:
            for root in tree:
                self._walk(root, None)
            self.empty = self._vertex()
            self.lo[self.empty], self.hi[self.empty] = self.pos, self.pos + 1
            for n in range(NX):                        # a node the hierarchy does not name: a root and its own leaf
                if n not in self.lo:
                    self.pos += 1
                    self.lo[n], self.hi[n], self.leaf_pos[n] = self.pos, self.pos + 1, self.pos
            self.pos += 1
        self.hier_nil = int(tree is None)

    def _vertex(self):
        self.n_vertices += 1
        return self.n_vertices - 1

    def _walk(self, t, up):
        if isinstance(t, list):
            v = self._vertex()
            self.lo[v] = self.pos
            for child in t:
                self._walk(child, v)
            self.hi[v] = self.pos
        else:
            v = self._vertex() if t is None else t
            self.lo[v], self.hi[v] = self.pos, self.pos + 1
            if t is not None:
                self.leaf_pos[t] = self.pos
            self.pos += 1
        if up is not None:
            self.parent[v] = up
        return v

    def arrays(self):
        VX = self.n_vertices if not self.hier_nil else 0
        parent = [self.parent.get(v, self.empty) for v in range(VX)]
        return parent, [self.lo[v] for v in range(VX)], [self.hi[v] for v in range(VX)]

    def text(self):
        parent, lo, hi = self.arrays()
        words = [self.N, self.NX, self.P, len(self.prio), self.top, self.add_nil, self.na, self.hier_nil]
        words += self.prio + list(self.removed) + list(self.added) + list(self.has_weight) + list(self.leaf_pos)
        words += [len(parent), 0 if self.hier_nil else self.empty] + parent + lo + hi
        words += [len(self.rules)] + [r[0] for r in self.rules] + [r[1] for r in self.rules]
        return " ".join(str(int(x)) for x in words)


def run(worlds, tmp_path, sanitized):
    """The program's answers: per world a dict of its lines, the rules' under ("rule", r)."""
    exe, why = build_program(sanitized)
    if exe is None:
        pytest.skip("-fsanitize=address does not link or start on this machine: " + why)
    cases, answers = tmp_path / "cases.txt", tmp_path / "answers.txt"
    cases.write_text("%d\n%s\n" % (len(worlds), "\n".join(w.text() for w in worlds)))
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=1"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    got = subprocess.run([exe, str(cases), str(answers)], capture_output=True, text=True, timeout=300, env=env)
    assert got.returncode == 0, got.stderr[-4000:]
    assert "AddressSanitizer" not in got.stderr and "runtime error" not in got.stderr, got.stderr[-4000:]
    out, cur = [], None
    lines = answers.read_text().strip().split("\n")
    assert lines[-1] == "ran %d cases" % len(worlds)
    for ln in lines[:-1]:
        name, *vals = ln.split()
        if name == "case":
            out.append({})
            cur = out[-1]
        elif name == "rule":
            cur = out[-1].setdefault(("rule", int(vals[0])), {})
        else:
            cur[name] = [int(v) for v in vals]
    assert len(out) == len(worlds)
    return out


BUILDS = [pytest.param(False, id="plain"), pytest.param(True, id="sanitized")]


# ---- references, from the definitions ------------------------------------------------------------------------------------------

def ref_nodes(w):
    """nodesNext = the cluster's nodes (ids below N) not in nodesToRemove (plan.go:77); ids from N on are names only."""
    alive = [int(n < w.N and not w.removed[n]) for n in range(w.NX)]
    ids = [n for n in range(w.NX) if alive[n]]
    rank = [ids.index(n) if alive[n] else -1 for n in range(w.NX)]
    return dict(n_alive=[len(ids)], any_removed=[int(w.removed.any())], any_node_weight=[int(w.has_weight.any())],
                alive=alive + [0], alive_ids=ids + [-1], alive_rank=rank + [-1])


def ref_order(w):
    """partitionSorter's category (plan.go:542-561) of a partition that holds the node set H, with no node to remove:
    "2" when nodesToAdd is nil, else "1" when H and nodesToAdd are disjoint, else "2".  With a node to remove "0" is possible
    and nothing is claimed.  A pass is uniform when every H the upload cannot rule out gives the same category.  What the
    upload knows of H: nothing held (na == 0, sweep 1's first pass); at least one node of nodesNext and possibly more (the
    later passes of such a plan, when there is a node to give); one node of nodesNext (cycle_order_stands: the second pass of a
    plan from nothing whose first pass was a round robin); else nothing."""
    alive = [n for n in range(w.NX) if n < w.N and not w.removed[n]]
    added = set(np.nonzero(w.added)[0])
    names = range(w.NX)

    def categories(holdings):
        return {"2" if w.add_nil or (set(H) & added) else "1" for H in holdings}

    def subsets(pool, must=()):
        pool = list(pool)[:6]                       # (enough to tell the categories apart: one added and one not added name)
        return [tuple(must) + c for k in range(len(pool) + 1) for c in itertools.combinations(pool, k)]

    any_held = subsets(sorted(names, key=lambda n: (n in added, n))[:3] + sorted(names, key=lambda n: (n not in added, n))[:3])
    first = [()] if w.na == 0 else any_held
    if w.na == 0 and alive:
        later = [h for a in alive for h in subsets(sorted(added)[:2], must=(a,))]
    else:
        later = any_held
    one_each = [(a,) for a in alive]
    calm = not w.removed.any()
    prio = w.prio
    return dict(uniform_first=[int(calm and len(categories(first)) == 1)],
                uniform_all=[int(calm and len(categories(first)) == 1 and len(categories(later)) == 1)],
                cycle_order_stands=[int(calm and len(categories(one_each)) <= 1)],
                top_prio_strict=[int(len(prio) > 0 and all(prio[m] > prio[w.top] for m in range(len(prio)) if m != w.top))])


def ref_rule(w, r):
    """The rule's regions, exclude classes, k_stay_by_top's work table and k_cycle.h's tables, or None where the rule does not
    cut the leaves into region chains.  leaves(findAncestor(v, level)) as plan.go:723-734 walks them."""
    parent, lo, hi = w.arrays()
    n_leaves = max(hi)

    def leaves(v, level):
        for _ in range(level):
            v = parent[v]
        return (lo[v], hi[v])

    inc = {a: leaves(a, w.rules[r][0]) for a in range(w.NX)}
    exc = {a: leaves(a, w.rules[r][1]) for a in range(w.NX)}
    placed = [a for a in range(w.NX) if w.leaf_pos[a] >= 0]
    inside = lambda a, iv: iv[0] <= w.leaf_pos[a] < iv[1]
    regions = sorted({inc[a] for a in placed if inside(a, inc[a])})
    if len(regions) < 2 or any(x[1] > y[0] for x, y in zip(regions, regions[1:])):
        return None
    node_region = [-1] * w.NX
    for a in placed:
        for g, reg in enumerate(regions):
            if inside(a, reg):
                if inc[a] != reg:
                    return None                     # a node inside a region that is not its include set
                node_region[a] = g
    if max(h - l for l, h in regions) > CHAIN_MAX_LEAVES:
        return None
    leaf_node = [-1] * n_leaves
    for a in placed:
        leaf_node[w.leaf_pos[a]] = a
    leaf_cls, cls_size, sizes, runs = [-1] * n_leaves, [0] * n_leaves, set(), True
    for (l, h) in regions:
        at = [leaf_node[p] for p in range(l, h) if leaf_node[p] >= 0]
        classes = sorted({exc[a] for a in at if l <= exc[a][0] and exc[a][1] <= h and exc[a][1] - exc[a][0] < h - l})
        if any(x[1] > y[0] for x, y in zip(classes, classes[1:])):
            return None
        for i, (cl, ch) in enumerate(classes):
            cls_size[l + i] = ch - cl
            sizes.add(ch - cl)
            runs = runs and (cl - l) % (ch - cl) == 0 and all(leaf_node[p] >= 0 for p in range(cl, ch))
        for a in at:
            for i, cls in enumerate(classes):
                if inside(a, cls):
                    if exc[a] != cls:
                        return None
                    leaf_cls[w.leaf_pos[a]] = i
    S = sizes.pop() if len(sizes) == 1 else 0
    cls_run = S if runs and S in (1, 2, 4, 8, 16, 32, 64) else 0
    work = [(g, ch) for g, (l, h) in enumerate(regions) for ch in range(-(-(h - l) // 64))]
    ref = dict(ok=[1], n_regions=[len(regions)], max_size=[max(h - l for l, h in regions)], cls_run=[cls_run], n_stay_wgs=[len(work)],
               node_region=node_region, reg_lo=[l for l, _ in regions], reg_hi=[h for _, h in regions], leaf_cls=leaf_cls,
               cls_size=cls_size, wg_region=[g for g, _ in work], wg_chunk=[ch for _, ch in work])
    # k_cycle.h: step j of a round robin over nodesNext has top priority node alive_ids[j % A]
    alive = [n for n in range(w.NX) if n < w.N and not w.removed[n]]
    distinct = len({int(w.leaf_pos[a]) for a in placed}) == len(placed)
    ref["cyc_ok"] = [int(distinct and len(alive) >= 1 and all(node_region[n] >= 0 for n in alive))]
    if ref["cyc_ok"][0]:
        A = len(alive)
        steps_of = [len(range(a, w.P, A)) for a in range(A)]                       # the steps j < P with j % A == a
        cyc = []
        for a, n in enumerate(alive):
            peers = [m for m in alive if node_region[m] == node_region[n]]
            cyc += [node_region[n], peers.index(n), int(w.leaf_pos[n]), len(peers)]
        chain_len = [sum(steps_of[a] for a, n in enumerate(alive) if node_region[n] == g) for g in range(len(regions))]
        at_leaf = [0] * n_leaves
        for a, n in enumerate(alive):
            at_leaf[w.leaf_pos[n]] = steps_of[a]
        ref.update(cyc=cyc, cyc_reg_off=[int(x) for x in np.concatenate([[0], np.cumsum(chain_len)])],
                   cyc_top_off=[int(x) for x in np.concatenate([[0], np.cumsum(at_leaf)])])
    return ref


def same_rule(got, want, name):
    if want is None:
        for k in ("ok", "n_regions", "cls_run", "n_stay_wgs", "cyc_ok"):
            assert got[k] == [0], (name, k, got[k])
        return
    for k, v in want.items():
        assert got[k] == [int(x) for x in v], (name, k, got[k][:24], v[:24])
    if not want["cyc_ok"][0]:
        assert got["cyc"] == [] and got["cyc_reg_off"] == [] and got["cyc_top_off"] == [], name


# ---- regions ------------------------------------------------------------------------------------------------------------------

def racks(*sizes, first=0):
    """A zone of racks of these sizes, the nodes numbered from `first`."""
    zone, n = [], first
    for s in sizes:
        zone.append(list(range(n, n + s)))
        n += s
    return zone


def overlapping_classes():
    w = World(8, [racks(2, 2), racks(2, 2, first=4)], [(2, 1)])
    rack0 = w.parent[0]
    w.hi[rack0] += 1                                   # rack 0 = leaves [0, 3), rack 1 = [2, 4)
    return w


REGION_WORLDS = {
    # name -> (world, ok, n_regions, cls_run) of rule 0
    "two_zones_of_two_racks": (lambda: World(8, [racks(2, 2), racks(2, 2, first=4)], [(2, 1)]), 1, 2, 2),
    "rack_sizes_2_and_3": (lambda: World(10, [racks(2, 3), racks(2, 3, first=5)], [(2, 1)]), 1, 2, 0),
    "class_with_a_leaf_without_a_node": (lambda: World(7, [[[0, 1], [2, None]], racks(2, 2, first=3)], [(2, 1)]), 1, 2, 0),
    "class_of_three": (lambda: World(12, [racks(3, 3), racks(3, 3, first=6)], [(2, 1)]), 1, 2, 0),
    "class_at_an_odd_offset": (lambda: World(8, [[[None], [0, 1], [2, 3]], [[None], [4, 5], [6, 7]]], [(2, 1)]), 1, 2, 0),
    "one_zone_only": (lambda: World(4, [racks(2, 2)], [(2, 1)]), 0, 0, 0),
    "node_one_level_higher_under_a_root": (lambda: World(9, [[racks(2, 2) + [8], racks(2, 2, first=4)]], [(2, 1)]), 0, 0, 0),
    "node_in_a_region_not_its_include_set": (lambda: World(9, [racks(2, 2) + [8], racks(2, 2, first=4)], [(2, 1)]), 0, 0, 0),
    "exclude_intervals_overlap": (overlapping_classes, 0, 0, 0),
    "exclude_interval_covers_its_region": (lambda: World(8, [racks(2, 2), racks(2, 2, first=4)], [(2, 2)]), 1, 2, 0),
    "region_of_512": (lambda: World(514, [list(range(512)), [512, 513]], [(1, 0)]), 1, 2, 1),
    "region_of_513": (lambda: World(515, [list(range(513)), [513, 514]], [(1, 0)]), 0, 0, 0),
    # (a run length other than 2, so that cls_run is seen to be the classes' size)
    "classes_of_four": (lambda: World(16, [racks(4, 4), racks(4, 4, first=8)], [(2, 1)]), 1, 2, 4),
}


@pytest.mark.parametrize("sanitized", BUILDS)
def test_regions(tmp_path, sanitized):
    names = list(REGION_WORLDS)
    worlds = [REGION_WORLDS[n][0]() for n in names]
    for name, w, got in zip(names, worlds, run(worlds, tmp_path, sanitized)):
        _, ok, n_regions, cls_run = REGION_WORLDS[name]
        rule = got[("rule", 0)]
        assert (rule["ok"], rule["n_regions"], rule["cls_run"]) == ([ok], [n_regions], [cls_run]), (name, rule["ok"], rule["n_regions"], rule["cls_run"])
        same_rule(rule, ref_rule(w, 0), name)
        if name == "exclude_interval_covers_its_region":
            assert set(rule["leaf_cls"]) == {-1} and not any(rule["cls_size"])
        if name == "two_zones_of_two_racks":
            assert rule["leaf_cls"][:8] == [0, 0, 1, 1, 0, 0, 1, 1] and rule["cls_size"][:8] == [2, 2, 0, 0, 2, 2, 0, 0]
            assert rule["node_region"] == [0, 0, 0, 0, 1, 1, 1, 1] and got["leaf_node"][:8] == list(range(8)) and got["leaves_distinct"] == [1]


def test_anchor_table(tmp_path):
    """The leaf intervals of every (rule, anchor), the anchor "" included: leaves(findAncestor(a, level)), two rules."""
    w = World(8, [racks(2, 2), racks(2, 2, first=4)], [(2, 1), (1, 0)])
    got = run([w], tmp_path, False)[0]
    parent, lo, hi = w.arrays()
    want = []
    for inc, exc in w.rules:
        for a in list(range(w.NX)) + [w.empty]:
            vi = ve = a
            for _ in range(inc):
                vi = parent[vi]
            for _ in range(exc):
                ve = parent[ve]
            want += [lo[vi], hi[vi], lo[ve], hi[ve]]
    assert got["anchors"] == want
    assert got["n_leaves"] == [9]                      # (eight nodes and the leaf of "")
    same_rule(got[("rule", 1)], ref_rule(w, 1), "racks as regions")
    assert got[("rule", 1)]["n_regions"] == [4] and got[("rule", 1)]["cls_run"] == [1]


# ---- k_stay_by_top's work table -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sanitized", BUILDS)
def test_stay_work_table(tmp_path, sanitized):
    """Regions of 63, 64, 65 and 128 leaves: 1, 1, 2 and 2 chunks of 64 leaves, in the order of the regions."""
    sizes, tree, n = [63, 64, 65, 128], [], 0
    for s in sizes:
        tree.append(list(range(n, n + s)))
        n += s
    w = World(n, tree, [(1, 0)])
    rule = run([w], tmp_path, sanitized)[0][("rule", 0)]
    assert rule["ok"] == [1] and rule["n_stay_wgs"] == [6]
    assert list(zip(rule["wg_region"], rule["wg_chunk"])) == [(0, 0), (1, 0), (2, 0), (2, 1), (3, 0), (3, 1)]
    same_rule(rule, ref_rule(w, 0), "chunks")


# ---- k_cycle.h's tables ---------------------------------------------------------------------------------------------------------

def cycle_world(name):
    """A world of tests/cycle_case_tables.py as a two-level hierarchy: a region is a vertex, its leaves are its children, a
    leaf's node (ids by leaf order) or none.  The rule (include 1, exclude 0) makes the regions the world's."""
    sizes, has_node, P = CT.WORLDS[name]
    cw = CT.world(sizes, has_node, P)
    tree, n = [], 0
    for r, sz in enumerate(sizes):
        region = []
        for lf in range(sz):
            region.append(n if has_node(r, lf) else None)
            n += 1 if has_node(r, lf) else 0
        tree.append(region)
    return cw, World(cw["NX"], tree, [(1, 0)], P=P)


@pytest.mark.parametrize("sanitized", BUILDS)
def test_cycle_tables(tmp_path, sanitized):
    """cyc, cyc_reg_off and cyc_top_off of every world of the single-kernel suites: the definitions' (ref_rule) and the suites'
    own builder's (cycle_case_tables.tables).  The upload numbers only the regions that hold a node and counts the leaf of ""
    behind the world's leaves; the builder's tables are taken to that numbering first.  A world with fewer than two such
    regions is no cut at all (ok = 0): the plan runs without region chains and the tables are not built."""
    names = list(CT.WORLDS)
    pairs = [cycle_world(n) for n in names]
    for name, (cw, w), got in zip(names, pairs, run([w for _, w in pairs], tmp_path, sanitized)):
        rule = got[("rule", 0)]
        same_rule(rule, ref_rule(w, 0), name)
        held = sorted(set(int(r) for r in cw["node_region"]))
        if len(held) < 2:
            assert name == "one_alive_node" and rule["ok"] == [0] and rule["cyc_ok"] == [0]
            continue
        assert rule["ok"] == [1] and rule["cyc_ok"] == [1], name
        cyc, reg_off, top_off = CT.tables(cw, CYC_WORDS)
        cyc = cyc.reshape(-1, CYC_WORDS).copy()
        cyc[:, 0] = [held.index(int(r)) for r in cyc[:, 0]]
        lengths = np.diff(reg_off)
        assert not lengths[[r for r in range(cw["B"]) if r not in held]].any()
        assert rule["cyc"] == [int(x) for x in cyc.reshape(-1)], name
        assert rule["cyc_reg_off"] == [0] + [int(x) for x in np.cumsum(lengths[held])], name
        assert rule["cyc_top_off"] == [int(x) for x in top_off] + [int(top_off[-1])], name


@pytest.mark.parametrize("sanitized", BUILDS)
def test_cycle_tables_are_not_built(tmp_path, sanitized):
    """Two nodes at one leaf; a node of nodesNext in no region; nodesNext empty.  The regions stand in all three."""
    shared = World(8, [racks(2, 2), racks(2, 2, first=4)], [(2, 1)])
    shared.leaf_pos[1] = shared.leaf_pos[0]
    stray = World(9, [racks(2, 2), racks(2, 2, first=4)], [(2, 1)])          # node 8: named by no vertex of the hierarchy
    none_alive = World(8, [racks(2, 2), racks(2, 2, first=4)], [(2, 1)], removed=range(8))
    cluster_empty = World(8, [racks(2, 2), racks(2, 2, first=4)], [(2, 1)], N=0)
    stray_not_alive = World(9, [racks(2, 2), racks(2, 2, first=4)], [(2, 1)], N=8)
    worlds = [shared, stray, none_alive, cluster_empty, stray_not_alive]
    got = run(worlds, tmp_path, sanitized)
    for i, (w, g) in enumerate(zip(worlds, got)):
        rule = g[("rule", 0)]
        assert rule["ok"] == [1] and rule["n_regions"] == [2] and rule["cyc_ok"] == [int(i == 4)], i
        same_rule(rule, ref_rule(w, 0), i)
    assert got[0]["leaves_distinct"] == [0] and got[1]["leaves_distinct"] == [1]
    assert got[1][("rule", 0)]["node_region"][8] == -1


# ---- order facts --------------------------------------------------------------------------------------------------------------

def order_worlds():
    """any node removed x nodesToAdd nil x nodesToAdd names (nothing | some node, not every node of nodesNext | every node of
    nodesNext) x na (0 | not) x nodesNext (empty | three nodes).  Four names, the last outside the cluster (never in nodesNext);
    a removed node is node 2, or -- with an empty cluster -- the name outside it."""
    out = []
    for removed, add_nil, add, na, some_alive in itertools.product((0, 1), (0, 1), ("none", "some", "all"), (0, 5), (0, 1)):
        N = 3 if some_alive else 0
        gone = ([2] if some_alive else [3]) if removed else []
        alive = [n for n in range(N) if n not in gone]
        added = {"none": [], "some": alive[:1] if alive else [3], "all": alive}[add]
        out.append(World(4, None, (), N=N, na=na, removed=gone, added=added, add_nil=add_nil))
    return out


@pytest.mark.parametrize("sanitized", BUILDS)
def test_order_truth_table(tmp_path, sanitized):
    worlds = order_worlds()
    assert len(worlds) == 48
    seen = set()
    for w, got in zip(worlds, run(worlds, tmp_path, sanitized)):
        want = ref_order(w)
        for k, v in want.items():
            assert got[k] == v, (k, vars(w))
        seen.add((got["uniform_first"][0], got["uniform_all"][0], got["cycle_order_stands"][0]))
    assert {(0, 0, 0), (1, 1, 1), (1, 0, 0), (1, 0, 1), (0, 0, 1)} <= seen      # (the table reaches every outcome there is)


def test_order_reference_by_hand():
    """The reference on the rows a reader can check against plan.go:542-561 in the head."""
    row = lambda **kw: ref_order(World(4, None, (), N=3, **kw))
    assert row(add_nil=1, na=5) == dict(uniform_first=[1], uniform_all=[1], cycle_order_stands=[1], top_prio_strict=[1])
    assert row(add_nil=1, na=5, removed=[2])["uniform_first"] == [0]                          # "0" is possible
    assert row(na=5, added=[0])["uniform_first"] == [0]                                       # "1" or "2", by what is held
    assert row(na=0, added=[0]) == dict(uniform_first=[1], uniform_all=[0], cycle_order_stands=[0], top_prio_strict=[1])
    assert row(na=0, added=[0, 1, 2]) == dict(uniform_first=[1], uniform_all=[1], cycle_order_stands=[1], top_prio_strict=[1])
    assert row(na=0, added=[3]) == dict(uniform_first=[1], uniform_all=[0], cycle_order_stands=[1], top_prio_strict=[1])


@pytest.mark.parametrize("sanitized", BUILDS)
def test_top_priority_strict(tmp_path, sanitized):
    cases = [((0, 1), 0, 1), ((0, 0), 0, 0), ((2, 1, 3), 1, 1), ((2, 1, 1), 1, 0), ((2, 1, 0), 1, 0), ((7,), 0, 1)]
    worlds = [World(4, None, (), prio=p, top=t) for p, t, _ in cases]
    for (p, t, strict), w, got in zip(cases, worlds, run(worlds, tmp_path, sanitized)):
        assert got["top_prio_strict"] == [strict] == ref_order(w)["top_prio_strict"], (p, t)


# ---- node facts ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sanitized", BUILDS)
def test_node_facts(tmp_path, sanitized):
    worlds = [World(6, None, (), N=4, removed=[1]),               # a removed node of the cluster
              World(6, None, (), N=4, removed=[5]),               # ... and one beyond n_nodes: nodesNext is whole
              World(6, None, (), N=4, removed=[0, 1, 2, 3]),      # nothing alive: the sentinel alone
              World(6, None, (), N=0),
              World(6, None, (), N=6, weights=[5], added=[2])]
    got = run(worlds, tmp_path, sanitized)
    for w, g in zip(worlds, got):
        for k, v in ref_nodes(w).items():
            assert g[k] == [int(x) for x in v], (k, vars(w))
    assert got[0]["alive_ids"] == [0, 2, 3, -1] and got[0]["alive_rank"] == [0, -1, 1, 2, -1, -1, -1]
    assert got[1]["any_removed"] == [1] and got[1]["n_alive"] == [4]
    assert got[2]["alive_ids"] == [-1] == got[3]["alive_ids"] and got[2]["n_alive"] == [0]
    assert got[4]["any_node_weight"] == [1] and got[0]["any_node_weight"] == [0]
