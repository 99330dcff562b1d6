"""Host-side mirror of the reference's planner API (api.go:24-190) over the HIP
library: same names, argument meaning, warnings text and caller-visible
mutations -- PlanNextMapEx() here is what `plan_hip.go` does
in Go.  Partition maps are dicts {name: Partition}.

There is no CPU fallback in this package: inputs outside the device envelope
raise problem.Unsupported / hip.BlanceError (the Go shim would call the Go
planner there).
"""
from . import abi, hip, problem

MaxIterationsPerPlan = 10            # plan.go:21
# plan.go:580: the hook that replaces the node sorter.  Anything but None (the default sorter) is a
# callback of the caller's language and cannot run on the device: PlanNextMapEx refuses (the Go shim
# runs plan.go then).  plan.go:693 NodeScoreBooster: only the cbgt booster (control_test.go:19-26) is
# built in -- pass booster="cbgt"; any other callable is refused the same way.
CustomNodeSorter = None


class Partition:
    """api.go:28-36"""
    __slots__ = ("Name", "NodesByState")

    def __init__(self, Name="", NodesByState=None):
        self.Name = Name
        self.NodesByState = NodesByState

    def __eq__(self, other):
        return isinstance(other, Partition) and self.Name == other.Name and self.NodesByState == other.NodesByState

    def __repr__(self):
        return "Partition(%r, %r)" % (self.Name, self.NodesByState)


class PartitionModelState:
    """api.go:46-62"""
    __slots__ = ("Priority", "Constraints")

    def __init__(self, Priority=0, Constraints=0):
        self.Priority = Priority
        self.Constraints = Constraints


class HierarchyRule:
    """api.go:96-105"""
    __slots__ = ("IncludeLevel", "ExcludeLevel")

    def __init__(self, IncludeLevel=0, ExcludeLevel=0):
        self.IncludeLevel = IncludeLevel
        self.ExcludeLevel = ExcludeLevel


class PlanNextMapOptions:
    """api.go:183-190; every field may be None (a nil map)."""

    def __init__(self, ModelStateConstraints=None, PartitionWeights=None, StateStickiness=None,
                 NodeWeights=None, NodeHierarchy=None, HierarchyRules=None):
        self.ModelStateConstraints = ModelStateConstraints
        self.PartitionWeights = PartitionWeights
        self.StateStickiness = StateStickiness
        self.NodeWeights = NodeWeights
        self.NodeHierarchy = NodeHierarchy
        self.HierarchyRules = HierarchyRules


_planner = None


def default_planner():
    global _planner
    if _planner is None:
        _planner = hip.Planner(device_id=0)
    return _planner


def _build_call(prevMap, partitionsToAssign, nodesAll, nodesToRemove, nodesToAdd, model, options=None, booster=None):
    """The flat problem of one PlanNextMapEx call (refuses what the device cannot run)."""
    options = options or PlanNextMapOptions()
    if CustomNodeSorter is not None:
        raise problem.Unsupported("CustomNodeSorter is not the default sorter (plan.go:580)")
    if booster is not None and booster != "cbgt":
        raise problem.Unsupported("NodeScoreBooster is an arbitrary callback (plan.go:693)")
    return problem.build_problem(prevMap, partitionsToAssign, nodesAll, nodesToRemove, nodesToAdd, model,
                                 options.ModelStateConstraints, options.PartitionWeights,
                                 options.StateStickiness, options.NodeWeights, options.NodeHierarchy,
                                 options.HierarchyRules, booster, max_iterations=MaxIterationsPerPlan)


def _finish_call(fp, res, prevMap, partitionsToAssign):
    """(nextMap, warnings) of one call from its result, with the caller-visible write-back of plan.go:49-52."""
    if res.iterations == 0:                     # MaxIterationsPerPlan <= 0: (nil, nil)
        return None, None
    flat, warnings = problem.decode_result(fp, res)
    nextMap = {name: Partition(name, p["nodesByState"]) for name, p in flat.items()}
    # plan.go:49-52: every non-converged sweep stores its partitions into BOTH input maps.
    # The last such store holds the final map's content.
    # When the call converged (in sweep n > 1) the stored objects are sweep n - 1's: equal in content to the returned
    # ones but distinct objects (plan.go:334-343 makes fresh ones every sweep); at the iteration cap they are the returned
    # objects themselves.
    if res.iterations > 1 or not res.converged:
        for name, part in nextMap.items():
            stored = part
            if res.converged:
                stored = Partition(part.Name, None if part.NodesByState is None else
                                   {s: (None if l is None else list(l)) for s, l in part.NodesByState.items()})
            prevMap[name] = stored
            partitionsToAssign[name] = stored
    return nextMap, warnings


def PlanNextMapEx(prevMap, partitionsToAssign, nodesAll, nodesToRemove, nodesToAdd, model, options=None,
                  booster=None, planner=None):
    """api.go:147-157.  Returns (nextMap, warnings); mutates prevMap and
    partitionsToAssign the way planNextMapEx does (plan.go:49-52)."""
    fp = _build_call(prevMap, partitionsToAssign, nodesAll, nodesToRemove, nodesToAdd, model, options, booster)
    res = (planner or default_planner()).plan(fp)
    return _finish_call(fp, res, prevMap, partitionsToAssign)


def PlanNextMapExBatch(calls, planner=None):
    """Many independent PlanNextMapEx calls planned by ONE blance_plan_batch (one upload, one launch per size class, one
    download; problems outside the batched envelope go the single-problem path inside the same call).  `calls` is a list of
    argument sets of PlanNextMapEx: tuples (prevMap, partitionsToAssign, nodesAll, nodesToRemove, nodesToAdd, model
    [, options [, booster]]) or dicts with those names.  Returns [(nextMap, warnings)] in call order and performs every
    call's write-back into its own prevMap / partitionsToAssign exactly as PlanNextMapEx does."""
    names = ("prevMap", "partitionsToAssign", "nodesAll", "nodesToRemove", "nodesToAdd", "model", "options", "booster")
    args = [dict(c) if isinstance(c, dict) else dict(zip(names, c)) for c in calls]
    fps = [_build_call(**a) for a in args]
    results, _ = (planner or default_planner()).plan_batch(fps)
    return [_finish_call(fp, res, a["prevMap"], a["partitionsToAssign"]) for fp, res, a in zip(fps, results, args)]


def PlanNextMapExBatchMoves(calls, favorMinNodes=False, planner=None):
    """PlanNextMapExBatch, and each plan's partition moves from the same device call (blance_plan_batch_moves): for every
    partition of partitionsToAssign, CalcPartitionMoves(sortStateNames(model), prevMap[name].NodesByState,
    nextMap[name].NodesByState, favorMinNodes) with prevMap as it was before the call -- what OrchestrateMoves computes
    next (orchestrate.go:273-287).  favorMinNodes: one bool or one per call.  Returns [(nextMap, warnings,
    {partition name: [NodeStateOp]})] in call order, with every call's write-back done as PlanNextMapEx does; a call
    whose plan returns no map (MaxIterationsPerPlan <= 0) gets (None, None, None)."""
    from . import abi
    names = ("prevMap", "partitionsToAssign", "nodesAll", "nodesToRemove", "nodesToAdd", "model", "options", "booster")
    args = [dict(c) if isinstance(c, dict) else dict(zip(names, c)) for c in calls]
    fps = [_build_call(**a) for a in args]
    favor = list(favorMinNodes) if isinstance(favorMinNodes, (list, tuple)) else [favorMinNodes] * len(fps)
    if len(favor) != len(fps):
        raise ValueError("favorMinNodes: one bool or one per call")
    ask, other = [], []
    for fp, a, f in zip(fps, args, favor):
        ask.append(bool(f) if fp.max_iterations > 0 else None)
        other.append(_beg_other(fp, a["prevMap"]))
    results, moves, _ = (planner or default_planner()).plan_batch_moves(fps, ask, other)
    out = []
    for fp, res, a, mv in zip(fps, results, args, moves):
        nextMap, warnings = _finish_call(fp, res, a["prevMap"], a["partitionsToAssign"])
        if nextMap is None or mv is None:
            out.append((nextMap, warnings, None))
            continue
        op_off, op_node, op_state, op_kind = mv
        byname = {}
        for p, name in enumerate(fp.part_names):
            byname[name] = [NodeStateOp(fp.node_names[op_node[j]], "" if op_state[j] < 0 else fp.state_names[op_state[j]],
                                        abi.OP_NAMES[op_kind[j]]) for j in range(op_off[p], op_off[p + 1])]
        out.append((nextMap, warnings, byname))
    return out


def PlanNextMapExBatchStats(calls, planner=None):
    """PlanNextMapExBatch, and each plan's quality numbers from the same device call (blance_plan_batch_stats): per state
    the load over nodesNext (min, max, sum, sum of squares; a node's load is the summed weight of the partitions it holds
    in that state), the nodes in use, the constraint slots left unmet and the (partition, slot) pairs that break a hierarchy
    rule of the state.  Returns [(nextMap, warnings, {state name: {load_min, load_max, load_sum, load_sumsq, nodes_used,
    unmet_slots, rule_violations}}, n_nodes_next)] in call order, with every call's write-back done as PlanNextMapEx does;
    a call whose plan returns no map (MaxIterationsPerPlan <= 0) gets (None, None) with every number 0."""
    from . import abi
    names = ("prevMap", "partitionsToAssign", "nodesAll", "nodesToRemove", "nodesToAdd", "model", "options", "booster")
    args = [dict(c) if isinstance(c, dict) else dict(zip(names, c)) for c in calls]
    fps = [_build_call(**a) for a in args]
    results, _, stats, _ = (planner or default_planner()).plan_batch_stats(fps, True)
    out = []
    for fp, res, a, st in zip(fps, results, args, stats):
        nextMap, warnings = _finish_call(fp, res, a["prevMap"], a["partitionsToAssign"])
        cols = {k: st[k].tolist() for k in abi.PLAN_STATS_ARRAYS}
        bystate = {name: {k: cols[k][m] for k in abi.PLAN_STATS_ARRAYS} for m, name in enumerate(fp.state_names)}
        out.append((nextMap, warnings, bystate, st["n_nodes_next"]))
    return out


def PlanNextMapExBatchWire(calls, planner=None):
    """PlanNextMapExBatch, and each plan as json.Marshal(PartitionMap) bytes from the same device call
    (blance_plan_batch_wire): what a caller persists and ships.  Returns [(nextMap, warnings, document_bytes)] in call
    order, with every call's write-back done as PlanNextMapEx does; a call whose plan returns no map
    (MaxIterationsPerPlan <= 0) gets (None, None, None).  The names are prepared per call here; a caller that plans the
    same indexes again keeps Planner.batch_names objects and calls Planner.plan_batch_wire itself."""
    names = ("prevMap", "partitionsToAssign", "nodesAll", "nodesToRemove", "nodesToAdd", "model", "options", "booster")
    args = [dict(c) if isinstance(c, dict) else dict(zip(names, c)) for c in calls]
    fps = [_build_call(**a) for a in args]
    pl = planner or default_planner()
    prepared = [pl.batch_names(fp) if fp.max_iterations > 0 else None for fp in fps]
    try:
        results, _, _, docs, _ = pl.plan_batch_wire(fps, prepared)
    finally:
        for nm in prepared:
            if nm is not None:
                nm.close()
    out = []
    for fp, res, a, doc in zip(fps, results, args, docs):
        nextMap, warnings = _finish_call(fp, res, a["prevMap"], a["partitionsToAssign"])
        out.append((nextMap, warnings, doc if nextMap is not None else None))
    return out


def PlanNextMapExBatchDocs(calls, planner=None):
    """Many rebalances planned from the stored PartitionMap documents by ONE blance_plan_batch_docs: the documents are decoded
    on the device, straight into the batch's input.  A call is a dict with the arguments of PlanNextMapEx but prevMap, and
    `document`: the bytes of json.Marshal(PartitionMap); prevMap and partitionsToAssign are both the document's map, and
    partitionsToAssign is only read for the partition names (a map or a list of names; the document must hold every one).
    An index whose document the device does not plan -- outside its subset, a missing partition, a duplicate -- goes the
    host route (wire.decode, lists_of_wire_map, problem.wire_adopted_problem, a plan of its own), so every call ends in a
    plan or in the host decoder's error (wire.WireError, problem.Unsupported).  Returns [(nextMap, warnings, route)] in call
    order, route "device" or "host"."""
    import numpy as np
    from . import wire
    pl = planner or default_planner()
    fps, docs = [], []
    for c in calls:
        c = dict(c)
        doc = c.pop("document")
        names = list(c.pop("partitionsToAssign"))
        gone, come = c.pop("nodesToRemove", None) or [], c.pop("nodesToAdd", None)
        fp = _build_call({}, {n: Partition(n, {}) for n in names}, c.pop("nodesAll"), [], None, c.pop("model"), **c)
        ids = {x: i for i, x in enumerate(fp.node_names)}
        flags = lambda lst: np.bincount([ids[x] for x in lst if x in ids], minlength=fp.n_nodes_ext).astype(bool).astype(np.uint8)   # noqa: E731
        fp.set("node_removed", flags(gone))
        fp.set("node_added", flags(come or []))
        fp.scalars["nodes_to_add_nil"] = int(come is None)
        fps.append(fp)
        docs.append(bytes(doc))
    dicts = [pl.batch_dict(fp) for fp in fps]
    try:
        results, _, _, _, outcomes, _ = pl.plan_batch_docs(fps, docs, dicts)
        out = []
        for fp, doc, d, res, oc in zip(fps, docs, dicts, results, outcomes):
            route = "device"
            if oc["status"] != 0:
                route = "host"
                wm = wire.decode(doc)
                try:
                    lists = lists_of_wire_map(wm, d)
                finally:
                    wm.close()
                new = problem.wire_adopted_problem(fp, lists, fp.node_removed[:fp.n_nodes_ext], fp.node_added[:fp.n_nodes_ext],
                                                   bool(fp.nodes_to_add_nil), True, False, row_stride=0xffff)
                res = pl.plan(new)
            nextMap, warnings = _finish_call(fp, res, {}, {})
            out.append((nextMap, warnings, route))
        return out
    finally:
        for d in dicts:
            d.close()


def _beg_other(fp, prevMap):
    """prevMap's nodes under state keys outside the model, CSR over fp's partitions in its node id space (None if none)."""
    import numpy as np
    known = set(fp.state_names)
    ids = {x: i for i, x in enumerate(fp.node_names)}
    off, nodes = [0], []
    for name in fp.part_names:
        prev = (prevMap or {}).get(name)
        nbs = (prev.NodesByState if hasattr(prev, "NodesByState") else (prev or {}).get("nodesByState")) or {}
        for s, lst in nbs.items():
            if s not in known:
                nodes.extend(ids[x] for x in (lst or []))
        off.append(len(nodes))
    if not nodes:
        return None
    return np.asarray(off, dtype=np.int32), np.asarray(nodes, dtype=np.int32)


def lists_of_wire_map(wm, wdict):
    """The host route to what Planner.decode_wire returns: a map the host decoder made (wire.decode) carried over from its
    first-seen ids to the ids of the dictionary `wdict`, in the layout of prev_* / assign_* (part_kind [P], off [P*M + 1],
    kind [P*M], nodes).  Also names_differ [P]: the partition's Name is not its key (the device refuses such a document).
    Raises problem.Unsupported for what the arrays cannot hold: a nil map, a nil partition, a name outside the dictionary."""
    import numpy as np
    if wm.map_is_nil:
        raise problem.Unsupported("the document is null (a nil PartitionMap)")
    P, M = wdict.n_parts, wdict.n_states
    ids = getattr(wdict, "_ids", None)
    if ids is None:
        as_bytes = lambda names: {(x if isinstance(x, bytes) else x.encode("utf-8", "surrogatepass")): i for i, x in enumerate(names)}   # noqa: E731
        ids = wdict._ids = (as_bytes(wdict.part_names), as_bytes(wdict.node_names), as_bytes(wdict.state_names))

    def carry(names, table, what):
        try:
            return np.asarray([table[x] for x in names], dtype=np.int64)
        except KeyError as e:
            raise problem.Unsupported("%s %r is not in the dictionary" % (what, e.args[0]))

    keys = wm.keys()
    pid = carry(keys, ids[0], "partition")
    node_id = carry(wm.nodes(), ids[1], "node")
    state_id = carry(wm.states(), ids[2], "state")
    if (wm.part_kind == 0).any():
        raise problem.Unsupported("a nil *Partition in the document")
    part_kind = np.zeros(P, dtype=np.uint8)
    part_kind[pid] = wm.part_kind
    names_differ = np.zeros(P, dtype=bool)
    names_differ[pid] = [k != n for k, n in zip(keys, wm.names())]
    n_entries = len(wm.entry_state)
    part_of = np.repeat(np.arange(len(keys)), np.diff(wm.part_off))
    slot = pid[part_of] * M + state_id[wm.entry_state] if n_entries else np.zeros(0, dtype=np.int64)
    lens_e = np.diff(wm.entry_off)
    kind = np.zeros(P * M, dtype=np.uint8)
    kind[slot] = wm.entry_kind
    lens = np.zeros(P * M, dtype=np.int64)
    lens[slot] = lens_e
    off = np.zeros(P * M + 1, dtype=np.int32)
    off[1:] = np.cumsum(lens)
    order = np.argsort(slot, kind="stable")
    ln = lens_e[order]
    total = int(ln.sum())
    begin = np.cumsum(ln) - ln
    src = np.repeat(wm.entry_off[:-1][order] - begin, ln) + np.arange(total)
    nodes = node_id[wm.entry_nodes[src]].astype(np.int32) if total else np.zeros(0, dtype=np.int32)
    return {"part_kind": part_kind, "off": off, "kind": kind, "nodes": nodes, "names_differ": names_differ,
            "n_node_refs": total, "n_parts_seen": len(keys)}


def decode_partition_map(planner, wdict, doc):
    """A PartitionMap document as the lists blance_problem takes for prev_* / assign_*: decoded on the device
    (Planner.decode_wire); a document the device refuses -- it is outside the device's subset, or no valid document -- goes
    to the host decoder (wire.decode, which raises wire.WireError for a syntax or type error) and lists_of_wire_map.  Returns
    the arrays of decode_wire, names_differ, and route: "device" or "host" (then with the device's refusal).  The device is
    asked twice, for the count and then for the lists (decode_wire with capacity=None): simple, not the fastest way in."""
    import numpy as np
    from . import wire
    got = (planner or default_planner()).decode_wire(wdict, doc)
    if not got["refusal"]:
        return dict(got, names_differ=np.zeros(wdict.n_parts, dtype=bool), route="device")
    wm = wire.decode(doc.tobytes() if hasattr(doc, "tobytes") else doc)
    try:
        out = lists_of_wire_map(wm, wdict)
    finally:
        wm.close()
    return dict(out, refusal=got["refusal"], refusal_at=got["refusal_at"], device_ms=got["device_ms"],
                total_ms=got["total_ms"], route="host")


def adopt_partition_map(planner, wdict, doc, fp=None, node_removed=None, node_added=None, nodes_to_add_nil=True, assign_too=True,
                        keep_prev_only=False, force_host=False):
    """A PartitionMap document as the next call's prevMap (assign_too: and partitionsToAssign) of the problem `planner`
    holds: on the device (Planner.adopt_wire).  A document the device refuses, or one with a list longer than the context's
    rows hold, goes the host route: the host decoder (wire.decode, which raises wire.WireError for a syntax or type
    error), problem.wire_adopted_problem of `fp` -- the problem the planner holds, as arrays; None: the one it uploaded
    last, right only while nothing was adopted since -- and a fresh upload.  The other reasons (abi.WIRE_ADOPT: a missing
    partition, a duplicate, a removal without prevMap, a load overflow) raise problem.Unsupported with .why / .why_at, on
    either route.  force_host: the host route at once (tests).  Returns adopt_wire's dict with route ("device" / "host") and
    problem (the host route's new problem, else None); plan_resident then plans."""
    from . import wire
    planner = planner or default_planner()
    info = None
    if not force_host:
        info = planner.adopt_wire(wdict, doc, node_removed, node_added, nodes_to_add_nil, assign_too, keep_prev_only)
        if info["adopted"]:
            return dict(info, route="device", problem=None)
        if not info["refusal"] and info["why"] != abi.WIRE_ADOPT["list_too_long"]:
            e = problem.Unsupported("blance_wire_adopt refused: " + abi.WIRE_ADOPT_WHYS[info["why"]])
            e.why, e.why_at = info["why"], info["why_at"]
            raise e
    fp = fp if fp is not None else getattr(planner, "_fp", None)
    if fp is None:
        raise ValueError("adopt_partition_map: no problem to adopt the document into")
    wm = wire.decode(doc.tobytes() if hasattr(doc, "tobytes") else doc)
    try:
        lists = lists_of_wire_map(wm, wdict)
    finally:
        wm.close()
    new = problem.wire_adopted_problem(fp, lists, node_removed, node_added, nodes_to_add_nil, assign_too, keep_prev_only,
                                       row_stride=0xffff)      # (a fresh upload sizes its rows itself)
    planner.upload(new)
    out = {"refusal": 0, "refusal_at": -1, "why": 0, "why_at": -1, "device_ms": 0.0, "total_ms": 0.0}
    out.update(info or {})
    return dict(out, adopted=True, n_node_refs=lists["n_node_refs"], n_parts_seen=lists["n_parts_seen"],
                result_capacity=new.result_capacity(), route="host", problem=new)


def PlanNextMap(prevMap, partitionsToAssign, nodesAll, nodesToRemove, nodesToAdd, model,
                modelStateConstraints=None, partitionWeights=None, stateStickiness=None, nodeWeights=None,
                nodeHierarchy=None, hierarchyRules=None, planner=None):
    """api.go:109-132 (deprecated positional wrapper)."""
    return PlanNextMapEx(prevMap, partitionsToAssign, nodesAll, nodesToRemove, nodesToAdd, model,
                         PlanNextMapOptions(modelStateConstraints, partitionWeights, stateStickiness, nodeWeights,
                                            nodeHierarchy, hierarchyRules), planner=planner)


class NodeStateOp:
    """moves.go:17-21"""
    __slots__ = ("Node", "State", "Op")

    def __init__(self, Node, State, Op):
        self.Node, self.State, self.Op = Node, State, Op

    def __eq__(self, other):
        return (self.Node, self.State, self.Op) == (other.Node, other.State, other.Op)

    def __repr__(self):
        return "NodeStateOp(%r, %r, %r)" % (self.Node, self.State, self.Op)


def CalcPartitionMovesBatch(states, begMap, endMap, favorMinNodes, planner=None):
    """CalcPartitionMoves (moves.go:41-119) for every partition of begMap / endMap at
    once -- what OrchestrateMoves does in a loop (orchestrate.go:273-287).  Maps are
    {name: nodesByState} or {name: Partition}; returns {name: [NodeStateOp]}."""
    import numpy as np
    from . import abi
    names = list(endMap.keys()) if endMap is not None else []
    for n in (begMap or {}):
        if n not in (endMap or {}):
            names.append(n)
    ids, node_names = {}, []

    def nid(x):
        i = ids.get(x)
        if i is None:
            i = ids[x] = len(node_names)
            node_names.append(x)
        return i

    def nbs_of(m, name):
        p = (m or {}).get(name)
        if p is None:
            return {}
        return (p.NodesByState if hasattr(p, "NodesByState") else p) or {}

    M = len(states)
    known = set(states)

    def csr(m):
        off, nodes = [0], []
        for name in names:
            nbs = nbs_of(m, name)
            for s in states:
                nodes.extend(nid(x) for x in (nbs.get(s) or []))
                off.append(len(nodes))
            for s, lst in nbs.items():               # keys outside `states` only feed flattenNodesByState
                if s not in known:
                    nodes.extend(nid(x) for x in (lst or []))
            off.append(len(nodes))
        return np.asarray(off, dtype=np.int32), np.asarray(nodes, dtype=np.int32)

    boff, bnod = csr(begMap)
    eoff, enod = csr(endMap)
    op_off, op_node, op_state, op_kind, _ = (planner or default_planner()).calc_moves(M, favorMinNodes, boff, bnod, eoff, enod)
    out = {}
    for i, name in enumerate(names):
        out[name] = [NodeStateOp(node_names[op_node[j]], "" if op_state[j] < 0 else states[op_state[j]],
                                 abi.OP_NAMES[op_kind[j]]) for j in range(op_off[i], op_off[i + 1])]
    return out


def CalcPartitionMoves(states, begNodesByState, endNodesByState, favorMinNodes, planner=None):
    """moves.go:41-119 for one partition."""
    return CalcPartitionMovesBatch(states, {"p": begNodesByState}, {"p": endNodesByState}, favorMinNodes, planner)["p"]


# misc.go:13-51, exported helpers callers may use
def StringsToMap(strs):
    return None if strs is None else {s: True for s in strs}


def StringsRemoveStrings(stringArr, removeArr):
    rm = StringsToMap(removeArr) or {}
    return [s for s in (stringArr or []) if s not in rm]


def StringsIntersectStrings(a, b):
    bm = StringsToMap(b) or {}
    rv, seen = [], set()
    for s in (a or []):
        if s in bm and s not in seen:
            seen.add(s)
            rv.append(s)
    return rv
