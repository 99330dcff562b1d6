"""ctypes binding of the C ABI (include/blance_hip.h) exported by
blance_amd/lib/libblance_hip.so -- the hand-written HIP planner for gfx950.

There is no CPU fallback: if the library is missing or no device is visible
the calls raise.  (tests/simt builds the same kernel source against a SIMT
emulator for GPU-less logic tests; that library is loaded only by tests, through
the `lib_path` argument.)
"""
import ctypes as C
import os

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libblance_hip.so")

EXPORTS = ["blance_abi_version", "blance_last_error", "blance_result_capacity", "blance_validate",
           "blance_ctx_create", "blance_ctx_destroy", "blance_plan", "blance_upload",
           "blance_plan_resident", "blance_download", "blance_calc_moves", "blance_plan_stats_get",
           "blance_comm_unique_id", "blance_comm_init_rccl", "blance_comm_set", "blance_comm_stats",
           "blance_is_emulated", "blance_host_alloc", "blance_host_free", "blance_comm_time_ms", "blance_host_trim",
           "blance_plan_moves_capacity", "blance_plan_moves_get", "blance_plan_wire_names", "blance_plan_wire_get",
           "blance_wire_dict_create", "blance_wire_dict_destroy", "blance_wire_decode_device", "blance_plan_adopt",
           "blance_wire_adopt"]

_libs = {}


class BlanceError(RuntimeError):
    def __init__(self, status, text):
        RuntimeError.__init__(self, "blance status %d: %s" % (status, text))
        self.status = status


def load_library(path=None):
    path = path or LIB_PATH
    lib = _libs.get(path)
    if lib is not None:
        return lib
    if not os.path.exists(path):
        raise ImportError("%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950); there is no CPU fallback" % path)
    lib = C.CDLL(path)
    lib.blance_abi_version.restype = C.c_int
    lib.blance_last_error.restype = C.c_char_p
    lib.blance_result_capacity.restype = C.c_int64
    lib.blance_result_capacity.argtypes = [C.POINTER(abi.Problem)]
    lib.blance_validate.restype = C.c_int
    lib.blance_validate.argtypes = [C.POINTER(abi.Problem)]
    lib.blance_ctx_create.restype = C.c_int
    lib.blance_ctx_create.argtypes = [C.POINTER(abi.Options), C.POINTER(C.c_void_p)]
    lib.blance_ctx_destroy.restype = None
    lib.blance_ctx_destroy.argtypes = [C.c_void_p]
    for name in ("blance_plan",):
        getattr(lib, name).restype = C.c_int
        getattr(lib, name).argtypes = [C.c_void_p, C.POINTER(abi.Problem), C.POINTER(abi.Result)]
    lib.blance_upload.restype = C.c_int
    lib.blance_upload.argtypes = [C.c_void_p, C.POINTER(abi.Problem)]
    lib.blance_plan_resident.restype = C.c_int
    lib.blance_plan_resident.argtypes = [C.c_void_p, C.POINTER(abi.Result)]
    lib.blance_download.restype = C.c_int
    lib.blance_download.argtypes = [C.c_void_p, C.POINTER(abi.Result)]
    lib.blance_plan_stats_get.restype = C.c_int
    lib.blance_plan_stats_get.argtypes = [C.c_void_p, C.POINTER(abi.PlanStats)]
    lib.blance_calc_moves.restype = C.c_int
    lib.blance_calc_moves.argtypes = [C.c_void_p, C.POINTER(abi.MovesProblem), C.POINTER(abi.MovesResult)]
    lib.blance_comm_unique_id.restype = C.c_int
    lib.blance_comm_unique_id.argtypes = [C.c_void_p]
    lib.blance_comm_init_rccl.restype = C.c_int
    lib.blance_comm_init_rccl.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.blance_comm_set.restype = C.c_int
    lib.blance_comm_set.argtypes = [C.c_void_p, C.POINTER(abi.Comm)]
    lib.blance_comm_stats.restype = C.c_int
    lib.blance_comm_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.blance_is_emulated.restype = C.c_int
    lib.blance_comm_time_ms.restype = C.c_int
    lib.blance_comm_time_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    lib.blance_host_alloc.restype = C.c_void_p
    lib.blance_host_alloc.argtypes = [C.c_size_t]
    lib.blance_host_free.restype = None
    lib.blance_host_free.argtypes = [C.c_void_p]
    lib.blance_host_trim.restype = None
    lib.blance_host_trim.argtypes = []
    # additive to ABI 6 (not in EXPORTS): a library without it still loads, Planner.plan_batch then refuses
    if hasattr(lib, "blance_plan_batch"):
        lib.blance_plan_batch.restype = C.c_int
        lib.blance_plan_batch.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.POINTER(abi.Problem)),
                                          C.POINTER(C.POINTER(abi.Result)), C.POINTER(abi.BatchInfo)]
    if hasattr(lib, "blance_plan_batch_moves"):
        lib.blance_plan_batch_moves.restype = C.c_int
        lib.blance_plan_batch_moves.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.POINTER(abi.Problem)),
                                                C.POINTER(C.POINTER(abi.Result)), C.POINTER(C.POINTER(abi.BatchMoves)),
                                                C.POINTER(abi.BatchInfo)]
        lib.blance_batch_moves_capacity.restype = C.c_int64
        lib.blance_batch_moves_capacity.argtypes = [C.POINTER(abi.Problem), C.POINTER(abi.BatchMoves)]
    if hasattr(lib, "blance_plan_batch_stats"):
        lib.blance_plan_batch_stats.restype = C.c_int
        lib.blance_plan_batch_stats.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.POINTER(abi.Problem)),
                                                C.POINTER(C.POINTER(abi.Result)), C.POINTER(C.POINTER(abi.BatchMoves)),
                                                C.POINTER(C.POINTER(abi.PlanStats)), C.POINTER(abi.BatchInfo)]
    if hasattr(lib, "blance_plan_batch_wire"):
        lib.blance_batch_names_create.restype = C.c_int
        lib.blance_batch_names_create.argtypes = [C.POINTER(abi.WireNames), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
        lib.blance_batch_names_destroy.restype = None
        lib.blance_batch_names_destroy.argtypes = [C.c_void_p]
        lib.blance_batch_wire_capacity.restype = C.c_size_t
        lib.blance_batch_wire_capacity.argtypes = [C.POINTER(abi.Problem), C.c_void_p]
        lib.blance_plan_batch_wire.restype = C.c_int
        lib.blance_plan_batch_wire.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.POINTER(abi.Problem)),
                                               C.POINTER(C.POINTER(abi.Result)), C.POINTER(C.POINTER(abi.BatchMoves)),
                                               C.POINTER(C.POINTER(abi.PlanStats)), C.POINTER(C.POINTER(abi.BatchWire)),
                                               C.POINTER(abi.BatchInfo)]
    if hasattr(lib, "blance_plan_batch_docs"):
        lib.blance_batch_dict_create.restype = C.c_int
        lib.blance_batch_dict_create.argtypes = [C.POINTER(abi.WireNames), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
        lib.blance_batch_dict_destroy.restype = None
        lib.blance_batch_dict_destroy.argtypes = [C.c_void_p]
        lib.blance_batch_doc_bounds.restype = C.c_int
        lib.blance_batch_doc_bounds.argtypes = [C.POINTER(abi.Problem), C.POINTER(abi.BatchDoc), C.c_void_p, C.POINTER(C.c_int64),
                                                C.POINTER(C.c_int64), C.POINTER(C.c_size_t)]
        lib.blance_plan_batch_docs.restype = C.c_int
        lib.blance_plan_batch_docs.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.POINTER(abi.Problem)),
                                               C.POINTER(C.POINTER(abi.Result)), C.POINTER(C.POINTER(abi.BatchMoves)),
                                               C.POINTER(C.POINTER(abi.PlanStats)), C.POINTER(C.POINTER(abi.BatchWire)),
                                               C.POINTER(C.POINTER(abi.BatchDoc)), C.POINTER(abi.BatchInfo)]
    # declared in blance_hip.h, additive to ABI 6: an older library of the same version loads, Planner.plan_moves refuses
    if hasattr(lib, "blance_plan_moves_get"):
        lib.blance_plan_moves_get.restype = C.c_int
        lib.blance_plan_moves_get.argtypes = [C.c_void_p, C.POINTER(abi.PlanMoves)]
        lib.blance_plan_moves_capacity.restype = C.c_int64
        lib.blance_plan_moves_capacity.argtypes = [C.POINTER(abi.Problem), C.POINTER(abi.PlanMoves)]
    if hasattr(lib, "blance_plan_wire_get"):                 # likewise: Planner.set_wire_names / plan_wire refuse without them
        lib.blance_plan_wire_names.restype = C.c_int
        lib.blance_plan_wire_names.argtypes = [C.c_void_p, C.POINTER(abi.WireNames)]
        lib.blance_plan_wire_get.restype = C.c_int
        lib.blance_plan_wire_get.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_double)]
    if hasattr(lib, "blance_wire_decode_device"):            # likewise: Planner.wire_dict / decode_wire refuse without them
        lib.blance_wire_dict_create.restype = C.c_int
        lib.blance_wire_dict_create.argtypes = [C.c_void_p, C.POINTER(abi.WireNames), C.c_int32, C.c_int32, C.c_int32,
                                                C.POINTER(C.c_void_p)]
        lib.blance_wire_dict_destroy.restype = None
        lib.blance_wire_dict_destroy.argtypes = [C.c_void_p, C.c_void_p]
        lib.blance_wire_decode_device.restype = C.c_int
        lib.blance_wire_decode_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(abi.WireLists)]
    if hasattr(lib, "blance_plan_adopt"):                    # likewise: Planner.adopt refuses without it
        lib.blance_plan_adopt.restype = C.c_int
        lib.blance_plan_adopt.argtypes = [C.c_void_p, C.POINTER(abi.Adopt)]
    if hasattr(lib, "blance_wire_adopt"):                    # likewise: Planner.adopt_wire refuses without it
        lib.blance_wire_adopt.restype = C.c_int
        lib.blance_wire_adopt.argtypes = [C.c_void_p, C.POINTER(abi.WireAdopt)]
    if lib.blance_abi_version() != abi.ABI_VERSION:
        raise ImportError("ABI version mismatch")
    _libs[path] = lib
    return lib


def moves_problem_of(fp, res, beg_other=None):
    """The arguments of Planner.calc_moves for "from fp's prevMap to the plan `res`": both maps as CSRs over
    p * (M + 1) + state (pseudo state M: beg_other, the (offsets [P + 1], node ids) of prevMap's keys outside the model).
    The host route to a plan's moves, which Planner.plan_moves replaces.  Returns (beg_off, beg_nodes, end_off, end_nodes)."""
    import numpy as np
    P, M = fp.scalars["n_parts"], fp.scalars["n_states"]

    def widen(off, nodes, other):
        off = np.asarray(off[:P * M + 1], dtype=np.int64)
        lens = np.zeros((P, M + 1), dtype=np.int64)
        lens[:, :M] = np.diff(off).reshape(P, M)
        total = int(off[-1])
        if other is None:
            out_nodes = np.asarray(nodes[:total], dtype=np.int32)
        else:
            ooff, onodes = np.asarray(other[0][:P + 1], dtype=np.int64), np.asarray(other[1], dtype=np.int32)
            lens[:, M] = np.diff(ooff)
            out_nodes = np.empty(total + int(ooff[-1]), dtype=np.int32)
            per_part = off[::M][:P + 1] if M else np.zeros(P + 1, dtype=np.int64)     # model entries in front of partition p
            part_of = np.repeat(np.arange(P), np.diff(per_part))
            out_nodes[np.arange(total) + ooff[part_of]] = nodes[:total]
            part_of = np.repeat(np.arange(P), np.diff(ooff))
            out_nodes[np.arange(int(ooff[-1])) + per_part[part_of + 1]] = onodes[:int(ooff[-1])]
        wide = np.zeros(P * (M + 1) + 1, dtype=np.int32)
        wide[1:] = np.cumsum(lens.reshape(-1))
        return wide, out_nodes

    beg_off, beg_nodes = widen(fp.arrays["prev_off"], fp.arrays["prev_nodes"], beg_other)
    end_off, end_nodes = widen(res.out_off, res.out_nodes, None)
    return beg_off, beg_nodes, end_off, end_nodes


class _PinnedBlock:
    """One block of blance_host_alloc; goes back to the library when the last numpy view of it is collected."""

    def __init__(self, lib, nbytes):
        self.lib = lib
        self.p = lib.blance_host_alloc(nbytes)
        if not self.p:
            raise MemoryError("blance_host_alloc(%d) failed" % nbytes)

    def __del__(self):
        try:
            if self.p:
                self.lib.blance_host_free(self.p)
                self.p = None
        except Exception:
            pass


class HostArena:
    """Page-locked host arrays from blance_host_alloc (include/blance_hip.h, ABI 5): numpy views the device copies from / to
    by DMA where they lie.  Every array keeps its block alive (the ctypes buffer it is a view of owns the block), so an array
    that outlives the arena -- a result kept after the arena is closed -- never aliases a block that was handed out again;
    a block goes back to the library when its last view is collected."""

    def __init__(self, lib_path=None):
        self.lib = load_library(lib_path)
        self.n_blocks = 0

    def empty(self, n, dtype):
        import numpy as np
        dt = np.dtype(dtype)
        nbytes = max(int(n), 1) * dt.itemsize
        block = _PinnedBlock(self.lib, nbytes)
        buf = (C.c_char * nbytes).from_address(block.p)
        buf._block = block                                  # the view's base owns the block
        self.n_blocks += 1
        return np.frombuffer(buf, dtype=dt, count=int(n))

    def copy_of(self, arr):
        a = self.empty(arr.size, arr.dtype)
        a[...] = arr.reshape(-1)
        return a

    def close(self):
        """Kept for callers of the earlier interface: the blocks are owned by the arrays, nothing to release here."""


def wire_names_struct(names, node_names, state_names):
    """abi.WireNames of three lists of names (str, or bytes for names that are no valid UTF-8) and what keeps its arrays alive."""
    import numpy as np
    nm, keep = abi.WireNames(), []
    for field, strs in (("part", names), ("node", node_names), ("state", state_names)):
        raw = [x if isinstance(x, bytes) else x.encode("utf-8", "surrogatepass") for x in strs]
        off = np.zeros(len(raw) + 1, dtype=np.int64)
        if raw:
            off[1:] = np.cumsum([len(x) for x in raw])
        blob = b"".join(raw)
        buf = C.create_string_buffer(blob, len(blob) + 1)
        keep += [buf, off]
        setattr(nm, field + "_bytes", C.cast(buf, C.c_void_p).value)
        setattr(nm, field + "_off", off.ctypes.data)
    return nm, keep


class WireDict:
    """A blance_wire_dict: the names a document is decoded against (Planner.wire_dict).  Owned by its planner's context:
    close() destroys it early, closing the planner does at the latest."""

    def __init__(self, planner, handle, part_names, node_names, state_names):
        self.planner, self._h = planner, handle
        self.part_names, self.node_names, self.state_names = list(part_names), list(node_names), list(state_names)
        self.n_parts, self.n_nodes_ext, self.n_states = len(self.part_names), len(self.node_names), len(self.state_names)

    def close(self):
        if self._h and getattr(self.planner, "_h", None):
            self.planner.lib.blance_wire_dict_destroy(self.planner._h, self._h)
        self._h = None


class BatchNames:
    """A blance_batch_names: the prepared names of one index for Planner.plan_batch_wire (Planner.batch_names).  Host memory
    only, tied to no context: it may serve any number of calls and planners; close() / __del__ destroys it."""

    def __init__(self, lib, handle, n_parts, n_nodes_ext, n_states):
        self.lib, self._h = lib, handle
        self.n_parts, self.n_nodes_ext, self.n_states = n_parts, n_nodes_ext, n_states

    def close(self):
        if getattr(self, "_h", None):
            self.lib.blance_batch_names_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BatchDict:
    """A blance_batch_dict: the names the documents of one index are decoded against in Planner.plan_batch_docs
    (Planner.batch_dict).  Host memory only, tied to no context: it may serve any number of calls and planners; close() /
    __del__ destroys it."""

    def __init__(self, lib, handle, part_names, node_names, state_names):
        self.lib, self._h = lib, handle
        self.part_names, self.node_names, self.state_names = list(part_names), list(node_names), list(state_names)
        self.n_parts, self.n_nodes_ext, self.n_states = len(self.part_names), len(self.node_names), len(self.state_names)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.blance_batch_dict_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _ResultShape:
    """What abi.FlatResult reads of a problem, for the problem a planner holds after adopt_wire: the uploaded problem's sizes
    and the result capacity blance_wire_adopt reported."""

    def __init__(self, fp, capacity):
        self.scalars = fp.scalars
        self._capacity = capacity

    def result_capacity(self):
        return self._capacity


class Planner:
    """One blance_ctx: a planner bound to one gfx950 device."""

    def __init__(self, device_id=0, engine=abi.ENGINE_AUTO, lib_path=None, force_threads=0,
                 chain_min_parts=0, seq_speculation=True, tree="auto", planes=True, stay_top="auto", periodic=True, queue=True,
                 shard_one_rank=False, period_known=True, cycle_group=True):
        self.lib = load_library(lib_path)
        opt = abi.Options()
        opt.engine = engine
        opt.device_id = device_id
        opt.reserved[0] = force_threads      # workgroup size of the sequential pass (0 = auto)
        opt.reserved[1] = chain_min_parts    # smallest pass run as region chains (0 = default)
        # test knobs: 1 = k_pass_seq without verified stays; k_pass_tree (flat passes): 2 = never,
        # 4 = every general step scores all nodes, 8 = also when a k_pass_seq workgroup size is forced,
        # 16 = every general step decodes its record (none served from the validating lane's registers)
        # 32 = the all-blank chain pass on k_pass_chain_blank (lane minima) instead of k_pass_chain_planes
        # 64 = never k_stay_by_top (a chain pass of stays verified per top priority node), 128 = try it in every
        # chain pass with NumPartitions > 0
        # 256 = the all-blank chain pass WITHOUT its periodic form (k_period.h: a pass whose step records repeat walks two
        # periods and copies the rest -- the default; also BLANCE_PERIODIC=0)
        # 512 = flat passes with k <= 2 never on k_pass_queue (k_pass_tree / k_pass_seq take them, as before round 4);
        # 1024 = k_pass_queue without its lean walk (every step that does not stay through its general code)
        # 2048 = ... and every general step of it scoring every node; 4096 = its lean walk as compiled C++ only (the device
        # build walks the plain k = 2 steps in hand-written assembly, k_queue_walk.h); 8192 = its window always rebuilt by the
        # exact selection (one helper wave), never by the helper waves' striped form
        # 16384 = a communicator of ONE rank takes the sharded branch of every chain pass (both collectives execute:
        # how ncclAllReduce / ncclAllGather run on a one-GPU box)
        # 32768 = its walking wave copies a batch's row bit maps itself (the helper waves do since round 6)
        # 65536 = the periodic pass behind a round robin searches for its period and verifies it, as every other periodic
        # pass does (the default takes it from the round robin: k_period_find's known mode; also BLANCE_PERIOD_KNOWN=0)
        # 131072 = the chain pass behind a round robin groups its steps by region and by top priority node with the counting
        # sorts every other pass uses (the default takes both groupings from tables of the upload: k_cycle.h; also
        # BLANCE_CYCLE_GROUP=0)
        qbits = {True: 0, "on": 0, False: 512, "off": 512, "general": 1024, "dense": 1024 | 2048, "lean-cpp": 4096,
                 "exact-rebuild": 8192, "bits-self": 32768}[queue]
        opt.reserved[2] = qbits | (16384 if shard_one_rank else 0) | (0 if period_known else 65536) | (0 if cycle_group else 131072) | (0 if periodic else 256) | {"auto": 0, "off": 64, "force": 128}[stay_top] | (0 if planes else 32) | (0 if seq_speculation else 1) | {"auto": 0, "off": 2, "dense": 4 | 8, "on": 8, "long": 8 | 16,
                                                          "dense-long": 4 | 8 | 16}[tree]
        h = C.c_void_p()
        self._check(self.lib.blance_ctx_create(C.byref(opt), C.byref(h)))
        self._h = h

    def _check(self, st):
        if st != abi.OK:
            raise BlanceError(st, (self.lib.blance_last_error() or b"").decode())

    def close(self):
        if getattr(self, "_h", None):
            self.lib.blance_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- one plan on several ranks (include/blance_hip.h "one plan on several GPUs") ----
    def comm_init_rccl(self, dist):
        """Join the library's RCCL communicator: one process per GPU, `dist` an initialised
        torch.distributed (any backend) that carries the 128-byte id from rank 0 to the others."""
        rank, world = dist.get_rank(), dist.get_world_size()
        buf = C.create_string_buffer(128)
        if rank == 0:
            self._check(self.lib.blance_comm_unique_id(buf))
        box = [buf.raw]
        dist.broadcast_object_list(box, src=0)
        ident = C.create_string_buffer(box[0], 128)
        self._check(self.lib.blance_comm_init_rccl(self._h, world, rank, ident))
        return world

    def comm_init_rccl_one_rank(self):
        """A RCCL communicator of this one rank (no torch.distributed needed).  With Planner(shard_one_rank=True) the
        chain passes then take their sharded branch and really issue ncclAllReduce / ncclAllGather."""
        buf = C.create_string_buffer(128)
        self._check(self.lib.blance_comm_unique_id(buf))
        self._check(self.lib.blance_comm_init_rccl(self._h, 1, 0, buf))
        return 1

    def comm_set_callback(self, rank, n_ranks, allreduce, allgather=None):
        """An embedder's collectives: allreduce(address, count) sums `count` int32 values in place over the
        ranks; allgather(address, count_per_rank) completes n_ranks blocks of which this rank's is filled in
        (None: the library sums zero-padded outputs with allreduce instead).  The addresses are device
        memory of this context (host memory under the SIMT emulator)."""
        def _wrap(fn):
            def _cb(_user, ptr, count):
                try:
                    fn(ptr, count)
                    return 0
                except Exception:                      # no exception may cross the C boundary
                    import traceback
                    traceback.print_exc()
                    return 1
            return abi.ALLREDUCE_FN(_cb)
        self._comm_cb = (_wrap(allreduce), _wrap(allgather) if allgather else abi.ALLREDUCE_FN())   # keep the trampolines alive
        comm = abi.Comm(rank, n_ranks, self._comm_cb[0], None, self._comm_cb[1])
        self._check(self.lib.blance_comm_set(self._h, C.byref(comm)))

    def comm_stats(self):
        """(collectives made, int32 words moved) by this context's sharded plans so far."""
        calls, words = C.c_int64(0), C.c_int64(0)
        self._check(self.lib.blance_comm_stats(self._h, C.byref(calls), C.byref(words)))
        return int(calls.value), int(words.value)

    def comm_time_ms(self):
        """Device ms spent inside RCCL collectives by this context's plans so far."""
        ms = C.c_double(0.0)
        self._check(self.lib.blance_comm_time_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def is_emulated(self):
        return bool(self.lib.blance_is_emulated())

    def comm_clear(self):
        self._check(self.lib.blance_comm_set(self._h, None))

    def validate(self, fp):
        return self.lib.blance_validate(C.byref(fp.as_struct()))

    def plan_into(self, fp, res):
        """blance_plan with the caller's result buffers (a FlatResult made for this problem shape) written again."""
        self._fp = fp
        self._adopted = False
        self._wire_adopted = None
        self._check(self.lib.blance_plan(self._h, C.byref(fp.as_struct()), C.byref(res.struct)))
        return res

    def plan(self, fp):
        """blance_plan(): host buffers in, host buffers out."""
        res = abi.FlatResult(fp)
        self._fp = fp
        self._adopted = False
        self._wire_adopted = None
        self._check(self.lib.blance_plan(self._h, C.byref(fp.as_struct()), C.byref(res.struct)))
        return res

    def plan_batch(self, fps):
        """blance_plan_batch(): many independent problems in one call.  Returns ([FlatResult], info dict) with
        n_batched / n_fallback / kernel_launches / steps_total / device_ms / total_ms."""
        if not hasattr(self.lib, "blance_plan_batch"):
            raise BlanceError(abi.ERR_UNSUPPORTED, "this library has no blance_plan_batch (build the current sources)")
        fps = list(fps)
        results = [abi.FlatResult(fp) for fp in fps]
        structs = [fp.as_struct() for fp in fps]               # (kept alive for the call)
        n = len(fps)
        pbs = (C.POINTER(abi.Problem) * max(n, 1))(*[C.pointer(s) for s in structs])
        rss = (C.POINTER(abi.Result) * max(n, 1))(*[C.pointer(r.struct) for r in results])
        info = abi.BatchInfo()
        self._adopted = False
        self._wire_adopted = None
        self._check(self.lib.blance_plan_batch(self._h, n, pbs, rss, C.byref(info)))
        return results, {name: getattr(info, name) for name, _ in abi.BatchInfo._fields_}

    def _moves_requests(self, fps, results, favor_min_nodes, beg_other, caps=None):
        """The moves requests of a batch as one numpy block viewed as blance_batch_moves[], the moves of all problems in one
        block: per problem op_off [P + 1], then op_node, op_state, op_kind [capacity] (no per-array ctypes conversions).
        caps: {problem index: capacity} where it is not the problem's own (a document problem's bound).
        Returns (the pointer array of the call, what _moves_unpack needs -- it also keeps the buffers alive)."""
        import numpy as np
        n = len(fps)
        favor = list(favor_min_nodes) if isinstance(favor_min_nodes, (list, tuple)) else [favor_min_nodes] * n
        other = list(beg_other) if beg_other is not None else [None] * n
        ask = [i for i in range(n) if favor[i] is not None]
        req = np.zeros(max(len(ask), 1), dtype=abi.BATCH_MOVES_DTYPE)
        keep = []
        P = np.array([fps[i].scalars["n_parts"] for i in ask], dtype=np.int64)
        # = blance_batch_moves_capacity: prevMap entries + keys outside the model + blance_result_capacity
        cap = np.array([fps[i].arrays["prev_off"][-1] for i in ask], dtype=np.int64) + \
            np.array([results[i].struct.out_capacity for i in ask], dtype=np.int64)
        for j, i in enumerate(ask):
            if caps and i in caps:
                cap[j] = caps[i]
        req["favor_min_nodes"][:len(ask)] = [bool(favor[i]) for i in ask]
        for j, i in enumerate(ask):
            if other[i] is not None:
                off, nodes = [np.ascontiguousarray(a, dtype=np.int32) for a in other[i]]
                nodes = nodes if nodes.size else np.zeros(1, dtype=np.int32)
                keep += [off, nodes]
                cap[j] += int(off[P[j]])
                req["beg_other_off"][j], req["beg_other_nodes"][j] = off.ctypes.data, nodes.ctypes.data
        words = P + 1 + 3 * np.maximum(cap, 1)
        base = np.zeros(len(ask) + 1, np.int64)
        base[1:] = np.cumsum(words)
        block = np.empty(max(int(base[-1]), 1), dtype=np.int32)          # every word read back is written by the call
        addr = block.ctypes.data + 4 * base[:-1]
        req["op_off"][:len(ask)] = addr
        req["op_node"][:len(ask)] = addr + 4 * (P + 1)
        req["op_state"][:len(ask)] = addr + 4 * (P + 1 + np.maximum(cap, 1))
        req["op_kind"][:len(ask)] = addr + 4 * (P + 1 + 2 * np.maximum(cap, 1))
        req["capacity"][:len(ask)] = cap
        ptrs = np.zeros(max(n, 1), dtype=np.uint64)
        ptrs[ask] = req.ctypes.data + req.itemsize * np.arange(len(ask), dtype=np.uint64)
        return ptrs, (n, ask, P, cap, base, block, req, keep)

    @staticmethod
    def _moves_unpack(state):
        n, ask, P, cap, base, block, _, _ = state
        moves = [None] * n
        ends = (base[:-1] + P).tolist()
        totals = block[base[:-1] + P].tolist() if ask else []
        for j, i in enumerate(ask):
            e, t, c = ends[j] + 1, totals[j], max(int(cap[j]), 1)
            moves[i] = (block[e - int(P[j]) - 1:e], block[e:e + t], block[e + c:e + c + t], block[e + 2 * c:e + 2 * c + t])
        return moves

    def plan_batch_moves(self, fps, favor_min_nodes, beg_other=None):
        """blance_plan_batch_moves(): plan_batch, and for each problem CalcPartitionMoves from its prevMap as passed to its
        plan for every partition in partition id order.  favor_min_nodes: one bool, or one per problem where None asks for
        no moves; beg_other: None, or per problem None or (offsets [P + 1], node ids) of prevMap's keys outside the model.
        Returns ([FlatResult], [(op_off, op_node, op_state, op_kind) or None], info dict)."""
        if not hasattr(self.lib, "blance_plan_batch_moves"):
            raise BlanceError(abi.ERR_UNSUPPORTED, "this library has no blance_plan_batch_moves (build the current sources)")
        fps = list(fps)
        n = len(fps)
        results = [abi.FlatResult(fp) for fp in fps]
        structs = [fp.as_struct() for fp in fps]
        ptrs, state = self._moves_requests(fps, results, favor_min_nodes, beg_other)
        pbs = (C.POINTER(abi.Problem) * max(n, 1))(*[C.pointer(s) for s in structs])
        rss = (C.POINTER(abi.Result) * max(n, 1))(*[C.pointer(r.struct) for r in results])
        info = abi.BatchInfo()
        self._adopted = False
        self._wire_adopted = None
        self._check(self.lib.blance_plan_batch_moves(self._h, n, pbs, rss,
                                                     ptrs.ctypes.data_as(C.POINTER(C.POINTER(abi.BatchMoves))),
                                                     C.byref(info)))
        return results, self._moves_unpack(state), {name: getattr(info, name) for name, _ in abi.BatchInfo._fields_}

    @staticmethod
    def _stats_requests(fps, want):
        """The statistics requests of a batch (want: one bool per problem).  Returns (the pointer array of the call, what
        _stats_unpack needs -- it also keeps the buffers alive)."""
        import numpy as np
        n = len(fps)
        # the requests as one numpy block viewed as blance_plan_stats[], the arrays of all problems in one int64 block: per
        # problem seven slots of max(M, 1) values in the order of abi.PLAN_STATS_ARRAYS (nodes_used: int32 in its slot)
        ask = [i for i in range(n) if want[i]]
        M = np.array([fps[i].scalars["n_states"] for i in ask], dtype=np.int64)
        slot = np.maximum(M, 1)
        base = np.zeros(len(ask) + 1, np.int64)
        base[1:] = np.cumsum(len(abi.PLAN_STATS_ARRAYS) * slot)
        block = np.zeros(max(int(base[-1]), 1), dtype=np.int64)
        req = np.zeros(max(len(ask), 1), dtype=abi.PLAN_STATS_DTYPE)
        req["n_states"][:len(ask)] = M
        for k, name in enumerate(abi.PLAN_STATS_ARRAYS):
            req[name][:len(ask)] = block.ctypes.data + 8 * (base[:-1] + k * slot)
        st_ptrs = np.zeros(max(n, 1), dtype=np.uint64)
        st_ptrs[ask] = req.ctypes.data + req.itemsize * np.arange(len(ask), dtype=np.uint64)
        return st_ptrs, (n, ask, M, slot, base, block, req)

    @staticmethod
    def _stats_unpack(state):
        import numpy as np
        n, ask, M, slot, base, block, req = state
        out = [None] * n
        block32 = block.view(np.int32)
        n_next = req["n_nodes_next"].tolist()
        starts, slots, ms = base.tolist(), slot.tolist(), M.tolist()
        for j, i in enumerate(ask):
            d = {}
            for k, name in enumerate(abi.PLAN_STATS_ARRAYS):
                at = starts[j] + k * slots[j]
                d[name] = block32[2 * at:2 * at + ms[j]] if name == "nodes_used" else block[at:at + ms[j]]
            d["n_nodes_next"] = n_next[j]
            out[i] = d
        return out

    def plan_batch_stats(self, fps, stats=True, favor_min_nodes=None, beg_other=None):
        """blance_plan_batch_stats(): plan_batch, and for each problem that asks the plan statistics of Planner.plan_stats
        from the same device call.  stats: one bool or one per problem; favor_min_nodes / beg_other as in plan_batch_moves,
        None: no moves at all.  Returns ([FlatResult], [moves or None], [stats dict or None], info dict); a stats dict has
        the keys of Planner.plan_stats."""
        import numpy as np
        if not hasattr(self.lib, "blance_plan_batch_stats"):
            raise BlanceError(abi.ERR_UNSUPPORTED, "this library has no blance_plan_batch_stats (build the current sources)")
        fps = list(fps)
        n = len(fps)
        results = [abi.FlatResult(fp) for fp in fps]
        structs = [fp.as_struct() for fp in fps]
        want = list(stats) if isinstance(stats, (list, tuple)) else [stats] * n
        if len(want) != n:
            raise ValueError("stats: one bool or one per problem")
        mv_ptrs, mv_state = self._moves_requests(fps, results, favor_min_nodes, beg_other)
        st_ptrs, st_state = self._stats_requests(fps, want)
        pbs = (C.POINTER(abi.Problem) * max(n, 1))(*[C.pointer(s) for s in structs])
        rss = (C.POINTER(abi.Result) * max(n, 1))(*[C.pointer(r.struct) for r in results])
        info = abi.BatchInfo()
        self._adopted = False
        self._wire_adopted = None
        self._check(self.lib.blance_plan_batch_stats(self._h, n, pbs, rss,
                                                     mv_ptrs.ctypes.data_as(C.POINTER(C.POINTER(abi.BatchMoves))),
                                                     st_ptrs.ctypes.data_as(C.POINTER(C.POINTER(abi.PlanStats))),
                                                     C.byref(info)))
        return (results, self._moves_unpack(mv_state), self._stats_unpack(st_state),
                {name: getattr(info, name) for name, _ in abi.BatchInfo._fields_})

    def batch_names(self, names, node_names=None, state_names=None):
        """blance_batch_names_create(): the prepared names of one index, for plan_batch_wire.  names: a problem (its
        part_names, node_names, state_names), or the partition names with the two other lists beside them; str or bytes.
        The names of an index do not change between rebalances: make the object once and keep it."""
        if not hasattr(self.lib, "blance_plan_batch_wire"):
            raise BlanceError(abi.ERR_UNSUPPORTED, "this library has no blance_plan_batch_wire (build the current sources)")
        if node_names is None and state_names is None:
            names, node_names, state_names = names.part_names, names.node_names, names.state_names
        nm, keep = wire_names_struct(names, node_names, state_names)
        h = C.c_void_p()
        self._check(self.lib.blance_batch_names_create(C.byref(nm), len(names), len(node_names), len(state_names), C.byref(h)))
        del keep
        return BatchNames(self.lib, h, len(names), len(node_names), len(state_names))

    def plan_batch_wire(self, fps, names, stats=False, favor_min_nodes=None, beg_other=None):
        """blance_plan_batch_wire(): plan_batch_stats, and for each problem with a names object its plan as
        json.Marshal(PartitionMap) bytes from the same device call -- the bytes wire.encode makes of the decoded result.
        names: one BatchNames per problem (Planner.batch_names), None: no document for that problem; stats /
        favor_min_nodes / beg_other as in plan_batch_stats.  Returns ([FlatResult], [moves or None], [stats dict or None],
        [bytes or None], info dict)."""
        import numpy as np
        if not hasattr(self.lib, "blance_plan_batch_wire"):
            raise BlanceError(abi.ERR_UNSUPPORTED, "this library has no blance_plan_batch_wire (build the current sources)")
        fps = list(fps)
        n = len(fps)
        names = list(names)
        if len(names) != n:
            raise ValueError("names: one BatchNames or None per problem")
        results = [abi.FlatResult(fp) for fp in fps]
        structs = [fp.as_struct() for fp in fps]
        want = list(stats) if isinstance(stats, (list, tuple)) else [stats] * n
        if len(want) != n:
            raise ValueError("stats: one bool or one per problem")
        mv_ptrs, mv_state = self._moves_requests(fps, results, favor_min_nodes, beg_other)
        st_ptrs, st_state = self._stats_requests(fps, want)
        # the document requests as one numpy block viewed as blance_batch_wire[], all documents in one byte block
        ask = [i for i in range(n) if names[i] is not None]
        cap = np.array([self.lib.blance_batch_wire_capacity(C.byref(structs[i]), names[i]._h) for i in ask], dtype=np.int64)
        base = np.zeros(len(ask) + 1, np.int64)
        base[1:] = np.cumsum(cap)
        docs_block = np.empty(max(int(base[-1]), 1), dtype=np.uint8)
        wreq = np.zeros(max(len(ask), 1), dtype=abi.BATCH_WIRE_DTYPE)
        wreq["names"][:len(ask)] = [names[i]._h.value for i in ask]
        wreq["buf"][:len(ask)] = docs_block.ctypes.data + base[:-1]
        wreq["cap"][:len(ask)] = cap
        wr_ptrs = np.zeros(max(n, 1), dtype=np.uint64)
        wr_ptrs[ask] = wreq.ctypes.data + wreq.itemsize * np.arange(len(ask), dtype=np.uint64)
        pbs = (C.POINTER(abi.Problem) * max(n, 1))(*[C.pointer(s) for s in structs])
        rss = (C.POINTER(abi.Result) * max(n, 1))(*[C.pointer(r.struct) for r in results])
        info = abi.BatchInfo()
        self._adopted = False
        self._wire_adopted = None
        self._check(self.lib.blance_plan_batch_wire(self._h, n, pbs, rss,
                                                    mv_ptrs.ctypes.data_as(C.POINTER(C.POINTER(abi.BatchMoves))),
                                                    st_ptrs.ctypes.data_as(C.POINTER(C.POINTER(abi.PlanStats))),
                                                    wr_ptrs.ctypes.data_as(C.POINTER(C.POINTER(abi.BatchWire))),
                                                    C.byref(info)))
        docs = [None] * n
        need, starts = wreq["need"].tolist(), base.tolist()
        for j, i in enumerate(ask):
            docs[i] = docs_block[starts[j]:starts[j] + need[j]].tobytes()
        return (results, self._moves_unpack(mv_state), self._stats_unpack(st_state), docs,
                {name: getattr(info, name) for name, _ in abi.BatchInfo._fields_})

    def batch_dict(self, names, node_names=None, state_names=None):
        """blance_batch_dict_create(): the dictionary of one index, for plan_batch_docs.  names: a problem (its part_names,
        node_names, state_names), or the partition names with the two other lists beside them; str or bytes.  The ids of
        a document's names are their positions here: they must be the problem's ids."""
        if not hasattr(self.lib, "blance_plan_batch_docs"):
            raise BlanceError(abi.ERR_UNSUPPORTED, "this library has no blance_plan_batch_docs (build the current sources)")
        if node_names is None and state_names is None:
            names, node_names, state_names = names.part_names, names.node_names, names.state_names
        nm, keep = wire_names_struct(names, node_names, state_names)
        h = C.c_void_p()
        self._check(self.lib.blance_batch_dict_create(C.byref(nm), len(names), len(node_names), len(state_names), C.byref(h)))
        del keep
        return BatchDict(self.lib, h, names, node_names, state_names)

    def plan_batch_docs(self, fps, docs, dicts, assign_too=True, keep_prev_only=False, names=None, stats=False,
                        favor_min_nodes=None, poison=None):
        """blance_plan_batch_docs(): plan_batch_wire where problem i with docs[i] is not None is planned from that
        PartitionMap document (bytes), decoded on the device against dicts[i] (Planner.batch_dict): prevMap, and with
        assign_too the partitions to assign, are the document's; node_removed / node_added / nodes_to_add_nil are fps[i]'s.
        assign_too / keep_prev_only: one bool or one per problem; names / stats / favor_min_nodes as in plan_batch_wire
        (names None: no documents out).  Returns ([FlatResult or None], [moves or None], [stats or None], [bytes or None],
        [outcome dict or None], info dict): an outcome has status, refusal, refusal_at, why, why_at, n_node_refs,
        n_parts_seen; where its status is not 0 the problem was not planned, every other entry of that index is None and the
        caller takes the host route.  poison: a byte every output buffer is filled with beforehand; the entries of a refused
        index are then the untouched buffers (for tests)."""
        import numpy as np
        if not hasattr(self.lib, "blance_plan_batch_docs"):
            raise BlanceError(abi.ERR_UNSUPPORTED, "this library has no blance_plan_batch_docs (build the current sources)")
        fps = list(fps)
        n = len(fps)
        docs, dicts = list(docs), list(dicts)
        names = [None] * n if names is None else list(names)
        per = lambda v: list(v) if isinstance(v, (list, tuple)) else [v] * n
        a_too, keep_only, want = per(assign_too), per(keep_prev_only), per(stats)
        if not (len(docs) == len(dicts) == len(names) == len(a_too) == len(keep_only) == len(want) == n):
            raise ValueError("docs, dicts, names, assign_too, keep_prev_only, stats: one per problem")
        structs = [fp.as_struct() for fp in fps]
        dreq = (abi.BatchDoc * max(n, 1))()
        dc_ptrs = (C.POINTER(abi.BatchDoc) * max(n, 1))()
        keep = []
        rcaps, mcaps, wcaps = {}, {}, {}
        for i in range(n):
            if docs[i] is None:
                continue
            buf = C.create_string_buffer(bytes(docs[i]), len(docs[i]) + 1)
            keep.append(buf)
            d = dreq[i]
            d.dict = dicts[i]._h if dicts[i] is not None else None
            d.json, d.len = C.cast(buf, C.c_void_p).value, len(docs[i])
            d.assign_too, d.keep_prev_only = int(bool(a_too[i])), int(bool(keep_only[i]))
            d.status = d.refusal = d.why = -77                       # (the call writes all seven outputs)
            dc_ptrs[i] = C.pointer(d)
            rc, mc, wc = C.c_int64(), C.c_int64(), C.c_size_t()
            self._check(self.lib.blance_batch_doc_bounds(C.byref(structs[i]), C.byref(d), names[i]._h if names[i] is not None else None,
                                                         C.byref(rc), C.byref(mc), C.byref(wc)))
            rcaps[i], mcaps[i], wcaps[i] = rc.value, mc.value, wc.value
        results = [abi.FlatResult(_ResultShape(fp, rcaps[i]) if i in rcaps else fp) for i, fp in enumerate(fps)]
        mv_ptrs, mv_state = self._moves_requests(fps, results, favor_min_nodes, None, caps=mcaps)
        st_ptrs, st_state = self._stats_requests(fps, want)
        ask = [i for i in range(n) if names[i] is not None]
        cap = np.array([wcaps[i] if i in wcaps else self.lib.blance_batch_wire_capacity(C.byref(structs[i]), names[i]._h)
                        for i in ask], dtype=np.int64)
        base = np.zeros(len(ask) + 1, np.int64)
        base[1:] = np.cumsum(cap)
        docs_block = np.empty(max(int(base[-1]), 1), dtype=np.uint8)
        wreq = np.zeros(max(len(ask), 1), dtype=abi.BATCH_WIRE_DTYPE)
        wreq["names"][:len(ask)] = [names[i]._h.value for i in ask]
        wreq["buf"][:len(ask)] = docs_block.ctypes.data + base[:-1]
        wreq["cap"][:len(ask)] = cap
        wr_ptrs = np.zeros(max(n, 1), dtype=np.uint64)
        wr_ptrs[ask] = wreq.ctypes.data + wreq.itemsize * np.arange(len(ask), dtype=np.uint64)
        if poison is not None:
            for r in results:
                for a in (r.out_off, r.out_nodes, r.out_kind, r.warn_part, r.warn_state):
                    a.view(np.uint8)[:] = poison
            mv_state[5].view(np.uint8)[:] = poison
            st_state[5].view(np.uint8)[:] = poison
            docs_block[:] = poison
            wreq["need"][:] = poison
        pbs = (C.POINTER(abi.Problem) * max(n, 1))(*[C.pointer(s) for s in structs])
        rss = (C.POINTER(abi.Result) * max(n, 1))(*[C.pointer(r.struct) for r in results])
        info = abi.BatchInfo()
        self._adopted = False
        self._wire_adopted = None
        self._check(self.lib.blance_plan_batch_docs(self._h, n, pbs, rss,
                                                    mv_ptrs.ctypes.data_as(C.POINTER(C.POINTER(abi.BatchMoves))),
                                                    st_ptrs.ctypes.data_as(C.POINTER(C.POINTER(abi.PlanStats))),
                                                    wr_ptrs.ctypes.data_as(C.POINTER(C.POINTER(abi.BatchWire))),
                                                    dc_ptrs, C.byref(info)))
        outcomes = [None if docs[i] is None else {f: int(getattr(dreq[i], f)) for f in abi.BATCH_DOC_OUT} for i in range(n)]
        refused = [o is not None and o["status"] != 0 for o in outcomes]
        out_docs = [None] * n
        need, starts = wreq["need"].tolist(), base.tolist()
        for j, i in enumerate(ask):
            out_docs[i] = docs_block[starts[j]:starts[j + 1]] if refused[i] else docs_block[starts[j]:starts[j] + need[j]].tobytes()
        moves = self._moves_unpack_some(mv_state, refused)
        stats_out = self._stats_unpack(st_state)
        if poison is not None:                                    # the refused indexes: the raw, untouched buffers
            ask_mv, mbase, mblock = mv_state[1], mv_state[4], mv_state[5]
            for j, i in enumerate(ask_mv):
                if refused[i]:
                    moves[i] = mblock[int(mbase[j]):int(mbase[j + 1])]
        else:
            for i in range(n):
                if refused[i]:
                    results[i] = stats_out[i] = out_docs[i] = None
        return (results, moves, stats_out, out_docs, outcomes, {name: getattr(info, name) for name, _ in abi.BatchInfo._fields_})

    @staticmethod
    def _moves_unpack_some(state, skip):
        """_moves_unpack for the problems i with not skip[i] (the others' blocks were not written); None for the rest."""
        n, ask, P, cap, base, block, _, _ = state
        moves = [None] * n
        for j, i in enumerate(ask):
            if skip[i]:
                continue
            e = int(base[j]) + int(P[j]) + 1
            t, c = int(block[e - 1]), max(int(cap[j]), 1)
            moves[i] = (block[e - int(P[j]) - 1:e], block[e:e + t], block[e + c:e + c + t], block[e + 2 * c:e + 2 * c + t])
        return moves

    def plan_stats(self, n_states):
        """Per-state load statistics of the map the last plan produced (blance_plan_stats_get):
        dict of numpy arrays load_min / load_max / load_sum / load_sumsq / nodes_used / unmet_slots / rule_violations
        plus n_nodes_next."""
        import numpy as np
        a = {k: np.zeros(max(n_states, 1), dtype=np.int64) for k in ("load_min", "load_max", "load_sum", "load_sumsq", "unmet_slots", "rule_violations")}
        used = np.zeros(max(n_states, 1), dtype=np.int32)
        st = abi.PlanStats()
        st.n_states = n_states
        for k, v in a.items():
            setattr(st, k, v.ctypes.data_as(C.POINTER(C.c_int64)))
        st.nodes_used = used.ctypes.data_as(C.POINTER(C.c_int32))
        self._check(self.lib.blance_plan_stats_get(self._h, C.byref(st)))
        out = {k: v[:n_states] for k, v in a.items()}
        out["nodes_used"] = used[:n_states]
        out["n_nodes_next"] = int(st.n_nodes_next)
        return out

    def plan_moves(self, favor_min_nodes, beg_other=None, count_only=False, capacity=None, arena=None):
        """blance_plan_moves_get(): CalcPartitionMoves from prevMap as uploaded to the map the last plan / plan_resident of
        this planner produced, for every partition in partition id order, computed from the maps on the device.
        beg_other: None or (offsets [P + 1], node ids) of prevMap's keys outside the model; capacity: entries of the three
        move arrays (None: blance_plan_moves_capacity, which always suffices); arena: a HostArena for the output arrays.
        Returns ((op_off, op_node, op_state, op_kind), info) -- the arrays cut to the moves made -- or (None, info) when
        count_only; info: n_moves, n_by_kind {"add", "del", "promote", "demote"}, n_parts_moved, device_ms.  A capacity
        that is too small raises BlanceError(ERR_CAPACITY) with the counters in its `info`."""
        import numpy as np
        if not hasattr(self.lib, "blance_plan_moves_get"):
            raise BlanceError(abi.ERR_UNSUPPORTED, "this library has no blance_plan_moves_get (build the current sources)")
        mv = abi.PlanMoves()
        mv.favor_min_nodes = int(bool(favor_min_nodes))
        keep = []
        if beg_other is not None:
            off, nodes = [np.ascontiguousarray(a, dtype=np.int32) for a in beg_other]
            keep = [off, nodes if nodes.size else np.zeros(1, dtype=np.int32)]
            mv.beg_other_off, mv.beg_other_nodes = [a.ctypes.data_as(C.POINTER(C.c_int32)) for a in keep]
        out = None
        if not count_only:
            fp = getattr(self, "_fp", None)
            if fp is None:
                raise BlanceError(abi.ERR_BAD_ARG, "nothing planned yet")
            if capacity is None and getattr(self, "_wire_adopted", None) is not None:
                # prevMap is an adopted document: its entries, and the new plan's at most the result capacity
                capacity = sum(self._wire_adopted)
            if capacity is None and getattr(self, "_adopted", False):
                # prevMap is an adopted plan: at most the uploaded problem's result capacity, like the new plan
                capacity = 2 * fp.result_capacity()
            if capacity is None:
                capacity = int(self.lib.blance_plan_moves_capacity(C.byref(fp.as_struct()), C.byref(mv)))
            new = (lambda n, dt: np.empty(n, dtype=dt)) if arena is None else arena.empty
            out = [new(fp.scalars["n_parts"] + 1, np.int32)] + [new(max(int(capacity), 1), np.int32) for _ in range(3)]
            mv.out.op_off, mv.out.op_node, mv.out.op_state, mv.out.op_kind = [a.ctypes.data_as(C.POINTER(C.c_int32)) for a in out]
            mv.out.capacity = int(capacity)
        st = self.lib.blance_plan_moves_get(self._h, C.byref(mv))
        info = {"n_moves": int(mv.n_moves), "n_by_kind": {k: int(mv.n_by_kind[i]) for i, k in enumerate(abi.OP_NAMES)},
                "n_parts_moved": int(mv.n_parts_moved), "device_ms": float(mv.out.device_ms)}
        if st != abi.OK:
            err = BlanceError(st, (self.lib.blance_last_error() or b"").decode())
            err.info = info if st == abi.ERR_CAPACITY else None
            raise err
        if count_only:
            return None, info
        n = info["n_moves"]
        return (out[0], out[1][:n], out[2][:n], out[3][:n]), info

    def set_wire_names(self, names, node_names=None, state_names=None):
        """blance_plan_wire_names(): the names of the problem this planner holds (after upload / plan), for plan_wire.
        names: the problem (its part_names, node_names, state_names), or the partition names with the two other lists
        beside them; every name a str or bytes (bytes carry invalid UTF-8).  Whatever replaces the planner's problem drops
        the names (upload, plan, any plan_batch*); plan_resident keeps them."""
        import numpy as np
        if not hasattr(self.lib, "blance_plan_wire_names"):
            raise BlanceError(abi.ERR_UNSUPPORTED, "this library has no blance_plan_wire_names (build the current sources)")
        if node_names is None and state_names is None:
            names, node_names, state_names = names.part_names, names.node_names, names.state_names
        nm, keep = abi.WireNames(), []
        for field, strs in (("part", names), ("node", node_names), ("state", state_names)):
            raw = [x if isinstance(x, bytes) else x.encode("utf-8", "surrogatepass") for x in strs]
            off = np.zeros(len(raw) + 1, dtype=np.int64)
            if raw:
                off[1:] = np.cumsum([len(x) for x in raw])
            blob = b"".join(raw)
            buf = C.create_string_buffer(blob, len(blob) + 1)
            keep += [buf, off]
            setattr(nm, field + "_bytes", C.cast(buf, C.c_void_p).value)
            setattr(nm, field + "_off", off.ctypes.data)
        self._check(self.lib.blance_plan_wire_names(self._h, C.byref(nm)))

    def plan_wire(self, size_only=False, capacity=None, arena=None):
        """blance_plan_wire_get(): json.Marshal(PartitionMap) of the map the last plan / plan_resident of this planner
        produced, composed on the device -- the bytes wire.encode makes of the downloaded result.  Needs set_wire_names.
        capacity: bytes of the output buffer (None: a size-only call first, then exactly the document's length); arena: a
        HostArena for that buffer.  Returns (bytes, info), or (None, info) when size_only; info: need, device_ms.  A capacity
        that is too small raises BlanceError(ERR_CAPACITY) with `need` in its `info`."""
        import numpy as np
        if not hasattr(self.lib, "blance_plan_wire_get"):
            raise BlanceError(abi.ERR_UNSUPPORTED, "this library has no blance_plan_wire_get (build the current sources)")
        need, ms = C.c_size_t(0), C.c_double(0.0)

        def call(ptr, cap):
            st = self.lib.blance_plan_wire_get(self._h, ptr, cap, C.byref(need), C.byref(ms))
            info = {"need": int(need.value), "device_ms": float(ms.value)}
            if st != abi.OK:
                err = BlanceError(st, (self.lib.blance_last_error() or b"").decode())
                err.info = info if st == abi.ERR_CAPACITY else None
                raise err
            return info

        if size_only:
            return None, call(None, 0)
        if capacity is None:
            capacity = call(None, 0)["need"]
        new = (lambda n, dt: np.empty(n, dtype=dt)) if arena is None else arena.empty
        out = new(max(int(capacity), 1), np.uint8)
        info = call(out.ctypes.data, int(capacity))
        return out[:info["need"]].tobytes(), info

    def wire_dict(self, names, node_names=None, state_names=None):
        """blance_wire_dict_create(): the dictionary decode_wire decodes against.  names: a problem (its part_names,
        node_names, state_names), or the partition names with the two other lists beside them; str or bytes.  Independent of
        the problem the planner holds; it lives until its close() or the planner's."""
        if not hasattr(self.lib, "blance_wire_dict_create"):
            raise BlanceError(abi.ERR_UNSUPPORTED, "this library has no blance_wire_dict_create (build the current sources)")
        if node_names is None and state_names is None:
            names, node_names, state_names = names.part_names, names.node_names, names.state_names
        nm, keep = wire_names_struct(names, node_names, state_names)
        h = C.c_void_p()
        self._check(self.lib.blance_wire_dict_create(self._h, C.byref(nm), len(names), len(node_names), len(state_names), C.byref(h)))
        del keep
        return WireDict(self, h, names, node_names, state_names)

    def decode_wire(self, wdict, doc, count_only=False, capacity=None, arena=None):
        """blance_wire_decode_device(): the PartitionMap document `doc` (bytes, or a uint8 numpy array -- one from a HostArena
        is read by DMA where it lies) decoded on the device against `wdict`, into the layout of prev_* / assign_*.
        capacity: entries of `nodes` (None: a count-only call first, then exactly n_node_refs -- two calls: the document
        crosses the bus twice and the record split and the first parse run twice; a caller that decodes at the device's speed
        passes a capacity it knows, or a bound such as len(doc) // 3); arena: a HostArena for the output arrays.  Returns a dict: part_kind [P], off [P*M + 1], kind [P*M], nodes [n_node_refs] (None each when
        count_only or refused), n_node_refs, n_parts_seen, refusal (0: accepted, else abi.WIRE_REFUSED's code), refusal_at,
        device_ms, total_ms.  A refusal is returned, not raised: the caller takes the host decoder
        (planner.decode_partition_map does).  Every other error status raises; ERR_CAPACITY with the counters in `info`."""
        import numpy as np
        if not hasattr(self.lib, "blance_wire_decode_device"):
            raise BlanceError(abi.ERR_UNSUPPORTED, "this library has no blance_wire_decode_device (build the current sources)")
        if isinstance(doc, np.ndarray):
            src = np.ascontiguousarray(doc).view(np.uint8).reshape(-1)
            ptr, n = src.ctypes.data, int(src.size)
        else:
            src = bytes(doc)
            ptr, n = C.cast(C.c_char_p(src), C.c_void_p).value, len(src)
        P, M = wdict.n_parts, wdict.n_states

        def call(arrays, cap):
            wl = abi.WireLists()
            if arrays is not None:
                wl.part_kind, wl.off, wl.kind, wl.nodes = [a.ctypes.data for a in arrays]
            wl.capacity = cap
            st = self.lib.blance_wire_decode_device(self._h, wdict._h, ptr, n, C.byref(wl))
            info = {"n_node_refs": int(wl.n_node_refs), "n_parts_seen": int(wl.n_parts_seen), "refusal": int(wl.refusal),
                    "refusal_at": int(wl.refusal_at), "device_ms": float(wl.device_ms), "total_ms": float(wl.total_ms)}
            if st != abi.OK and not (st == abi.ERR_UNSUPPORTED and wl.refusal != 0):
                err = BlanceError(st, (self.lib.blance_last_error() or b"").decode())
                err.info = info if st == abi.ERR_CAPACITY else None
                raise err
            return info

        none = {"part_kind": None, "off": None, "kind": None, "nodes": None}
        if count_only:
            return dict(none, **call(None, 0))
        if capacity is None:
            first = call(None, 0)
            if first["refusal"]:
                return dict(none, **first)
            capacity = first["n_node_refs"]
        new = (lambda k, dt: np.empty(k, dtype=dt)) if arena is None else arena.empty
        arrays = [new(max(P, 1), np.uint8), new(P * M + 1, np.int32), new(max(P * M, 1), np.uint8), new(max(int(capacity), 1), np.int32)]
        info = call(arrays, int(capacity))
        if info["refusal"]:
            return dict(none, **info)
        return dict({"part_kind": arrays[0][:P], "off": arrays[1], "kind": arrays[2][:P * M],
                     "nodes": arrays[3][:info["n_node_refs"]]}, **info)

    def calc_moves(self, n_states, favor_min_nodes, beg_off, beg_nodes, end_off, end_nodes):
        """blance_calc_moves(): CalcPartitionMoves for every partition (CSR over
        p * (n_states + 1) + state).  Returns (op_off, op_node, op_state, op_kind, device_ms)."""
        import numpy as np
        arr = [np.ascontiguousarray(a, dtype=np.int32) for a in (beg_off, beg_nodes, end_off, end_nodes)]
        keep = [a if a.size else np.zeros(1, dtype=np.int32) for a in arr]
        P = (arr[0].size - 1) // (n_states + 1)
        pb = abi.MovesProblem()
        pb.n_parts, pb.n_states, pb.favor_min_nodes = P, n_states, int(bool(favor_min_nodes))
        pb.beg_off, pb.beg_nodes, pb.end_off, pb.end_nodes = [a.ctypes.data_as(C.POINTER(C.c_int32)) for a in keep]
        cap = int(arr[0][-1]) + int(arr[2][-1])
        out = [np.zeros(P + 1, dtype=np.int32)] + [np.zeros(max(cap, 1), dtype=np.int32) for _ in range(3)]
        res = abi.MovesResult()
        res.op_off, res.op_node, res.op_state, res.op_kind = [a.ctypes.data_as(C.POINTER(C.c_int32)) for a in out]
        res.capacity = cap
        self._check(self.lib.blance_calc_moves(self._h, C.byref(pb), C.byref(res)))
        return out[0], out[1], out[2], out[3], float(res.device_ms)

    def upload(self, fp):
        self._fp = fp
        self._adopted = False
        self._wire_adopted = None
        self._check(self.lib.blance_upload(self._h, C.byref(fp.as_struct())))

    def adopt(self, node_removed=None, node_added=None, nodes_to_add_nil=True, keep_prev_only=False):
        """blance_plan_adopt(): the map the last plan / plan_resident produced becomes prevMap and partitionsToAssign of the
        problem this planner holds, where it lies on the device (problem.adopted_problem is the definition), with the node
        change of the next call: node_removed / node_added [n_nodes_ext] (None: all zero).  plan_resident then plans it;
        the names of set_wire_names and every WireDict stay valid.  The round loop:
        adopt -> plan_resident -> plan_moves -> plan_wire."""
        import numpy as np
        if not hasattr(self.lib, "blance_plan_adopt"):
            raise BlanceError(abi.ERR_UNSUPPORTED, "this library has no blance_plan_adopt (build the current sources)")
        fp = getattr(self, "_fp", None)
        if fp is None:
            raise BlanceError(abi.ERR_BAD_ARG, "nothing planned yet")
        NX = fp.scalars["n_nodes_ext"]
        arrs = []
        for a in (node_removed, node_added):
            a = np.zeros(NX, dtype=np.uint8) if a is None else np.ascontiguousarray(a, dtype=np.uint8)
            if a.size != NX:
                raise ValueError("node_removed / node_added: one byte per node name of the problem (%d)" % NX)
            arrs.append(a if a.size else np.zeros(1, dtype=np.uint8))
        ad = abi.Adopt()
        ad.node_removed, ad.node_added = [a.ctypes.data_as(C.POINTER(C.c_uint8)) for a in arrs]
        ad.nodes_to_add_nil = int(bool(nodes_to_add_nil))
        ad.keep_prev_only = int(bool(keep_prev_only))
        self._check(self.lib.blance_plan_adopt(self._h, C.byref(ad)))
        self._adopted = True
        if getattr(self, "_wire_adopted", None) is not None:     # (an adopted plan is no larger than the capacity it was planned with)
            self._wire_adopted = (self._wire_adopted[0], self._wire_adopted[0])

    def adopt_wire(self, wdict, doc, node_removed=None, node_added=None, nodes_to_add_nil=True, assign_too=True,
                   keep_prev_only=False):
        """blance_wire_adopt(): the PartitionMap document `doc` (bytes, or a uint8 numpy array -- one from a HostArena is read
        by DMA where it lies), decoded on the device against `wdict`, becomes prevMap -- and with assign_too the partitions to
        assign -- of the problem this planner holds, where the decoder left it (problem.wire_adopted_problem is the
        definition), with the node change of the next call.  Needs an uploaded problem, not a plan.  Returns a dict: refusal,
        refusal_at (the document's own refusal, as decode_wire reports it), why, why_at (abi.WIRE_ADOPT: the document decoded
        but the problem cannot be taken), n_node_refs, n_parts_seen, result_capacity, device_ms, total_ms, and adopted: True
        when the planner now holds the new problem.  Both kinds of refusal are returned, not raised -- the planner is then as
        it was; planner.adopt_partition_map is the switch to the host route.  Every other error status raises."""
        import numpy as np
        if not hasattr(self.lib, "blance_wire_adopt"):
            raise BlanceError(abi.ERR_UNSUPPORTED, "this library has no blance_wire_adopt (build the current sources)")
        fp = getattr(self, "_fp", None)
        if fp is None:
            raise BlanceError(abi.ERR_BAD_ARG, "nothing uploaded yet")
        NX = fp.scalars["n_nodes_ext"]
        arrs = []
        for a in (node_removed, node_added):
            a = np.zeros(NX, dtype=np.uint8) if a is None else np.ascontiguousarray(a, dtype=np.uint8)
            if a.size != NX:
                raise ValueError("node_removed / node_added: one byte per node name of the problem (%d)" % NX)
            arrs.append(a if a.size else np.zeros(1, dtype=np.uint8))
        if isinstance(doc, np.ndarray):
            src = np.ascontiguousarray(doc).view(np.uint8).reshape(-1)
            ptr, n = src.ctypes.data, int(src.size)
        else:
            src = bytes(doc)
            ptr, n = C.cast(C.c_char_p(src), C.c_void_p).value, len(src)
        wa = abi.WireAdopt()
        wa.dict, wa.json, wa.len = wdict._h, ptr, n
        wa.node_removed, wa.node_added = [a.ctypes.data_as(C.POINTER(C.c_uint8)) for a in arrs]
        wa.nodes_to_add_nil = int(bool(nodes_to_add_nil))
        wa.assign_too = int(bool(assign_too))
        wa.keep_prev_only = int(bool(keep_prev_only))
        st = self.lib.blance_wire_adopt(self._h, C.byref(wa))
        info = {name: getattr(wa, name) for name in ("refusal", "refusal_at", "why", "why_at", "n_node_refs", "n_parts_seen",
                                                     "result_capacity", "device_ms", "total_ms")}
        info["adopted"] = st == abi.OK
        if st != abi.OK and not (st == abi.ERR_UNSUPPORTED and (wa.refusal != 0 or wa.why != 0)):
            raise BlanceError(st, (self.lib.blance_last_error() or b"").decode())
        if st == abi.OK:
            self._adopted = True
            # what download() and plan_moves size their arrays by: the new problem's result capacity and prevMap entries
            self._wire_adopted = (int(wa.result_capacity), int(wa.n_node_refs))
        return info

    def plan_resident(self):
        """Run the whole planNextMapEx loop on the uploaded problem; returns the
        timing/statistics part of blance_result."""
        r = abi.Result()
        self._check(self.lib.blance_plan_resident(self._h, C.byref(r)))
        return r

    def download(self, arena=None, into=None):
        """arena: a HostArena -- the result's arrays in page-locked memory (the device writes them by DMA); into: a FlatResult
        of an earlier download of the same problem shape, written again (no allocation)."""
        shape = self._fp
        if into is None and getattr(self, "_wire_adopted", None) is not None:
            shape = _ResultShape(self._fp, self._wire_adopted[0])
        res = into if into is not None else abi.FlatResult(shape, arena)
        self._check(self.lib.blance_download(self._h, C.byref(res.struct)))
        return res
