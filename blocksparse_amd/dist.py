"""Data-parallel use of the hot path: replicate layout tables and W, shard the minibatch N over ranks
(one process per GPU), sum the partial weight gradients with ONE all-reduce per step.  fprop/bprop need no
communication: every minibatch column is independent.  Replaces the reference's AllreduceNccl op
for this path (/root/reference/src/nccl_op.cc:166-201, blocksparse/nccl.py:27-56).

On ROCm devices the collective is RCCL over xGMI, called through the library's own C entry points
(include/bsmm_dist.h: communicator + side stream + two events per handle, the record-on-compute / wait-on-comm
pattern of src/nccl_op.cc:513,168) -- no Python-side async machinery between the kernels of a step.
``torch.distributed`` is only the bootstrap channel that carries the 128-byte RCCL id from rank 0 to the others
(any backend), and the data path for CPU tensors in the gloo tests."""
import ctypes

import torch
import torch.distributed as dist


def shard_bounds(N, rank, world):
    """Contiguous, balanced split of N minibatch columns: the first N % world ranks get one extra."""
    q, r = divmod(N, world)
    lo = rank * q + min(rank, r)
    return lo, lo + q + (1 if rank < r else 0)


def shard_minibatch(t, feature_axis, rank, world):
    """This rank's slice of an activation tensor: columns for axis 0 (C, N), rows for axis 1 (N, C)."""
    if feature_axis == 0:
        flat = t.reshape(t.shape[0], -1)
        lo, hi = shard_bounds(flat.shape[1], rank, world)
        return flat[:, lo:hi].contiguous()
    flat = t.reshape(-1, t.shape[-1])
    lo, hi = shard_bounds(flat.shape[0], rank, world)
    return flat[lo:hi].contiguous()


def sums_capacity(sums):
    """floats the storage of ``sums`` holds from its first element on (a view of an updat workspace has the padding the fused
    reduction needs behind it; a clone or an accumulated tensor is exactly sized)"""
    return int((sums.untyped_storage().nbytes() - sums.storage_offset() * sums.element_size()) // 4)


class RcclComm(object):
    """One RCCL communicator of the library (bsmm_dist_*) for this process' device.  world == 1 needs no bootstrap;
    otherwise torch.distributed (already initialised, any backend) broadcasts rank 0's id."""

    def __init__(self, device=None, group=None):
        from . import _lib
        self._lib = _lib.load()
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        if dist.is_initialized():
            self.rank, self.world = dist.get_rank(group), dist.get_world_size(group)
        else:
            self.rank, self.world = 0, 1
        ident = ctypes.create_string_buffer(128)
        rc = 0
        if self.rank == 0:
            rc = self._lib.bsmm_dist_unique_id(ident)
        if self.world > 1:
            # every rank takes part in the broadcast whatever happened on rank 0 (a rank that raised before it would leave the
            # others blocked in a collective nobody matches); rank 0's verdict travels with the id
            box = [(rc, ident.raw)]
            dist.broadcast_object_list(box, src=0, group=group)
            rc, raw = box[0]
            ident = ctypes.create_string_buffer(raw, 128)
        _lib.check(rc, "bsmm_dist_unique_id (rank 0)")
        h = ctypes.c_void_p()
        _lib.check(self._lib.bsmm_dist_create(ctypes.byref(h), ident, self.rank, self.world, self.device.index or 0), "bsmm_dist_create")
        self._h = h
        self._check, self._dtype_code = _lib.check, _lib.require_dtype_code

    def begin(self, t):
        """in-place all-reduce(sum) of a contiguous CUDA tensor, ordered after the work enqueued so far on the current stream"""
        st = torch.cuda.current_stream(t.device).cuda_stream
        self._check(self._lib.bsmm_dist_allreduce_begin(self._h, t.data_ptr(), t.numel(), self._dtype_code(t.dtype), st), "bsmm_dist_allreduce_begin")

    def end(self):
        """make the current stream wait for the collective"""
        st = torch.cuda.current_stream(self.device).cuda_stream
        self._check(self._lib.bsmm_dist_allreduce_end(self._h, st), "bsmm_dist_allreduce_end")

    def shard_elems(self, blocks, bsize):
        return int(self._lib.bsmm_dist_dw_shard_elems(self.world, blocks, bsize))

    def dw_begin(self, sums, dw, staging, gate, blocks, bsize, alpha, beta):
        """fused reduction of the weight gradient (bsmm_dist_dw_begin): reduce-scatter of the fp32 sums, finalize of this rank's
        shard, all-gather of the finished shards into ``dw`` -- all on the handle's stream, ordered after the current stream.
        ``sums`` must have room for world * shard floats behind its first element (the library checks the capacity we declare:
        what the tensor's storage really holds)."""
        st = torch.cuda.current_stream(dw.device).cuda_stream
        self._check(self._lib.bsmm_dist_dw_begin(self._h, sums.data_ptr(), sums_capacity(sums), dw.data_ptr(), staging.data_ptr(),
                                                 gate.data_ptr() if gate is not None else None, blocks, bsize, self._dtype_code(dw.dtype),
                                                 alpha, beta, st), "bsmm_dist_dw_begin")

    def close(self):
        if self._h:
            self._lib.bsmm_dist_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DwAllReduce(object):
    """Sum partial dw over ranks, overlapped with whatever the caller enqueues next (normally bprop).

    start(t) issues the collective and returns at once; wait() makes the current stream wait for it.  CUDA tensors go
    through the library's RCCL handle (``comm``, created on first use) IN PLACE -- pass the fp32 sums of
    ``BlocksparseMatMul.updat(sums_only=True)`` and the cross-rank sum is never rounded to 16 bit; a 16-bit tensor is
    reduced in its own type unless ``accumulate_fp32`` (then through an fp32 copy).  CPU tensors (gloo tests) use
    torch.distributed."""

    def __init__(self, group=None, accumulate_fp32=False, comm=None, force=False):
        self.group = group
        self.accumulate_fp32 = accumulate_fp32
        self.comm = comm
        self.force = force          # run the RCCL path also at world size 1 (self-test of the overlap machinery)
        self._work = None
        self._buf = None
        self._dst = None
        self._direct = False
        self._fallback = False      # True: the library handle could not be made on every rank -> torch.distributed collectives

    @property
    def via(self):
        return "torch.distributed" if self._fallback else "bsmm_dist (library RCCL handle)"

    def _active(self):
        return self.force or (dist.is_initialized() and dist.get_world_size(self.group) > 1)

    def start(self, t):
        self._direct = False
        if not self._active():
            return t
        if t.is_cuda and self.comm is None and not self._fallback:
            # the library's own communicator; every rank must end up on the same path, so the ranks agree on whether all of
            # them got one (otherwise: torch.distributed's collective on the same tensor, said loudly on stderr)
            try:
                self.comm = RcclComm(t.device, self.group)
                ok = 1
            except Exception as e:          # noqa: BLE001 -- any failure of the bootstrap means "use the other path"
                self.comm, ok = None, 0
                import sys
                print("blocksparse_amd.dist: library RCCL handle unavailable (%s); falling back to torch.distributed" % (e,), file=sys.stderr)
            if dist.is_initialized() and dist.get_world_size(self.group) > 1:
                flag = torch.tensor([ok], device=t.device, dtype=torch.int32)
                dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=self.group)
                ok = int(flag.item())
            if not ok:
                if self.comm is not None:
                    self.comm.close()
                self.comm, self._fallback = None, True
                if not dist.is_initialized():
                    raise RuntimeError("blocksparse_amd.dist: no RCCL handle and torch.distributed is not initialised")
        if t.is_cuda and self.comm is not None:
            if self.accumulate_fp32 and t.dtype != torch.float32:
                if self._buf is None or self._buf.shape != t.shape:
                    self._buf = torch.empty(t.shape, dtype=torch.float32, device=t.device)
                self._buf.copy_(t)
                self._dst = t
                self.comm.begin(self._buf)
            else:
                self._dst = None
                self._buf = t                      # keep the tensor alive until wait(): the collective runs on another stream
                self.comm.begin(t)
            self._direct = True
            return t
        if self.accumulate_fp32 and t.dtype != torch.float32:
            self._buf = t.float()
            self._dst = t
        else:
            self._buf = t
            self._dst = None
        self._work = dist.all_reduce(self._buf, op=dist.ReduceOp.SUM, group=self.group, async_op=True)
        return t

    def wait(self):
        if self._direct:
            self.comm.end()
            if self._dst is not None:
                self._dst.copy_(self._buf)
                self._dst = None
            else:
                self._buf = None
            self._direct = False
            return
        if self._work is not None:
            self._work.wait()
            self._work = None
            if self._dst is not None:
                self._dst.copy_(self._buf)
        self._buf = None
        self._dst = None


class DwReduce(object):
    """The data-parallel weight-gradient reduction of one ``BlocksparseMatMul`` (bsize-32 streaming updat), fused:

        sums = bsmm.updat(x, dy, sums_only=True)        # this rank's raw fp32 sums
        red.start(sums, dw, alpha, beta, gate)          # reduce-scatter(fp32) -> finalize 1/world -> all-gather(storage type) -> dw
        ... bprop, the next step's fprop ...            # dw is not needed before the optimiser
        red.wait()

    25 % fewer bytes on the wire than an fp32 all-reduce, 1 / world of the finalize per rank, ONE rounding after the cross-rank
    sum (the reference all-reduces fp16 gradients, src/nccl_op.cc:166-201).  CUDA tensors go through the library's RCCL handle
    (include/bsmm_dist.h) -- the collectives are issued from C on the handle's own stream; CPU tensors (gloo tests) through
    torch.distributed with the same arithmetic.  ``force`` runs the RCCL path at world size 1 too (self-test)."""

    def __init__(self, bsmm, group=None, comm=None, force=False):
        self.bsmm, self.group, self.comm, self.force = bsmm, group, comm, force
        self._staging = None
        self._hold = None
        self._cpu = None

    @property
    def via(self):
        return "bsmm_dist_dw (library RCCL handle: reduce-scatter f32 + shard finalize + all-gather)"

    def _active(self):
        return self.force or (dist.is_initialized() and dist.get_world_size(self.group) > 1)

    def start(self, sums, dw, alpha=1.0, beta=0.0, gate=None):
        b = self.bsmm
        if not self._active():
            b.updat_finalize(sums, alpha=alpha, beta=beta, dw=dw, gate=gate)
            return dw
        if not sums.is_cuda:          # gloo: the SAME three steps and shard arithmetic (bsmm_dist_dw_layout) through torch.distributed
            from . import _lib
            rank, world = dist.get_rank(self.group), dist.get_world_size(self.group)
            total = b.blocks * b.bsize * b.bsize
            shard, lo, hi, cap = _lib.dw_layout(world, rank, b.blocks, b.bsize)
            padded = torch.zeros(cap, dtype=torch.float32)
            padded[:total] = sums.reshape(-1)
            # 1. reduce-scatter of `world` shard-sized pieces (gloo has no reduce_scatter: one reduce per owner)
            works = [dist.reduce(padded[r * shard:(r + 1) * shard], dst=dist.get_global_rank(self.group, r) if self.group is not None else r,
                                 op=dist.ReduceOp.SUM, group=self.group, async_op=True) for r in range(world)]
            self._cpu = (works, padded, dw, alpha, beta, gate, (rank, world, total, shard, lo, hi))
            return dw
        if self.comm is None:
            self.comm = RcclComm(sums.device, self.group)      # raises on every rank alike if rank 0 could not make an id
        shard = self.comm.shard_elems(b.blocks, b.bsize)
        need = self.comm.world * shard
        if self._staging is None or self._staging.numel() < need or self._staging.dtype != dw.dtype:
            self._staging = torch.empty(need, dtype=dw.dtype, device=dw.device)
        if sums_capacity(sums) < need:
            # an exactly-sized tensor (a clone, accumulated sums): the reduce-scatter works on world * shard floats -- give it the room
            # (the library refuses a short buffer with BSMM_ERR_WORKSPACE instead of reading past its end)
            padded = torch.zeros(need, dtype=torch.float32, device=sums.device)
            padded[:sums.numel()] = sums.reshape(-1)
            sums = padded
        self._hold = (sums, dw, gate)                           # alive until wait(): the work runs on the handle's stream
        self.comm.dw_begin(sums, dw, self._staging, gate, b.blocks, b.bsize, alpha, beta)
        return dw

    def wait(self):
        if self._cpu is not None:
            works, padded, dw, alpha, beta, gate, (rank, world, total, shard, lo, hi) = self._cpu
            for wk in works:
                wk.wait()
            # 2. alpha / beta / gate and the ONE rounding on this rank's elements [lo, hi) only
            staging = torch.zeros(world * shard, dtype=dw.dtype)
            if hi > lo:
                v = padded[lo:hi] * alpha
                if gate is not None:
                    v = v * gate.reshape(-1)[torch.arange(lo, hi) // (self.bsmm.bsize * self.bsmm.bsize)]
                if beta != 0.0:
                    v = v + beta * dw.reshape(-1)[lo:hi].float()
                staging[lo:hi] = v.to(dw.dtype)
            # 3. all-gather of the shard-sized pieces in the storage type, then the copy into dw
            pieces = [torch.empty(shard, dtype=dw.dtype) for _ in range(world)]
            dist.all_gather(pieces, staging[rank * shard:(rank + 1) * shard].clone(), group=self.group)
            dw.copy_(torch.cat(pieces)[:total].reshape(dw.shape))
            self._cpu = None
            return
        if self._hold is not None:
            self.comm.end()
            self._hold = None
