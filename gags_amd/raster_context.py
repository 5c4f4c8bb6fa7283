"""What `rasterization(...)` remembers or is told between calls: the RasterContext, its persistent gradient buffer
(_KeptGrad), and the two ways a 4-byte count comes back from the device (_read_count, _DeferredCount)."""
import ctypes
import threading

import torch

from . import _lib
from . import raster_tunables as T
from ._lib import check, ptr


def _dev_key(dev):
    """The device's index as a dictionary key (a bare "cuda" is the current device)."""
    return dev.index if dev.index is not None else torch.cuda.current_device()


class RasterContext:
    """Everything `rasterization(...)` remembers or is told between calls -- SURVEY 8b asks for a boundary that is
    "re-entrant per stream, no global state": the C library has none, and the Python layer keeps its own in an object the
    caller may own.  `rasterization(..., context=ctx)` / `render(..., context=ctx)` use `ctx`; without one, the calling
    THREAD's default context (default_context()) is used, so two renderers in one process -- a training view inside a
    gradient-exchange block and an evaluation view, two threads -- never see each other's hooks or capacities.

    grad_range_hook / grad_rows_hook / grad_range_channels
        Multi-GPU by-view step (gags_amd/dist.py: OverlappedGradReducer): when grad_range_hook is set, the staged
        colours-only backward produces the feature gradient one channel range at a time and calls
            grad_range_hook(v_colors_alias [N,D], ch_begin, ch_end)
        right after the kernels of each range were enqueued, so that the exchange of one range overlaps the computation of
        the next (the alias shares storage with the tensor handed to autograd).  With grad_rows_hook also set, the backward
        first calls grad_rows_hook(mask uint8 [N]): mask[g] = 1 for every Gaussian that blended into a pixel of this view,
        i.e. the only rows of the gradient that can be non-zero ("gradients are sparse in rows").
        With grad_wire_hook set, the backward asks it before the reduce stage of every range,
            grad_wire_hook(ch_begin, ch_end) -> (pos int32 [N], wire fp32 [rows, ch_end - ch_begin]) or None,
        and the reduce kernel writes row pos[g] of `wire` for every Gaussian with pos[g] >= 0 next to the gradient itself
        (gags_raster_bwd_colors_staged: wire_pos, wire); grad_range_hook then gets `wire` as a fourth argument.  grad_range_channels: an
        int or a tuple of range widths (see GRAD_RANGE_CHANNELS).
    capacity_mode, cap_isects, cap_rows
        Capacity mode (OFF by default): the two counts a view produces on the device -- tile intersections, partial
        gradient rows -- are NOT waited for before the kernels that need them are launched.  Buffers are sized by a capacity
        remembered from earlier views of the same (N, width, height), the kernels take their ranges from device memory
        (isect_offsets' last entry, sentinel keys), and the counts are read from a second stream once everything is
        enqueued: the host still learns them (info["n_isects"] is exact, capacities are checked) but the queue never
        drains.  A count above its capacity -- nothing is written out of bounds -- re-runs that pass with exact sizes; the
        first view of a shape runs the exact path.  Measured A/B on one box (C3, D = 512 / D = 16): 10.76-10.94 ms
        against 10.62-10.68 ms, 2.59 against 2.51-2.54 ms with a 25 % margin -- the two readbacks cost the GPU ~40 us of
        idle queue per step (the host is far ahead of the device), the sentinel keys cost more in the two sorts.  Kept as a
        switch for callers whose host is the bottleneck.
    overlap_zero_fill
        Experiment, OFF: zero-fill the colour gradient on a second stream during the forward's binning and let the reduce
        stage write only the rows that exist (GAGS_STAGED_PREZEROED; 73 % of the Gaussians blend nothing at C3).  Measured at C3:
        reduce 1.27 -> 0.95 ms, but the fill kernel takes the CUs from whatever it runs beside -- under the rows kernel that
        kernel slowed by 0.38 ms, under the binning kernels the step grew by 1.7 ms.  The C-ABI flag stays for callers
        that own a zeroed buffer anyway.
    early_rowmap
        ON by default (GAGS_EARLY_ROWMAP=0): the staged backward begins by numbering the view's partial gradient rows (a prefix
        sum over the forward's hit flags, gags_bwd_rowmap) and has to know their COUNT on the host before it can size its
        scratch -- a 4-byte readback in the middle of the backward, with the launch queue drained around it (60-90 us).  None of
        that depends on the cotangent: a forward that will be differentiated w.r.t. the colours alone enqueues the row map right
        behind its own kernels and sends the count to pinned memory; by the time the loss has been computed it has long arrived
        and the backward opens with the rows kernel.  A forward that is never differentiated has run 0.12 ms of small kernels for nothing.
    Also here: the pinned 4-byte buffers of the deferred count readbacks, the side streams, and render()'s cache of the
    intrinsics matrix."""

    def __init__(self, capacity_mode=None, overlap_zero_fill=False):
        self.grad_range_hook = None
        self.grad_rows_hook = None
        self.grad_wire_hook = None
        self.grad_range_channels = T.GRAD_RANGE_CHANNELS
        self.grad_rows_group = T.GRAD_ROWS_GROUP
        self.capacity_mode = T.CAPACITY_MODE if capacity_mode is None else bool(capacity_mode)
        self.cap_isects = {}
        self.cap_rows = {}
        self.overlap_zero_fill = bool(overlap_zero_fill)
        # the backward's row map enqueued behind the forward, its count on the way to the host meanwhile (_early_rowmap)
        self.early_rowmap = T.EARLY_ROWMAP
        self._pinned_pool = {}
        self.k_cache = {}
        self._pinned = {}
        self._side = {}
        # list trimming for heavy views (_trim_lists): None = automatic above TRIM_AUTO_BYTES of forward scratch
        self.trim_lists = T.TRIM_LISTS
        # persistent gradient buffer of the colours-only backward (_KeptGrad): on unless GAGS_KEEP_GRAD=0
        self.keep_grad_buffer = T.KEEP_GRAD
        self._kept = {}        # (n, d, dtype, device) -> _KeptGrad, at most KEEP_GRAD_SHAPES shapes (least recently used out)
        self._kept_fails = {}  # consecutive steps that found the buffer still referenced / written

    def forget_kept(self, n, d, dtype, dev):
        self._kept.pop((n, d, dtype, dev.index), None)

    def forget_all_kept(self):
        self._kept.clear()

    def kept_grad(self, n, d, dtype, dev):
        """(alias, flags_prev, flags_cur) of this shape's persistent gradient buffer, or None when it is not to be used."""
        if not self.keep_grad_buffer or not _CAN_COUNT_REFS or n * d < T.KEEP_GRAD_MIN_ELEMS or n == 0:
            return None
        key = (n, d, dtype, dev.index)
        if self._kept_fails.get(key, 0) >= 3:
            return None
        ent = self._kept.pop(key, None)
        if ent is not None and ent.released() and not ent.untouched():
            # written since it was handed out (an in-place collective, an optimizer's clipping, grad_written()) and released
            # again: its rows are no longer "zero except last step's", but nobody else holds the storage -- start over from a
            # clean buffer (one fill, what a fresh torch.zeros would cost, without the allocation) and do not count the step
            # towards the switch-off: a loop that reduces its gradient in place every step keeps the one buffer
            ent.wipe()
        if ent is not None and not ent.untouched():
            self._kept_fails[key] = self._kept_fails.get(key, 0) + 1  # the holder keeps that storage; a new one below
            ent = None
            if self._kept_fails[key] >= 3:
                return None
        elif ent is not None:
            self._kept_fails[key] = 0
        if ent is None:
            ent = _KeptGrad(n, d, dtype, dev)
        self._kept[key] = ent  # (re-inserted last: most recently used)
        while len(self._kept) > T.KEEP_GRAD_SHAPES:
            self._kept.pop(next(iter(self._kept)))
        return ent.hand_out()

    def side_stream(self, dev):
        key = _dev_key(dev)
        if key not in self._side:
            self._side[key] = torch.cuda.Stream(device=dev)
        return self._side[key]

    def take_pinned(self, dev):
        """A pinned int32 of the caller's own (returned with give_pinned): counts of several forwards may be in flight."""
        key = _dev_key(dev)
        pool = self._pinned_pool.setdefault(key, [])
        return pool.pop() if pool else torch.empty(1, dtype=torch.int32).pin_memory()

    def give_pinned(self, dev, t):
        key = _dev_key(dev)
        pool = self._pinned_pool.setdefault(key, [])
        if len(pool) < 8:
            pool.append(t)

    def pinned_i64(self, dev):
        key = ("i64", _dev_key(dev))
        if key not in self._pinned:
            self._pinned[key] = torch.empty(1, dtype=torch.int64).pin_memory()
        return self._pinned[key]

    def pinned_i32(self, dev):
        key = _dev_key(dev)
        if key not in self._pinned:
            self._pinned[key] = torch.empty(1, dtype=torch.int32).pin_memory()
        return self._pinned[key]


def grad_written(grad):
    """Tell the library that `grad` -- a gradient this package's backward produced, e.g. `pc._semantic_feature.grad` -- was
    written by something torch's version counter does not see: a c10d collective (`dist.all_reduce(p.grad)` leaves
    `_version` alone), a DLPack consumer, a kernel launched on its data_ptr().  The persistent gradient buffer
    (_KeptGrad) then starts the next step from zeros instead of trusting that only last step's flagged rows are non-zero.
    Every writer inside this package calls it itself (gags_amd/dist.py: reduce_feature_grad); torch's own in-place operators
    need nothing.  Returns `grad`.  (memory model; GAGS_KEEP_GRAD=0 turns the buffer off altogether.)"""
    torch.autograd.graph.increment_version(grad)
    return grad


_TLS = threading.local()


def default_context():
    """The calling thread's own RasterContext (created on first use)."""
    ctx = getattr(_TLS, "ctx", None)
    if ctx is None:
        ctx = _TLS.ctx = RasterContext()
    return ctx


def _storage_refs(t):
    """References to `t`'s storage (the temporary made here included: only compared with a baseline taken the same way)."""
    return torch._C._storage_Use_Count(t.untyped_storage()._cdata)


# (a private torch binding: without it nobody can tell whether a buffer is still held elsewhere, and the mechanism stays off)
_CAN_COUNT_REFS = hasattr(torch._C, "_storage_Use_Count")


class _KeptGrad:
    """The persistent gradient buffer of the colours-only backward (RasterContext.keep_grad_buffer).  d loss / d colors is a
    dense [N, D] tensor of which 73 % of the rows are zero at C3 (Gaussians that blend nothing); written afresh every step
    those zeros are 2.2 GB of HBM writes.  Here the context keeps ONE zero-initialised buffer per (N, D, dtype), every
    backward hands autograd a fresh alias of it (own TensorImpl, same storage: autograd adopts it without a copy) and the
    reduce stage only writes the rows that have partial rows now and re-zeroes the rows that had some in the previous step
    (two flag arrays: keep_prev / keep_cur of gags_raster_bwd_colors_staged).  The buffer is only reused when NOBODY else still refers to its
    storage (reference count back at its baseline: the previous step's .grad was released, e.g. zero_grad(set_to_none=True)
    or `.grad = None`) and nobody wrote to it in place (version counter unchanged: torch's in-place operators move it, this
    package's own writers of a gradient -- dist.reduce_feature_grad -- move it through grad_written(), and a caller whose own
    collective or kernel writes a gradient must call grad_written() too: c10d collectives and raw pointers leave the counter
    alone; the staged backward's kernels are the one writer that does not, on purpose).  A buffer that was written and then
    released is wiped and used again; one that is still held stays with its holder and this step runs on a new buffer, and
    after three such steps in a row the mechanism switches itself off for the shape (a loop that accumulates into a live
    .grad)."""

    def __init__(self, n, d, dtype, dev):
        self.buf = torch.zeros(n, d, dtype=dtype, device=dev)
        self.flags = torch.zeros(2, max(n, 1), dtype=torch.uint8, device=dev)
        self.cur = 0
        self.base = _storage_refs(self.buf)
        self.version = self.buf._version

    def released(self):
        return _storage_refs(self.buf) <= self.base

    def untouched(self):
        return self.released() and self.buf._version == self.version

    def wipe(self):
        """Back to the state of a new buffer, in place (only when released(): nobody else reads this storage)."""
        self.buf.zero_()
        self.flags.zero_()
        self.version = self.buf._version

    def hand_out(self):
        prev, cur = self.flags[self.cur], self.flags[1 - self.cur]
        self.cur ^= 1
        return self.buf.detach(), prev, cur


def _read_count(lib, total):
    """The int32 `total` holds on the device, on the host: a blocking 4-byte readback behind the current stream."""
    host = ctypes.c_int32(0)
    check(lib.gags_read_i32(ptr(total), ctypes.byref(host), _lib.stream()), "gags_read_i32")
    return int(host.value)


class _DeferredCount:
    """A device-side int32 read back without draining the launch stream: the copy runs on a second stream behind an
    event recorded right after the kernel that produced the value."""

    def __init__(self, scalar, rctx):
        self.t = scalar
        self.rctx = rctx
        self.ev = torch.cuda.Event()
        self.ev.record()

    def get(self):
        dev = self.t.device
        side = self.rctx.side_stream(dev)
        host = self.rctx.pinned_i32(dev)
        done = torch.cuda.Event()
        with torch.cuda.stream(side):
            side.wait_event(self.ev)
            host.copy_(self.t, non_blocking=True)
            done.record()
        self.t.record_stream(side)
        done.synchronize()
        return int(host[0])
