"""`rasterization(...)`: the operator the reference imports from gsplat
(/root/reference/gaussian_renderer/__init__.py:17,56-70), re-implemented on hand-written
gfx950 kernels behind the C ABI of include/gags_raster.h.

Same names, argument meaning, return triple and `info` keys as the call the reference makes:
    render_colors [1,H,W,D'], render_alphas [1,H,W,1], info = rasterization(
        means=[N,3], quats=[N,4] wxyz, scales=[N,3], opacities=[N], colors=[N,D] | [N,K,3],
        viewmats=[1,4,4], Ks=[1,3,3], backgrounds=[1,D], width=, height=, packed=False,
        sh_degree=None|int, render_mode="RGB"|"D"|"ED"|"RGB+D"|"RGB+ED")
Defaults the reference relies on by not passing them are gsplat's: near_plane=0.01,
far_plane=1e10, radius_clip=0, eps2d=0.3, tile_size=16, rasterize_mode="classic".

Autograd is split in the same places gsplat splits it, so that `info["means2d"]` is a
non-leaf tensor callers can `retain_grad()` (gaussian_renderer/__init__.py:75-78):
    _Project (K1/K2)  ->  [_SH (K3)]  ->  _Rasterize (K4-K10)
When only `colors` requires grad -- the GAD flow, scene/gaussian_model.py:192-208 -- the
backward launches the colours-only kernel and nothing else.
PyTorch supplies device memory, streams and autograd plumbing; all arithmetic is in HIP.
"""
import ctypes
import os
import threading
from typing import Any, NamedTuple

import torch

from . import _lib, profiler
from ._lib import check, ptr

TILE = 16
MAX_ISECTS = 1 << 28  # GAGS_MAX_ISECTS of the C ABI (include/gags_raster.h: 32-bit offsets into the slot tables)
ZERO_FILL_MIN_ELEMS = 1 << 24  # (below that the second stream's hand-over costs more than the zeros)
GEOM_COMPACT_ROWS = True   # gags_raster_bwd_geom: per-slot rows numbered compactly (one prefix sum + a 4-byte readback)
CAP_MARGIN = 1.05
# Channel ranges of the range-staged backward of a by-view multi-GPU step (RasterContext.grad_range_channels): an int (uniform
# ranges) or a tuple of widths (multiples of 128) applied in order, the last one repeated / cut to cover D.
GRAD_RANGE_CHANNELS = 128
# Channels per launch of the rows kernel under the range-staged backward (whole ranges; see _backward_staged).  256 costs 0.15-
# 0.3 ms less on ONE GPU (the weight tiles travel from HBM twice instead of four times) but delivers the first range 0.6 ms
# later; with ~1 ms of xGMI time per 128-channel range the exchange, not the GPU, paces the step at N = 8, and it is kept busy
# earliest by one launch per range (DESIGN.md section 6 has the arithmetic; bench.py reports both).
GRAD_ROWS_GROUP = 128
PROW_MAX_BYTES = 24 << 30  # staged backward: partial rows beyond this are produced per 128-channel range (see _backward_staged)
# List trimming (RasterContext.trim_lists; _trim_lists): None = automatic, for views whose forward scratch would exceed
# TRIM_AUTO_BYTES; True / False force it on / off (GAGS_TRIM_LISTS=1 / 0)
TRIM_LISTS = {"1": True, "0": False}.get(os.environ.get("GAGS_TRIM_LISTS", ""), None)
TRIM_AUTO_BYTES = 48 << 30
# Persistent gradient buffer of the colours-only backward (_KeptGrad): default ON
KEEP_GRAD = os.environ.get("GAGS_KEEP_GRAD", "1") != "0"
KEEP_GRAD_MIN_ELEMS = 0   # (every shape: the small test scenes exercise the same path as C3)
KEEP_GRAD_SHAPES = 2      # buffers a context keeps alive at once (least recently used shape is dropped)
# Row map of the colours-only backward at FORWARD time (RasterContext.early_rowmap; _early_rowmap): default ON
EARLY_COUNT = os.environ.get("GAGS_EARLY_COUNT", "1") != "0"  # 0: the intersection count is read back after the prefix sum
EARLY_ROWMAP = os.environ.get("GAGS_EARLY_ROWMAP", "1") != "0"
# Default of RasterContext.capacity_mode (GAGS_CAPACITY_MODE=1; OFF otherwise): see RasterContext.
CAPACITY_MODE = os.environ.get("GAGS_CAPACITY_MODE", "0") == "1"


def _tiles(width, height):
    """(tile_w, tile_h, number of tiles) of a width x height view."""
    tile_w, tile_h = (width + TILE - 1) // TILE, (height + TILE - 1) // TILE
    return tile_w, tile_h, tile_w * tile_h


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
        self.grad_range_channels = GRAD_RANGE_CHANNELS
        self.grad_rows_group = GRAD_ROWS_GROUP
        self.capacity_mode = CAPACITY_MODE if capacity_mode is None else bool(capacity_mode)
        self.cap_isects = {}
        self.cap_rows = {}
        self.overlap_zero_fill = bool(overlap_zero_fill)
        # the backward's row map enqueued behind the forward, its count on the way to the host meanwhile (_early_rowmap)
        self.early_rowmap = EARLY_ROWMAP
        self._pinned_pool = {}
        self.k_cache = {}
        self._pinned = {}
        self._side = {}
        # list trimming for heavy views (_trim_lists): None = automatic above TRIM_AUTO_BYTES of forward scratch
        self.trim_lists = TRIM_LISTS
        # persistent gradient buffer of the colours-only backward (_KeptGrad): on unless GAGS_KEEP_GRAD=0
        self.keep_grad_buffer = KEEP_GRAD
        self._kept = {}        # (n, d, dtype, device) -> _KeptGrad, at most KEEP_GRAD_SHAPES shapes (least recently used out)
        self._kept_fails = {}  # consecutive steps that found the buffer still referenced / written

    def forget_kept(self, n, d, dtype, dev):
        self._kept.pop((n, d, dtype, dev.index), None)

    def forget_all_kept(self):
        self._kept.clear()

    def kept_grad(self, n, d, dtype, dev):
        """(alias, flags_prev, flags_cur) of this shape's persistent gradient buffer, or None when it is not to be used."""
        if not self.keep_grad_buffer or not _CAN_COUNT_REFS or n * d < KEEP_GRAD_MIN_ELEMS or n == 0:
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
        while len(self._kept) > KEEP_GRAD_SHAPES:
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


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need_cuda(*ts):
    cur = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("gags_amd.rasterization: all tensors must live on the GPU "
                               "(there is no CPU path; see oracle/ for the test-only CPU restatement)")
        if cur is None:
            cur = torch.cuda.current_device()
        if t.device.index != cur:  # kernels are launched on the current device's stream
            raise RuntimeError(f"gags_amd.rasterization: tensor on cuda:{t.device.index} but the current device is "
                               f"cuda:{cur}; one process per GPU, torch.cuda.set_device(local_rank) first")


def _c(t):
    return t if (t.is_contiguous() and t.dtype == torch.float32) else t.contiguous().float()


class _Project(torch.autograd.Function):
    """K1 + K4 forward, K2 backward.  aa (rasterize_mode "antialiased"): one more output, the compensations [N], and its
    cotangent in the backward (gags_project_fwd_aa / gags_project_bwd_aa); the caller multiplies them into the opacities."""

    @staticmethod
    def forward(ctx, means, quats, scales, viewmat, K, width, height, eps2d, near, far, radius_clip, aa=False):
        lib = _lib.load()
        means, quats, scales, viewmat, K = _c(means), _c(quats), _c(scales), _c(viewmat), _c(K)
        n = means.shape[0]
        dev = means.device
        radii = torch.empty(n, dtype=torch.int32, device=dev)
        means2d = torch.empty(n, 2, dtype=torch.float32, device=dev)
        depths = torch.empty(n, dtype=torch.float32, device=dev)
        conics = torch.empty(n, 3, dtype=torch.float32, device=dev)
        tiles = torch.empty(n, dtype=torch.int32, device=dev)
        comp = torch.empty(n, dtype=torch.float32, device=dev) if aa else None
        with profiler.stage("project_fwd"):
            if aa:
                check(lib.gags_project_fwd_aa(n, ptr(means), ptr(quats), ptr(scales), ptr(viewmat), ptr(K), width, height,
                                              eps2d, near, far, radius_clip, ptr(radii), ptr(means2d), ptr(depths),
                                              ptr(conics), ptr(tiles), ptr(comp), _stream()), "gags_project_fwd_aa")
            else:
                check(lib.gags_project_fwd(n, ptr(means), ptr(quats), ptr(scales), ptr(viewmat), ptr(K), width, height,
                                           eps2d, near, far, radius_clip, ptr(radii), ptr(means2d), ptr(depths),
                                           ptr(conics), ptr(tiles), _stream()), "gags_project_fwd")
        ctx.save_for_backward(means, quats, scales, viewmat, K, radii, conics)
        ctx.cfg = (width, height, eps2d, aa)
        ctx.mark_non_differentiable(radii, tiles)
        if aa:
            return radii, means2d, depths, conics, tiles, comp
        return radii, means2d, depths, conics, tiles

    @staticmethod
    def backward(ctx, _v_radii, v_means2d, v_depths, v_conics, _v_tiles, v_comp=None):
        lib = _lib.load()
        means, quats, scales, viewmat, K, radii, conics = ctx.saved_tensors
        width, height, eps2d, aa = ctx.cfg
        n = means.shape[0]
        dev = means.device
        v_means2d = torch.zeros(n, 2, device=dev) if v_means2d is None else _c(v_means2d)
        v_conics = torch.zeros(n, 3, device=dev) if v_conics is None else _c(v_conics)
        v_depths = None if v_depths is None else _c(v_depths)
        v_means = torch.empty(n, 3, device=dev)
        v_quats = torch.empty(n, 4, device=dev)
        v_scales = torch.empty(n, 3, device=dev)
        if aa:
            v_comp = None if v_comp is None else _c(v_comp)
            check(lib.gags_project_bwd_aa(n, ptr(means), ptr(quats), ptr(scales), ptr(viewmat), ptr(K), width, height,
                                          eps2d, ptr(radii), ptr(v_means2d), ptr(v_depths), ptr(v_conics), ptr(v_comp),
                                          ptr(v_means), ptr(v_quats), ptr(v_scales), _stream()), "gags_project_bwd_aa")
        else:
            check(lib.gags_project_bwd(n, ptr(means), ptr(quats), ptr(scales), ptr(viewmat), ptr(K), width, height,
                                       eps2d, ptr(radii), ptr(conics), ptr(v_means2d), ptr(v_depths), ptr(v_conics),
                                       ptr(v_means), ptr(v_quats), ptr(v_scales), _stream()), "gags_project_bwd")
        return v_means, v_quats, v_scales, None, None, None, None, None, None, None, None, None


class _ProjectRaw(torch.autograd.Function):
    """K1 + K4 on the STORED parameters (gags_project_fwd_raw / gags_project_bwd_raw): the getters of
    scene/gaussian_model.py:116-139 -- exp, F.normalize, sigmoid -- and render()'s `* scaling_modifier` run inside the
    projection kernel, bit for bit as torch evaluates them; the backward returns gradients of the stored parameters.
    aa (rasterize_mode "antialiased"): the kernel folds the compensation into the activated opacity and the record
    (gags_project_fwd_raw_aa), the compensations [N] are one more -- non-differentiable -- output, and the backward takes the
    compensation's cotangent from the opacity's (gags_project_bwd_raw_aa)."""

    @staticmethod
    def forward(ctx, means, rotation, scaling_log, opacity_logit, viewmat, K, width, height, eps2d, near, far, radius_clip,
                scaling_modifier, want_records, aa=False):
        lib = _lib.load()
        means, rotation, scaling_log, viewmat, K = _c(means), _c(rotation), _c(scaling_log), _c(viewmat), _c(K)
        logit = _c(opacity_logit.reshape(-1))
        n = means.shape[0]
        dev = means.device
        radii = torch.empty(n, dtype=torch.int32, device=dev)
        means2d = torch.empty(n, 2, dtype=torch.float32, device=dev)
        depths = torch.empty(n, dtype=torch.float32, device=dev)
        conics = torch.empty(n, 3, dtype=torch.float32, device=dev)
        tiles = torch.empty(n, dtype=torch.int32, device=dev)
        opac = torch.empty(n, dtype=torch.float32, device=dev)
        # the per-Gaussian records of the matrix-core raster kernels (K8b), written on the way: no record kernel in the binning
        grec = torch.empty(max(n, 1), 8, dtype=torch.float32, device=dev) if want_records else torch.empty(0, device=dev)
        comp = torch.empty(n, dtype=torch.float32, device=dev) if aa else None
        with profiler.stage("project_fwd"):
            if aa:
                check(lib.gags_project_fwd_raw_aa(n, ptr(means), ptr(rotation), ptr(scaling_log), ptr(logit), scaling_modifier,
                                                  ptr(viewmat), ptr(K), width, height, eps2d, near, far, radius_clip, ptr(radii),
                                                  ptr(means2d), ptr(depths), ptr(conics), ptr(tiles), ptr(opac), None, None,
                                                  ptr(grec) if want_records else None, ptr(comp), _stream()),
                      "gags_project_fwd_raw_aa")
            else:
                check(lib.gags_project_fwd_raw(n, ptr(means), ptr(rotation), ptr(scaling_log), ptr(logit), scaling_modifier,
                                               ptr(viewmat), ptr(K), width, height, eps2d, near, far, radius_clip, ptr(radii),
                                               ptr(means2d), ptr(depths), ptr(conics), ptr(tiles), ptr(opac), None, None,
                                               ptr(grec) if want_records else None, _stream()), "gags_project_fwd_raw")
        ctx.save_for_backward(means, rotation, scaling_log, logit, viewmat, K, radii)
        ctx.cfg = (width, height, eps2d, scaling_modifier, tuple(opacity_logit.shape), aa)
        if aa:
            ctx.mark_non_differentiable(radii, tiles, grec, comp)
            return radii, means2d, depths, conics, tiles, opac, grec, comp
        ctx.mark_non_differentiable(radii, tiles, grec)
        return radii, means2d, depths, conics, tiles, opac, grec

    @staticmethod
    def backward(ctx, _v_radii, v_means2d, v_depths, v_conics, _v_tiles, v_opac, _v_grec, _v_comp=None):
        lib = _lib.load()
        means, rotation, scaling_log, logit, viewmat, K, radii = ctx.saved_tensors
        width, height, eps2d, modifier, oshape, aa = ctx.cfg
        n = means.shape[0]
        dev = means.device
        v_means2d = torch.zeros(n, 2, device=dev) if v_means2d is None else _c(v_means2d)
        v_conics = torch.zeros(n, 3, device=dev) if v_conics is None else _c(v_conics)
        v_depths = None if v_depths is None else _c(v_depths)
        v_opac = None if v_opac is None else _c(v_opac)
        v_means = torch.empty(n, 3, device=dev)
        v_rot = torch.empty(n, 4, device=dev)
        v_scal = torch.empty(n, 3, device=dev)
        v_logit = torch.empty(n, device=dev) if ctx.needs_input_grad[3] else None
        entry, name = ((lib.gags_project_bwd_raw_aa, "gags_project_bwd_raw_aa") if aa
                       else (lib.gags_project_bwd_raw, "gags_project_bwd_raw"))
        check(entry(n, ptr(means), ptr(rotation), ptr(scaling_log), ptr(logit), modifier, ptr(viewmat),
                    ptr(K), width, height, eps2d, ptr(radii), ptr(v_means2d), ptr(v_depths),
                    ptr(v_conics), ptr(v_opac), ptr(v_means), ptr(v_rot), ptr(v_scal), ptr(v_logit),
                    _stream()), name)
        return (v_means, v_rot, v_scal, None if v_logit is None else v_logit.reshape(oshape), None, None, None, None, None,
                None, None, None, None, None, None)


class _SH(torch.autograd.Function):
    """K3: SH colour and its backward: coefficients, and -- when positions are trainable -- the view direction
    (d colour / d means through normalize(mean - campos), as gsplat propagates it)."""

    @staticmethod
    def forward(ctx, coeffs, means, campos, radii, degree):
        lib = _lib.load()
        coeffs, means, campos = _c(coeffs), _c(means), _c(campos)
        n, kc = coeffs.shape[0], coeffs.shape[1]
        out = torch.empty(n, 3, device=coeffs.device)
        check(lib.gags_sh_fwd(n, kc, degree, ptr(means), ptr(campos), ptr(coeffs), ptr(radii), ptr(out), _stream()),
              "gags_sh_fwd")
        ctx.save_for_backward(means, campos, radii, out, coeffs if ctx.needs_input_grad[1] else None)
        ctx.cfg = (kc, degree)
        return out

    @staticmethod
    def backward(ctx, v_out):
        lib = _lib.load()
        means, campos, radii, out, coeffs = ctx.saved_tensors
        kc, degree = ctx.cfg
        n = means.shape[0]
        v_out = _c(v_out)
        v_coeffs = v_means = None
        if ctx.needs_input_grad[0]:
            v_coeffs = torch.empty(n, kc, 3, device=means.device)
            check(lib.gags_sh_bwd(n, kc, degree, ptr(means), ptr(campos), ptr(radii), ptr(out), ptr(v_out),
                                  ptr(v_coeffs), _stream()), "gags_sh_bwd")
        if ctx.needs_input_grad[1]:
            v_means = torch.empty(n, 3, device=means.device)
            check(lib.gags_sh_bwd_dirs(n, kc, degree, ptr(means), ptr(campos), ptr(coeffs), ptr(radii), ptr(out),
                                       ptr(v_out), ptr(v_means), _stream()), "gags_sh_bwd_dirs")
        return v_coeffs, v_means, None, None, None


class Binning(NamedTuple):
    """tile_binning's result, in the order its callers unpack it (see there)."""
    isect_ids: Any
    flatten_ids: Any
    isect_offsets: Any
    n_isects: Any
    packed: Any
    offsets_full: Any


def tile_binning(means2d, radii, depths, tiles_per_gauss, width, height, conics=None, opacities=None, cap=None, records=None,
                 context=None):
    """K5-K8 (+K8b) on device.  Returns (isect_ids sorted int64, flatten_ids sorted int32, isect_offsets [th,tw] int32,
    n_isects, packed [N,8] per-Gaussian records or None, offsets_full = the buffer behind isect_offsets: th * tw + 1 entries
    whose last one is the count).
    cap None: one host readback (n_isects), as in gsplat; the id arrays have exactly n_isects entries.
    cap = capacity: nothing is read back here; the id arrays have `cap` entries (sentinels past the count) and n_isects is a
    _DeferredCount the caller resolves after enqueuing what follows."""
    lib = _lib.load()
    st = _stream()
    dev = means2d.device
    n = radii.shape[0]
    tile_w, tile_h, n_tiles = _tiles(width, height)
    tile_bits = max(1, n_tiles.bit_length())  # (room for the sentinel tile id n_tiles of the capacity mode)
    cum = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    total = torch.empty(1, dtype=torch.int32, device=dev)
    early = None
    if cap is None and EARLY_COUNT and n > 0:
        # the count does not depend on the order: summed and sent to the host BEFORE the depth sort and the prefix sum are
        # enqueued, so that the readback's round trip and the host work behind it (allocations, the next launches) run under
        # those ~0.2 ms of kernels instead of after them with the queue empty (round 6: a 60-200 us bubble per view)
        host64 = (context or default_context()).pinned_i64(dev)
        host64.copy_(tiles_per_gauss.sum().reshape(1), non_blocking=True)
        early = torch.cuda.Event()
        early.record()
    # Gaussians in depth order first (N keys), intersections emitted in that order: the per-intersection sort
    # (n_isects ~ 5 N keys) then only groups by tile -- 2 radix passes instead of 6, same sorted result
    order = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    dsb = lib.gags_depth_order_scratch_bytes(n)
    dscratch = torch.empty(dsb, dtype=torch.uint8, device=dev)
    check(lib.gags_depth_order(n, ptr(depths), None, ptr(order), None, ptr(dscratch), dsb, st), "gags_depth_order")
    sb = lib.gags_scan_scratch_bytes(n)
    scratch = torch.empty(sb, dtype=torch.uint8, device=dev)
    # prefix sum of the tile counts IN DEPTH ORDER, read through `order` (no permuted copy)
    check(lib.gags_cumsum_gather_i32(n, ptr(tiles_per_gauss), ptr(order), ptr(cum), ptr(total), ptr(scratch), sb, st),
          "gags_cumsum_gather_i32")
    if cap is None:
        if early is not None:
            early.synchronize()
            n_isects = int(host64[0])
        else:
            host = ctypes.c_int32(0)
            check(lib.gags_read_i32(ptr(total), ctypes.byref(host), st), "gags_read_i32")
            n_isects = int(host.value)
        _check_isects(n_isects, n_tiles)
        size, count = n_isects, n_isects
    else:
        size, count = int(cap), _DeferredCount(total, context or default_context())
    offsets = torch.empty(n_tiles + 1, dtype=torch.int32, device=dev)
    ids = torch.empty(max(size, 1), dtype=torch.int64, device=dev)
    flat = torch.empty(max(size, 1), dtype=torch.int32, device=dev)
    ids_s = torch.empty_like(ids)
    flat_s = torch.empty_like(flat)
    if size > 0:
        check(lib.gags_tile_emit_cap(n, ptr(means2d), ptr(radii), ptr(depths), ptr(cum), ptr(order), tile_w, tile_h,
                                     ptr(ids), ptr(flat), size, ptr(total) if cap is not None else None, st),
              "gags_tile_emit_cap")
        ssb = lib.gags_sort_scratch_bytes(size)
        sscratch = torch.empty(ssb, dtype=torch.uint8, device=dev)
        check(lib.gags_sort_pairs(size, tile_bits, 1, ptr(ids), ptr(flat), ptr(ids_s), ptr(flat_s), ptr(sscratch),
                                  ssb, st), "gags_sort_pairs")
    check(lib.gags_tile_offsets(size, ptr(ids_s), n_tiles, ptr(offsets), st), "gags_tile_offsets")
    packed = records  # (gags_project_fwd_raw already wrote the per-Gaussian table)
    if conics is not None and packed is None:
        # one 32-byte record per GAUSSIAN; the raster kernels gather it through flatten_ids themselves
        # (GAGS_RECS_BY_GAUSSIAN): no per-intersection copy of the records, no gather kernel
        packed = torch.empty(max(n, 1), 8, dtype=torch.float32, device=dev)
        check(lib.gags_pack_isects(n, size, ptr(flat_s), ptr(means2d), ptr(conics), ptr(opacities), ptr(radii),
                                   ptr(packed), None, st), "gags_pack_isects")
    # `offsets` has n_tiles + 1 entries, the last one = the intersection count (gags_tile_offsets): the raster kernels read
    # isect_offsets[tile + 1] as a tile's end.  Callers get gsplat's [tile_h, tile_w] view AND the buffer itself.
    off_view = offsets[:n_tiles].view(tile_h, tile_w)
    return Binning(ids_s[:size], flat_s[:size], off_view, count, packed, offsets)


def _trim_lists(lib, n, width, height, offsets_full, flatten_ids, n_isects, packed):
    """Round 6, heavy views: every tile's sorted list cut to the entries its pixels actually read before the tile is done
    (gags_raster_list_need: the weights pass's own walk, outputs dropped), so that the split forward's scratch -- ~1 KB per
    list entry -- and every pass over the lists shrink by the same factor (C5H: 169 M entries, a few hundred of a tile's 20 k
    are read).  Returns (offsets [n_tiles + 1] with the count, flatten_ids, count) of the trimmed lists: on them every raster
    entry computes bit for bit what it computes on the full lists; only last_ids index the trimmed list
    (gags_trim_last_ids translates a copy back).  One more 4-byte readback (the trimmed count sizes the id list)."""
    st = _stream()
    dev = flatten_ids.device
    n_tiles = _tiles(width, height)[2]
    need = torch.empty(n_tiles, dtype=torch.int32, device=dev)
    with profiler.stage("list_need"):
        check(lib.gags_raster_list_need(n, width, height, ptr(offsets_full), ptr(flatten_ids), n_isects, ptr(packed),
                                        _lib.GAGS_RECS_BY_GAUSSIAN, ptr(need), st), "gags_raster_list_need")
    cum = torch.empty(n_tiles, dtype=torch.int32, device=dev)
    total = torch.empty(1, dtype=torch.int32, device=dev)
    sb = lib.gags_scan_scratch_bytes(n_tiles)
    scratch = torch.empty(sb, dtype=torch.uint8, device=dev)
    check(lib.gags_cumsum_i32(n_tiles, ptr(need), ptr(cum), ptr(total), ptr(scratch), sb, st), "gags_cumsum_i32")
    host = ctypes.c_int32(0)
    check(lib.gags_read_i32(ptr(total), ctypes.byref(host), st), "gags_read_i32")
    t = int(host.value)
    offs_t = torch.empty(n_tiles + 1, dtype=torch.int32, device=dev)
    flat_t = torch.empty(t, dtype=torch.int32, device=dev)
    check(lib.gags_trim_lists(width, height, ptr(offsets_full), ptr(cum), ptr(flatten_ids), ptr(offs_t),
                              ptr(flat_t) if t > 0 else None, st), "gags_trim_lists")
    return offs_t, flat_t, t


def _check_isects(n_isects, n_tiles=0):
    # the int32 prefix sum wrapped, or the slot space (4 I + 64 tiles + 64 slots, 32-bit byte offsets of its id table) would
    if n_isects < 0 or n_isects >= MAX_ISECTS or 4 * n_isects + 64 * n_tiles + 64 >= (1 << 30):
        raise RuntimeError(f"gags_amd.rasterization: {n_isects if n_isects >= 0 else '> 2^31'} tile intersections in one "
                           f"view; the kernels index at most 2^28 = {MAX_ISECTS} less 16 per tile (INTEGRATION.md, memory model)")


_FWD_VALU, _FWD_FUSED, _FWD_SPLIT, _FWD_LEAN16 = "valu", "fused", "split", "lean16"
_BWD_NONE, _BWD_STAGED, _BWD_STAGED_GEOM, _BWD_VALU = "none", "staged", "staged+geom", "valu"


class _Route(NamedTuple):
    """Which kernels serve one rasterization() call and what the forward prepares for the backward: decided once by _route(),
    read by projection, binning, trimming, the zero-fill, _Rasterize.forward and -- from ctx -- _Rasterize.backward.
    (DESIGN.md section 1 has the table.)"""
    fwd: str             # _FWD_VALU; _FWD_FUSED (single matrix-core kernel, no scratch); _FWD_SPLIT (weights pass + feature
    #                      stream through a scratch of 1 KB per intersection); _FWD_LEAN16 (the weights pass with the 16-channel
    #                      feature pass fused in: no scratch, nothing kept)
    fwd_per_kernel: bool  # profiler on: the split forward's two kernels in two launches, one event pair each
    records: bool        # projection / binning produce the per-Gaussian record table of the matrix-core kernels
    half: bool           # the fp16 table is read as it is (widened in the feature pass); its gradient comes back in fp16
    bwd: str             # _BWD_NONE (nothing requires grad); _BWD_STAGED (colours only, atomic-free); _BWD_STAGED_GEOM (geometry
    #                      through gags_raster_bwd_geom, colours -- if wanted -- staged); _BWD_VALU (gags_raster_bwd: VALU / atomic)
    geom: bool           # the backward produces v_means2d, v_conics, v_opacities
    colors: bool         # ... and v_colors
    early_rowmap: bool   # the forward enqueues the backward's row map behind its own kernels (RasterContext.early_rowmap)
    trim: Any            # list trimming: False = never, None = automatic above TRIM_AUTO_BYTES, True = forced
    zero_fill: bool      # the gradient's zero-fill starts on a second stream before the binning (RasterContext.overlap_zero_fill)
    flags: int           # the caller's raster_flags, for the kernel-variant bits the translations below read (never the route);
    #                      GAGS_FWD_F16MFMA only where it applies (an fp16 table read as it is, D >= 128)
    absgrad: bool = False  # the backward also produces absgrad (only with geom; _BWD_STAGED_GEOM, or _BWD_VALU at D <= 32)

    @property
    def keeps_scratch(self):
        """The forward's scratch and slot counts are saved for the backward: exactly when a staged backward will read them."""
        return self.bwd in (_BWD_STAGED, _BWD_STAGED_GEOM)

    def without_isects(self):
        """Late fact 1, known after the binning: no tile intersection.  The split forward runs as it is, in one launch (the lean
        kernel wants a list to walk), and there is no row to number ahead of the backward."""
        return self._replace(fwd=_FWD_SPLIT if self.fwd == _FWD_LEAN16 else self.fwd, fwd_per_kernel=False, early_rowmap=False)

    def without_scratch(self):
        """Late fact 2: the split forward's scratch could not be allocated.  The scratch-free kernels, which read an fp32 table:
        single-kernel forward, gags_raster_bwd."""
        return self._replace(fwd=_FWD_FUSED, fwd_per_kernel=False, half=False, early_rowmap=False,
                             bwd=_BWD_NONE if self.bwd == _BWD_NONE else _BWD_VALU)


ABSGRAD_VALU_MAX_D = 32  # gags_raster_bwd_abs: one channel chunk must cover D


def _route(n, d, f16, needs, raster_flags, profiling, capacity_mode=False, early_rowmap=True, overlap_zero_fill=False,
           hooked=False, trim_lists=None, absgrad=False):
    """The _Route of a call, from plain values: n Gaussians, d = the FINAL channel count, f16 = the table is fp16, needs = which
    of (means2d, conics, colors, opacities, backgrounds) require grad while a graph is recorded, the caller's raster_flags,
    profiler.ENABLED, and the RasterContext settings that matter (hooked: grad_range_hook is set).
    The widths: the matrix-core forward serves every D >= 16 (gags_mfma_width in csrc/common.h; 16 is what the reference
    rasterizes, 513 = 512 + 1 is BASELINE.json configs[4]), the staged backward D <= 1024, gags_raster_bwd_geom D % 8 == 0
    of those (below 16 the VALU kernel is faster).  absgrad: asked for by the caller; the route carries it only where a geometry
    gradient is produced (rasterization() refuses the one route that cannot serve it: _BWD_VALU at D > ABSGRAD_VALU_MAX_D)."""
    wide = d >= 16
    mfma = wide and n > 0 and not (raster_flags & (_lib.GAGS_FWD_NO_MFMA | _lib.GAGS_FWD_FUSED))
    half = mfma and f16
    geom = needs[0] or needs[1] or needs[3]
    # a 16-channel fp32 render that nothing will be differentiated through (evaluation: render.py, the relevancy queries)
    lean = (mfma and d == 16 and not half and not any(needs) and not (raster_flags & _lib.GAGS_FWD_EXACT) and not profiling)
    fwd = (_FWD_LEAN16 if lean else _FWD_SPLIT if mfma
           else _FWD_FUSED if (wide and not (raster_flags & _lib.GAGS_FWD_NO_MFMA)) else _FWD_VALU)
    staged_ok = fwd == _FWD_SPLIT and d <= 1024 and not (raster_flags & _lib.GAGS_BWD_ATOMIC)
    # (every gradient at a width gags_raster_bwd_geom does not serve: the VALU kernel, and nothing is kept for it)
    bwd = (_BWD_NONE if not any(needs) else _BWD_STAGED_GEOM if (staged_ok and geom and d % 8 == 0)
           else _BWD_STAGED if (staged_ok and needs[2] and not geom) else _BWD_VALU)
    if not (half and d >= 128):
        raster_flags &= ~_lib.GAGS_FWD_F16MFMA
    return _Route(fwd=fwd, fwd_per_kernel=bool(profiling) and fwd == _FWD_SPLIT, records=wide, half=half, bwd=bwd,
                  geom=bool(geom), colors=bool(needs[2]), flags=int(raster_flags),
                  early_rowmap=bwd == _BWD_STAGED and bool(early_rowmap) and not capacity_mode,
                  trim=trim_lists if fwd in (_FWD_SPLIT, _FWD_LEAN16) else False,
                  zero_fill=bool(overlap_zero_fill) and not hooked and bwd == _BWD_STAGED and n * d >= ZERO_FILL_MIN_ELEMS,
                  absgrad=bool(absgrad) and bool(geom) and bwd in (_BWD_STAGED_GEOM, _BWD_VALU))


class _Rasterize(torch.autograd.Function):
    """K9 forward / K10 backward over pre-binned intersections, on the kernels the call's _Route names.

    Matrix-core widths (D >= 16) run the split forward: one weights pass (alpha, transmittance,
    stop rule: once per view) that leaves weight tiles in a scratch buffer, then the feature stream.
    The same scratch feeds the staged, atomic-free colours-only backward."""

    @staticmethod
    def forward(ctx, means2d, conics, colors, opacities, backgrounds, offsets, flatten_ids, packed, width, height, route, rctx,
                prezero=None, abs_holder=None):
        """offsets: the buffer of n_tiles + 1 int32 entries tile_binning returns as `offsets_full` (last entry = the
        intersection count).  route: _route() of the call; rctx: its RasterContext.  abs_holder (route.absgrad): a list whose
        first entry is the [1,N,2] tensor the backward attaches `.absgrad` to (the node callers hold, as gsplat does)."""
        lib = _lib.load()
        n_isects = flatten_ids.shape[0]  # (capacity mode: the buffers' size; the kernels take the count from `offsets`)
        if n_isects == 0:
            route = route.without_isects()
        means2d, conics, opacities = _c(means2d), _c(conics), _c(opacities)
        # an fp16 feature table (BASELINE.json configs[4]) is read as it is by the matrix-core feature pass: widened
        # exactly, same fp32 arithmetic; every other kernel gets fp32
        colors = (colors if colors.is_contiguous() else colors.contiguous()) if route.half else _c(colors)
        backgrounds = None if backgrounds is None else _c(backgrounds)
        n, d = colors.shape
        dev = colors.device
        n_tiles = _tiles(width, height)[2]
        if offsets.shape != (n_tiles + 1,) or offsets.dtype != torch.int32 or not offsets.is_contiguous():
            raise ValueError(f"isect_offsets must be tile_binning's offsets_full: {n_tiles + 1} int32 entries, the last one the count")
        out = torch.empty(height, width, d, device=dev)
        alphas = torch.empty(height, width, device=dev)
        last_ids = torch.empty(height, width, dtype=torch.int32, device=dev)
        scratch, blk_rows, nbytes = None, None, 0
        if route.fwd == _FWD_SPLIT:
            nbytes = lib.gags_raster_fwd_scratch_bytes(n_isects, width, height)
            for _attempt in range(2):
                try:
                    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
                    break
                except torch.OutOfMemoryError:
                    # the kept gradient buffers (_KeptGrad: up to KEEP_GRAD_SHAPES x [N, D]) are the memory this context can
                    # give back: released, then one more attempt
                    rctx.forget_all_kept()
            if scratch is None:
                # slot space (1 KB per intersection) does not fit even after the caching allocator gave its blocks
                # back: scratch-free kernels, which read an fp32 table only.  Said out loud: they are several times slower
                # (single-kernel forward, atomic backward) and the caller should know why
                import warnings
                warnings.warn(f"gags_amd.rasterization: {nbytes / 2 ** 30:.1f} GiB of forward scratch for {n_isects} tile "
                              "intersections could not be allocated; this view runs on the scratch-free kernels "
                              "(INTEGRATION.md, memory model)", RuntimeWarning, stacklevel=3)
                route, nbytes, colors = route.without_scratch(), 0, _c(colors)
                _check_absgrad_route(route, d)
        if route.fwd == _FWD_SPLIT:
            blk_rows = torch.empty(n_tiles * 4, dtype=torch.int32, device=dev)  # per 8x8 pixel block
        cflags = _fwd_flags(route)

        def launch(extra=0):
            check(lib.gags_raster_fwd(d, n, width, height, ptr(means2d), ptr(conics), ptr(opacities), ptr(colors),
                                      ptr(backgrounds), ptr(offsets), ptr(flatten_ids), n_isects, ptr(packed),
                                      ptr(out), ptr(alphas), ptr(last_ids), ptr(scratch), nbytes, ptr(blk_rows),
                                      cflags | extra, _stream()), "gags_raster_fwd")

        with profiler.stage("raster_fwd"):
            if route.fwd_per_kernel:  # one event pair per kernel, for bench.py's roofline line
                with profiler.stage("raster_weights"):
                    launch(_lib.GAGS_FWD_ONLY_WEIGHTS)
                with profiler.stage("raster_fwd_feat"):
                    launch(_lib.GAGS_FWD_ONLY_FEATURES)
            else:
                launch()
        if route.fwd == _FWD_SPLIT:
            profiler.note("fwd_blk_rows", blk_rows)
        early = None
        if route.early_rowmap:
            with profiler.stage("bwd_rowcount"):
                early = _early_rowmap(lib, rctx, _FwdState(offsets, n_isects, blk_rows, scratch, flatten_ids, n, d, width, height))
        keep = route.keeps_scratch  # (wide-D geometry gradients on the matrix cores also consume the forward's scratch)
        ctx.save_for_backward(means2d, conics, colors, opacities, backgrounds, offsets, flatten_ids, packed, alphas,
                              last_ids, scratch if keep else None, blk_rows if keep else None)
        ctx.route = route
        ctx.abs_holder = abs_holder if route.absgrad else None
        ctx.cfg = (width, height, rctx, prezero if route.bwd == _BWD_STAGED else None, early)
        ctx.mark_non_differentiable(last_ids)
        return out, alphas, last_ids

    @staticmethod
    def backward(ctx, v_out, v_alphas, _v_last):
        lib = _lib.load()
        route = ctx.route
        (means2d, conics, colors, opacities, backgrounds, offsets, flatten_ids, packed, alphas,
         last_ids, fwd_scratch, blk_rows) = ctx.saved_tensors
        width, height, rctx, prezero, early = ctx.cfg
        n, d = colors.shape
        fwd = _FwdState(offsets, flatten_ids.shape[0], blk_rows, fwd_scratch, flatten_ids, n, d, width, height)
        v_out = torch.zeros(height, width, d, device=colors.device) if v_out is None else _c(v_out)
        v_alphas = None if v_alphas is None else _c(v_alphas)
        v_bg = None
        if backgrounds is not None and ctx.needs_input_grad[4]:
            v_bg = ((1.0 - alphas)[..., None] * v_out).sum(dim=(0, 1))
        if route.bwd == _BWD_STAGED:
            # an fp16 table gets its gradient in fp16 straight from the reduce kernel (fp32 sums, rounded once): no fp32
            # tensor + cast pass (autograd wants the table's dtype; an fp32 master sits behind a .half() cast)
            grads = (None, None, _backward_staged(lib, rctx, fwd, v_out, _stage_bits(route.flags, route.half), prezero, early=early),
                     None)
        elif route.bwd == _BWD_STAGED_GEOM:
            grads = _backward_geom_mfma(lib, rctx, route, fwd, colors, backgrounds, packed, v_out, v_alphas)
        else:
            grads = _backward_valu(lib, route, fwd, means2d, conics, opacities, colors, backgrounds, packed, alphas, last_ids,
                                   v_out, v_alphas)
        if route.absgrad:
            # overwritten by each backward, never accumulated; [1,N,2] like the tensor it goes on
            grads, v_abs = grads[:4], grads[4]
            if ctx.abs_holder:
                ctx.abs_holder[0].absgrad = v_abs[None]
        return _raster_grads(*grads[:4], v_bg)


def _raster_grads(v_m2d, v_con, v_colors, v_opac, v_bg):
    """_Rasterize.backward's return: the five gradients in the slots of forward's tensor arguments, None for the rest."""
    return (v_m2d, v_con, v_colors, v_opac, v_bg) + (None,) * 9


def _check_absgrad_route(route, d):
    """absgrad on the one route that cannot serve it: the VALU kernel splits a pixel's channels over blocks above
    ABSGRAD_VALU_MAX_D, and an absolute value of a partial sum is not the rule."""
    if route.absgrad and route.bwd == _BWD_VALU and d > ABSGRAD_VALU_MAX_D:
        raise NotImplementedError(
            f"absgrad=True with geometry gradients at D = {d} on the VALU backward: served for D <= {ABSGRAD_VALU_MAX_D} there, "
            "and for every D % 8 == 0 in 16..1024 on the matrix-core geometry pass (DESIGN.md section 7, N16)")


def _backward_geom_mfma(lib, rctx, route, fwd, colors, backgrounds, packed, v_out, v_alphas):
    """Wide D, geometry wanted: colours (if wanted) through the staged backward, geometry through the matrix-core dot pass +
    scalar pass of gags_raster_bwd_geom, both on the forward's scratch.  Returns (v_means2d, v_conics, v_colors, v_opacities)
    and -- route.absgrad -- absgrad [N,2] as a fifth."""
    dev = colors.device
    v_colors = _backward_staged(lib, rctx, fwd, v_out, _stage_bits(route.flags, route.half)) if route.colors else None
    if route.half:  # the geometry kernels read an fp32 table: widen the halves (exact) for this backward
        colors = colors.float()
    # compact numbering of the per-slot rows: one small prefix sum and a 4-byte readback instead of sorting the
    # whole sparse slot space (6x the keys)
    if GEOM_COMPACT_ROWS:
        incl = torch.cumsum(fwd.blk_rows, 0, dtype=torch.int32)
        row_base = (incl - fwd.blk_rows).contiguous()
        n_rows = int(incl[-1].item()) if incl.numel() else 0
    else:  # the C ABI's other numbering: rows (and the dot products) in the sparse slot space, no count needed
        row_base, n_rows = None, -1
    nb = lib.gags_raster_bwd_geom_scratch_bytes(fwd.n_isects, fwd.width, fwd.height, fwd.n, fwd.d, n_rows)
    gscratch = torch.empty(nb, dtype=torch.uint8, device=dev)
    v_geo = torch.empty(fwd.n, 8, device=dev)
    with profiler.stage("raster_bwd_geom"):
        check(lib.gags_raster_bwd_geom(fwd.d, fwd.n, fwd.width, fwd.height, ptr(colors), ptr(backgrounds), ptr(fwd.offsets),
                                       fwd.n_isects, ptr(packed), ptr(v_out), ptr(v_alphas), ptr(fwd.blk_rows),
                                       ptr(fwd.fwd_scratch), fwd.fwd_scratch.numel(), ptr(gscratch), nb, ptr(v_geo),
                                       ptr(fwd.flatten_ids), ptr(row_base), n_rows, _geom_flags(route), _stream()),
              "gags_raster_bwd_geom")
    grads = (v_geo[:, 3:5].contiguous(), v_geo[:, 0:3].contiguous(), v_colors, v_geo[:, 5].contiguous())
    return grads + (v_geo[:, 6:8].contiguous(),) if route.absgrad else grads


def _backward_valu(lib, route, fwd, means2d, conics, opacities, colors, backgrounds, packed, alphas, last_ids, v_out, v_alphas):
    """gags_raster_bwd, the VALU / atomic kernels: colours, and -- route.geom -- geometry.  They read an fp32 table: the halves
    are widened (exact) and the gradient goes back in the table's dtype.  Returns (v_means2d, v_conics, v_colors, v_opacities)
    and -- route.absgrad, through gags_raster_bwd_abs -- absgrad [N,2] as a fifth."""
    dev = colors.device
    if route.half:
        colors = colors.float()
    v_colors = torch.zeros(fwd.n, fwd.d, device=dev)
    v_opac, v_m2d, v_con = ([torch.zeros(fwd.n, *k, device=dev) for k in ((), (2,), (3,))] if route.geom else (None, None, None))
    if route.absgrad:
        _check_absgrad_route(route, fwd.d)
        v_abs = torch.zeros(fwd.n, 2, device=dev)
        with profiler.stage("raster_bwd"):
            check(lib.gags_raster_bwd_abs(fwd.d, fwd.width, fwd.height, ptr(means2d), ptr(conics), ptr(opacities), ptr(colors),
                                          ptr(backgrounds), ptr(fwd.offsets), ptr(fwd.flatten_ids), fwd.n_isects, ptr(packed),
                                          ptr(alphas), ptr(last_ids), ptr(v_out), ptr(v_alphas), ptr(v_colors),
                                          ptr(v_opac), ptr(v_m2d), ptr(v_con), ptr(v_abs), _bwd_flags(route), _stream()),
                  "gags_raster_bwd_abs")
        return v_m2d, v_con, v_colors.half() if route.half else v_colors, v_opac, v_abs
    with profiler.stage("raster_bwd"):
        check(lib.gags_raster_bwd(fwd.d, fwd.width, fwd.height, ptr(means2d), ptr(conics), ptr(opacities), ptr(colors),
                                  ptr(backgrounds), ptr(fwd.offsets), ptr(fwd.flatten_ids), fwd.n_isects, ptr(packed),
                                  ptr(alphas), ptr(last_ids), ptr(v_out), ptr(v_alphas), ptr(v_colors),
                                  ptr(v_opac), ptr(v_m2d), ptr(v_con), _bwd_flags(route), _stream()), "gags_raster_bwd")
    return v_m2d, v_con, v_colors.half() if route.half else v_colors, v_opac


def _channel_ranges(d, spec):
    """[(c0, c1), ...] covering [0, d) for the range-staged backward, or None when D is served in one piece.  spec: an int
    (uniform ranges; D must be a multiple) or a tuple of widths, multiples of 128, applied in order -- the last one
    repeats until D is covered, a range that would overshoot is cut at D (which must then be a multiple of 128)."""
    if isinstance(spec, int):
        if spec <= 0 or d % spec != 0 or d <= spec or spec % 32 != 0:
            return None
        return [(c, c + spec) for c in range(0, d, spec)]
    widths = [int(w) for w in spec]
    if not widths or any(w <= 0 or w % 128 != 0 for w in widths) or d % 128 != 0 or d <= widths[0]:
        return None
    out, c, i = [], 0, 0
    while c < d:
        w = min(widths[min(i, len(widths) - 1)], d - c)
        out.append((c, c + w))
        c, i = c + w, i + 1
    return out


class _EarlyRowmap:
    """The backward's row map, enqueued by the forward (RasterContext.early_rowmap): the map, and its total on the way to a
    pinned buffer behind an event."""

    def __init__(self, trow, total, stmp, host, ev, rctx, dev):
        self.trow, self.total, self.stmp, self.host, self.ev, self.rctx, self.dev = trow, total, stmp, host, ev, rctx, dev
        self._rows = None

    def rows(self):
        if self._rows is None:
            self.ev.synchronize()  # (long passed by the time a backward asks)
            self._rows = int(self.host[0])
            self.rctx.give_pinned(self.dev, self.host)
            self.host = None
        return self._rows

    def __del__(self):
        # a forward that was never differentiated: its pinned word goes back to the pool only when the copy into it has
        # landed (the event has completed).  While the copy may still be in flight the word is dropped instead: handed to the
        # next forward -- possibly on another stream -- it could be overwritten by THIS forward's count after that one's arrived
        try:
            if self.host is not None:
                if self.ev.query():
                    self.rctx.give_pinned(self.dev, self.host)
                self.host = None
        except Exception:
            pass


class _FwdState(NamedTuple):
    """What a split forward hands the staged backward of its view (read by name: tools/ wrap _backward_staged)."""
    offsets: Any      # n_tiles + 1 int32 entries, the last one = the intersection count
    n_isects: int     # entries of the id lists (capacity mode: the buffers' size)
    blk_rows: Any     # the forward's slot counts, four per tile
    fwd_scratch: Any  # the forward's scratch: weight tiles, hit flags
    flatten_ids: Any
    n: int
    d: int
    width: int
    height: int


_STAGE_NAMES = {_lib.GAGS_STAGE_ROWS: "bwd_rows", _lib.GAGS_STAGE_SORT: "bwd_sort", _lib.GAGS_STAGE_REDUCE: "bwd_reduce"}


def _stage_bits(raster_flags, half):
    """The public raster_flags' choice of a rows kernel, and `half` = the gradient of an fp16 table, as bits of the `stage`
    argument of gags_raster_bwd_colors_staged."""
    return ((_lib.GAGS_STAGED_F32MFMA if (raster_flags & _lib.GAGS_BWD_F32MFMA) else 0)
            | (_lib.GAGS_STAGED_OUT_F16 if half else 0)
            | (_lib.GAGS_STAGED_BLOCKWAVES if (raster_flags & _lib.GAGS_BWD_BLOCKWAVES) else 0)
            | (_lib.GAGS_STAGED_EXACT_WEIGHTS if (raster_flags & _lib.GAGS_BWD_EXACT_WEIGHTS) else 0))


# the two raster_flags whose public value IS the header's: they travel to gags_raster_fwd / gags_raster_bwd as they are (the
# forward reads only the second)
_C_SHARED = _lib.GAGS_BWD_COLORS_ONLY | _lib.GAGS_FWD_NO_MFMA


def _fwd_flags(route):
    """`flags` of gags_raster_fwd (the profiler's per-kernel launches add GAGS_FWD_ONLY_*)."""
    return ((route.flags & (_C_SHARED | _lib.GAGS_FWD_EXACT)) | _lib.GAGS_RECS_BY_GAUSSIAN
            | (_lib.GAGS_FEAT_F16 if route.half else 0)
            | (_lib.GAGS_FWD_F16MFMA_C if (route.half and route.flags & _lib.GAGS_FWD_F16MFMA) else 0))


def _bwd_flags(route):
    """`flags` of gags_raster_bwd."""
    return (route.flags & _C_SHARED) | _lib.GAGS_RECS_BY_GAUSSIAN | (0 if route.geom else _lib.GAGS_BWD_COLORS_ONLY)


def _geom_flags(route):
    """`flags` of gags_raster_bwd_geom."""
    return (_lib.GAGS_RECS_BY_GAUSSIAN | (_lib.GAGS_GEOM_F32MFMA if (route.flags & _lib.GAGS_BWD_F32MFMA) else 0)
            | (_lib.GAGS_GEOM_ABSGRAD if route.absgrad else 0))


def _rowmap(lib, fwd):
    """The view's partial gradient rows numbered on the device (gags_bwd_rowmap, enqueued on the current stream; the one place
    that knows that call).  Returns (rowmap, total = the row count, int32 [1] on the device, the scan's scratch)."""
    dev = fwd.blk_rows.device
    ne = lib.gags_bwd_rowmap_elems(fwd.n_isects, fwd.width, fwd.height)
    trow = torch.empty(ne, dtype=torch.int32, device=dev)
    total = torch.empty(1, dtype=torch.int32, device=dev)
    sb = lib.gags_bwd_rowmap_scratch_bytes(fwd.n_isects)
    stmp = torch.empty(max(sb, 4), dtype=torch.uint8, device=dev)
    check(lib.gags_bwd_rowmap(fwd.n_isects, fwd.width, fwd.height, ptr(fwd.offsets), ptr(fwd.blk_rows), ptr(fwd.fwd_scratch),
                              fwd.fwd_scratch.numel(), ptr(trow), ne, ptr(total), ptr(stmp), sb, _stream()), "gags_bwd_rowmap")
    return trow, total, stmp


def _early_rowmap(lib, rctx, fwd):
    trow, total, stmp = _rowmap(lib, fwd)
    dev = total.device
    host = rctx.take_pinned(dev)
    host.copy_(total, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    return _EarlyRowmap(trow, total, stmp, host, ev, rctx, dev)


def _row_count(lib, rctx, fwd, early, capacity):
    """(rowmap, total, rows, pending): the row map and the row count the backward sizes its scratch by, one of three ways.
    early (an _EarlyRowmap): the forward enqueued the row map behind its own kernels and its count has reached the host
    meanwhile: no prefix sum, no readback, no drained queue here.  capacity (the count remembered from earlier views; see
    RasterContext.capacity_mode): `rows` is a capacity and the count stays on the device until the backward is enqueued --
    `pending` is its _DeferredCount.  Neither: one 4-byte readback."""
    if early is not None:
        return early.trow, early.total, early.rows(), None
    with profiler.stage("bwd_rowcount"):
        trow, total, _ = _rowmap(lib, fwd)
        if capacity is not None:
            return trow, total, min(max(fwd.n_isects, 1), int(capacity * CAP_MARGIN) + 1024), _DeferredCount(total, rctx)
        host = ctypes.c_int32(0)
        check(lib.gags_read_i32(ptr(total), ctypes.byref(host), _stream()), "gags_read_i32")
        return trow, total, int(host.value), None


def _grad_buffer(rctx, fwd, bits, dev, hook, wire_hook, pending, prezero):
    """(v_colors, kept, bits): the tensor the reduce stage writes.  In this order:
    prezero = (buffer, event) of a zero-fill the forward started (RasterContext.overlap_zero_fill), outside the exchange hooks:
    that buffer, and the reduce stage writes only the rows that exist (GAGS_STAGED_PREZEROED);
    else the context's persistent buffer (kept = _KeptGrad.hand_out(): an alias and two flag arrays; rows of Gaussians that blend
    nothing are never written again): not with a zero-fill, not in capacity mode (`pending`), and under the exchange hooks
    (the ranks' sum lands in rows this view did not write) only when the reduce stage writes the exchanged block itself: its
    rows -- where finish() writes the ranks' sum -- then count as written (wire_pos / wire of the staged entry);
    else a fresh tensor, written in full."""
    v_dtype = torch.float16 if (bits & _lib.GAGS_STAGED_OUT_F16) else torch.float32
    if prezero is not None:
        # the forward started a zero-fill of this tensor on a second stream while the binning kernels (small, latency-bound:
        # the memory system idles) ran; the reduce stage then writes only the rows that exist -- 73 % of the Gaussians
        # blend nothing at C3: 3.07 GB -> 0.83 GB written here.  (Filled under the rows kernel instead, the fill slowed
        # that kernel by as much as the reduce stage gained.)
        buf, ev = prezero
        if hook is None and buf.shape == (fwd.n, fwd.d) and buf.dtype == v_dtype:
            torch.cuda.current_stream().wait_event(ev)
            return buf, None, bits | _lib.GAGS_STAGED_PREZEROED
    elif pending is None and (hook is None or (wire_hook is not None and rctx.grad_rows_hook is not None)):
        kept = rctx.kept_grad(fwd.n, fwd.d, v_dtype, dev)
        if kept is not None:
            return kept[0], kept, bits
    return torch.empty(fwd.n, fwd.d, device=dev, dtype=v_dtype), None, bits


def _bind_staged(lib, fwd, v_out, trow, rows, scratch, v_colors):
    """gags_raster_bwd_colors_staged with everything bound that does not vary within one backward.  What remains per call:
    stage (with its bits), the channel range [c0, c0 + cw), rows_dev (capacity mode: the true row count on the device),
    wire = (pos, block) of the exchange, keep = the persistent buffer's hand-out -- its flag arrays travel only with a call
    that holds the reduce stage."""
    fixed = (fwd.d, fwd.n, fwd.width, fwd.height, ptr(fwd.offsets), fwd.n_isects, ptr(v_out), ptr(fwd.blk_rows), ptr(trow), rows,
             ptr(fwd.fwd_scratch), fwd.fwd_scratch.numel(), ptr(scratch), scratch.numel(), ptr(v_colors))
    st = _stream()
    with_reduce = (_lib.GAGS_STAGE_ALL, _lib.GAGS_STAGE_REDUCE)

    def call(stage, c0, cw, rows_dev=None, wire=None, keep=None):
        if keep is not None and (stage & _lib.GAGS_STAGE_MASK) not in with_reduce:
            keep = None
        check(lib.gags_raster_bwd_colors_staged(
            *fixed, stage, c0, cw, rows_dev, ptr(wire[0]) if wire else None, ptr(wire[1]) if wire else None,
            ptr(keep[1]) if keep else None, ptr(keep[2]) if keep else None, st), "gags_raster_bwd_colors_staged")

    return call


def _run_whole(call, bits, d, rows_dev, kept, hook, v_colors):
    """The whole view, all channels: one call, or one per stage under the profiler (one event pair per kernel (group), for the
    roofline line of bench.py).  An exchange hook whose ranges do not divide this width gets the gradient in one piece."""
    if profiler.ENABLED:
        for stage, name in _STAGE_NAMES.items():
            with profiler.stage(name):
                call(stage | bits, 0, d, rows_dev, None, kept)
    else:
        call(_lib.GAGS_STAGE_ALL | bits, 0, d, rows_dev, None, kept)
    if hook is not None:
        hook(v_colors.detach(), 0, d)


def _run_range_scratch(call, bits, d, kept):
    """A heavy view (PROW_MAX_BYTES): the gradient one 128-channel range at a time through a [rows, 128] scratch."""
    for c0 in range(0, d, 128):
        for stage in ((_lib.GAGS_STAGE_ROWS, _lib.GAGS_STAGE_SORT, _lib.GAGS_STAGE_REDUCE) if c0 == 0
                      else (_lib.GAGS_STAGE_ROWS, _lib.GAGS_STAGE_REDUCE)):
            with profiler.stage(_STAGE_NAMES[stage]):
                call(stage | bits | _lib.GAGS_STAGED_RANGE_SCRATCH, c0, 128, None, None, kept)


def _run_ranged(call, rctx, fwd, bits, ranges, hook, wire_hook, kept, v_colors):
    """Under the exchange hooks: rows for `grad_rows_group` channels per launch (the sort with the first), then per range the
    reduce stage -- which also writes the exchanged block when the wire hook hands one out -- and the range hook."""
    alias = v_colors.detach()  # own TensorImpl, same storage: autograd may still adopt v_colors without a copy
    # the partial rows are produced for `grad_rows_group` channels per launch: every rows launch streams the view's weight
    # tiles from HBM once for all of its 128-channel slices (they share them through L2), so wider groups re-read them less
    # often -- and deliver their first range later; the reduce stage and the exchange keep the narrower range either way
    group = max(int(rctx.grad_rows_group), 1)
    rows_done = 0
    for c0, c1 in ranges:
        if c1 > rows_done:
            g1 = rows_done
            while g1 < c1 or (g1 - rows_done < group and g1 < fwd.d):
                g1 = next(b for a, b in ranges if a == g1)
            for stage in ((_lib.GAGS_STAGE_ROWS, _lib.GAGS_STAGE_SORT) if rows_done == 0 else (_lib.GAGS_STAGE_ROWS,)):
                with profiler.stage(_STAGE_NAMES[stage]):
                    call(stage | bits, rows_done, g1 - rows_done)
            rows_done = g1
        # the rows the ranks exchange leave from the reduce kernel itself (no pack pass over the range afterwards)
        w = wire_hook(c0, c1) if wire_hook is not None else None
        if w is None and kept is not None:
            # the exchange packs for itself after all (bf16 wire, all rows): its sum may land in rows the flags do not
            # cover.  This step's reduce writes every row; the buffer is not kept
            rctx.forget_kept(fwd.n, fwd.d, v_colors.dtype, v_colors.device)
            kept = None
        with profiler.stage("bwd_reduce"):
            call(_lib.GAGS_STAGE_REDUCE | bits, c0, c1 - c0, None, w, kept)
        if w is not None:
            hook(alias, c0, c1, w[1])
        else:
            hook(alias, c0, c1)


def _backward_staged(lib, rctx, fwd, v_out, stage_bits=0, prezero=None, exact_rows=False, early=None):
    """Colours-only backward without atomics: hit flags of the forward -> prefix sum (one row per (tile, Gaussian)
    pair that blended anything) -> the total of rows (_row_count) -> merged partial rows -> sort by Gaussian ->
    segmented sum.  fwd: the forward's _FwdState; stage_bits: _stage_bits(); prezero, early: what the forward prepared
    (a zero-filled gradient, the row map); exact_rows: the re-run of a capacity-mode backward whose capacity was too small."""
    dev = v_out.device
    n, d = fwd.n, fwd.d
    hook = rctx.grad_range_hook
    if rctx.grad_rows_hook is not None and hook is not None:
        mask = torch.empty(n, dtype=torch.uint8, device=dev)
        check(lib.gags_blended_mask(fwd.n_isects, fwd.width, fwd.height, n, ptr(fwd.flatten_ids), ptr(fwd.fwd_scratch),
                                    fwd.fwd_scratch.numel(), ptr(mask), _stream()), "gags_blended_mask")
        rctx.grad_rows_hook(mask)  # before the readback below: the ranks agree on the union while the backward starts
    ranges = _channel_ranges(d, rctx.grad_range_channels) if hook is not None else None
    cap_key = (n, fwd.width, fwd.height, dev.index)
    capacity = rctx.cap_rows.get(cap_key) if (rctx.capacity_mode and hook is None and not exact_rows) else None
    trow, total, rows, pending = _row_count(lib, rctx, fwd, early, capacity)
    # a heavy view's partial rows ([rows, D] fp32) can outgrow the device (C5H: 80 M rows x 2 KB): beyond PROW_MAX_BYTES the
    # gradient is produced one 128-channel range at a time through a [rows, 128] scratch (GAGS_STAGED_RANGE_SCRATCH)
    narrow = (hook is None and pending is None and d % 128 == 0 and d > 128 and rows * d * 4 > PROW_MAX_BYTES)
    nbytes = lib.gags_bwd_staged_scratch_bytes(rows, n, 128 if narrow else d)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    wire_hook = rctx.grad_wire_hook if (ranges is not None and not (stage_bits & _lib.GAGS_STAGED_OUT_F16)) else None
    v_colors, kept, bits = _grad_buffer(rctx, fwd, stage_bits, dev, hook, wire_hook, pending, prezero)
    call = _bind_staged(lib, fwd, v_out, trow, rows, scratch, v_colors)
    if narrow:
        _run_range_scratch(call, bits, d, kept)
    elif ranges is not None:
        _run_ranged(call, rctx, fwd, bits, ranges, hook, wire_hook, kept, v_colors)
    else:
        _run_whole(call, bits, d, ptr(total) if pending is not None else None, kept, hook, v_colors)
    if pending is not None:
        true_rows = pending.get()
        if true_rows > rows:  # more rows than the remembered capacity (none was stored out of bounds): again, exact
            rctx.cap_rows[cap_key] = true_rows
            return _backward_staged(lib, rctx, fwd, v_out, stage_bits, None, exact_rows=True)
        rows = true_rows
    if hook is None and rctx.capacity_mode:
        rctx.cap_rows[cap_key] = max(rows, int(0.97 * rctx.cap_rows.get(cap_key, 0)))
    profiler.note("bwd_rows", rows)
    return v_colors


def _table_ahead(means, quats, scales, opacities, colors, viewmats, Ks, backgrounds, sh, render_mode, raw_params, aa=False):
    """What _Rasterize will be handed, known before anything runs: (d, f16, needs) = the final channel count (after SH
    evaluation and the depth channel of RGB+D / RGB+ED), whether the final table is fp16 (only a table passed through as it
    is), and which of (means2d, conics, colors, opacities, backgrounds) will require grad -- autograd's own rule: an output
    requires grad when a graph is recorded and any tensor it was computed from does.  rasterization() checks all three
    against the tensors themselves before it rasterizes.  aa: the opacities are multiplied by the projection's compensations."""
    def rg(*ts):
        return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts)
    proj = rg(means, quats, scales, viewmats, Ks) or (raw_params and rg(opacities))  # (means2d, conics, depths)
    v_opac = proj if raw_params else (rg(opacities) or (aa and proj))
    if render_mode in ("D", "ED"):
        return 1, False, (proj, proj, proj, v_opac, False)
    depth = render_mode != "RGB"
    d = (3 if sh else colors.shape[-1]) + (1 if depth else 0)
    v_cols = rg(colors) or (sh and rg(means, viewmats)) or (depth and proj)
    return (d, colors.dtype == torch.float16 and not sh and not depth,
            (proj, proj, v_cols, v_opac, rg(backgrounds)))


def rasterization(means, quats, scales, opacities, colors, viewmats, Ks, width, height,
                  near_plane=0.01, far_plane=1e10, radius_clip=0.0, eps2d=0.3, sh_degree=None, packed=False,
                  tile_size=16, backgrounds=None, render_mode="RGB", sparse_grad=False, absgrad=False,
                  rasterize_mode="classic", channel_chunk=32, distributed=False, camera_model="pinhole",
                  covars=None, raster_flags=0, raw_params=False, scaling_modifier=1.0, context=None):
    """See module docstring.  `channel_chunk` is accepted and ignored: any D is composited in a
    single pass over the sorted lists (SURVEY A12 shows this is identical per channel).
    raw_params=True (not part of gsplat's signature): `quats`, `scales`, `opacities` are the STORED parameters of
    scene/gaussian_model.py:48-61 -- `_rotation` [N,4] un-normalised, `_scaling` [N,3] log-space, `_opacity` [N] or [N,1]
    logits -- and the getters of :116-139 together with `* scaling_modifier` run inside the projection kernel
    (gags_project_fwd_raw; bit-identical to torch's exp / F.normalize / sigmoid): no elementwise launches, no extra passes
    over N, and the backward returns the gradients of the stored parameters.
    context (not part of gsplat's signature): the RasterContext that carries this caller's hooks and capacities; None = the
    calling thread's default_context().
    rasterize_mode="antialiased": Mip-Splatting's opacity compensation, comp = sqrt(max(0, det(cov2d) / det(cov2d + eps2d I)))
    from the projection kernel (no constant in the divisor); the opacity every later stage sees --
    and info["opacities"] -- is opacity * comp, and info["compensations"] is [1,N] (None in classic mode).
    absgrad=True: after backward(), info["means2d"].absgrad is the [1,N,2] sum over pixels of the absolute per-pixel
    screen-space gradients (AbsGS), overwritten by each backward; set only where a geometry gradient is produced."""
    rctx = context if context is not None else default_context()
    if tile_size != TILE:
        raise NotImplementedError("tile_size must be 16 (the gsplat default the reference relies on)")
    if rasterize_mode not in ("classic", "antialiased"):
        raise ValueError(f"unknown rasterize_mode {rasterize_mode!r} (\"classic\" or \"antialiased\")")
    if not isinstance(absgrad, bool):
        raise ValueError("absgrad must be True or False")
    aa = rasterize_mode == "antialiased"
    if camera_model != "pinhole" or covars is not None or distributed:
        raise NotImplementedError("only the options the reference uses are implemented "
                                  "(pinhole camera, quats+scales, one process per view)")
    if render_mode not in ("RGB", "D", "ED", "RGB+D", "RGB+ED"):
        raise ValueError(f"unknown render_mode {render_mode}")
    if viewmats.dim() != 3 or viewmats.shape[0] != 1 or Ks.shape[0] != 1:
        raise NotImplementedError("one camera per call (the reference renders one view per iteration, train.py:134-142)")
    n = means.shape[0]
    if means.shape != (n, 3) or quats.shape != (n, 4) or scales.shape != (n, 3):
        raise ValueError("means [N,3], quats [N,4], scales [N,3] expected")
    if opacities.shape != (n,) and not (raw_params and opacities.shape == (n, 1)):  # (the stored logits are [N,1])
        raise ValueError("opacities [N] expected" + (" (or the stored [N,1] logits with raw_params)" if raw_params else ""))
    width, height = int(width), int(height)
    viewmat, K = viewmats[0], Ks[0]

    # the final channel count -- after SH evaluation and the depth channel of RGB+D / RGB+ED -- and with it the route, once
    d, f16, needs = _table_ahead(means, quats, scales, opacities, colors, viewmats, Ks, backgrounds, sh_degree is not None,
                                 render_mode, raw_params, aa)
    route = _route(n, d, f16, needs, int(raster_flags), profiler.ENABLED, rctx.capacity_mode, rctx.early_rowmap,
                   rctx.overlap_zero_fill, rctx.grad_range_hook is not None, rctx.trim_lists, absgrad=absgrad)
    _check_absgrad_route(route, d)  # (before any launch, and before the tensors are looked at: plain values decide it)
    _need_cuda(means, quats, scales, opacities, colors, viewmats, Ks, backgrounds)

    records, compensations = None, None
    if raw_params:
        radii, means2d, depths, conics, tiles, opacities, records, *comp = _ProjectRaw.apply(
            means, quats, scales, opacities, viewmat, K, width, height, float(eps2d), float(near_plane), float(far_plane),
            float(radius_clip), float(scaling_modifier), route.records and n > 0, aa)
        if records.numel() == 0:
            records = None
        if aa:  # (already folded into `opacities` and the records by the kernel)
            compensations = comp[0]
    else:
        radii, means2d, depths, conics, tiles, *comp = _Project.apply(means, quats, scales, viewmat, K, width, height,
                                                                      float(eps2d), float(near_plane), float(far_plane),
                                                                      float(radius_clip), aa)
        if aa:  # a torch multiply: autograd carries both factors
            compensations = comp[0]
            opacities = opacities * compensations
    # [1,N,2] node callers may retain_grad() on (gaussian_renderer/__init__.py:75-78); the
    # rasterizer consumes a view of it so its .grad receives d loss / d means2d.
    means2d_c = means2d[None]
    means2d = means2d_c[0]
    if sh_degree is not None:
        if colors.dim() != 3 or colors.shape[2] != 3:
            raise ValueError("SH colours must be [N,K,3]")
        campos = torch.inverse(viewmat.double())[:3, 3].float()
        cols = _SH.apply(colors, means, campos, radii, int(sh_degree))
    else:
        if colors.dim() != 2 or colors.shape[0] != n:
            raise ValueError("colors must be [N,D] when sh_degree is None")
        cols = colors
    bg = None if backgrounds is None else backgrounds.reshape(-1)
    if render_mode in ("RGB+D", "RGB+ED"):
        cols = torch.cat([cols, depths[:, None]], dim=-1)
        if bg is not None:
            bg = torch.cat([bg, torch.zeros(1, device=bg.device)])
    elif render_mode in ("D", "ED"):
        cols = depths[:, None]
        bg = None if bg is None else torch.zeros(1, device=bg.device)

    if (d, f16, needs) != (cols.shape[-1], cols.dtype == torch.float16, tuple(
            torch.is_grad_enabled() and t is not None and t.requires_grad for t in (means2d, conics, cols, opacities, bg))):
        raise RuntimeError("gags_amd.rasterization: the colour table is not what the route was built for (_table_ahead)")

    prezero = None
    if route.zero_fill:
        # colours-only (GAD) backward ahead: its gradient tensor is mostly rows of zeros.  Fill it now, on a second stream,
        # under the binning kernels; the backward's reduce stage then writes only the rows that exist (_backward_staged)
        vbuf = torch.empty(n, d, device=cols.device, dtype=torch.float16 if f16 else torch.float32)
        side = rctx.side_stream(cols.device)
        ev0, ev1 = torch.cuda.Event(), torch.cuda.Event()
        ev0.record()
        with torch.cuda.stream(side):
            side.wait_event(ev0)
            vbuf.zero_()
            ev1.record()
        vbuf.record_stream(side)
        prezero = (vbuf, ev1)

    cap_key = (n, width, height, means.device.index)

    def run(cap):
        with torch.no_grad(), profiler.stage("binning"):
            b = tile_binning(means2d, radii, depths, tiles, width, height, conics if route.records else None,
                             _c(opacities) if route.records else None, cap, records=records, context=rctx)
        offs, flat = b.offsets_full, b.flatten_ids
        # heavy views: the lists cut to what their tiles read (_trim_lists) -- the raster passes, their scratch and the backward
        # work on the cut lists; callers still get the full ones in `info`
        trimmed = None
        n_full = flat.shape[0]
        if cap is None and n_full > 0 and route.trim is not False:
            lib_ = _lib.load()
            if route.trim or lib_.gags_raster_fwd_scratch_bytes(n_full, width, height) > TRIM_AUTO_BYTES:
                with torch.no_grad():
                    trimmed = _trim_lists(lib_, n, width, height, offs, flat, n_full, b.packed)
                offs, flat = trimmed[0], trimmed[1]
        # any width in ONE rasterization: 513 = 512 CLIP channels + 1 (BASELINE.json configs[4] "512-d feat + granularity")
        # is four 128-channel slices and one lane of a narrow slice on the same matrix-core kernels, into one output tensor
        r = _Rasterize.apply(means2d, conics, cols, opacities, bg, offs, flat, b.packed, width, height, route, rctx, prezero,
                             [means2d_c] if route.absgrad else None)
        if trimmed is not None:
            # last_ids are sorted indices: a COPY goes back to the full lists' numbering for the caller (the autograd node keeps
            # its own, which matches the lists it saved)
            with torch.no_grad():
                last_user = r[2].clone()
                check(_lib.load().gags_trim_last_ids(width, height, ptr(b.offsets_full), ptr(offs), ptr(r[1]), ptr(last_user), _stream()),
                      "gags_trim_last_ids")
            profiler.note("isects_trimmed", trimmed[2])
            r = (r[0], r[1], last_user, trimmed[2])
        else:
            r = (r[0], r[1], r[2], None)
        return b, r

    cap = None
    if rctx.capacity_mode and cap_key in rctx.cap_isects:
        cap = min(MAX_ISECTS - 1, int(rctx.cap_isects[cap_key] * CAP_MARGIN) + 4096)
    (isect_ids, flatten_ids, isect_offsets, n_isects, packed, _), (out, alphas, last_ids, n_trimmed) = run(cap)
    if cap is not None:
        n_true = n_isects.get()  # (the scan that produced it finished long ago: everything above is already enqueued)
        _check_isects(n_true, _tiles(width, height)[2])
        if n_true > cap:  # more intersections than the remembered capacity: nothing was written out of bounds; run again, exact
            (isect_ids, flatten_ids, isect_offsets, n_isects, packed, _), (out, alphas, last_ids, n_trimmed) = run(None)
        else:
            n_isects = n_true
            isect_ids, flatten_ids = isect_ids[:n_true], flatten_ids[:n_true]
    if rctx.capacity_mode:
        rctx.cap_isects[cap_key] = max(n_isects, int(0.97 * rctx.cap_isects.get(cap_key, 0)))
    if render_mode in ("ED", "RGB+ED"):
        if out.requires_grad:
            out = torch.cat([out[..., :-1], out[..., -1:] / alphas[..., None].clamp(min=1e-10)], dim=-1)
        else:  # K12 in place
            check(_lib.load().gags_ed_normalize(height * width, out.shape[-1], ptr(out), ptr(alphas), _stream()),
                  "gags_ed_normalize")

    tile_w, tile_h, _ = _tiles(width, height)
    info = {
        "camera_ids": None, "gaussian_ids": None,
        "radii": radii[None], "means2d": means2d_c, "depths": depths[None], "conics": conics[None],
        "opacities": opacities[None], "compensations": None if compensations is None else compensations[None],
        "tile_width": tile_w, "tile_height": tile_h,
        "tiles_per_gauss": tiles[None], "isect_ids": isect_ids, "flatten_ids": flatten_ids,
        "isect_offsets": isect_offsets[None], "last_ids": last_ids, "width": width, "height": height,
        "tile_size": TILE, "n_cameras": 1, "n_isects": n_isects,
        "n_isects_trimmed": n_trimmed,  # (not gsplat's: list entries the raster passes worked on when the lists were trimmed, else None)
    }
    return out[None], alphas[None, ..., None], info
