"""The staged colours-only backward: the row map (at forward or backward time), the gradient buffer, and the three drivers of
gags_raster_bwd_colors_staged (whole view, range-sized scratch, ranges under the exchange hooks)."""
from typing import Any, NamedTuple

import torch

from . import _lib, profiler
from . import raster_tunables as T
from ._lib import check, ptr
from .raster_context import _DeferredCount, _read_count


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


def _rowmap(lib, fwd):
    """The view's partial gradient rows numbered on the device (gags_bwd_rowmap, enqueued on the current stream; the one place
    that knows that call).  Returns (rowmap, total = the row count, int32 [1] on the device, the scan's scratch)."""
    dev = fwd.blk_rows.device
    ne = lib.gags_bwd_rowmap_elems(fwd.n_isects, fwd.width, fwd.height)
    trow = torch.empty(ne, dtype=torch.int32, device=dev)
    total = torch.empty(1, dtype=torch.int32, device=dev)
    sb = lib.gags_bwd_rowmap_scratch_bytes(fwd.n_isects)
    stmp = _lib.scratch(max(sb, 4), dev)
    check(lib.gags_bwd_rowmap(fwd.n_isects, fwd.width, fwd.height, ptr(fwd.offsets), ptr(fwd.blk_rows), ptr(fwd.fwd_scratch),
                              fwd.fwd_scratch.numel(), ptr(trow), ne, ptr(total), ptr(stmp), sb, _lib.stream()), "gags_bwd_rowmap")
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
            return trow, total, min(max(fwd.n_isects, 1), int(capacity * T.CAP_MARGIN) + 1024), _DeferredCount(total, rctx)
        return trow, total, _read_count(lib, total), None


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
    st = _lib.stream()
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
    segmented sum.  fwd: the forward's _FwdState; stage_bits: raster_route._stage_bits(); prezero, early: what the forward prepared
    (a zero-filled gradient, the row map); exact_rows: the re-run of a capacity-mode backward whose capacity was too small."""
    dev = v_out.device
    n, d = fwd.n, fwd.d
    hook = rctx.grad_range_hook
    if rctx.grad_rows_hook is not None and hook is not None:
        mask = torch.empty(n, dtype=torch.uint8, device=dev)
        check(lib.gags_blended_mask(fwd.n_isects, fwd.width, fwd.height, n, ptr(fwd.flatten_ids), ptr(fwd.fwd_scratch),
                                    fwd.fwd_scratch.numel(), ptr(mask), _lib.stream()), "gags_blended_mask")
        rctx.grad_rows_hook(mask)  # before the readback below: the ranks agree on the union while the backward starts
    ranges = _channel_ranges(d, rctx.grad_range_channels) if hook is not None else None
    cap_key = (n, fwd.width, fwd.height, dev.index)
    capacity = rctx.cap_rows.get(cap_key) if (rctx.capacity_mode and hook is None and not exact_rows) else None
    trow, total, rows, pending = _row_count(lib, rctx, fwd, early, capacity)
    # a heavy view's partial rows ([rows, D] fp32) can outgrow the device (C5H: 80 M rows x 2 KB): beyond PROW_MAX_BYTES the
    # gradient is produced one 128-channel range at a time through a [rows, 128] scratch (GAGS_STAGED_RANGE_SCRATCH)
    narrow = (hook is None and pending is None and d % 128 == 0 and d > 128 and rows * d * 4 > T.PROW_MAX_BYTES)
    nbytes = lib.gags_bwd_staged_scratch_bytes(rows, n, 128 if narrow else d)
    scratch = _lib.scratch(nbytes, dev)
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
