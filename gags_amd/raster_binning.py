"""Binning of a view's Gaussians into sorted per-tile lists (tile_binning), and the trimming of those lists for heavy views."""
from typing import Any, NamedTuple

import torch

from . import _lib, profiler
from . import raster_tunables as T
from ._lib import check, ptr
from .raster_context import _DeferredCount, _read_count, default_context


def _tiles(width, height):
    """(tile_w, tile_h, number of tiles) of a width x height view."""
    tile_w, tile_h = (width + T.TILE - 1) // T.TILE, (height + T.TILE - 1) // T.TILE
    return tile_w, tile_h, tile_w * tile_h


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
    st = _lib.stream()
    dev = means2d.device
    n = radii.shape[0]
    tile_w, tile_h, n_tiles = _tiles(width, height)
    tile_bits = max(1, n_tiles.bit_length())  # (room for the sentinel tile id n_tiles of the capacity mode)
    cum = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    total = torch.empty(1, dtype=torch.int32, device=dev)
    early = None
    if cap is None and T.EARLY_COUNT and n > 0:
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
    dscratch = _lib.scratch(dsb, dev)
    check(lib.gags_depth_order(n, ptr(depths), None, ptr(order), None, ptr(dscratch), dsb, st), "gags_depth_order")
    sb = lib.gags_scan_scratch_bytes(n)
    scratch = _lib.scratch(sb, dev)
    # prefix sum of the tile counts IN DEPTH ORDER, read through `order` (no permuted copy)
    check(lib.gags_cumsum_gather_i32(n, ptr(tiles_per_gauss), ptr(order), ptr(cum), ptr(total), ptr(scratch), sb, st),
          "gags_cumsum_gather_i32")
    if cap is None:
        if early is not None:
            early.synchronize()
            n_isects = int(host64[0])
        else:
            n_isects = _read_count(lib, total)
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
        sscratch = _lib.scratch(ssb, dev)
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
    st = _lib.stream()
    dev = flatten_ids.device
    n_tiles = _tiles(width, height)[2]
    need = torch.empty(n_tiles, dtype=torch.int32, device=dev)
    with profiler.stage("list_need"):
        check(lib.gags_raster_list_need(n, width, height, ptr(offsets_full), ptr(flatten_ids), n_isects, ptr(packed),
                                        _lib.GAGS_RECS_BY_GAUSSIAN, ptr(need), st), "gags_raster_list_need")
    cum = torch.empty(n_tiles, dtype=torch.int32, device=dev)
    total = torch.empty(1, dtype=torch.int32, device=dev)
    sb = lib.gags_scan_scratch_bytes(n_tiles)
    scratch = _lib.scratch(sb, dev)
    check(lib.gags_cumsum_i32(n_tiles, ptr(need), ptr(cum), ptr(total), ptr(scratch), sb, st), "gags_cumsum_i32")
    t = _read_count(lib, total)
    offs_t = torch.empty(n_tiles + 1, dtype=torch.int32, device=dev)
    flat_t = torch.empty(t, dtype=torch.int32, device=dev)
    check(lib.gags_trim_lists(width, height, ptr(offsets_full), ptr(cum), ptr(flatten_ids), ptr(offs_t),
                              ptr(flat_t) if t > 0 else None, st), "gags_trim_lists")
    return offs_t, flat_t, t


def _check_isects(n_isects, n_tiles=0):
    # the int32 prefix sum wrapped, or the slot space (4 I + 64 tiles + 64 slots, 32-bit byte offsets of its id table) would
    if n_isects < 0 or n_isects >= T.MAX_ISECTS or 4 * n_isects + 64 * n_tiles + 64 >= (1 << 30):
        raise RuntimeError(f"gags_amd.rasterization: {n_isects if n_isects >= 0 else '> 2^31'} tile intersections in one "
                           f"view; the kernels index at most 2^28 = {T.MAX_ISECTS} less 16 per tile (INTEGRATION.md, memory model)")
