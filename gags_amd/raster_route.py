"""Which kernels serve one rasterization() call (_route, decided once from plain values), and the translations of the public
raster_flags into the flag / stage words of the C entries."""
from typing import Any, NamedTuple

from . import _lib
from . import raster_tunables as T

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
                  zero_fill=bool(overlap_zero_fill) and not hooked and bwd == _BWD_STAGED and n * d >= T.ZERO_FILL_MIN_ELEMS,
                  absgrad=bool(absgrad) and bool(geom) and bwd in (_BWD_STAGED_GEOM, _BWD_VALU))


def _check_absgrad_route(route, d):
    """absgrad on the one route that cannot serve it: the VALU kernel splits a pixel's channels over blocks above
    ABSGRAD_VALU_MAX_D, and an absolute value of a partial sum is not the rule."""
    if route.absgrad and route.bwd == _BWD_VALU and d > T.ABSGRAD_VALU_MAX_D:
        raise NotImplementedError(
            f"absgrad=True with geometry gradients at D = {d} on the VALU backward: served for D <= {T.ABSGRAD_VALU_MAX_D} there, "
            "and for every D % 8 == 0 in 16..1024 on the matrix-core geometry pass (DESIGN.md section 7, N16)")


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
