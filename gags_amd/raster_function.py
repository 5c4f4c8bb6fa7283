"""_Rasterize: the autograd function over pre-binned intersections, and its three backwards (staged colours-only, staged +
matrix-core geometry, VALU).  Every caller of _backward_staged lives here."""
import torch

from . import _lib, profiler
from . import raster_tunables as T
from ._lib import check, ptr
from .raster_binning import _tiles
from .raster_project import _c
from .raster_route import (_BWD_STAGED, _BWD_STAGED_GEOM, _FWD_SPLIT, _bwd_flags, _check_absgrad_route, _fwd_flags,
                           _geom_flags, _stage_bits)
from .raster_staged import _FwdState, _backward_staged, _early_rowmap


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
                    scratch = _lib.scratch(nbytes, dev)
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
                                      cflags | extra, _lib.stream()), "gags_raster_fwd")

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
    if T.GEOM_COMPACT_ROWS:
        incl = torch.cumsum(fwd.blk_rows, 0, dtype=torch.int32)
        row_base = (incl - fwd.blk_rows).contiguous()
        n_rows = int(incl[-1].item()) if incl.numel() else 0
    else:  # the C ABI's other numbering: rows (and the dot products) in the sparse slot space, no count needed
        row_base, n_rows = None, -1
    nb = lib.gags_raster_bwd_geom_scratch_bytes(fwd.n_isects, fwd.width, fwd.height, fwd.n, fwd.d, n_rows)
    gscratch = _lib.scratch(nb, dev)
    v_geo = torch.empty(fwd.n, 8, device=dev)
    with profiler.stage("raster_bwd_geom"):
        check(lib.gags_raster_bwd_geom(fwd.d, fwd.n, fwd.width, fwd.height, ptr(colors), ptr(backgrounds), ptr(fwd.offsets),
                                       fwd.n_isects, ptr(packed), ptr(v_out), ptr(v_alphas), ptr(fwd.blk_rows),
                                       ptr(fwd.fwd_scratch), fwd.fwd_scratch.numel(), ptr(gscratch), nb, ptr(v_geo),
                                       ptr(fwd.flatten_ids), ptr(row_base), n_rows, _geom_flags(route), _lib.stream()),
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
                                          ptr(v_opac), ptr(v_m2d), ptr(v_con), ptr(v_abs), _bwd_flags(route), _lib.stream()),
                  "gags_raster_bwd_abs")
        return v_m2d, v_con, v_colors.half() if route.half else v_colors, v_opac, v_abs
    with profiler.stage("raster_bwd"):
        check(lib.gags_raster_bwd(fwd.d, fwd.width, fwd.height, ptr(means2d), ptr(conics), ptr(opacities), ptr(colors),
                                  ptr(backgrounds), ptr(fwd.offsets), ptr(fwd.flatten_ids), fwd.n_isects, ptr(packed),
                                  ptr(alphas), ptr(last_ids), ptr(v_out), ptr(v_alphas), ptr(v_colors),
                                  ptr(v_opac), ptr(v_m2d), ptr(v_con), _bwd_flags(route), _lib.stream()), "gags_raster_bwd")
    return v_m2d, v_con, v_colors.half() if route.half else v_colors, v_opac
