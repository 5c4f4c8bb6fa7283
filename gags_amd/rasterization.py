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

The parts live in one module each and are re-exported here under their names: raster_context (RasterContext, the persistent
gradient buffer), raster_project (_Project, _ProjectRaw, _SH), raster_binning (tile_binning, list trimming), raster_route
(_route and the flag translations), raster_staged (the staged colours-only backward), raster_function (_Rasterize).  The
tunables are NOT re-exported: they are read, and changed, on raster_tunables alone.
"""
from typing import Any, NamedTuple

import torch

from . import _lib, profiler
from . import raster_tunables as T
from ._lib import check, ptr
from .raster_binning import Binning, _check_isects, _tiles, _trim_lists, tile_binning  # noqa: F401
from .raster_context import RasterContext, _KeptGrad, default_context, grad_written  # noqa: F401
from .raster_function import _Rasterize
from .raster_project import _c, _Project, _ProjectRaw, _SH
from .raster_route import _Route, _bwd_flags, _check_absgrad_route, _fwd_flags, _geom_flags, _route, _stage_bits  # noqa: F401
from .raster_staged import _EarlyRowmap  # noqa: F401


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


def _table_ahead(means, quats, scales, opacities, colors, viewmats, Ks, backgrounds, sh, render_mode, raw_params, aa=False,
                 radial_coeffs=None):
    """What _Rasterize will be handed, known before anything runs: (d, f16, needs) = the final channel count (after SH
    evaluation and the depth channel of RGB+D / RGB+ED), whether the final table is fp16 (only a table passed through as it
    is), and which of (means2d, conics, colors, opacities, backgrounds) will require grad -- autograd's own rule: an output
    requires grad when a graph is recorded and any tensor it was computed from does.  rasterization() checks all three
    against the tensors themselves before it rasterizes.  aa: the opacities are multiplied by the projection's compensations."""
    def rg(*ts):
        return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts)
    proj = rg(means, quats, scales, viewmats, Ks, radial_coeffs) or (raw_params and rg(opacities))  # (means2d, conics, depths)
    v_opac = proj if raw_params else (rg(opacities) or (aa and proj))
    if render_mode in ("D", "ED"):
        return 1, False, (proj, proj, proj, v_opac, False)
    depth = render_mode != "RGB"
    d = (3 if sh else colors.shape[-1]) + (1 if depth else 0)
    v_cols = rg(colors) or (sh and rg(means, viewmats)) or (depth and proj)
    return (d, colors.dtype == torch.float16 and not sh and not depth,
            (proj, proj, v_cols, v_opac, rg(backgrounds)))


def _kb_block(K, coeffs):
    """The 13 floats GAGS_PROJ_KB reads, [K row-major, k1 .. k4] (N21).  When K [3,3] and coeffs already lie so in memory
    (render() keeps the block in its context's k_cache and hands over two views of it) that memory is the block: no launch.
    When K or coeffs requires grad (N23) the block is a torch.cat of the two, not detached: autograd splits the block's
    13-float gradient into Ks.grad and radial_coeffs.grad."""
    if torch.is_grad_enabled() and (K.requires_grad or coeffs.requires_grad):
        return torch.cat([K.reshape(9).float(), coeffs.reshape(4)])
    K, c = K.detach(), coeffs.detach().reshape(4)
    if (K.dtype == torch.float32 and K.is_contiguous() and c.is_contiguous() and K.device == c.device
            and K.untyped_storage().data_ptr() == c.untyped_storage().data_ptr() and c.storage_offset() == K.storage_offset() + 9):
        return torch.as_strided(K, (13,), (1,))
    return torch.cat([K.reshape(9).float(), c])


class _Pass(NamedTuple):
    """One binning + rasterize pass of rasterization() (`run` there)."""
    binning: Binning
    out: Any
    alphas: Any
    last_ids: Any   # in the full lists' numbering
    n_trimmed: Any  # entries of the trimmed lists, or None when the lists were not trimmed


def rasterization(means, quats, scales, opacities, colors, viewmats, Ks, width, height,
                  near_plane=0.01, far_plane=1e10, radius_clip=0.0, eps2d=0.3, sh_degree=None, packed=False,
                  tile_size=16, backgrounds=None, render_mode="RGB", sparse_grad=False, absgrad=False,
                  rasterize_mode="classic", channel_chunk=32, distributed=False, camera_model="pinhole",
                  covars=None, raster_flags=0, raw_params=False, scaling_modifier=1.0, context=None, radial_coeffs=None):
    """See module docstring.  `channel_chunk` is accepted and ignored: any D is composited in a
    single pass over the sorted lists (SURVEY A12 shows this is identical per channel).
    raw_params=True (not part of gsplat's signature): `quats`, `scales`, `opacities` are the STORED parameters of
    scene/gaussian_model.py:48-61 -- `_rotation` [N,4] un-normalised, `_scaling` [N,3] log-space, `_opacity` [N] or [N,1]
    logits -- and the getters of :116-139 together with `* scaling_modifier` run inside the projection kernel
    (GAGS_PROJ_RAW; bit-identical to torch's exp / F.normalize / sigmoid): no elementwise launches, no extra passes
    over N, and the backward returns the gradients of the stored parameters.
    context (not part of gsplat's signature): the RasterContext that carries this caller's hooks and capacities; None = the
    calling thread's default_context().
    rasterize_mode="antialiased": Mip-Splatting's opacity compensation, comp = sqrt(max(0, det(cov2d) / det(cov2d + eps2d I)))
    from the projection kernel (no constant in the divisor); the opacity every later stage sees --
    and info["opacities"] -- is opacity * comp, and info["compensations"] is [1,N] (None in classic mode).
    viewmats.requires_grad (N17): after backward(), viewmats.grad [1,4,4] is d loss / d viewmats -- the
    projection backward produces it on the way (GAGS_PROJ_POSE, a deterministic sum over N, row 3 exactly zero), and the
    SH view direction reaches it through campos = inverse(viewmat)[:3, 3], as in gsplat (torch's backward of the 4 x 4 inverse:
    with sh_degree row 3 gets what that puts there).  Scene tensors that need no gradient
    get none computed (pose refinement against a frozen scene).  With viewmats not requiring grad nothing changes: same
    launches, same bits.
    Ks.requires_grad / radial_coeffs.requires_grad (N23): after backward(), Ks.grad [1,3,3] holds the
    cotangents of fx, fy, cx, cy (exact zeros in the five constant entries) and radial_coeffs.grad (shaped as given) those of
    k1 .. k4: the exact derivative of the projection as it is written, the culls not differentiated, a deterministic sum over
    N (gags_project_bwd_calib: the pose kernel with eight more sums; it composes with viewmats.requires_grad and with frozen
    scene tensors).  With neither requiring grad nothing changes: the same two projection entries, same launches, same bits.
    camera_model (N20): "pinhole", "ortho" (means2d = (fx x + cx, fy y + cy); fx, fy pixels per world unit)
    or "fisheye" (equidistant, distortion coefficients through radial_coeffs; z < near_plane is still culled, so the field of view stays below
    180 degrees).  Only the projection kernels differ: every model, the pinhole included, goes through the flagged pair
    gags_project_fwd_cam / gags_project_bwd_cam(camera_model, flags) -- the package calls no other projection entry; the named
    entries (gags_project_fwd, ..._raw_aa, gags_project_bwd_pose) are compatibility forms of the pair for external callers, and
    the pinhole kernels are the ones they launch.  info["camera_model"] repeats it.
    radial_coeffs (N21; only with camera_model="fisheye"): the lens' distortion coefficients (k1, k2, k3, k4) of OpenCV's fisheye
    model / COLMAP's OPENCV_FISHEYE, theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8), a float32 tensor
    [4] or [1,4] on the GPU.  They reach the projection kernels as 13 floats [K, k1 .. k4] behind GAGS_PROJ_KB and go through
    the same linearisation (cov2d = J Sc J^T) as every model; a Gaussian past the angle where theta_d stops growing is culled;
    they get a gradient when they require one (N23, above).  The block is built on the device with one copy kernel -- unless
    Ks[0] and radial_coeffs already lie so in memory, as the views render() hands over do (and neither requires grad: then the
    block is a torch.cat autograd can split).  None: the call without the argument, same
    launches, flags and bits.  info["radial_coeffs"] repeats the tensor (or None).
    absgrad=True: after backward(), info["means2d"].absgrad is the [1,N,2] sum over pixels of the absolute per-pixel
    screen-space gradients (AbsGS), overwritten by each backward; set only where a geometry gradient is produced."""
    rctx = context if context is not None else default_context()
    if tile_size != T.TILE:
        raise NotImplementedError("tile_size must be 16 (the gsplat default the reference relies on)")
    if rasterize_mode not in ("classic", "antialiased"):
        raise ValueError(f"unknown rasterize_mode {rasterize_mode!r} (\"classic\" or \"antialiased\")")
    if not isinstance(absgrad, bool):
        raise ValueError("absgrad must be True or False")
    aa = rasterize_mode == "antialiased"
    if not isinstance(camera_model, str) or camera_model not in _lib.CAMERA_MODELS:  # (plain values: before any tensor is looked at)
        raise ValueError(f"unknown camera_model {camera_model!r} (\"pinhole\", \"ortho\" or \"fisheye\")")
    cam = _lib.CAMERA_MODELS[camera_model]
    kb = radial_coeffs is not None
    if kb:
        if camera_model != "fisheye":
            raise ValueError(f"radial_coeffs are the distortion coefficients of camera_model=\"fisheye\", not of {camera_model!r}")
        if not torch.is_tensor(radial_coeffs) or tuple(radial_coeffs.shape) not in ((4,), (1, 4)) or radial_coeffs.dtype != torch.float32:
            raise ValueError("radial_coeffs must be a float32 tensor [4] or [1,4]: (k1, k2, k3, k4)")
    if covars is not None or distributed:
        raise NotImplementedError("only the options the reference uses are implemented "
                                  "(quats+scales, one process per view)")
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
                                 render_mode, raw_params, aa, radial_coeffs=radial_coeffs)
    route =_route(n, d, f16, needs, int(raster_flags), profiler.ENABLED, rctx.capacity_mode, rctx.early_rowmap,
                   rctx.overlap_zero_fill, rctx.grad_range_hook is not None, rctx.trim_lists, absgrad=absgrad)
    _check_absgrad_route(route, d)  # (before any launch, and before the tensors are looked at: plain values decide it)
    _need_cuda(means, quats, scales, opacities, colors, viewmats, Ks, backgrounds, radial_coeffs)
    if kb:
        K = _kb_block(K, radial_coeffs)

    records, compensations = None, None
    if raw_params:
        radii, means2d, depths, conics, tiles, opacities, records, *comp = _ProjectRaw.apply(
            means, quats, scales, opacities, viewmat, K, width, height, float(eps2d), float(near_plane), float(far_plane),
            float(radius_clip), float(scaling_modifier), route.records and n > 0, aa, cam, kb)
        if records.numel() == 0:
            records = None
        if aa:  # (already folded into `opacities` and the records by the kernel)
            compensations = comp[0]
    else:
        radii, means2d, depths, conics, tiles, *comp = _Project.apply(means, quats, scales, viewmat, K, width, height,
                                                                      float(eps2d), float(near_plane), float(far_plane),
                                                                      float(radius_clip), aa, cam, kb)
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
            if route.trim or lib_.gags_raster_fwd_scratch_bytes(n_full, width, height) > T.TRIM_AUTO_BYTES:
                with torch.no_grad():
                    trimmed = _trim_lists(lib_, n, width, height, offs, flat, n_full, b.packed)
                offs, flat = trimmed[0], trimmed[1]
        # any width in ONE rasterization: 513 = 512 CLIP channels + 1 (BASELINE.json configs[4] "512-d feat + granularity")
        # is four 128-channel slices and one lane of a narrow slice on the same matrix-core kernels, into one output tensor
        out, alphas, last_ids = _Rasterize.apply(means2d, conics, cols, opacities, bg, offs, flat, b.packed, width, height, route,
                                                 rctx, prezero, [means2d_c] if route.absgrad else None)
        if trimmed is None:
            return _Pass(b, out, alphas, last_ids, None)
        # last_ids are sorted indices: a COPY goes back to the full lists' numbering for the caller (the autograd node keeps
        # its own, which matches the lists it saved)
        with torch.no_grad():
            last_user = last_ids.clone()
            check(_lib.load().gags_trim_last_ids(width, height, ptr(b.offsets_full), ptr(offs), ptr(alphas), ptr(last_user),
                                                 _lib.stream()), "gags_trim_last_ids")
        profiler.note("isects_trimmed", trimmed[2])
        return _Pass(b, out, alphas, last_user, trimmed[2])

    cap = None
    if rctx.capacity_mode and cap_key in rctx.cap_isects:
        cap = min(T.MAX_ISECTS - 1, int(rctx.cap_isects[cap_key] * T.CAP_MARGIN) + 4096)
    p = run(cap)
    isect_ids, flatten_ids, n_isects = p.binning.isect_ids, p.binning.flatten_ids, p.binning.n_isects
    if cap is not None:
        n_isects = n_isects.get()  # (the scan that produced it finished long ago: everything above is already enqueued)
        _check_isects(n_isects, _tiles(width, height)[2])
        if n_isects > cap:  # more intersections than the remembered capacity: nothing was written out of bounds; run again, exact
            p = run(None)
            isect_ids, flatten_ids, n_isects = p.binning.isect_ids, p.binning.flatten_ids, p.binning.n_isects
        else:
            isect_ids, flatten_ids = isect_ids[:n_isects], flatten_ids[:n_isects]
    if rctx.capacity_mode:
        rctx.cap_isects[cap_key] = max(n_isects, int(0.97 * rctx.cap_isects.get(cap_key, 0)))
    out, alphas = p.out, p.alphas
    if render_mode in ("ED", "RGB+ED"):
        if out.requires_grad:
            out = torch.cat([out[..., :-1], out[..., -1:] / alphas[..., None].clamp(min=1e-10)], dim=-1)
        else:  # K12 in place
            check(_lib.load().gags_ed_normalize(height * width, out.shape[-1], ptr(out), ptr(alphas), _lib.stream()),
                  "gags_ed_normalize")

    tile_w, tile_h, _ = _tiles(width, height)
    info = {
        "camera_ids": None, "gaussian_ids": None,
        "radii": radii[None], "means2d": means2d_c, "depths": depths[None], "conics": conics[None],
        "opacities": opacities[None], "compensations": None if compensations is None else compensations[None],
        "tile_width": tile_w, "tile_height": tile_h,
        "tiles_per_gauss": tiles[None], "isect_ids": isect_ids, "flatten_ids": flatten_ids,
        "isect_offsets": p.binning.isect_offsets[None], "last_ids": p.last_ids, "width": width, "height": height,
        "tile_size": T.TILE, "n_cameras": 1, "n_isects": n_isects, "camera_model": camera_model,
        "radial_coeffs": radial_coeffs,
        "n_isects_trimmed": p.n_trimmed,  # (not gsplat's: list entries the raster passes worked on when the lists were trimmed, else None)
    }
    return out[None], alphas[None, ..., None], info
