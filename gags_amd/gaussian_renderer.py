"""Drop-in for /root/reference/gaussian_renderer/__init__.py: `render(...)`.

Same signature, same attribute reads on `viewpoint_camera` (FoVx, FoVy, image_width,
image_height, world_view_transform) and `pc` (get_xyz, get_opacity, get_scaling,
get_rotation, get_semantic_feature, get_features, active_sh_degree), same returned dict
(`render` [D',H,W] as a permuted view of [H,W,D'], `viewspace_points` [1,N,2],
`visibility_filter` [N] bool, `radii` [N] int32).  `pipe` is accepted and ignored, as in the
reference (its PipelineParams are never read on this path).  The only difference is what
executes underneath: gags_amd.rasterization instead of gsplat.rasterization.
"""
import math

import torch

from .rasterization import default_context, rasterization
from .scene import GaussianModel

# The reference re-uploads K with torch.tensor(..., device="cuda") on every call
# (gaussian_renderer/__init__.py:31-38).  K depends only on (FoVx, FoVy, W, H); the device copy stays resident in the
# caller's RasterContext instead of paying a pageable H2D copy per iteration.
def camera_model_of(viewpoint_camera):
    """The camera's model (N20): its `camera_model` attribute, "pinhole" for a camera without one (the reference's)."""
    return getattr(viewpoint_camera, "camera_model", "pinhole")


def _intrinsics(viewpoint_camera, device, cache):
    """K [3,3] on `device`.  A camera that carries a `K` attribute is rendered with that K (N20: the only way to give a fisheye
    or orthographic camera its intrinsics -- FoV -> focal is a pinhole relation and is not reinterpreted); its nine values are
    part of the cache key, so that cameras that differ only in K do not share an entry."""
    explicit = getattr(viewpoint_camera, "K", None)
    if explicit is not None:
        vals = tuple(float(v) for v in torch.as_tensor(explicit).detach().reshape(-1).tolist())
        if len(vals) != 9:
            raise ValueError("a camera's K must be [3,3]")
        key = ("K", vals, str(device))
        K = cache.get(key)
        if K is None:
            K = torch.tensor(vals, dtype=torch.float32, device=device).reshape(3, 3)
            if len(cache) > 4096:
                cache.clear()
            cache[key] = K
        return K
    if camera_model_of(viewpoint_camera) != "pinhole":
        raise ValueError(f"a {camera_model_of(viewpoint_camera)!r} camera needs an explicit K [3,3] attribute: FoVx / FoVy define "
                         "a focal length for a pinhole camera only")
    key = (float(viewpoint_camera.FoVx), float(viewpoint_camera.FoVy), int(viewpoint_camera.image_width),
           int(viewpoint_camera.image_height), str(device))
    K = cache.get(key)
    if K is None:
        tanfovx = math.tan(viewpoint_camera.FoVx * 0.5)
        tanfovy = math.tan(viewpoint_camera.FoVy * 0.5)
        focal_length_x = viewpoint_camera.image_width / (2 * tanfovx)
        focal_length_y = viewpoint_camera.image_height / (2 * tanfovy)
        K = torch.tensor(
            [[focal_length_x, 0, viewpoint_camera.image_width / 2.0],
             [0, focal_length_y, viewpoint_camera.image_height / 2.0],
             [0, 0, 1]], device=device)
        if len(cache) > 4096:
            cache.clear()
        cache[key] = K
    return K


def _intrinsics_kb(viewpoint_camera, device, cache):
    """(K [3,3], radial_coeffs [4]) of a camera that carries distortion coefficients (N21): two views of ONE resident block of
    13 floats, [K row-major, k1 .. k4], which is what the projection kernels read behind GAGS_PROJ_KB -- rasterization()
    recognises the layout and launches nothing to build it.  The block lives in `cache` as K does; the nine values of K and
    the four coefficients are the key, so that cameras that differ only in their coefficients do not share an entry."""
    explicit = getattr(viewpoint_camera, "K", None)
    if explicit is None:
        raise ValueError("a camera with radial_coeffs needs an explicit K [3,3] attribute")
    vals = tuple(float(v) for v in torch.as_tensor(explicit).detach().reshape(-1).tolist())
    coeffs = tuple(float(v) for v in torch.as_tensor(viewpoint_camera.radial_coeffs).detach().reshape(-1).tolist())
    if len(vals) != 9 or len(coeffs) != 4:
        raise ValueError("a camera's K must be [3,3] and its radial_coeffs [4]")
    key = ("KB", vals, coeffs, str(device))
    block = cache.get(key)
    if block is None:
        block = torch.tensor(vals + coeffs, dtype=torch.float32, device=device)
        if len(cache) > 4096:
            cache.clear()
        cache[key] = block
    return block[:9].view(3, 3), block[9:]


def _trainable(t):
    return torch.is_tensor(t) and t.requires_grad


def _intrinsics_trainable(viewpoint_camera, device):
    """(K [3,3], radial_coeffs [4] or None) of a camera whose K or radial_coeffs is a tensor that requires grad (N23): the
    tensors are handed through as they are, so that rasterization()'s gradient reaches whatever they were computed from
    (pose.IntrinsicsDelta) -- no cache entry, no host readback.  They must already be what the kernels read: float32, on the
    scene's device, [3,3] / [4]; anything else is a ValueError before any launch.  The one of the two that does not require
    grad may be anything torch.as_tensor takes: it is brought to that form here."""
    K = getattr(viewpoint_camera, "K", None)
    coeffs = getattr(viewpoint_camera, "radial_coeffs", None)
    if K is None:
        raise ValueError("a camera with trainable intrinsics needs an explicit K [3,3] attribute")

    def as_given(t, shape, name):
        if _trainable(t):
            if t.device != device or t.dtype != torch.float32 or tuple(t.shape) != shape:
                raise ValueError(f"a camera's trainable {name} must be a float32 tensor {list(shape)} on {device}, not "
                                 f"{t.dtype} {list(t.shape)} on {t.device}")
            return t
        t = torch.as_tensor(t).detach()
        if t.numel() != shape[0] * (shape[1] if len(shape) > 1 else 1):
            raise ValueError("a camera's K must be [3,3] and its radial_coeffs [4]")
        return t.to(device=device, dtype=torch.float32).reshape(shape)

    return as_given(K, (3, 3), "K"), None if coeffs is None else as_given(coeffs, (4,), "radial_coeffs")


# R2 folded into R4 (the getters are "4 elementwise kernels/iter over N (fusable into projection)"): when `pc`
# stores its parameters the way scene/gaussian_model.py:48-61 does and activates them the way :36-42 does (exp, sigmoid,
# F.normalize), render() hands the STORED tensors to the projection kernel, which applies those getters itself -- bit for
# bit what torch computes (tools/micro/actprobe.py; tests/test_parity_gpu.py::test_raw_parameter_projection_*).  Any other
# `pc` goes through its getters, as in the reference.  False: always the getters.
RAW_PARAMS = True


def _stored_parameters(pc):
    """(rotation, scaling_log, opacity_logit) when `pc` provably activates its parameters the way
    scene/gaussian_model.py:36-42,116-139 does, else None (the getters are called, as in the reference).

    "Provably": `pc` is this package's GaussianModel with its getters NOT overridden (a subclass that clamps, masks or
    re-activates in get_scaling / get_opacity / get_rotation goes through its getters), or any other model that carries the
    reference's three activation attributes and they ARE torch.exp / torch.sigmoid / F.normalize (the reference's
    GaussianModel.setup_functions).  A duck-typed model without those attributes is never assumed to use them."""
    if not RAW_PARAMS:
        return None
    try:
        rot, scal, opac = pc._rotation, pc._scaling, pc._opacity
    except AttributeError:
        return None
    F = torch.nn.functional
    cls = type(pc)
    own = isinstance(pc, GaussianModel) and all(
        getattr(cls, name, None) is getattr(GaussianModel, name) for name in ("get_scaling", "get_rotation", "get_opacity"))
    if not own:
        try:
            if (pc.scaling_activation is not torch.exp or pc.opacity_activation is not torch.sigmoid
                    or pc.rotation_activation is not F.normalize):
                return None
        except AttributeError:
            return None
        if isinstance(pc, GaussianModel):  # (a subclass of ours with overridden getters: the attributes do not describe them)
            return None
    n = pc.get_xyz.shape[0]
    if not all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 for t in (rot, scal, opac)):
        return None
    if tuple(rot.shape) != (n, 4) or tuple(scal.shape) != (n, 3) or tuple(opac.shape) != (n, 1):
        return None
    return rot, scal, opac


def render(viewpoint_camera, pc, pipe, bg_color: torch.Tensor, feature_mode=True, scaling_modifier=1.0,
           override_color=None, render_mode="RGB", raster_flags=0, context=None, rasterize_mode="classic", absgrad=False,
           bilateral_grid=None):
    """Render the scene.  Background tensor (bg_color) must be on GPU!
    raster_flags / context are this package's additions to the reference's signature (kernel selection; the RasterContext
    holding this caller's hooks, capacities and caches -- None = the calling thread's default).
    rasterize_mode / absgrad: gsplat's options of the same names, handed to rasterization() (antialiased opacity
    compensation; `viewspace_points.absgrad` after backward(), which densify.accumulate(..., absgrad=True) reads).
    The camera model (N20) is read from the camera: `viewpoint_camera.camera_model` ("pinhole" when absent, "ortho", "fisheye"),
    and `viewpoint_camera.K` [3,3], when present, replaces the FoV-derived intrinsics; a non-pinhole camera must carry one.  `viewpoint_camera.radial_coeffs` (N21; None when
    absent): a fisheye camera's distortion coefficients (k1 .. k4), resident on the device next to K after the first render.
    A `K` or `radial_coeffs` that is a tensor requiring grad (N23; pose.IntrinsicsDelta.camera makes such cameras) is handed to
    rasterization() as it is -- float32, on the scene's device, [3,3] / [4], else ValueError -- and gets its gradient; no cache
    entry is made for such a camera.
    bilateral_grid (N24): a bilagrid.BilateralGrid; "render" is then the image corrected by grid `viewpoint_camera.uid` and
    "render_raw" the uncorrected view (gradients reach the scene through the transform and through the luminance that indexes
    it).  RGB renders only: feature_mode=True is a ValueError, another render_mode a NotImplementedError, before any launch."""
    if bilateral_grid is not None:
        if feature_mode:
            raise ValueError("render: a bilateral grid corrects colours; feature_mode=True renders features")
        if render_mode != "RGB":
            raise NotImplementedError(f"render: a bilateral grid is implemented for render_mode='RGB' only, not {render_mode!r}")
    rctx = context if context is not None else default_context()
    means3D = pc.get_xyz
    radial_coeffs = None
    if _trainable(getattr(viewpoint_camera, "K", None)) or _trainable(getattr(viewpoint_camera, "radial_coeffs", None)):
        K, radial_coeffs = _intrinsics_trainable(viewpoint_camera, means3D.device)  # (N23)
    elif getattr(viewpoint_camera, "radial_coeffs", None) is not None:
        K, radial_coeffs = _intrinsics_kb(viewpoint_camera, means3D.device, rctx.k_cache)
    else:
        K = _intrinsics(viewpoint_camera, means3D.device, rctx.k_cache)
    stored = _stored_parameters(pc)
    if stored is not None:
        rotations, scales, opacity = stored
    else:
        opacity = pc.get_opacity
        scales = pc.get_scaling * scaling_modifier
        rotations = pc.get_rotation
    if feature_mode:
        colors = pc.get_semantic_feature  # [N, D]
        sh_degree = None
        bg_color = bg_color[0].repeat(colors.shape[-1])
    elif override_color is not None:
        colors = override_color  # [N, 3]
        sh_degree = None
    else:
        colors = pc.get_features  # [N, K, 3]
        sh_degree = pc.active_sh_degree

    viewmat = viewpoint_camera.world_view_transform.transpose(0, 1)  # [4, 4]
    render_colors, render_alphas, info = rasterization(
        means=means3D, quats=rotations, scales=scales, opacities=opacity.squeeze(-1), colors=colors,
        viewmats=viewmat[None], Ks=K[None], backgrounds=bg_color[None],
        width=int(viewpoint_camera.image_width), height=int(viewpoint_camera.image_height),
        packed=False, sh_degree=sh_degree, render_mode=render_mode, raster_flags=raster_flags,
        raw_params=stored is not None, scaling_modifier=float(scaling_modifier), context=rctx,
        rasterize_mode=rasterize_mode, absgrad=absgrad, camera_model=camera_model_of(viewpoint_camera),
        radial_coeffs=radial_coeffs)

    # squeeze (not [0]): its backward is a view, [0]'s is a zero-fill + copy of the whole map
    rendered_image = render_colors.squeeze(0).permute(2, 0, 1)  # [1,H,W,D'] -> [D',H,W]
    radii = info["radii"].squeeze(0)  # [N,]
    try:
        info["means2d"].retain_grad()  # [1, N, 2]
    except Exception:
        pass
    pkg = {"render": rendered_image,
           "viewspace_points": info["means2d"],
           "visibility_filter": radii > 0,
           "radii": radii,
           "alphas": render_alphas[0, ..., 0],
           "info": info}
    if bilateral_grid is not None:
        pkg["render_raw"] = rendered_image
        pkg["render"] = bilateral_grid(rendered_image, int(viewpoint_camera.uid))  # [3,H,W] over [H,W,3] memory, like the raw view
    return pkg
