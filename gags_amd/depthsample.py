"""depth_SAM.py on the GPU (include/gags_next.h N6): the point-to-pixel min-depth mapping between the ED render and SAM's
depth-aware prompt grid in the reference's GAS stage (GAS.sh: render.py --render_mode RGB+ED, then depth_SAM.py).

For every Gaussian centre and training camera: project with the camera's world-to-camera matrix and K, round half to even,
keep the centres that land inside the image and agree with the rendered depth there (|d - zc| <= vis_thresh d), take each
Gaussian's minimum such rendered depth over all cameras, and write it back at the pixel of every camera that sees it.

    camera_rig(cameras)                               viewmats [C, 4, 4], Ks [C, 3, 3], model names [C], radial_coeffs, (H, W)
    camera_matrices(cameras)                          viewmats, Ks, (H, W) of a pinhole rig (refuses any other)
    point_pixel_mapping(xyz, viewmats, Ks, depths)    pcd_pxl_mapping [N, C, 2] int32 (v, u), pcd_pxl_mask [N, C] bool
    point_min_depth(xyz, viewmats, Ks, depths)        pcd_depth [N] (inf where no camera sees the point)
    depth_samples(xyz, viewmats, Ks, depths)          the <name>_depth_sample.npy maps [C, H, W]
    render_depths(gaussians, cameras, bg_color)       channel 3 of render(..., feature_mode=False, render_mode="RGB+ED")
    depth_sample_scene(gaussians, cameras, ...)       depth_SAM.main without the file I/O
    load_rendered_depths / save_depth_samples         <name>_depth.npy in, <name>_depth_sample.npy out, paired by name

Deviations from the reference, all deliberate: several visible Gaussians on one pixel -> the highest point index wins (the
reference's result under single-threaded torch; with threads its index_put_ keeps any of them); depth files are paired with
cameras by name (the reference pairs sorted file names with cameras sorted by image_name, which differ when one name is a
prefix of another); every camera and depth map must share one (H, W).

Camera models (N22; include/gags_next.h "N22" has the rule): the three functions of the mapping take camera_models= (one of
"pinhole", "ortho", "fisheye" per camera, mixed freely) and radial_coeffs= ([C, 4], the fisheyes' k1 .. k4), the scene
functions read both from the cameras through camera_rig.  Only where a centre lands depends on the model -- and a centre the
rasterizer culls by position (behind render()'s near plane, or past a fisheye's fold) is outside.  Every rig, the pinhole one
included, runs through gags_rig_depth_map / gags_rig_depth_scatter."""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr
from .gaussian_renderer import _intrinsics, camera_model_of, render


@torch.no_grad()
def camera_matrices(cameras, device="cuda"):
    """(viewmats [C, 4, 4] fp32 = world_view_transform.T, Ks [C, 3, 3] fp32 as render() forms them, (H, W)) for objects
    carrying FoVx, FoVy, image_width, image_height and world_view_transform.  Every camera must share one size."""
    cameras = list(cameras)
    if not cameras:
        raise ValueError("camera_matrices: no cameras")
    models = {getattr(c, "camera_model", "pinhole") for c in cameras} - {"pinhole"}
    if models:  # (its three values cannot carry a model: camera_rig is the general form, N22)
        raise NotImplementedError(f"camera_matrices: {sorted(models)} cameras; these are the matrices of pinhole cameras only "
                                  "(camera_rig returns the models and coefficients of any rig)")
    sizes = {(int(c.image_height), int(c.image_width)) for c in cameras}
    if len(sizes) != 1:
        raise ValueError(f"camera_matrices: the cameras differ in size {sorted(sizes)}; depth_SAM needs one (H, W)")
    viewmats = torch.stack([c.world_view_transform.transpose(0, 1).to(device, torch.float32) for c in cameras]).contiguous()
    Ks = torch.stack([_intrinsics(c, torch.device(device), {}).float() for c in cameras]).contiguous()
    return viewmats, Ks, sizes.pop()


@torch.no_grad()
def camera_rig(cameras, device="cuda"):
    """(viewmats [C, 4, 4] fp32 = world_view_transform.T, Ks [C, 3, 3] fp32, models [C] of "pinhole" | "ortho" | "fisheye",
    radial_coeffs [C, 4] fp32 or None, (H, W)) of cameras of any model, mixed freely (N22).  K is what render() uses: the
    camera's `K` attribute where it has one -- a non-pinhole camera must (ValueError otherwise, as in render()) -- else FoV-
    derived.  radial_coeffs: the `radial_coeffs` of the fisheye cameras that carry any, zero rows for the others; None when no
    camera carries any.  Every camera must share one size."""
    cameras = list(cameras)
    if not cameras:
        raise ValueError("camera_rig: no cameras")
    models = [camera_model_of(c) for c in cameras]
    for m in models:
        if not isinstance(m, str) or m not in _lib.CAMERA_MODELS:
            raise ValueError(f"camera_rig: unknown camera_model {m!r} (\"pinhole\", \"ortho\" or \"fisheye\")")
    sizes = {(int(c.image_height), int(c.image_width)) for c in cameras}
    if len(sizes) != 1:
        raise ValueError(f"camera_rig: the cameras differ in size {sorted(sizes)}; depth_SAM needs one (H, W)")
    rows = [getattr(c, "radial_coeffs", None) for c in cameras]
    coeffs = None
    if any(r is not None for r in rows):
        block = np.zeros((len(cameras), 4), np.float32)
        for k, (r, m) in enumerate(zip(rows, models)):
            if r is None:
                continue
            if m != "fisheye":
                raise ValueError(f"camera_rig: camera {k} is a {m!r} camera with radial_coeffs (a fisheye's coefficients)")
            block[k] = np.asarray(torch.as_tensor(r).detach().cpu(), np.float32).reshape(4)
        coeffs = torch.from_numpy(block).to(device)
    viewmats = torch.stack([c.world_view_transform.transpose(0, 1).to(device, torch.float32) for c in cameras]).contiguous()
    Ks = torch.stack([_intrinsics(c, torch.device(device), {}).float() for c in cameras]).contiguous()
    return viewmats, Ks, models, coeffs, sizes.pop()


def _rig(camera_models, radial_coeffs, depths):
    """(the host int32 array of model ids or None, radial_coeffs or None) for the C entries.  ValueError on plain values --
    names, lengths, shape and dtype -- before any tensor's device or content is looked at."""
    if camera_models is None:
        if radial_coeffs is not None:
            raise ValueError("radial_coeffs are the distortion coefficients of \"fisheye\" cameras: camera_models names none")
        return None, None
    if isinstance(camera_models, str):
        raise ValueError("camera_models: one model name per camera, not one string")
    names = list(camera_models)
    for m in names:
        if not isinstance(m, str) or m not in _lib.CAMERA_MODELS:
            raise ValueError(f"unknown camera model {m!r} (\"pinhole\", \"ortho\" or \"fisheye\")")
    c = depths.shape[0] if hasattr(depths, "shape") and len(depths.shape) == 3 else None
    if c is not None and len(names) != c:
        raise ValueError(f"camera_models names {len(names)} cameras, depths holds {c} maps")
    if radial_coeffs is not None:
        if "fisheye" not in names:
            raise ValueError("radial_coeffs are the distortion coefficients of \"fisheye\" cameras: camera_models names none")
        if not torch.is_tensor(radial_coeffs) or tuple(radial_coeffs.shape) != (len(names), 4) \
                or radial_coeffs.dtype != torch.float32:
            raise ValueError(f"radial_coeffs must be a float32 tensor [C, 4] with C = {len(names)} cameras")
    return (ctypes.c_int32 * len(names))(*[_lib.CAMERA_MODELS[m] for m in names]), radial_coeffs


def _args(xyz, viewmats, Ks, depths, cut_bound):
    _lib.on_gpu("depthsample", xyz, viewmats, Ks, depths)
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"xyz must be [N, 3], got {tuple(xyz.shape)}")
    if depths.dim() != 3:
        raise ValueError(f"depths must be [C, H, W], got {tuple(depths.shape)}")
    c = depths.shape[0]
    if c < 1 or depths.shape[1] < 1 or depths.shape[2] < 1:
        raise ValueError(f"depths must hold at least one non-empty map, got {tuple(depths.shape)}")
    if tuple(viewmats.shape) != (c, 4, 4) or tuple(Ks.shape) != (c, 3, 3):
        raise ValueError(f"viewmats {tuple(viewmats.shape)} and Ks {tuple(Ks.shape)} must be [C, 4, 4] and [C, 3, 3] "
                         f"with C = {c} depth maps")
    if int(cut_bound) < 0:
        raise ValueError("cut_bound must be >= 0")
    f = lambda t: t.float().contiguous()  # noqa: E731
    return f(xyz), f(viewmats), f(Ks), f(depths)


def _scratch(lib, n, c, h, w, device):
    nb = lib.gags_rig_depth_scratch_bytes(n, c, h, w)
    return _lib.scratch(nb, device), nb


def _coeffs(radial_coeffs):
    if radial_coeffs is None:
        return None
    _lib.on_gpu("depthsample", radial_coeffs)
    return radial_coeffs.contiguous()


def _map(xyz, viewmats, Ks, depths, vis_thresh, cut_bound, dense, camera_models=None, radial_coeffs=None):
    ids, radial_coeffs = _rig(camera_models, radial_coeffs, depths)
    xyz, viewmats, Ks, depths = _args(xyz, viewmats, Ks, depths, cut_bound)
    radial_coeffs = _coeffs(radial_coeffs)
    n, (c, h, w) = xyz.shape[0], depths.shape
    dev = xyz.device
    min_depth = torch.empty(n, device=dev)
    mapping = torch.empty(n, c, 2, dtype=torch.int32, device=dev) if dense else None
    visible = torch.empty(n, c, dtype=torch.uint8, device=dev) if dense else None
    lib = _lib.load()
    scratch, nb = _scratch(lib, n, c, h, w, dev)
    check(lib.gags_rig_depth_map(n, c, h, w, ptr(xyz), ptr(viewmats), ptr(Ks), ids, ptr(radial_coeffs), ptr(depths),
                                 float(vis_thresh), int(cut_bound), ptr(min_depth), ptr(mapping), ptr(visible), ptr(scratch), nb,
                                 _lib.stream()),
          "gags_rig_depth_map")
    return min_depth, mapping, visible


@torch.no_grad()
def point_pixel_mapping(xyz, viewmats, Ks, depths, vis_thresh=0.25, cut_bound=0, *, camera_models=None, radial_coeffs=None):
    """depth_SAM.py's pcd_pxl_mapping [N, C, 2] int32 (v, u) and pcd_pxl_mask [N, C] bool: (v, u) where camera c sees
    point i, (0, 0) and False elsewhere.  xyz [N, 3], viewmats [C, 4, 4], Ks [C, 3, 3], depths [C, H, W], all on the GPU.
    camera_models (N22): C names of "pinhole" | "ortho" | "fisheye", None = all pinhole; radial_coeffs: [C, 4] float32 on the
    GPU, the fisheyes' k1 .. k4 (rows of other cameras are not read), None = all zero."""
    _, mapping, visible = _map(xyz, viewmats, Ks, depths, vis_thresh, cut_bound, True, camera_models, radial_coeffs)
    return mapping, visible.bool()


@torch.no_grad()
def point_min_depth(xyz, viewmats, Ks, depths, vis_thresh=0.25, cut_bound=0, *, camera_models=None, radial_coeffs=None):
    """depth_SAM.py's pcd_depth [N] fp32: the minimum over the cameras that see point i of the rendered depth at its pixel
    (not the point's own depth), +inf where no camera sees it.  camera_models, radial_coeffs: see point_pixel_mapping."""
    return _map(xyz, viewmats, Ks, depths, vis_thresh, cut_bound, False, camera_models, radial_coeffs)[0]


@torch.no_grad()
def depth_samples(xyz, viewmats, Ks, depths, vis_thresh=0.25, cut_bound=0, return_min_depth=False, *, camera_models=None,
                  radial_coeffs=None):
    """save_pcd_depth's maps [C, H, W] fp32: at every pixel a visible point lands on, the min depth of the highest-index
    such point; 0 elsewhere.  With return_min_depth also point_min_depth's [N].  camera_models, radial_coeffs: see
    point_pixel_mapping."""
    min_depth, _, _ = _map(xyz, viewmats, Ks, depths, vis_thresh, cut_bound, False, camera_models, radial_coeffs)
    ids, radial_coeffs = _rig(camera_models, radial_coeffs, depths)
    xyz, viewmats, Ks, depths = _args(xyz, viewmats, Ks, depths, cut_bound)
    radial_coeffs = _coeffs(radial_coeffs)
    n, (c, h, w) = xyz.shape[0], depths.shape
    samples = torch.empty(c, h, w, device=xyz.device)
    lib = _lib.load()
    scratch, nb = _scratch(lib, n, c, h, w, xyz.device)
    check(lib.gags_rig_depth_scatter(n, c, h, w, ptr(xyz), ptr(viewmats), ptr(Ks), ids, ptr(radial_coeffs), ptr(depths),
                                     float(vis_thresh), int(cut_bound), ptr(min_depth), ptr(samples), ptr(scratch), nb,
                                     _lib.stream()),
          "gags_rig_depth_scatter")
    return (samples, min_depth) if return_min_depth else samples


@torch.no_grad()
def render_depths(gaussians, cameras, bg_color):
    """[C, H, W]: channel 3 of render(cam, gaussians, None, bg_color, feature_mode=False, render_mode="RGB+ED")["render"]
    per camera (what render.py saves as <image_name>_depth.npy, render.py:118-133); camera-space z under every camera model."""
    cameras = list(cameras)
    _, _, _, _, (h, w) = camera_rig(cameras, device=gaussians.get_xyz.device)
    out = torch.empty(len(cameras), h, w, device=gaussians.get_xyz.device)
    for c, cam in enumerate(cameras):
        out[c] = render(cam, gaussians, None, bg_color, feature_mode=False, render_mode="RGB+ED")["render"][3]
    return out


def _names(cameras, names):
    if names is None:
        names = [getattr(cam, "image_name", None) for cam in cameras]
        if any(nm is None for nm in names):
            names = [f"{i:05d}" for i in range(len(cameras))]
    names = [str(nm) for nm in names]
    if len(names) != len(cameras) or len(set(names)) != len(names):
        raise ValueError("names: one distinct name per camera")
    return names


@torch.no_grad()
def depth_sample_scene(gaussians, cameras, depths=None, names=None, bg_color=None, vis_thresh=0.25, cut_bound=0,
                       return_mapping=False):
    """depth_SAM.py:main without the file I/O: the ED depth of every camera (rendered here when `depths` [C, H, W] is not
    given, on bg_color, default black), then the min depths and the sample maps.  Returns a dict: names, depths,
    samples [C, H, W], min_depth [N]; with return_mapping also mapping [N, C, 2] and visible [N, C].  The cameras may be of
    any model (N22: camera_rig); an all-pinhole scene runs as it always has."""
    cameras = list(cameras)
    names = _names(cameras, names)
    xyz = gaussians.get_xyz
    viewmats, Ks, models, coeffs, (h, w) = camera_rig(cameras, device=xyz.device)
    rig = {} if all(m == "pinhole" for m in models) else {"camera_models": models, "radial_coeffs": coeffs}
    if depths is None:
        bg = bg_color if bg_color is not None else torch.zeros(3, device=xyz.device)
        depths = render_depths(gaussians, cameras, bg)
    elif tuple(depths.shape) != (len(cameras), h, w):
        raise ValueError(f"depths {tuple(depths.shape)} do not match {len(cameras)} cameras of {h} x {w}")
    samples, min_depth = depth_samples(xyz, viewmats, Ks, depths, vis_thresh, cut_bound, return_min_depth=True, **rig)
    res = {"names": names, "depths": depths, "samples": samples, "min_depth": min_depth}
    if return_mapping:
        res["mapping"], res["visible"] = point_pixel_mapping(xyz, viewmats, Ks, depths, vis_thresh, cut_bound, **rig)
    return res


def load_rendered_depths(directory, names, device="cuda"):
    """[C, H, W] fp32 from <directory>/<name>_depth.npy for every name, in the order of `names` (paired by name, not by the
    sorted file list).  Every map must have one size."""
    maps = []
    for nm in names:
        p = os.path.join(directory, f"{nm}_depth.npy")
        if not os.path.exists(p):
            raise FileNotFoundError(f"no rendered depth for camera {nm!r}: {p}")
        maps.append(np.load(p))
    sizes = {m.shape for m in maps}
    if len(sizes) != 1 or len(next(iter(sizes))) != 2:
        raise ValueError(f"{directory}: depth maps must all be [H, W] of one size, got {sorted(sizes)}")
    return torch.from_numpy(np.stack(maps).astype(np.float32, copy=False)).to(device)


def save_depth_samples(directory, names, samples, min_depth=None, visible=None, mapping=None):
    """<directory>/<name>_depth_sample.npy ([H, W] float32, save_pcd_depth's files) for every camera; optionally also
    pcd_depth.npy, pcd_pxl_mask.npy and pcd_pxl_mapping.npy (the outputs save_pcd_depth has commented out).  Returns the
    paths written."""
    if len(names) != samples.shape[0]:
        raise ValueError(f"{len(names)} names for {samples.shape[0]} sample maps")
    os.makedirs(directory, exist_ok=True)
    s = samples.detach().float().cpu().numpy()
    paths = []
    for nm, m in zip(names, s):
        paths.append(os.path.join(directory, f"{nm}_depth_sample.npy"))
        np.save(paths[-1], m)
    for fname, t in (("pcd_depth.npy", min_depth), ("pcd_pxl_mask.npy", visible), ("pcd_pxl_mapping.npy", mapping)):
        if t is not None:
            paths.append(os.path.join(directory, fname))
            np.save(paths[-1], t.detach().cpu().numpy())
    return paths
