"""Offline feature render on the GPU (include/gags_next.h N11): what render.py --feature_mode does with a trained scene
(:33-66, :147-175) -- the PCA-coloured decoded feature map, the four PCA-coloured ground-truth maps (mixed, s, m, l; the
max mode of read_sam_clip_feature) and the scale-map images -- without the host copy of [H W / 3, C] floats and the host
PCA fit of feature_visualize_saving.

    feature_moments(feature)               (sum [C], gram [C, C]) float64 of the normalised rows of every third pixel
    feature_pca_basis(feature)             (mean [C], components [3, C], q1, q99)
    feature_project(feature, mean, comps)  t [H W, 3]
    order_statistics(values, ranks)        exact k-th smallest values, no sort
    percentiles(values, qs)                numpy's default (linear) percentiles from them
    feature_colour(t, q1, q99, H, W)       clamp((t - q1) / (q99 - q1), 0, 1) as [H, W, 3]
    feature_visualize(feature, basis=None, return_uint8=False)     [H, W, 3] on the device
    feature_visualize_saving / scale_visualize_saving / process_scale_map / process_feature_map   render.py's functions
    render_feature_view(...) / save_feature_view(...)              one view of render.py:148-175, and its PNG files

A map is [C, H, W] float32, channel-major contiguous (the ground-truth assembly) or a permuted view of [H, W, C] memory (the
decoders); both are read in place.  C % 16 == 0, 16 <= C <= 1024.  GPU tensors only: there is no CPU path.

The fit is sklearn >= 1.5's for these shapes (solver covariance_eigh, svd_flip(u_based_decision=False)): mean = sum / S,
cov = (gram - S mean mean^T) / (S - 1) in float64 on the host (ONE C x C readback per map: an offline path), the eigenvectors
of the three largest eigenvalues in descending order, each signed so that its entry of largest magnitude is positive.
Deliberately not here: matplotlib depth PNGs, the feature_npy dump, the argparse front end, median_mode."""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr
from .losses import _pixel_major, read_sam_clip_feature


def row_chunk():
    """Sampled pixels one workgroup of the moments kernel reduces; more are split across workgroups."""
    return int(_lib.load().gags_featvis_row_chunk())


def _map(feature):
    """(tensor whose memory the kernels read, layout, C, H, W)."""
    _lib.on_gpu("featurevis", feature)
    if feature.dim() != 3:
        raise ValueError(f"feature must be [C, H, W], got {tuple(feature.shape)}")
    C, H, W = feature.shape
    if C % 16 or not 16 <= C <= 1024:
        raise ValueError(f"feature width must be a multiple of 16 in [16, 1024], got {C}")
    if H * W < 1:
        raise ValueError(f"feature must have at least one pixel, got {tuple(feature.shape)}")
    if _pixel_major(feature):
        return feature, 1, C, H, W
    x = feature if (feature.is_contiguous() and feature.dtype == torch.float32) else feature.contiguous().float()
    return x, 0, C, H, W


def _samples(P):
    return (P + 2) // 3


@torch.no_grad()
def feature_moments(feature):
    """(sum [C], gram [C, C]) float64 on the device: sums of x^ and x^ x^T over the pixels p = y W + x with p % 3 == 0,
    x^ = x / max(||x||, 1e-12).  Two runs give the same bits."""
    x, layout, C, H, W = _map(feature)
    P = H * W
    if _samples(P) < 4:
        raise ValueError(f"feature_moments: {P} pixels give {_samples(P)} samples; at least 4 are needed")
    lib = _lib.load()
    s = torch.empty(C, dtype=torch.float64, device=x.device)
    g = torch.empty(C, C, dtype=torch.float64, device=x.device)
    nb = lib.gags_featvis_moments_scratch_bytes(C, P)
    scratch = _lib.scratch(nb, x.device)
    check(lib.gags_featvis_moments(C, P, ptr(x), layout, ptr(s), ptr(g), ptr(scratch), nb, _lib.stream()), "gags_featvis_moments")
    return s, g


def pca_from_moments(s, g, S):
    """(mean [C], components [3, C]) float64 CPU tensors from the moments of S samples."""
    s, g = s.detach().to("cpu", torch.float64), g.detach().to("cpu", torch.float64)
    mean = s / S
    cov = (g - S * torch.outer(mean, mean)) / (S - 1)
    _, vec = torch.linalg.eigh(cov)                      # ascending eigenvalues, eigenvectors in columns
    comps = vec[:, -3:].flip(1).t().contiguous()         # the three largest, descending, as rows
    big = comps.abs().argmax(dim=1)
    sign = torch.sign(comps[torch.arange(3), big])
    sign[sign == 0] = 1
    return mean, comps * sign[:, None]


@torch.no_grad()
def feature_project(feature, mean, components):
    """t [H W, 3] float32: t[p, k] = sum_c (x^[c] - mean[c]) components[k, c] for every pixel."""
    x, layout, C, H, W = _map(feature)
    mean = mean.to(x.device, torch.float32).contiguous()
    components = components.to(x.device, torch.float32).contiguous()
    if tuple(mean.shape) != (C,) or tuple(components.shape) != (3, C):
        raise ValueError(f"mean {tuple(mean.shape)} / components {tuple(components.shape)} do not fit {C} channels")
    t = torch.empty(H * W, 3, device=x.device)
    check(_lib.load().gags_featvis_project(C, H * W, ptr(x), layout, ptr(mean), ptr(components), ptr(t), _lib.stream()),
          "gags_featvis_project")
    return t


@torch.no_grad()
def order_statistics(values, ranks, group=1, stride=1, n=None):
    """float32 tensor [len(ranks)] on the device: the ranks[j]-th smallest (0-based) of the pooled values, exactly.  The pool is
    element i = values.flatten()[(i // group) * stride + i % group] for i < n (default: the whole tensor)."""
    _lib.on_gpu("featurevis", values)
    v = values if (values.is_contiguous() and values.dtype == torch.float32) else values.contiguous().float()
    n = v.numel() if n is None else int(n)
    ranks = [int(k) for k in ranks]
    if n < 1 or (n - 1) // group * stride + (n - 1) % group >= v.numel():
        raise ValueError(f"order_statistics: a pool of {n} values (group {group}, stride {stride}) does not fit {v.numel()} floats")
    if not 1 <= len(ranks) <= 8 or any(not 0 <= k < n for k in ranks):
        raise ValueError(f"order_statistics: 1 to 8 ranks in [0, {n}), got {ranks}")
    lib = _lib.load()
    out = torch.empty(len(ranks), device=v.device)
    nb = lib.gags_featvis_select_scratch_bytes(len(ranks))
    scratch = _lib.scratch(nb, v.device)
    karr = (ctypes.c_int64 * len(ranks))(*ranks)
    check(lib.gags_featvis_select(n, ptr(v), int(group), int(stride), len(ranks), karr, ptr(out), ptr(scratch), nb, _lib.stream()),
          "gags_featvis_select")
    return out


def percentile_ranks(n, qs):
    """numpy's default ("linear") percentile of n values: for every q the two neighbouring ranks and the weight of the upper
    one.  The position q / 100 (n - 1) is a float64, as np.percentile(float32 array, [q...]) evaluates it."""
    quant = np.true_divide(np.asanyarray(list(qs)), np.float32(100))
    virtual = (n - 1) * quant
    prev = np.floor(virtual)
    gamma = virtual - prev
    prev = prev.astype(np.int64)
    nxt = np.minimum(prev + 1, n - 1)
    return prev, nxt, gamma


def lerp_percentiles(lo, hi, gamma):
    """numpy's _lerp on float32 neighbours and float64 weights: float64 results."""
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    diff = hi - lo
    out = lo + diff * gamma
    return np.where(gamma >= 0.5, hi - diff * (1 - gamma), out)


@torch.no_grad()
def percentiles(values, qs=(1, 99), group=1, stride=1, n=None):
    """np.percentile(pool, qs) (float64 array) of the pooled float32 values: exact order statistics from the device, numpy's
    interpolation on the host.  One readback of 2 len(qs) floats."""
    n = values.numel() if n is None else int(n)
    prev, nxt, gamma = percentile_ranks(n, qs)
    stats = order_statistics(values, list(prev) + list(nxt), group, stride, n).cpu().numpy()
    return lerp_percentiles(stats[:len(prev)], stats[len(prev):], gamma)


def _fit(feature):
    """((mean, components, q1, q99), t): the basis of a map and the projection it was fitted on."""
    x, layout, C, H, W = _map(feature)
    P = H * W
    S = _samples(P)
    s, g = feature_moments(feature)
    mean, comps = pca_from_moments(s, g, S)
    mean, comps = mean.to(x.device, torch.float32), comps.to(x.device, torch.float32)
    t = feature_project(feature, mean, comps)
    q1, q99 = percentiles(t, (1, 99), group=3, stride=9, n=3 * S)   # the sampled rows of t: every third
    return (mean, comps, float(q1), float(q99)), t


@torch.no_grad()
def feature_pca_basis(feature):
    """(mean [C], components [3, C], q1, q99) of render.py:36-43: the 3-component PCA of the normalised rows of every third
    pixel, and the pooled 1 % / 99 % percentiles of those rows' projections (Python floats)."""
    return _fit(feature)[0]


@torch.no_grad()
def feature_visualize(feature, basis=None, return_uint8=False):
    """render.py:33-48 on the device: [H, W, 3] float32 in [0, 1]; with return_uint8 also trunc(255 vis) as uint8
    (render.py:166's astype).  basis = a feature_pca_basis() result colours this map in another map's basis."""
    x, layout, C, H, W = _map(feature)
    if basis is None:
        (mean, comps, q1, q99), t = _fit(feature)
    else:
        mean, comps, q1, q99 = basis
        t = feature_project(feature, mean, comps)
    return feature_colour(t, q1, q99, H, W, return_uint8)


@torch.no_grad()
def feature_colour(t, q1, q99, H, W, return_uint8=False):
    """vis [H, W, 3] float32 = clamp((t - q1) / (q99 - q1), 0, 1) from t [H W, 3]; with return_uint8 (vis, trunc(255 vis))."""
    if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != 3 * H * W:
        raise ValueError(f"feature_colour: t must be a contiguous float32 GPU tensor of {H * W} x 3 values")
    vis = torch.empty(H, W, 3, device=t.device)
    u8 = torch.empty(H, W, 3, dtype=torch.uint8, device=t.device) if return_uint8 else None
    sub, div = float(np.float32(q1)), float(np.float32(np.float64(q99) - np.float64(q1)))
    check(_lib.load().gags_featvis_colour(3 * H * W, ptr(t), sub, div, ptr(vis), ptr(u8), _lib.stream()), "gags_featvis_colour")
    return (vis, u8) if return_uint8 else vis


def feature_visualize_saving(feature):
    """render.py:33-48 with the reference's name and return value: an [H, W, 3] CPU float tensor."""
    return feature_visualize(feature).cpu()


def scale_visualize_saving(scale_map):
    """render.py:50-53: the arg-max level over 2 (0, 0.5, 1), [H, W]."""
    return torch.argmax(scale_map, dim=0) / 2


def process_scale_map(scale_map):
    """render.py:55-59: the three one-level scale maps."""
    scale_maps = [torch.zeros_like(scale_map) for _ in range(3)]
    for i, sm in enumerate(scale_maps):
        sm[i] = 1
    return scale_maps


@torch.no_grad()
def process_feature_map(view, scale_map):
    """render.py:61-66: the ground-truth maps of the levels s, m, l alone."""
    img_embed, seg_map = view.img_embed.to(scale_map.device), view.seg_map.to(scale_map.device)
    gt_feature_maps = []
    for sm in process_scale_map(scale_map):
        gt_feature_map, mask = read_sam_clip_feature(img_embed, seg_map, sm, max_mode=True)
        gt_feature_maps.append(gt_feature_map.mul_(mask))
    return gt_feature_maps


@torch.no_grad()
def render_feature_view(view, gaussians, pipe, bg, cnn_decoder, cnn_scale_decoder, speedup=True):
    """One view of render.py:148-175 as a dict of device tensors:
        scale_map [3, H, W] float, scale_class [H, W] float,
        feature_vis, gt_feature_vis, gt_feature_vis_s, gt_feature_vis_m, gt_feature_vis_l   [H, W, 3] uint8."""
    from .gaussian_renderer import render
    feature_map = render(view, gaussians, pipe, bg, feature_mode=True)["render"].detach()
    scale_map = cnn_scale_decoder(feature_map)
    images = {"scale_map": scale_map, "scale_class": scale_visualize_saving(scale_map)}
    gt_feature_map, mask = read_sam_clip_feature(view.img_embed.to(scale_map.device), view.seg_map.to(scale_map.device),
                                                 scale_map, max_mode=True)
    gt_feature_map.mul_(mask)
    gt_s, gt_m, gt_l = process_feature_map(view, scale_map)
    if speedup:
        feature_map = cnn_decoder(feature_map)
    for key, fmap in (("feature_vis", feature_map), ("gt_feature_vis", gt_feature_map), ("gt_feature_vis_s", gt_s),
                      ("gt_feature_vis_m", gt_m), ("gt_feature_vis_l", gt_l)):
        images[key] = feature_visualize(fmap, return_uint8=True)[1]
    return images


def _save_image(t, path):
    """torchvision.utils.save_image of one image: x 255 + 0.5, clamped to 0..255, as uint8; a 2-D map becomes three equal
    channels."""
    from PIL import Image
    t = t.detach().float()
    if t.dim() == 2:
        t = t[None].expand(3, -1, -1)
    arr = t.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8).numpy()
    Image.fromarray(arr).save(path)


def save_feature_view(model_path, name, iteration, idx, images):
    """Write render_feature_view's images under the reference's folder and file names (render.py:79-81,150-175); returns
    {key: path}."""
    from PIL import Image
    root = os.path.join(model_path, name, "ours_{}".format(iteration))
    stem = "{0:05d}".format(idx)
    where = {"scale_map": ("scale_map", stem + ".png"), "scale_class": ("scale_map", stem + "_class.png"),
             "feature_vis": ("feature_map", stem + "_feature_vis.png"),
             "gt_feature_vis": ("gt_feature_map", stem + "_feature_vis.png"),
             "gt_feature_vis_s": ("gt_feature_map", stem + "_feature_vis_s.png"),
             "gt_feature_vis_m": ("gt_feature_map", stem + "_feature_vis_m.png"),
             "gt_feature_vis_l": ("gt_feature_map", stem + "_feature_vis_l.png")}
    paths = {}
    for key, (folder, fname) in where.items():
        os.makedirs(os.path.join(root, folder), exist_ok=True)
        paths[key] = os.path.join(root, folder, fname)
        img = images[key]
        if img.dtype == torch.uint8:
            Image.fromarray(img.cpu().numpy()).save(paths[key])
        else:
            _save_image(img, paths[key])
    return paths
