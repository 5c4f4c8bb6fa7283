"""SAM's prompt grids (include/gags_next.h N13): the step between the depth samples of gags_amd.depthsample (N6) and SAM in
the reference's GAS stage -- preprocess.py:114-184 (build_depth_point_grid, project_from_sampled_pcd, sample_from_pcd) and
utils/SAM_utils.py:189-242, 294-366 (build_point_grid, generate_crop_boxes, sample_based_mapping,
build_mindepth_point_grid), called once per image by preprocess.py:create.  The step holds no model: per image it is 64 crop
means, 64 masked means and 6400 counts over sub-crops, then a few thousand draws of Python's `random`.

GPU (one segmented-reduction kernel over [C, H, W] for all cameras, csrc/promptgrid.hip; there is no CPU path):
    crop_stats(depths, samples=None, n_per_side=8)   depth_sum / depth_count [C, n^2], sample_sum / sample_count [C, n^2],
                                                     sub_count [C, n^2, 100]
    depth_point_grids(depths, ...)                   build_all_layer_depth_point_grids for every camera
    mindepth_point_grids(depths, samples, ...)       build_all_layer_mindepth_point_grids for every camera
    sample_from_pcd / project_from_sampled_pcd       the candidate set and the selection run on the device with torch
    prompt_scene(gaussians, cameras, mode, ...)      depthsample.depth_sample_scene chained into the builders

Host (numpy float64 and Python's random, the reference's arithmetic and the reference's order of draws):
    crop_layout(h, w, n_per_side)                    the integer start tables and the crop boxes
    build_point_grid / build_all_layer_point_grids / generate_crop_boxes      SAM_utils.py:189-242
    depth_grids_from_stats(stats, layout)            the lattice of preprocess.py:133-139 from the crop means
    mindepth_grids_from_stats(stats, layout, ...)    the weighted draws of sample_based_mapping from the sub-crop counts
    stats_to_host(stats)                             the statistics as numpy arrays, in one device -> host copy
    save_prompt_grids / load_prompt_grids            <dir>/<name>_prompts.npz, one array per layer (this project's format: the
                                                     reference keeps the grids in memory and hands them to SAM in-process)

The random draws stay on the host on purpose: with random.seed(s) beforehand and `rng` left at its default the stream of
rng.choices / rng.randint calls is the reference's for the same images in the same order (cameras outer, layers inner, crops
in order; per crop one choices() over the 100 sub-crops, then randint(x), randint(y) per draw), so a seeded run gives the
reference's points.  The crop means are float32(float64 sum / count); the reference's are torch's fp32 means, about 1e-5
away, which decides the same sample_num unless a mean (or ratio x nsample) sits that close to an integer.

Two behaviours of the reference worth knowing:
  * sample_from_pcd's sorted(set(...)) does NOT remove duplicates: the elements are 0-d tensors, which hash by identity, so
    k draws give k sorted indices.  Deviation switch: unique=False (default) keeps the duplicates as the reference does,
    unique=True removes them (what the code reads as).
  * N6's min depth is +inf for a point no camera sees.  Such points are never candidates here (the candidate set is the
    rows of `visible` with any camera), so no infinite weight is formed.
Crops leave gaps when W % n != 0, the last row and column of a crop belong to no sub-crop, and neighbouring sub-crops may
share a pixel: all three are the reference's geometry and are kept."""
import math
import os
import random
from itertools import product

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr

SUB = 10  # sample_based_mapping's crop_num
MODES = ("grid", "depth", "mindepth", "pcd")
PCD_FRACTION = 0.02  # preprocess.py:200


# ---- host: geometry -------------------------------------------------------------------------------------------------------------

def crop_layout(h, w, n_per_side):
    """The integer geometry of build_depth_point_grid / sample_based_mapping for an h x w image, in float64 as numpy does:
    x0, y0 [n] int32 crop starts, crop_w, crop_h, sx, sy [10] int32 sub-crop starts inside a crop, and boxes [n^2, 4]
    float64 = [x0 / w, y0 / h, (x0 + crop_w) / w, (y0 + crop_h) / h] in crop order (k = ix n + iy)."""
    h, w, n = int(h), int(w), int(n_per_side)
    if h < 1 or w < 1 or n < 1:
        raise ValueError(f"crop_layout: h, w and n_per_side must be >= 1, got {h}, {w}, {n}")
    x0 = np.linspace(0, w - 1, n + 1)[:-1].astype(np.int32)
    crop_w = int(w / len(x0))
    y0 = np.linspace(0, h - 1, n + 1)[:-1].astype(np.int32)
    crop_h = int(h / len(y0))
    # x0[n - 1] + crop_w <= (w - 1)(n - 1) / n + w / n < w + 1: no crop is cut by the image, every crop is (crop_h, crop_w)
    assert int(x0[-1]) + crop_w <= w and int(y0[-1]) + crop_h <= h
    sx = np.linspace(0, crop_w - 1, SUB + 1)[:-1].astype(np.int32)
    sy = np.linspace(0, crop_h - 1, SUB + 1)[:-1].astype(np.int32)
    boxes = np.stack([np.array([a / w, b / h, (a + crop_w) / w, (b + crop_h) / h]) for a, b in product(x0, y0)], axis=0)
    return {"h": h, "w": w, "n": n, "x0": x0, "y0": y0, "crop_w": crop_w, "crop_h": crop_h, "sx": sx, "sy": sy, "boxes": boxes}


def build_point_grid(n_per_side):
    """SAM_utils.py:189-196: an n x n lattice of cell centres in [0, 1]^2, x fastest, [n^2, 2] float64."""
    half = 1 / (2 * n_per_side)
    ticks = np.linspace(half, 1 - half, n_per_side)
    gx, gy = np.meshgrid(ticks, ticks)  # gx varies along a row: x fastest
    return np.stack([gx, gy], axis=-1).reshape(-1, 2)


def _layer_sides(n_per_side, n_layers, scale_per_layer):
    if int(n_layers) < 0:
        raise ValueError("n_layers must be >= 0")
    return [int(n_per_side / (scale_per_layer ** i)) for i in range(int(n_layers) + 1)]


def build_all_layer_point_grids(n_per_side, n_layers, scale_per_layer):
    """SAM_utils.py:198-206: build_point_grid(int(n_per_side / scale_per_layer^i)) for i = 0 .. n_layers."""
    return [build_point_grid(n) for n in _layer_sides(n_per_side, n_layers, scale_per_layer)]


def generate_crop_boxes(im_size, n_layers, overlap_ratio):
    """SAM_utils.py:208-242: (boxes, layer of each box).  Layer 0 is the whole image; layer i >= 1 cuts it into 2^i x 2^i
    boxes [x0, y0, x1, y1] (x outer) that share int(overlap_ratio * short side * 2 / 2^i) pixels with their neighbours."""
    height, width = im_size
    boxes, layers = [[0, 0, width, height]], [0]
    for layer in range(1, n_layers + 1):
        per_side = 2 ** layer
        shared = int(overlap_ratio * min(height, width) * (2 / per_side))
        side_w = int(math.ceil((shared * (per_side - 1) + width) / per_side))
        side_h = int(math.ceil((shared * (per_side - 1) + height) / per_side))
        starts_x = [int((side_w - shared) * i) for i in range(per_side)]
        starts_y = [int((side_h - shared) * i) for i in range(per_side)]
        boxes += [[x, y, min(x + side_w, width), min(y + side_h, height)] for x in starts_x for y in starts_y]
        layers += [layer] * (per_side * per_side)
    return boxes, layers


# ---- GPU: the crop statistics ---------------------------------------------------------------------------------------------------

def _maps(depths, samples):
    _lib.on_gpu("prompts", depths, *(() if samples is None else (samples,)))
    if depths.dim() != 3 or min(depths.shape) < 1:
        raise ValueError(f"depths must be a non-empty [C, H, W], got {tuple(depths.shape)}")
    if samples is not None and samples.shape != depths.shape:
        raise ValueError(f"samples {tuple(samples.shape)} do not match depths {tuple(depths.shape)}")
    f = lambda t: None if t is None else t.float().contiguous()  # noqa: E731
    return f(depths), f(samples)


@torch.no_grad()
def crop_stats(depths, samples=None, n_per_side=8, layout=None):
    """The kernel's outputs for depths [C, H, W] (and samples [C, H, W]) on the GPU, as device tensors: depth_sum float64 and
    depth_count int32 [C, n^2]; with samples also sample_sum float64 / sample_count int32 [C, n^2] over the samples != 0
    (NaN and negative values count) and sub_count int32 [C, n^2, 100].  Inputs of another dtype or layout are converted to
    contiguous float32 first.  Crop k = ix n + iy; sub-crop i = jy 10 + jx."""
    depths, samples = _maps(depths, samples)
    c, h, w = depths.shape
    L = crop_layout(h, w, n_per_side) if layout is None else layout
    if (L["h"], L["w"]) != (h, w):
        raise ValueError(f"layout is for {L['h']} x {L['w']}, the maps are {h} x {w}")
    n, dev = L["n"], depths.device
    tab = torch.from_numpy(np.concatenate([L["x0"], L["y0"], L["sx"], L["sy"]]).astype(np.int32)).to(dev)
    out = {"depth_sum": torch.empty(c, n * n, dtype=torch.float64, device=dev),
           "depth_count": torch.empty(c, n * n, dtype=torch.int32, device=dev)}
    if samples is not None:
        out["sample_sum"] = torch.empty(c, n * n, dtype=torch.float64, device=dev)
        out["sample_count"] = torch.empty(c, n * n, dtype=torch.int32, device=dev)
        out["sub_count"] = torch.empty(c, n * n, SUB * SUB, dtype=torch.int32, device=dev)
    lib = _lib.load()
    nb = lib.gags_promptgrid_scratch_bytes(c, h, w, n, L["crop_h"])
    scratch = _lib.scratch(nb, dev)
    check(lib.gags_promptgrid_stats(c, h, w, n, L["crop_w"], L["crop_h"], ptr(depths), ptr(samples), ptr(tab),
                                    ptr(out["depth_sum"]), ptr(out["depth_count"]), ptr(out.get("sample_sum")),
                                    ptr(out.get("sample_count")), ptr(out.get("sub_count")), ptr(scratch), nb, _lib.stream()),
          "gags_promptgrid_stats")
    return out


# ---- host: the builders ---------------------------------------------------------------------------------------------------------

def stats_to_host(stats):
    """crop_stats' output as numpy arrays (host arrays pass through).  Device tensors travel in ONE device -> host copy: their bytes are concatenated on the
    device and cut apart again on the host."""
    dev = {k: v.detach().contiguous() for k, v in stats.items() if torch.is_tensor(v) and v.is_cuda}
    out = {k: (v.detach().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in stats.items() if k not in dev}
    if dev:
        flat = torch.cat([v.view(-1).view(torch.uint8) for v in dev.values()]).cpu().numpy()
        o = 0
        for k, v in dev.items():
            nb = v.numel() * v.element_size()
            out[k] = flat[o:o + nb].view(torch.empty(0, dtype=v.dtype).numpy().dtype).reshape(tuple(v.shape)).copy()
            o += nb
    return {k: out[k] for k in stats}


def _mean32(total, count):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.float32(np.float64(total) / np.float64(count))


def _depth_camera(stats, layout, c):
    """build_depth_point_grid for camera c of host statistics: (points [P, 2], boxes [n^2, 4]) float64."""
    h, w, crop_w, crop_h = layout["h"], layout["w"], layout["crop_w"], layout["crop_h"]
    lattices = []
    for k, (x0, y0) in enumerate(product(layout["x0"], layout["y0"])):
        mean_depth = _mean32(stats["depth_sum"][c, k], stats["depth_count"][c, k])
        if not np.isfinite(mean_depth):
            raise ValueError(f"camera {c}, crop {k}: the mean depth is {mean_depth}; no sample count can be formed from it")
        num = max(1, min(int(mean_depth), 20))
        # num x num cell centres of the crop: half a cell in from each side (the reference's expressions: the bits are pinned)
        half_x, half_y = crop_w / (2 * num), crop_h / (2 * num)
        xs = np.linspace(x0 + half_x, x0 + crop_w - half_x, num)
        ys = np.linspace(y0 + half_y, y0 + crop_h - half_y, num)
        gx, gy = np.meshgrid(xs, ys)  # x fastest
        lattices.append(np.stack([gx, gy], axis=-1).reshape(-1, 2))
    return np.concatenate(lattices, axis=0) / np.array([[w, h]]), layout["boxes"].copy()


def _mindepth_camera(stats, layout, c, nsample_min_distance, rng):
    """build_mindepth_point_grid for camera c of host statistics, drawing from rng in the reference's order."""
    h, w, crop_w, crop_h = layout["h"], layout["w"], layout["crop_w"], layout["crop_h"]
    # the inclusive pixel range randint draws from, per sub-crop column and row
    range_x = [(lo, min(crop_w - 1, lo + crop_w // SUB)) for lo in layout["sx"]]
    range_y = [(lo, min(crop_h - 1, lo + crop_h // SUB)) for lo in layout["sy"]]
    pixels = []
    for k, (x0, y0) in enumerate(product(layout["x0"], layout["y0"])):
        mean_depth = _mean32(stats["depth_sum"][c, k], stats["depth_count"][c, k])
        mean_sample = _mean32(stats["sample_sum"][c, k], stats["sample_count"][c, k])
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.float32(mean_depth) / np.float32(mean_sample)
            if r < 1 or np.isnan(r):
                num = 1
            else:
                scaled = np.float32(r * np.float32(nsample_min_distance))
                if not np.isfinite(scaled):  # samples that cancel to a zero mean: the reference's int(inf) raises as well
                    raise ValueError(f"camera {c}, crop {k}: mean depth / mean sample depth is {r}; no sample count can be "
                                     "formed from it")
                num = int(scaled)
        num = max(1, min(num, 20))
        counts = stats["sub_count"][c, k].astype(np.int64)
        if not counts.any():  # no sample in any sub-crop: uniform
            counts = np.ones(SUB * SUB, np.int64)
        for sub in rng.choices(range(SUB * SUB), counts / np.sum(counts), k=num * num):
            px = rng.randint(*range_x[sub % SUB])
            py = rng.randint(*range_y[sub // SUB])
            pixels.append((x0 + px, y0 + py))
    return np.array(pixels, np.int64) / np.array([[w, h]]), layout["boxes"].copy()


def _n_cams(stats):
    return int(np.shape(stats["depth_sum"])[0])


def depth_grids_from_stats(stats, layout):
    """build_depth_point_grid (preprocess.py:114-149) for every camera of crop_stats' output: per crop
    sample_num = clamp(int(mean_depth), 1, 20) with mean_depth = float32(depth_sum / depth_count), the sample_num x sample_num
    linspace lattice inside the crop (x fastest), divided by (W, H).  Returns [(points [P, 2], boxes [n^2, 4])] per camera,
    float64.  A non-finite mean raises ValueError naming the camera and the crop (the reference's int() raises there too)."""
    stats = stats_to_host(stats)
    return [_depth_camera(stats, layout, c) for c in range(_n_cams(stats))]


def mindepth_grids_from_stats(stats, layout, nsample_min_distance=4, rng=random):
    """build_mindepth_point_grid + sample_based_mapping (SAM_utils.py:294-353) for every camera of crop_stats' output, cameras
    in the order given: per crop r = float32(mean_depth) / float32(mean_sample), sample_num = 1 when r < 1 or NaN, else
    int(r * nsample_min_distance) in float32, clamped to [1, 20]; one rng.choices over the 100 sub-crops weighted by their
    non-zero counts (uniform when all are zero), then rng.randint(x) and rng.randint(y) inside the drawn sub-crop per draw.
    An infinite r (non-zero samples whose mean is 0) raises ValueError naming the camera and the crop; the reference's
    int(inf) raises OverflowError there.  Returns [(points [P, 2], boxes [n^2, 4])] per camera, float64."""
    stats = stats_to_host(stats)
    if "sub_count" not in stats:
        raise ValueError("mindepth_grids_from_stats: the statistics hold no samples (crop_stats(depths, samples))")
    return [_mindepth_camera(stats, layout, c, nsample_min_distance, rng) for c in range(_n_cams(stats))]


def _all_layers(depths, samples, n_per_side, n_layers, scale_per_layer, camera_fn):
    """One kernel call and one readback per layer over all cameras, then the host builder: cameras outer, layers inner (the
    reference's order of draws)."""
    if depths.dim() != 3:
        raise ValueError(f"depths must be [C, H, W], got {tuple(depths.shape)}")
    _, h, w = depths.shape
    layers = []
    for n in _layer_sides(n_per_side, n_layers, scale_per_layer):
        L = crop_layout(h, w, n)
        layers.append((L, stats_to_host(crop_stats(depths, samples, n, layout=L))))
    res = []
    for c in range(depths.shape[0]):
        per_layer = [camera_fn(stats, L, c) for L, stats in layers]
        res.append(([p for p, _ in per_layer], [b for _, b in per_layer]))
    return res


def depth_point_grids(depths, n_per_side=8, n_layers=0, scale_per_layer=1):
    """build_all_layer_depth_point_grids (preprocess.py:151-162) for every map of depths [C, H, W] on the GPU: per camera
    (points_by_layer, boxes_by_layer), lists of float64 arrays [P, 2] and [n^2, 4]."""
    return _all_layers(depths, None, n_per_side, n_layers, scale_per_layer, _depth_camera)


def mindepth_point_grids(depths, samples, n_per_side=8, n_layers=0, scale_per_layer=1, nsample_min_distance=4, rng=random):
    """build_all_layer_mindepth_point_grids (SAM_utils.py:355-366) for every pair of depths / samples [C, H, W] on the GPU: per
    camera (points_by_layer, boxes_by_layer).  With random.seed(s) beforehand the points are the reference's for the same
    images in the same order."""
    if samples is None:
        raise ValueError("mindepth_point_grids needs the depth-sample maps (gags_amd.depthsample.depth_samples)")
    return _all_layers(depths, samples, n_per_side, n_layers, scale_per_layer,
                       lambda stats, L, c: _mindepth_camera(stats, L, c, nsample_min_distance, rng))


# ---- the point-cloud mode -------------------------------------------------------------------------------------------------------

def sample_from_pcd(min_depth, visible, sample_num, rng=random, unique=False):
    """preprocess.py:176-184 on N6's tensors: min_depth [N] (depthsample.point_min_depth), visible [N, C] bool.  The
    candidates (points some camera sees) are found on the device; sample_num of them are drawn with rng.choices weighted by
    their min depth (numpy, in the input's dtype, as the reference forms them).  Returns the sorted indices, int64 [sample_num]
    WITH duplicates (the reference's sorted(set(...)) over 0-d tensors removes none); unique=True removes them."""
    visible = torch.as_tensor(visible)
    min_depth = torch.as_tensor(min_depth)
    if visible.dim() != 2 or min_depth.dim() != 1 or visible.shape[0] != min_depth.shape[0]:
        raise ValueError(f"min_depth {tuple(min_depth.shape)} must be [N] and visible {tuple(visible.shape)} [N, C]")
    if int(sample_num) < 0:
        raise ValueError("sample_num must be >= 0")
    point_ids = torch.nonzero(visible.to(min_depth.device).bool().any(dim=1)).flatten()
    if point_ids.numel() == 0:
        raise ValueError("sample_from_pcd: no camera sees any point")
    pcd_depth = min_depth[point_ids].cpu().numpy()
    weights = pcd_depth / np.sum(pcd_depth)
    drawn = rng.choices(point_ids.cpu().tolist(), weights, k=int(sample_num))
    return np.array(sorted(set(drawn)) if unique else sorted(drawn), dtype=np.int64)


def project_from_sampled_pcd(visible_c, mapping_c, n_layers, height, width):
    """preprocess.py:164-174: the pixels (v, u) of mapping_c [M, 2] where visible_c [M] holds, as float32 points
    (u / width, v / height), once per layer.  The selection runs where the tensors live."""
    visible_c = torch.as_tensor(visible_c).bool()
    mapping_c = torch.as_tensor(mapping_c)
    if mapping_c.dim() != 2 or mapping_c.shape[1] != 2 or visible_c.shape != mapping_c.shape[:1]:
        raise ValueError(f"visible_c {tuple(visible_c.shape)} must be [M] and mapping_c {tuple(mapping_c.shape)} [M, 2]")
    sel = mapping_c[visible_c.to(mapping_c.device)].cpu().numpy()
    points_by_layer = []
    for _ in range(int(n_layers) + 1):
        points = sel.astype(np.float32)
        points[:, 0] = points[:, 0] / height
        points[:, 1] = points[:, 1] / width
        points_by_layer.append(np.stack((points[:, 1], points[:, 0]), axis=-1))
    return points_by_layer


# ---- a scene --------------------------------------------------------------------------------------------------------------------

@torch.no_grad()
def prompt_scene(gaussians, cameras, mode, depths=None, names=None, bg_color=None, n_per_side=8, n_layers=0, scale_per_layer=1,
                 nsample_min_distance=4, vis_thresh=0.25, cut_bound=0, pcd_fraction=PCD_FRACTION, rng=random, unique=False):
    """The prompt grids of every camera, preprocess.py:create's four ways to make them, with the maps kept on the device:
      "grid"      build_all_layer_point_grids: the same regular lattice for every camera (no depth is rendered)
      "depth"     the ED depth of every camera (rendered here unless `depths` [C, H, W] is given) -> depth_point_grids
      "mindepth"  depthsample.depth_sample_scene -> mindepth_point_grids
      "pcd"       depth_sample_scene with the dense mapping -> sample_from_pcd(round(pcd_fraction N)) -> project_from_sampled_pcd
    The cameras may be of any model the rasterizer renders, mixed freely (N22: depthsample.camera_rig).
    Returns {"names": [C], "point_grids": per camera a list with one [P, 2] array per layer, points (x, y) in [0, 1]^2}."""
    from . import depthsample as DS
    if mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
    cameras = list(cameras)
    names = DS._names(cameras, names)
    if mode == "grid":
        grids = build_all_layer_point_grids(n_per_side, n_layers, scale_per_layer)
        return {"names": names, "point_grids": [[g.copy() for g in grids] for _ in cameras]}
    if mode == "depth":
        if depths is None:
            xyz = gaussians.get_xyz
            depths = DS.render_depths(gaussians, cameras, bg_color if bg_color is not None else torch.zeros(3, device=xyz.device))
        res = depth_point_grids(depths, n_per_side, n_layers, scale_per_layer)
        return {"names": names, "point_grids": [p for p, _ in res]}
    scene = DS.depth_sample_scene(gaussians, cameras, depths=depths, names=names, bg_color=bg_color, vis_thresh=vis_thresh,
                                  cut_bound=cut_bound, return_mapping=mode == "pcd")
    if mode == "mindepth":
        res = mindepth_point_grids(scene["depths"], scene["samples"], n_per_side, n_layers, scale_per_layer,
                                   nsample_min_distance, rng)
        return {"names": names, "point_grids": [p for p, _ in res]}
    _, h, w = scene["depths"].shape
    idx = sample_from_pcd(scene["min_depth"], scene["visible"], round(pcd_fraction * scene["min_depth"].shape[0]), rng, unique)
    idx = torch.from_numpy(idx).to(scene["visible"].device)
    visible, mapping = scene["visible"][idx], scene["mapping"][idx]
    return {"names": names, "point_grids": [project_from_sampled_pcd(visible[:, c], mapping[:, c], n_layers, h, w)
                                            for c in range(len(cameras))]}


def save_prompt_grids(directory, names, point_grids):
    """<directory>/<name>_prompts.npz for every camera, arrays layer0, layer1, ... (each [P, 2]): the grids for a SAM process
    elsewhere (SamAutomaticMaskGenerator(point_grids=...)).  Returns the paths written."""
    names = [str(nm) for nm in names]
    if len(names) != len(point_grids) or len(set(names)) != len(names):
        raise ValueError(f"{len(names)} names for {len(point_grids)} cameras' grids (one distinct name per camera)")
    os.makedirs(directory, exist_ok=True)
    paths = []
    for nm, layers in zip(names, point_grids):
        paths.append(os.path.join(directory, f"{nm}_prompts.npz"))
        np.savez(paths[-1], **{f"layer{i}": np.asarray(p) for i, p in enumerate(layers)})
    return paths


def load_prompt_grids(directory, names):
    """What save_prompt_grids wrote, in the order of `names`: per camera a list with one array per layer."""
    grids = []
    for nm in names:
        p = os.path.join(directory, f"{nm}_prompts.npz")
        if not os.path.exists(p):
            raise FileNotFoundError(f"no prompt grid for camera {nm!r}: {p}")
        with np.load(p) as z:
            grids.append([z[f"layer{i}"] for i in range(len(z.files))])
    return grids
