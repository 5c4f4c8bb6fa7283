"""Plain numpy / torch-CPU restatement of N13 (gags_amd/prompts.py, csrc/promptgrid.hip): the crop statistics and the three
prompt-grid builders of preprocess.py:114-184 and utils/SAM_utils.py:294-366, with every sum a numpy float64 sum over the
float32 values.  tests/golden/make_golden_prompts.py asserts that the reference's own functions give these results bit for
bit on the fixture cases; the tests compare the product against both.

The one place the restatement and the reference differ in arithmetic is the crop mean: torch.mean in fp32 there,
float32(float64 sum / count) here.  `margin` measures how far a case is from the points where that could decide another
sample count."""
import random
from itertools import product

import numpy as np

SUB = 10


def layout(h, w, n):
    """Integer geometry: crop starts x0, y0 [n], crop_w, crop_h, sub-crop starts sx, sy [10] of a (crop_h, crop_w) crop."""
    x0 = np.linspace(0, w - 1, n + 1)[:-1].astype(np.int32)
    y0 = np.linspace(0, h - 1, n + 1)[:-1].astype(np.int32)
    crop_w, crop_h = int(w / n), int(h / n)
    return {"h": h, "w": w, "n": n, "x0": x0, "y0": y0, "crop_w": crop_w, "crop_h": crop_h}


def sub_windows(hc, wc):
    """The 100 sub-crop windows (row0, row1, col0, col1) of a crop of shape (hc, wc), i = jy 10 + jx."""
    sx = np.linspace(0, wc - 1, SUB + 1)[:-1].astype(np.int32)
    sy = np.linspace(0, hc - 1, SUB + 1)[:-1].astype(np.int32)
    wins = []
    for i in range(SUB * SUB):
        jx, jy = i % SUB, i // SUB
        wins.append((int(sy[jy]), min(hc - 1, int(sy[jy]) + hc // SUB), int(sx[jx]), min(wc - 1, int(sx[jx]) + wc // SUB)))
    return wins


def crops(h, w, n):
    """(k, row slice, column slice) of every crop, k = ix n + iy."""
    L = layout(h, w, n)
    for k, (x0, y0) in enumerate(product(L["x0"], L["y0"])):
        x0, y0 = int(x0), int(y0)
        yield k, slice(y0, min(y0 + L["crop_h"], h)), slice(x0, min(x0 + L["crop_w"], w))


def crop_stats(depths, samples, n):
    """What gags_promptgrid_stats defines, for depths / samples [C, H, W] float32 (samples may be None)."""
    depths = np.asarray(depths, np.float32)
    c, h, w = depths.shape
    out = {"depth_sum": np.zeros((c, n * n), np.float64), "depth_count": np.zeros((c, n * n), np.int32)}
    if samples is not None:
        samples = np.asarray(samples, np.float32)
        out.update(sample_sum=np.zeros((c, n * n), np.float64), sample_count=np.zeros((c, n * n), np.int32),
                   sub_count=np.zeros((c, n * n, SUB * SUB), np.int32))
    with np.errstate(invalid="ignore"):
        for ci in range(c):
            for k, rows, cols in crops(h, w, n):
                d = depths[ci, rows, cols]
                out["depth_sum"][ci, k] = np.sum(d, dtype=np.float64)
                out["depth_count"][ci, k] = d.size
                if samples is None:
                    continue
                s = samples[ci, rows, cols]
                nz = s != 0
                out["sample_sum"][ci, k] = np.sum(s[nz], dtype=np.float64)
                out["sample_count"][ci, k] = int(nz.sum())
                for i, (r0, r1, c0, c1) in enumerate(sub_windows(*s.shape)):
                    out["sub_count"][ci, k, i] = int(nz[r0:r1, c0:c1].sum())
    return out


def _mean32(total, count):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.float32(np.float64(total) / np.float64(count))


def _boxes(L):
    return np.stack([np.array([x0 / L["w"], y0 / L["h"], (x0 + L["crop_w"]) / L["w"], (y0 + L["crop_h"]) / L["h"]])
                     for x0, y0 in product(L["x0"], L["y0"])], axis=0)


def depth_grid(n, depth_map):
    """build_depth_point_grid (preprocess.py:114-149)."""
    depth_map = np.asarray(depth_map, np.float32)
    h, w = depth_map.shape
    L = layout(h, w, n)
    st = crop_stats(depth_map[None], None, n)
    pts = []
    for k, (x0, y0) in enumerate(product(L["x0"], L["y0"])):
        num = int(_mean32(st["depth_sum"][0, k], st["depth_count"][0, k]))
        num = 20 if num > 20 else 1 if num < 1 else num
        ox, oy = L["crop_w"] / (2 * num), L["crop_h"] / (2 * num)
        ax = np.linspace(x0 + ox, x0 + L["crop_w"] - ox, num)
        ay = np.linspace(y0 + oy, y0 + L["crop_h"] - oy, num)
        gx, gy = np.meshgrid(ax, ay)  # x fastest
        pts.append(np.stack([gx, gy], axis=-1).reshape(-1, 2))
    return np.concatenate(pts, axis=0) / np.array([[w, h]]), _boxes(L)


def mindepth_grid(n, depth_map, sample_map, nsample_min_distance=4, rng=random):
    """build_mindepth_point_grid + sample_based_mapping (SAM_utils.py:294-353)."""
    depth_map, sample_map = np.asarray(depth_map, np.float32), np.asarray(sample_map, np.float32)
    h, w = depth_map.shape
    L = layout(h, w, n)
    st = crop_stats(depth_map[None], sample_map[None], n)
    hc, wc = L["crop_h"], L["crop_w"]
    wins = sub_windows(hc, wc)
    pts = []
    for k, (x0, y0) in enumerate(product(L["x0"], L["y0"])):
        md = _mean32(st["depth_sum"][0, k], st["depth_count"][0, k])
        ms = _mean32(st["sample_sum"][0, k], st["sample_count"][0, k])
        with np.errstate(divide="ignore", invalid="ignore"):
            r = md / ms
        num = 1 if (r < 1 or np.isnan(r)) else int(np.float32(r * np.float32(nsample_min_distance)))
        num = max(1, min(num, 20))
        counts = st["sub_count"][0, k].astype(np.int64)
        if not counts.any():
            counts[:] = 1
        for i in rng.choices(list(range(SUB * SUB)), counts / counts.sum(), k=num * num):
            r0, _, c0, _ = wins[i]
            px = rng.randint(c0, min(wc - 1, c0 + wc // SUB))
            py = rng.randint(r0, min(hc - 1, r0 + hc // SUB))
            pts.append((int(x0) + px, int(y0) + py))
    return np.array(pts, np.int64) / np.array([[w, h]]), _boxes(L)


def layer_sides(n_per_side, n_layers, scale_per_layer):
    return [int(n_per_side / (scale_per_layer ** i)) for i in range(n_layers + 1)]


def all_layer_depth_grids(n_per_side, n_layers, scale_per_layer, depth_map):
    res = [depth_grid(n, depth_map) for n in layer_sides(n_per_side, n_layers, scale_per_layer)]
    return [p for p, _ in res], [b for _, b in res]


def all_layer_mindepth_grids(n_per_side, n_layers, scale_per_layer, nsample_min_distance, depth_map, sample_map, rng=random):
    res = [mindepth_grid(n, depth_map, sample_map, nsample_min_distance, rng)
           for n in layer_sides(n_per_side, n_layers, scale_per_layer)]
    return [p for p, _ in res], [b for _, b in res]


def sample_from_pcd(pcd_depth, pcd_mask, sample_num, rng=random, unique=False):
    """preprocess.py:176-184.  The reference's sorted(set(...)) keeps duplicates (0-d tensors hash by identity): unique=False."""
    ids = np.nonzero(np.asarray(pcd_mask).any(axis=1))[0]
    d = np.asarray(pcd_depth)[ids]
    drawn = rng.choices(ids.tolist(), d / np.sum(d), k=sample_num)
    return np.array(sorted(set(drawn)) if unique else sorted(drawn), np.int64)


def project_from_sampled_pcd(mask, mapping, n_layers, height, width):
    """preprocess.py:164-174: float32 (u / width, v / height) of the masked (v, u) rows, once per layer."""
    vu = np.asarray(mapping)[np.asarray(mask, bool)].astype(np.float32)
    return [np.stack((vu[:, 1] / np.float32(width), vu[:, 0] / np.float32(height)), axis=-1) for _ in range(n_layers + 1)]


def margin(depth_map, sample_map, n, nsample_min_distance=4):
    """The smallest distance, in float64, of any crop's mean depth or ratio x nsample from an integer and of any ratio from 1:
    the fp32 mean of the reference is about 1e-5 from the float64 one, so a margin of 1e-3 pins every sample count."""
    depth_map = np.asarray(depth_map, np.float32)
    st = crop_stats(depth_map[None], None if sample_map is None else np.asarray(sample_map, np.float32)[None], n)
    md = st["depth_sum"][0] / st["depth_count"][0]
    m = float(np.min(np.abs(md - np.rint(md))))
    if sample_map is not None:
        has = st["sample_count"][0] > 0
        r = md[has] / (st["sample_sum"][0][has] / st["sample_count"][0][has])
        if r.size:
            q = r * nsample_min_distance
            m = min(m, float(np.min(np.abs(r - 1))), float(np.min(np.abs(q - np.rint(q)))))
    return m


def make_maps(seed, h, w, density=0.2, empty_left=0.0, lo=0.6, hi=14.0):
    """A synthetic (depth, sample) pair [h, w] float32: a smooth depth ramp from lo to hi with noise -- crop means from below
    1 to above the clamp region -- and sparse samples = a fraction of the depth (the min depth over the cameras is never
    above the rendered depth by much), none in the left `empty_left` share of the columns."""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    ramp = lo + (hi - lo) * (0.65 * xx / max(w - 1, 1) + 0.35 * yy / max(h - 1, 1))
    depth = (ramp * g.uniform(0.9, 1.1, (h, w))).astype(np.float32)
    frac = g.uniform(0.15, 1.1, (h, w)) * (0.3 + 0.7 * yy / max(h - 1, 1))
    sample = np.where(g.random((h, w)) < density, depth * frac, 0).astype(np.float32)
    sample[:, : int(w * empty_left)] = 0
    return depth, sample
