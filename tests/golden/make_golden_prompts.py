#!/usr/bin/env python
"""Generate tests/golden/prompts_vectors.npz by running the reference's OWN prompt-grid builders in this container, on the CPU:
preprocess.py's build_all_layer_depth_point_grids, sample_from_pcd, project_from_sampled_pcd and utils/SAM_utils.py's
build_all_layer_mindepth_point_grids (with sample_based_mapping), build_point_grid, build_all_layer_point_grids,
generate_crop_boxes.  Only data is stored.

    python tests/golden/make_golden_prompts.py

Both modules are imported unmodified; segment_anything, open_clip, cv2, torchvision, matplotlib, ... are empty stand-in
modules (as in the other make_golden_* scripts) -- the builders use none of them.  Every case runs under random.seed(42).

Cases (maps from tests/prompts_ref.py make_maps, the first seed that meets the margin below):
    a   37 x 70,  n = 8: crop sides 4 and 8 (under 10: empty sub-crops, uniform weights), gaps between crops, and no sample
                         in the left 60 % of the columns
    b   48 x 64,  n = 4
    c   135 x 240, n = 8: sub-crops of 13 x 24 that overlap by a pixel
    d   95 x 113, n = 3
    e   b's maps, two layers (n_layers = 1, scale_per_layer = 2: n = 4 and 2)
    f   b's maps and then a second 48 x 64 pair from ONE seeded stream (n = 4): f0_*, f1_*
    pcd N = 3000 points, 3 cameras of 48 x 64, 21 visible points, 60 = round(0.02 N) draws: the duplicate quirk of
        sorted(set(...)) over 0-d tensors (60 indices come back, asserted)

Margin, asserted for every crop of every layer of every case, in float64: the mean depth and ratio x nsample are at least 1e-3
from every integer and the ratio at least 1e-3 from 1.  The reference's fp32 torch.mean is about 1e-5 from the float64 mean
at these sizes, so with this margin the sample counts of float32(float64 sum / count) equal the reference's for every crop.
Also asserted: the reference's outputs equal tests/prompts_ref.py bit for bit.

Arrays.  cases [6] str; per case x: x_depth, x_sample [H, W] fp32 (e: none, b's), x_n, x_layers, x_scale; per layer i:
x_depth_points_i, x_depth_boxes_i, x_min_points_i, x_min_boxes_i (float64); x_margin.  f: f1_depth, f1_sample and f0_*, f1_*
results.  pcd_depth [N] fp32 (+inf where unseen), pcd_mask [N, 3] bool, pcd_mapping [N, 3, 2] int32, pcd_idx [60] int64,
pcd_points_c [M_c, 2] fp32.  grid_n = build_point_grid(n) for n in 1, 2, 8, 32; gridlayers_i = build_all_layer_point_grids(8, 2,
2)[i]; cropboxes_j / croplayers_j for the argument sets in cropboxes_args."""
import importlib.abc
import importlib.machinery
import os
import random
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "prompts_vectors.npz")
STUB_ROOTS = {"plyfile", "open3d", "cv2", "matplotlib", "open_clip", "segment_anything", "simple_knn", "gsplat",
              "torchvision", "mediapy", "jaxtyping", "tqdm", "sklearn", "PIL", "lpipsPyTorch", "scipy"}
MARGIN = 1e-3
NSAMPLE = 4
# name, H, W, n_per_side, n_layers, scale_per_layer, make_maps keywords
CASES = (("a", 37, 70, 8, 0, 1, {"density": 0.3, "empty_left": 0.6}),
         ("b", 48, 64, 4, 0, 1, {"density": 0.2}),
         ("c", 135, 240, 8, 0, 1, {"density": 0.15}),
         ("d", 95, 113, 3, 0, 1, {"density": 0.25, "empty_left": 0.2}))
CROPBOX_ARGS = (((48, 64), 0, 0.5), ((135, 240), 1, 512 / 1500), ((95, 113), 2, 0.25))


class _AnyModule(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        v = type(name, (), {"__init__": lambda self, *a, **k: None, "__class_getitem__": classmethod(lambda c, i: c)})
        setattr(self, name, v)
        return v


class _Stubs(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, name, path, target=None):
        if name.split(".")[0] in STUB_ROOTS:
            return importlib.machinery.ModuleSpec(name, self, is_package=True)

    def create_module(self, spec):
        m = _AnyModule(spec.name)
        m.__path__ = []
        return m

    def exec_module(self, m):
        pass


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), what


def main():
    sys.meta_path.insert(0, _Stubs())
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.dirname(HERE))
    import prompts_ref as R
    import preprocess as P
    import utils.SAM_utils as S
    P.print = lambda *a, **k: None
    S.print = lambda *a, **k: None
    out = {}
    seed_box = [500]

    def margin_of(depth, sample, n, layers, scale):
        return min(R.margin(depth, sample, m, NSAMPLE) for m in R.layer_sides(n, layers, scale))

    def next_maps(h, w, layer_sets, kw):
        """The next seed whose maps meet the margin for every (n, n_layers, scale) the case runs under."""
        while True:
            seed_box[0] += 1
            depth, sample = R.make_maps(seed_box[0], h, w, **kw)
            m = min(margin_of(depth, sample, *ls) for ls in layer_sets)
            if m >= MARGIN:
                return depth, sample, m

    def run(tag, images, n, layers, scale):
        """The reference and the restatement on a list of (depth, sample) images from ONE stream seeded with 42; stores
        <tag><i>_* (or <tag>_* for a single image)."""
        single = len(images) == 1
        random.seed(42)
        ref = [S.build_all_layer_mindepth_point_grids(n_per_side=n, n_layers=layers, scale_per_layer=scale,
                                                       nsample_min_distance=NSAMPLE, depth_map=torch.from_numpy(d),
                                                       depth_sample=torch.from_numpy(s)) for d, s in images]
        random.seed(42)
        mine = [R.all_layer_mindepth_grids(n, layers, scale, NSAMPLE, d, s) for d, s in images]
        for i, ((d, s), (rp, rb), (mp, mb)) in enumerate(zip(images, ref, mine)):
            key = tag if single else f"{tag}{i}"
            dp, db = P.build_all_layer_depth_point_grids(n_per_side=n, n_layers=layers, scale_per_layer=scale,
                                                         depth_map=torch.from_numpy(d))
            dp2, db2 = S.build_all_layer_depth_point_grids(n_per_side=n, n_layers=layers, scale_per_layer=scale,
                                                           depth_map=torch.from_numpy(d))
            mdp, mdb = R.all_layer_depth_grids(n, layers, scale, d)
            assert len(rp) == len(dp) == layers + 1
            for li in range(layers + 1):
                same(rp[li], mp[li], (key, "min points", li))
                same(rb[li], mb[li], (key, "min boxes", li))
                same(dp[li], mdp[li], (key, "depth points", li))
                same(db[li], mdb[li], (key, "depth boxes", li))
                same(dp[li], dp2[li], (key, "the two copies of build_depth_point_grid", li))
                assert rp[li].dtype == np.float64 and dp[li].dtype == np.float64 and rb[li].shape == (
                    R.layer_sides(n, layers, scale)[li] ** 2, 4)
                assert 0 <= rp[li].min() and rp[li].max() <= 1
                out[f"{key}_min_points_{li}"], out[f"{key}_min_boxes_{li}"] = rp[li], rb[li]
                out[f"{key}_depth_points_{li}"], out[f"{key}_depth_boxes_{li}"] = dp[li], db[li]
        return ref

    cases = []
    for name, h, w, n, layers, scale, kw in CASES:
        sets = [(n, layers, scale)] + ([(4, 1, 2)] if name == "b" else [])  # b also runs as e's two layers
        depth, sample, m = next_maps(h, w, sets, kw)
        out[f"{name}_depth"], out[f"{name}_sample"] = depth, sample
        out[f"{name}_n"], out[f"{name}_layers"], out[f"{name}_scale"], out[f"{name}_margin"] = n, layers, scale, m
        run(name, [(depth, sample)], n, layers, scale)
        cases.append(name)
        print(name, (h, w), "n", n, "margin %.2e" % m, "points", out[f"{name}_min_points_0"].shape[0],
              out[f"{name}_depth_points_0"].shape[0])
    b = (out["b_depth"], out["b_sample"])
    # e: two layers on b's maps
    out["e_n"], out["e_layers"], out["e_scale"], out["e_margin"] = 4, 1, 2, margin_of(*b, 4, 1, 2)
    assert out["e_margin"] >= MARGIN
    run("e", [b], 4, 1, 2)
    cases.append("e")
    # f: two consecutive images from one stream
    d1, s1, m1 = next_maps(48, 64, [(4, 0, 1)], {"density": 0.35, "hi": 9.0})
    out["f1_depth"], out["f1_sample"] = d1, s1
    out["f_n"], out["f_layers"], out["f_scale"], out["f_margin"] = 4, 0, 1, min(m1, margin_of(*b, 4, 0, 1))
    run("f", [b, (d1, s1)], 4, 0, 1)
    same(out["f0_min_points_0"], out["b_min_points_0"], "the first image of the stream is case b")
    assert not np.array_equal(out["f1_min_points_0"][:4], out["f0_min_points_0"][:4])
    cases.append("f")
    out["cases"] = np.array(cases)
    # the case list promises these properties
    st = R.crop_stats(out["a_depth"][None], out["a_sample"][None], 8)
    assert (st["sample_count"] == 0).sum() >= 24 and not st["sub_count"].any(), "a: many crops without a sample, no sub-crop"
    wins = R.sub_windows(135 // 8, 240 // 8)
    assert any(wins[i][3] > wins[i + 1][2] for i in range(9)), "c: neighbouring sub-crops share a column"
    nums = {k: out[f"{k}_depth_points_0"].shape[0] for k in "abcd"}
    assert all(v > out[f"{k}_n"] ** 2 for k, v in nums.items()), nums  # some crop has more than one point

    # the point-cloud mode
    g = np.random.default_rng(7)
    N, C, H, W = 3000, 3, 48, 64
    seen = np.sort(g.choice(N, 21, replace=False))
    mask = np.zeros((N, C), bool)
    mapping = np.zeros((N, C, 2), np.int32)
    for i in seen:
        cams = g.choice(C, g.integers(1, C + 1), replace=False)
        mask[i, cams] = True
        mapping[i, cams, 0] = g.integers(0, H, len(cams))
        mapping[i, cams, 1] = g.integers(0, W, len(cams))
    pcd_depth = np.full(N, np.inf, np.float32)
    pcd_depth[seen] = g.uniform(0.5, 9.0, 21).astype(np.float32)
    k = round(0.02 * N)
    random.seed(42)
    idx = P.sample_from_pcd(pcd_depth, mask, k)
    assert len(idx) == k == 60 and len({int(t) for t in idx}) < k, "the duplicate quirk: sorted(set(...)) removed nothing"
    idx = np.array([int(t) for t in idx], np.int64)
    random.seed(42)
    same(idx, R.sample_from_pcd(pcd_depth, mask, k), "pcd indices")
    random.seed(42)
    uniq = R.sample_from_pcd(pcd_depth, mask, k, unique=True)
    same(uniq, np.unique(idx), "unique=True")
    out.update(pcd_depth=pcd_depth, pcd_mask=mask, pcd_mapping=mapping, pcd_idx=idx)
    for c in range(C):
        pts = P.project_from_sampled_pcd(mask[idx, c].astype(bool), mapping[idx, c], n_layers=0, height=H, width=W)
        pts2 = S.project_from_sampled_pcd(mask[idx, c].astype(bool), mapping[idx, c], n_layers=0, h=H, w=W)
        mine = R.project_from_sampled_pcd(mask[idx, c], mapping[idx, c], 0, H, W)
        assert len(pts) == 1 and pts[0].dtype == np.float32 and pts[0].shape[0] > 0
        same(pts[0], mine[0], ("pcd points", c))
        same(pts[0], pts2[0], ("the two copies of project_from_sampled_pcd", c))
        out[f"pcd_points_{c}"] = pts[0]

    # the regular grids and SAM's crop boxes
    for n in (1, 2, 8, 32):
        out[f"grid_{n}"] = S.build_point_grid(n)
    for i, gr in enumerate(S.build_all_layer_point_grids(8, 2, 2)):
        out[f"gridlayers_{i}"] = gr
    out["cropboxes_args"] = np.array([[a[0][0], a[0][1], a[1], a[2]] for a in CROPBOX_ARGS], np.float64)
    for j, (size, layers, overlap) in enumerate(CROPBOX_ARGS):
        boxes, idxs = S.generate_crop_boxes(size, layers, overlap)
        out[f"cropboxes_{j}"], out[f"croplayers_{j}"] = np.array(boxes, np.int64), np.array(idxs, np.int64)

    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes; pcd", len(idx), "indices,", len(np.unique(idx)), "distinct")


if __name__ == "__main__":
    main()
