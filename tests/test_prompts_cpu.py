"""N13 on the host: the builders of gags_amd/prompts.py, fed with the statistics of tests/prompts_ref.py, against what the
reference's own functions produced (tests/golden/prompts_vectors.npz, made by tests/golden/make_golden_prompts.py): every
point, box, point-cloud index and regular grid bit for bit; the file round trip and the argument errors."""
import os
import random
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import prompts_ref as R  # noqa: E402

Z = np.load(os.path.join(HERE, "golden", "prompts_vectors.npz"))
NSAMPLE = 4


def same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), what


def images(case):
    """The (depth, sample) images of a fixture case, in stream order."""
    if case == "e":
        return [(Z["b_depth"], Z["b_sample"])]
    if case == "f":
        return [(Z["b_depth"], Z["b_sample"]), (Z["f1_depth"], Z["f1_sample"])]
    return [(Z[f"{case}_depth"], Z[f"{case}_sample"])]


def keys(case):
    return ["f0", "f1"] if case == "f" else [case]


def ref_crop_stats(depths, samples=None, n_per_side=8, layout=None):
    """prompts.crop_stats' stand-in without a GPU: the restatement's statistics."""
    return R.crop_stats(depths.numpy(), None if samples is None else samples.numpy(), n_per_side)


def test_crop_layout_is_the_restatements_geometry():
    from gags_amd import prompts as P
    for h, w, n in ((37, 70, 8), (48, 64, 4), (135, 240, 8), (95, 113, 3), (1080, 1920, 8), (3, 5, 1), (19, 20, 2), (5, 3, 8)):
        L, want = P.crop_layout(h, w, n), R.layout(h, w, n)
        for k in ("x0", "y0"):
            same(L[k], want[k], (h, w, n, k))
        assert (L["crop_w"], L["crop_h"]) == (want["crop_w"], want["crop_h"]) == (w // n, h // n)
        assert L["boxes"].shape == (n * n, 4) and L["boxes"].dtype == np.float64
        wins = R.sub_windows(L["crop_h"], L["crop_w"])
        assert [wn[2] for wn in wins[:10]] == L["sx"].tolist() and [wn[0] for wn in wins[::10]] == L["sy"].tolist()
        # every crop lies inside the image with the full (crop_h, crop_w) shape
        assert int(L["x0"][-1]) + L["crop_w"] <= w and int(L["y0"][-1]) + L["crop_h"] <= h
    assert P.crop_layout(37, 70, 8)["x0"].tolist() == [0, 8, 17, 25, 34, 43, 51, 60]  # gaps: 8 wide, 8 or 9 apart


@pytest.mark.parametrize("case", ["a", "b", "c", "d", "e", "f"])
def test_builders_reproduce_the_reference(case):
    """depth_grids_from_stats and mindepth_grids_from_stats per layer, cameras outer and layers inner from one stream seeded
    with 42, as the reference ran them."""
    from gags_amd import prompts as P
    n, layers, scale = int(Z[f"{case}_n"]), int(Z[f"{case}_layers"]), int(Z[f"{case}_scale"])
    assert float(Z[f"{case}_margin"]) >= 1e-3
    random.seed(42)
    for key, (depth, sample) in zip(keys(case), images(case)):
        for li, m in enumerate(R.layer_sides(n, layers, scale)):
            L = P.crop_layout(*depth.shape, m)
            stats = R.crop_stats(depth[None], sample[None], m)
            (pts, boxes), = P.mindepth_grids_from_stats(stats, L, NSAMPLE)
            same(pts, Z[f"{key}_min_points_{li}"], (key, li, "min points"))
            same(boxes, Z[f"{key}_min_boxes_{li}"], (key, li, "min boxes"))
            (pts, boxes), = P.depth_grids_from_stats({k: stats[k] for k in ("depth_sum", "depth_count")}, L)
            same(pts, Z[f"{key}_depth_points_{li}"], (key, li, "depth points"))
            same(boxes, Z[f"{key}_depth_boxes_{li}"], (key, li, "depth boxes"))
            same(boxes, L["boxes"], (key, li, "layout boxes"))


@pytest.mark.parametrize("case", ["e", "f"])
def test_all_layer_drivers_keep_the_reference_order(case, monkeypatch):
    """mindepth_point_grids / depth_point_grids over a stack of cameras and several layers (the statistics from the
    restatement instead of the kernel): one stream, cameras outer, layers inner."""
    from gags_amd import prompts as P
    monkeypatch.setattr(P, "crop_stats", ref_crop_stats)
    n, layers, scale = int(Z[f"{case}_n"]), int(Z[f"{case}_layers"]), int(Z[f"{case}_scale"])
    depths = torch.from_numpy(np.stack([d for d, _ in images(case)]))
    samples = torch.from_numpy(np.stack([s for _, s in images(case)]))
    random.seed(42)
    res = P.mindepth_point_grids(depths, samples, n, layers, scale, NSAMPLE)
    dres = P.depth_point_grids(depths, n, layers, scale)
    assert len(res) == len(dres) == len(keys(case))
    for key, (pts, boxes), (dpts, dboxes) in zip(keys(case), res, dres):
        assert len(pts) == len(boxes) == len(dpts) == len(dboxes) == layers + 1
        for li in range(layers + 1):
            same(pts[li], Z[f"{key}_min_points_{li}"], (key, li))
            same(boxes[li], Z[f"{key}_min_boxes_{li}"], (key, li))
            same(dpts[li], Z[f"{key}_depth_points_{li}"], (key, li))
            same(dboxes[li], Z[f"{key}_depth_boxes_{li}"], (key, li))
    # an own generator instead of the module's: the same stream
    res2 = P.mindepth_point_grids(depths, samples, n, layers, scale, NSAMPLE, rng=random.Random(42))
    for (p1, _), (p2, _) in zip(res, res2):
        for a, b in zip(p1, p2):
            same(a, b)


def test_sample_counts_clamp_and_nonfinite_means():
    from gags_amd import prompts as P
    L = P.crop_layout(20, 20, 1)
    st = lambda total: {"depth_sum": np.array([[total]], np.float64), "depth_count": np.array([[400]], np.int32)}  # noqa: E731
    for mean, num in ((0.2, 1), (-3.0, 1), (1.999, 1), (2.0, 2), (20.5, 20), (1e6, 20)):
        (pts, _), = P.depth_grids_from_stats(st(mean * 400), L)
        assert pts.shape == (num * num, 2), (mean, pts.shape)
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match=r"camera 0, crop 0"):
            P.depth_grids_from_stats(st(bad), L)
    empty = {"depth_sum": np.zeros((2, 1)), "depth_count": np.zeros((2, 1), np.int32)}
    empty["depth_sum"][0, 0], empty["depth_count"][0, 0] = 800.0, 400
    with pytest.raises(ValueError, match=r"camera 1, crop 0"):
        P.depth_grids_from_stats(empty, L)
    # min-depth mode: r < 1, NaN (no sample) -> 1 point; r * nsample truncates; clamp at 20 -> 400 points
    def mst(dsum, ssum, scount):
        return {"depth_sum": np.array([[dsum]], np.float64), "depth_count": np.array([[400]], np.int32),
                "sample_sum": np.array([[ssum]], np.float64), "sample_count": np.array([[scount]], np.int32),
                "sub_count": np.zeros((1, 1, 100), np.int32)}
    for dsum, ssum, scount, num in ((400.0, 10.0, 5, 1), (400.0, 0.0, 0, 1), (800.0, 10.0, 10, 8), (700.0, 10.0, 10, 7),
                                    (4000.0, 10.0, 10, 20), (np.nan, 10.0, 10, 1)):
        (pts, _), = P.mindepth_grids_from_stats(mst(dsum, ssum, scount), L, 4, rng=random.Random(1))
        assert pts.shape == (num * num, 2), (dsum, ssum, scount, pts.shape)
        assert pts.min() >= 0 and pts.max() < 1
    with pytest.raises(ValueError, match=r"camera 0, crop 0"):
        P.mindepth_grids_from_stats(mst(400.0, 0.0, 3), L, 4)  # mean sample 0: an infinite ratio
    with pytest.raises(ValueError, match="hold no samples"):
        P.mindepth_grids_from_stats(st(400.0), L)


def test_draws_follow_the_sub_crop_counts():
    """All weight on one sub-crop: every point falls into that window; the calls made on rng are choices once per crop, then
    randint(x), randint(y) per draw."""
    from gags_amd import prompts as P
    L = P.crop_layout(60, 80, 2)  # crops 30 x 40: sub-crops 3 x 4
    calls = []

    class Rec(random.Random):
        def choices(self, population, weights=None, *, cum_weights=None, k=1):
            calls.append(("choices", len(population), k))
            return super().choices(population, weights, cum_weights=cum_weights, k=k)

        def randint(self, a, b):
            calls.append(("randint", int(a), int(b)))
            return super().randint(a, b)

    sub = np.zeros((1, 4, 100), np.int32)
    sub[0, :, 57] = 9  # jy = 5, jx = 7
    stats = {"depth_sum": np.full((1, 4), 2400.0), "depth_count": np.full((1, 4), 1200, np.int32),
             "sample_sum": np.full((1, 4), 10.0), "sample_count": np.full((1, 4), 10, np.int32), "sub_count": sub}
    (pts, _), = P.mindepth_grids_from_stats(stats, L, 1, rng=Rec(3))  # r = 2 -> 2 x 2 draws per crop
    assert pts.shape == (16, 2)
    sx, sy = int(L["sx"][7]), int(L["sy"][5])
    assert [c for c in calls if c[0] == "choices"] == [("choices", 100, 4)] * 4
    assert calls[:9] == [("choices", 100, 4)] + [("randint", sx, sx + 4), ("randint", sy, sy + 3)] * 4
    px, py = np.rint(pts[:, 0] * 80).astype(int), np.rint(pts[:, 1] * 60).astype(int)
    for k, (x0, y0) in enumerate(((0, 0), (0, 29), (39, 0), (39, 29))):  # x outer
        assert ((px[4 * k:4 * k + 4] >= x0 + sx) & (px[4 * k:4 * k + 4] <= x0 + sx + 4)).all()
        assert ((py[4 * k:4 * k + 4] >= y0 + sy) & (py[4 * k:4 * k + 4] <= y0 + sy + 3)).all()


def test_regular_grids_and_crop_boxes():
    from gags_amd import prompts as P
    for n in (1, 2, 8, 32):
        same(P.build_point_grid(n), Z[f"grid_{n}"], n)
    for i, g in enumerate(P.build_all_layer_point_grids(8, 2, 2)):
        same(g, Z[f"gridlayers_{i}"], i)
    for j, (h, w, layers, overlap) in enumerate(Z["cropboxes_args"]):
        boxes, idxs = P.generate_crop_boxes((int(h), int(w)), int(layers), float(overlap))
        same(np.array(boxes, np.int64), Z[f"cropboxes_{j}"], j)
        same(np.array(idxs, np.int64), Z[f"croplayers_{j}"], j)


def test_pcd_mode_and_the_duplicate_quirk():
    from gags_amd import prompts as P
    depth, mask, mapping = torch.from_numpy(Z["pcd_depth"]), torch.from_numpy(Z["pcd_mask"]), torch.from_numpy(Z["pcd_mapping"])
    assert np.isinf(Z["pcd_depth"]).sum() == 3000 - 21  # N6's +inf: never candidates, no infinite weight
    random.seed(42)
    idx = P.sample_from_pcd(depth, mask, 60)
    same(idx, Z["pcd_idx"], "indices")
    assert len(idx) == 60 and len(np.unique(idx)) < 60  # the reference's sorted(set(...)) removed nothing
    random.seed(42)
    same(P.sample_from_pcd(depth, mask, 60, unique=True), np.unique(Z["pcd_idx"]), "unique")
    same(P.sample_from_pcd(depth, mask, 60, rng=random.Random(42)), Z["pcd_idx"], "own generator")
    for c in range(3):
        t = torch.from_numpy(idx)
        pts = P.project_from_sampled_pcd(mask[t, c], mapping[t, c], 0, 48, 64)
        assert len(pts) == 1
        same(pts[0], Z[f"pcd_points_{c}"], c)
        two = P.project_from_sampled_pcd(mask[t, c].numpy(), mapping[t, c].numpy(), 1, 48, 64)
        assert len(two) == 2 and np.array_equal(two[0], two[1]) and np.array_equal(two[0], pts[0])
    with pytest.raises(ValueError, match="no camera sees"):
        P.sample_from_pcd(depth, torch.zeros_like(mask), 5)
    with pytest.raises(ValueError):
        P.sample_from_pcd(depth[:10], mask, 5)
    with pytest.raises(ValueError):
        P.project_from_sampled_pcd(mask[:5, 0], mapping[:4, 0], 0, 48, 64)


def test_save_load_round_trip(tmp_path):
    from gags_amd import prompts as P
    grids = [[Z["e_min_points_0"], Z["e_min_points_1"]], [Z["pcd_points_0"]]]
    paths = P.save_prompt_grids(str(tmp_path / "out"), ["cam_a", "cam_b"], grids)
    assert [os.path.basename(p) for p in paths] == ["cam_a_prompts.npz", "cam_b_prompts.npz"]
    back = P.load_prompt_grids(str(tmp_path / "out"), ["cam_b", "cam_a"])
    assert len(back[0]) == 1 and len(back[1]) == 2
    same(back[0][0], grids[1][0])
    same(back[1][0], grids[0][0])
    same(back[1][1], grids[0][1])
    with pytest.raises(FileNotFoundError, match="cam_c"):
        P.load_prompt_grids(str(tmp_path / "out"), ["cam_c"])
    with pytest.raises(ValueError):
        P.save_prompt_grids(str(tmp_path / "out"), ["x"], grids)
    with pytest.raises(ValueError):
        P.save_prompt_grids(str(tmp_path / "out"), ["x", "x"], grids)


def test_argument_errors():
    from gags_amd import prompts as P
    for bad in ((0, 5, 1), (5, 0, 1), (5, 5, 0)):
        with pytest.raises(ValueError):
            P.crop_layout(*bad)
    with pytest.raises(RuntimeError, match="no CPU path"):
        P.crop_stats(torch.zeros(1, 8, 8))
    with pytest.raises(ValueError, match="n_layers"):
        P.build_all_layer_point_grids(8, -1, 1)
    with pytest.raises(ValueError, match="needs the depth-sample maps"):
        P.mindepth_point_grids(torch.zeros(1, 8, 8), None)
    with pytest.raises(ValueError, match="mode must be one of"):
        P.prompt_scene(None, [], "sam")
    assert P.MODES == ("grid", "depth", "mindepth", "pcd") and P.PCD_FRACTION == 0.02


def test_grid_mode_needs_no_gpu():
    from gags_amd import prompts as P

    class Cam:
        def __init__(self, name):
            self.image_name = name
    res = P.prompt_scene(None, [Cam("a"), Cam("b")], "grid", n_per_side=4, n_layers=1, scale_per_layer=2)
    assert res["names"] == ["a", "b"] and len(res["point_grids"]) == 2
    same(res["point_grids"][1][0], P.build_point_grid(4))
    same(res["point_grids"][1][1], P.build_point_grid(2))


def test_library_declares_the_entries():
    """The C entries exist and validate without launching (no GPU here)."""
    from gags_amd import _lib
    lib = _lib.load()
    assert lib.gags_abi_version() == 2
    assert lib.gags_promptgrid_stats(0, 8, 8, 1, 8, 8, *([None] * 8), None, 0, None) == -1
    assert lib.gags_promptgrid_stats(1, 8, 8, 1, 8, 8, *([None] * 8), None, 0, None) == -1   # null pointers
    assert lib.gags_promptgrid_stats(1, 8, 8, 1, 9, 8, *([None] * 8), None, 0, None) == -1   # crop wider than the image
    # scratch is needed exactly when a crop is split into row slabs
    assert lib.gags_promptgrid_scratch_bytes(200, 1080, 1920, 8, 135) == 0
    assert lib.gags_promptgrid_scratch_bytes(1, 270, 480, 1, 270) > 0
    assert lib.gags_promptgrid_scratch_bytes(1, 3, 5, 1, 3) == 0
    assert lib.gags_promptgrid_scratch_bytes(0, 3, 5, 1, 3) == 0
