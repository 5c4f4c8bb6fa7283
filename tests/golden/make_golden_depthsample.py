#!/usr/bin/env python
"""Generate tests/golden/depthsample_vectors.npz by running the reference's OWN `depth_SAM.main` (the GAS stage's
point-to-pixel min-depth mapping) in this container, single-threaded.  Only data is stored.

    python tests/golden/make_golden_depthsample.py

depth_SAM.main runs unmodified; what is replaced is what this container lacks or what touches files:
  * open3d, matplotlib, gsplat, plyfile, ... are empty stand-in modules (as in make_golden_pcd.py); tqdm is a pass-through.
  * `Scene` / `GaussianModel` are stand-ins that serve the scene's cloud (get_xyz) and its cameras (FoVx, FoVy, image_width,
    image_height, image_name, world_view_transform), sorted by image_name as the reference's Scene sorts them.
  * torch.tensor(..., device="cuda") and Tensor.to("cuda") keep the tensor on the CPU (there is no GPU here).
  * os.listdir / np.load of the depth directory serve the scene's depth maps; np.save records what is written;
    process_one_image and save_pcd_depth are wrapped to record their arguments (K, the world-to-camera matrix, the
    per-camera masks and mappings, pcd_depth).
torch runs with one thread: the reference's index_put_ with duplicate indices then keeps the highest point index.

Scenes (all cameras of a scene share one size): "even" 64 x 48 and "odd" 63 x 47, each with random look-at cameras around
and inside the cloud (points behind the camera and outside the image) and two axis-aligned cameras (identity rotation,
dyadic translation, dyadic focal length) that carry deliberate exact ties on dyadic points: u = k + 0.5 (x = 0 at odd W),
u = W - 0.5, u = -0.5, |d - zc| = 0.25 d on both sides.  Depth maps are the cloud's own z-buffer (float64 projection)
with perturbations: zero pixels, occluders in front (0.7 z), far background.  The reference's CPU matmul sums in its
BLAS's order, so under the random cameras a point is rejected when its float64 u or v lies within 1e-3 px of a half-
integer or | |d - zc| - 0.25 d | <= 1e-5 d; under the axis-aligned cameras every summation order gives the same floats.

Asserted here: the reference's outputs equal tests/depthsample_ref.py (float32, highest index wins), every branch of the
rule occurs in bulk, and the margin holds.

Arrays, per scene s in ("even", "odd"): s_xyz [N,3] f32, s_viewmats [C,4,4] f32 (world_view_transform.T), s_Ks [C,3,3]
f32 (the reference's K), s_depths [C,H,W] f32, s_exact [C] bool (axis-aligned), s_names [C] str, and the reference's
outputs s_mapping [N,C,2] int32 (v, u), s_visible [N,C] bool, s_min_depth [N] f32, s_samples [C,H,W] f32.
"""
import importlib.abc
import importlib.machinery
import math
import os
import sys
import types
import warnings

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "depthsample_vectors.npz")
STUB_ROOTS = {"plyfile", "open3d", "cv2", "matplotlib", "open_clip", "segment_anything", "simple_knn", "gsplat",
              "torchvision", "mediapy", "jaxtyping", "tqdm", "sklearn", "PIL", "lpipsPyTorch"}
DEPTH_DIR = "/depthsample-golden/train/ours_30000/depths"


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


class Cam:
    def __init__(self, name, w2c, fx, fy, w, h):
        self.image_name, self.image_width, self.image_height = name, w, h
        self.FoVx, self.FoVy = 2 * math.atan(w / (2 * fx)), 2 * math.atan(h / (2 * fy))
        self.world_view_transform = torch.tensor(w2c, dtype=torch.float32).T.contiguous()


def look_at(pos, target, rng):
    f = target - pos
    f /= np.linalg.norm(f)
    up = rng.standard_normal(3)
    r = np.cross(f, up)
    r /= np.linalg.norm(r)
    d = np.cross(f, r)
    R = np.stack([r, d, f])
    w2c = np.eye(4)
    w2c[:3, :3], w2c[:3, 3] = R, -R @ pos
    return w2c


def proj64(xyz, w2c32, K):
    p = xyz.astype(np.float64) @ w2c32[:3, :3].astype(np.float64).T + w2c32[:3, 3].astype(np.float64)
    with np.errstate(all="ignore"):
        return p[:, 0] * K[0, 0] / p[:, 2] + K[0, 2], p[:, 1] * K[1, 1] / p[:, 2] + K[1, 2], p[:, 2]


def k_of(cam):
    t = math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)
    return np.array([[cam.image_width / (2 * t[0]), 0, cam.image_width / 2.0],
                     [0, cam.image_height / (2 * t[1]), cam.image_height / 2.0], [0, 0, 1]], np.float32)


def near_half(t):
    return np.abs(t - np.floor(t) - 0.5) < 1e-3


def build_scene(rng, w, h, n):
    """(xyz, cams, depths, exact): random points in [-1, 1]^3, random cameras, two axis-aligned cameras and tie points."""
    cams, exact = [], []
    f_axis = 32.0  # dyadic focal length of the axis-aligned cameras
    for k in range(5):
        pos = rng.standard_normal(3)
        pos *= (1.2 if k < 2 else 2.6) / np.linalg.norm(pos)  # the first two inside the cloud's bounding sphere
        target = 0.3 * rng.standard_normal(3)
        cams.append(Cam("", look_at(pos, target, rng), 0.55 * w, 0.6 * w, w, h))
        exact.append(False)
    for t in ((0.0, 0.0, 3.0), (0.25, -0.125, 2.5)):
        w2c = np.eye(4)
        w2c[:3, 3] = t
        cams.append(Cam("", w2c, f_axis, f_axis, w, h))
        exact.append(True)
    Ks = [k_of(c) for c in cams]
    for c, K in zip(cams, Ks):
        if exact[cams.index(c)]:
            assert K[0, 0] == f_axis and K[1, 1] == f_axis, K
    w2cs = [c.world_view_transform.T.numpy() for c in cams]

    # random points away from the half-integer band under the random cameras
    xyz = rng.uniform(-1, 1, (3 * n, 3)).astype(np.float32)
    keep = np.ones(len(xyz), bool)
    for c in range(len(cams)):
        if not exact[c]:
            u, v, _ = proj64(xyz, w2cs[c], Ks[c])
            keep &= ~(near_half(u) | near_half(v))
    xyz = xyz[keep][:n]
    # dyadic tie points for the axis-aligned cameras (zc = z + 3 or z + 2.5): x = 0 -> u = W / 2; x fx / zc = integer ->
    # u = k + 0.5 at odd W; u = W - 0.5 and u = -0.5; v likewise
    ties = []
    for z in (-1.0, -0.5, 0.0, 0.5):
        zc = z + 3.0
        for x in (0.0, zc / 32 * 4, -zc / 32 * 3, zc / 32 * (w / 2 - 0.5), -zc / 32 * (w / 2 + 0.5)):
            for y in (0.0, zc / 32 * 2, zc / 32 * (h / 2 - 0.5), -zc / 32 * (h / 2 + 0.5)):
                ties.append((x, y, z))
    ties = np.array(ties, np.float32)
    assert np.array_equal(ties.astype(np.float64) * 4096, np.round(ties.astype(np.float64) * 4096))  # dyadic
    # the tie points must also stay off the band of the random cameras
    ok = np.ones(len(ties), bool)
    for c in range(len(cams)):
        if not exact[c]:
            u, v, _ = proj64(ties, w2cs[c], Ks[c])
            ok &= ~(near_half(u) | near_half(v))
    xyz = np.concatenate([xyz, ties[ok]])
    xyz = xyz[rng.permutation(len(xyz))]

    # depth maps: float64 z-buffer, then perturbations
    depths = np.zeros((len(cams), h, w), np.float32)
    for c in range(len(cams)):
        u, v, zc = proj64(xyz, w2cs[c], Ks[c])
        with np.errstate(invalid="ignore"):
            ui, vi = np.rint(u), np.rint(v)
            ins = (ui >= 0) & (ui < w) & (vi >= 0) & (vi < h) & (zc > 0)
        zb = np.full(h * w, np.inf)
        np.minimum.at(zb, (vi[ins] * w + ui[ins]).astype(np.int64), zc[ins])
        zb = zb.reshape(h, w)
        r = rng.random((h, w))
        zb = np.where(r < 0.08, 0.7 * zb, zb)       # occluders in front: the z-buffer point itself fails
        zb = np.where((r >= 0.08) & (r < 0.14), 0.0, zb)  # zero-depth pixels
        zb = np.where(np.isinf(zb), np.where(r < 0.5, 0.0, 40.0), zb)  # empty pixels: no hit or far background
        depths[c] = zb.astype(np.float32)
        if exact[c]:
            # exact occlusion ties: pixels under the tie points at zc = 2.5 and 3.5 (z = -0.5, 0.5 at t_z = 3) read d = 2 or
            # 2.8 / ... chosen so that |d - zc| == 0.25 d exactly for some and just past it for others
            tz = w2cs[c][2, 3]
            for x, y, z in ties:
                zc32 = np.float32(np.float32(z) + np.float32(tz))
                uu = (np.float32(x) + np.float32(w2cs[c][0, 3])) * np.float32(32) / zc32 + np.float32(w / 2)
                vv = (np.float32(y) + np.float32(w2cs[c][1, 3])) * np.float32(32) / zc32 + np.float32(h / 2)
                ui_, vi_ = int(np.rint(uu)), int(np.rint(vv))
                if 0 <= ui_ < w and 0 <= vi_ < h and (ui_ + vi_) % 3 == 0:
                    depths[c, vi_, ui_] = np.float32(zc32 / 1.25) if (ui_ // 3) % 2 == 0 else np.float32(zc32 / 0.75)
    # drop points in the occlusion band of a random camera (axis-aligned cameras are exact)
    keep = np.ones(len(xyz), bool)
    for c in range(len(cams)):
        if not exact[c]:
            u, v, zc = proj64(xyz, w2cs[c], Ks[c])
            with np.errstate(invalid="ignore"):
                ui, vi = np.rint(u), np.rint(v)
                ins = (ui >= 0) & (ui < w) & (vi >= 0) & (vi < h)
            d = np.where(ins, depths[c][np.where(ins, vi, 0).astype(np.int64), np.where(ins, ui, 0).astype(np.int64)], 0)
            d = d.astype(np.float64)
            keep &= ~(ins & (np.abs(np.abs(d - zc) - np.float32(0.25) * d) <= 1e-5 * np.abs(d)))
    xyz = xyz[keep]
    names = [f"cam_{k:02d}" for k in range(len(cams))]
    order = rng.permutation(len(cams))  # names not in construction order; the Scene sorts them
    for k, c in enumerate(order):
        cams[c].image_name = names[k]
    srt = sorted(range(len(cams)), key=lambda c: cams[c].image_name)
    return xyz, [cams[c] for c in srt], depths[srt], np.array([exact[c] for c in srt])


def main():
    sys.meta_path.insert(0, _Stubs())
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.dirname(HERE))
    import depthsample_ref as R
    torch.set_num_threads(1)
    sys.modules["tqdm"].tqdm = lambda x, *a, **k: x
    import builtins
    real_print = builtins.print
    builtins.print = lambda *a, **k: None
    try:
        import depth_SAM as DS
    finally:
        builtins.print = real_print
    DS.tqdm = lambda x, *a, **k: x
    DS.print = lambda *a, **k: None

    rng = np.random.default_rng(7)
    out = {}
    branches = {"behind": 0, "outside": 0, "occluded": 0, "visible": 0, "zero_depth": 0, "collision": 0,
                "half_even": 0, "tie_equal": 0, "u_w_minus_half": 0}
    real = dict(tensor=torch.tensor, to=torch.Tensor.to, listdir=os.listdir, load=np.load, save=np.save)
    for sname, (w, h) in (("even", (64, 48)), ("odd", (63, 47))):
        xyz, cams, depths, exact = build_scene(rng, w, h, 3000)
        files = {os.path.join(DEPTH_DIR, f"{c.image_name}_depth.npy"): depths[k] for k, c in enumerate(cams)}
        rec = {"pi": [], "saved": {}, "spd": None}

        class FakeGaussians:
            def __init__(self, sh_degree):
                self.get_xyz = torch.from_numpy(xyz.copy())

        class FakeScene:
            def __init__(self, args, gaussians, load_iteration=None, shuffle=True):
                pass

            def getTrainCameras(self, scale=1.0):
                return sorted(cams, key=lambda c: c.image_name)

        def tensor(*a, **k):
            k.pop("device", None)
            return real["tensor"](*a, **k)

        def to(self, *a, **k):
            if (a and str(a[0]).startswith("cuda")) or str(k.get("device", "")).startswith("cuda"):
                return self
            return real["to"](self, *a, **k)

        real_poi, real_spd = DS.process_one_image, DS.save_pcd_depth

        def poi(gs_pcd, w2c_RT, K, depth_map):
            rec["pi"].append((w2c_RT.numpy().copy(), K.numpy().copy(), depth_map.numpy().copy()))
            return real_poi(gs_pcd, w2c_RT, K, depth_map)

        def spd(pcd_depth, mask, mapping, cam_list, save_path, save_path_pcd=None):
            rec["spd"] = (pcd_depth.numpy().copy(), mask.numpy().copy(), mapping.numpy().copy(), [c.image_name for c in cam_list])
            return real_spd(pcd_depth, mask, mapping, cam_list, save_path, save_path_pcd)

        DS.GaussianModel, DS.Scene, DS.process_one_image, DS.save_pcd_depth = FakeGaussians, FakeScene, poi, spd
        torch.tensor, torch.Tensor.to = tensor, to
        DS.os.listdir = lambda p: [os.path.basename(f) for f in files] if p == DEPTH_DIR else real["listdir"](p)
        DS.np.load = lambda p, *a, **k: files[p].copy() if p in files else real["load"](p, *a, **k)
        DS.np.save = lambda p, arr, *a, **k: rec["saved"].__setitem__(p, np.array(arr))
        DS.os.makedirs = lambda *a, **k: None
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                DS.main(types.SimpleNamespace(model_path="/depthsample-golden", source_path="/depthsample-golden-src",
                                              sh_degree=3), 30000, 1.0)
        finally:
            torch.tensor, torch.Tensor.to = real["tensor"], real["to"]
            DS.os.listdir, DS.np.load, DS.np.save = real["listdir"], real["load"], real["save"]
            DS.os.makedirs = os.makedirs
            DS.process_one_image, DS.save_pcd_depth = real_poi, real_spd
        C = len(cams)
        viewmats = np.stack([r[0] for r in rec["pi"]]).astype(np.float32)
        Ks = np.stack([r[1] for r in rec["pi"]]).astype(np.float32)
        assert np.array_equal(np.stack([r[2] for r in rec["pi"]]), depths)
        md, vis, mapping, names = rec["spd"]
        assert names == [c.image_name for c in cams]
        samples = np.stack([rec["saved"][os.path.join("/depthsample-golden-src", "depths_sample", f"{nm}_depth_sample.npy")]
                            for nm in names])
        assert samples.dtype == np.float32 and md.dtype == np.float32 and mapping.dtype == np.int32 and vis.dtype == bool

        ref = R.depth_sample(xyz, viewmats, Ks, depths)
        assert np.array_equal(ref["visible"], vis), (ref["visible"] != vis).sum()
        assert np.array_equal(ref["mapping"], mapping)
        assert np.array_equal(ref["min_depth"], md)
        assert np.array_equal(ref["samples"], samples), "the reference's samples differ from the highest-index rule"

        # branches, in bulk
        for c in range(C):
            u, v, zc = R.project64(xyz, viewmats[c], Ks[c])
            with np.errstate(invalid="ignore"):
                ins = (np.rint(u) >= 0) & (np.rint(u) < w) & (np.rint(v) >= 0) & (np.rint(v) < h)
            branches["behind"] += int((zc <= 0).sum())
            branches["outside"] += int((~ins & (zc > 0)).sum())
            branches["occluded"] += int((ins & ~vis[:, c] & (zc > 0)).sum())
            branches["visible"] += int(vis[:, c].sum())
            dv = R.decide(xyz, viewmats[c], Ks[c], depths[c])
            branches["zero_depth"] += int((ins & (dv[3] == 0)).sum())
            pix = mapping[vis[:, c], c, 0].astype(np.int64) * w + mapping[vis[:, c], c, 1]
            branches["collision"] += int(len(pix) - len(np.unique(pix)))
            if exact[c]:
                x32 = R.decide(xyz, viewmats[c], Ks[c], depths[c])
                uu = (((viewmats[c][0, 0] * xyz[:, 0] + viewmats[c][0, 1] * xyz[:, 1]) + viewmats[c][0, 2] * xyz[:, 2])
                      + viewmats[c][0, 3]) * Ks[c][0, 0]
                zz = ((viewmats[c][2, 0] * xyz[:, 0] + viewmats[c][2, 1] * xyz[:, 1]) + viewmats[c][2, 2] * xyz[:, 2]) + viewmats[c][2, 3]
                with np.errstate(all="ignore"):
                    u32 = uu / zz + Ks[c][0, 2]
                branches["half_even"] += int((u32 - np.floor(u32) == 0.5).sum())
                branches["u_w_minus_half"] += int((u32 == np.float32(w - 0.5)).sum())
                branches["tie_equal"] += int((x32[0] & (np.abs(x32[3] - zz) == np.float32(0.25) * x32[3])).sum())
        out.update({f"{sname}_xyz": xyz, f"{sname}_viewmats": viewmats, f"{sname}_Ks": Ks, f"{sname}_depths": depths,
                    f"{sname}_exact": exact, f"{sname}_names": np.array(names), f"{sname}_mapping": mapping,
                    f"{sname}_visible": vis, f"{sname}_min_depth": md, f"{sname}_samples": samples})
    assert all(v >= 20 for v in branches.values()), branches
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes; branches", branches)


if __name__ == "__main__":
    main()
