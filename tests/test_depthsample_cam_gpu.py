"""N22 on the GPU: the min-depth mapping under camera models (gags_amd/depthsample.py, csrc/depthsample.hip, include/gags_next.h
"N22").  All-pinhole rigs through the new entries against the N6 entries, ortho against the float32 restatement bit for bit,
the fisheye (plain and with coefficient sets A, B, C) against the float64 decision outside the band
(tests/depthsample_cam_ref.py), mixed rigs, the 64-camera chunk, collisions, a side stream behind late producers, and
depth_sample_scene / prompt_scene end to end on fisheye cameras."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import depthsample_cam_ref as C  # noqa: E402

F = np.float32
KEYS = ("mapping", "visible", "min_depth", "samples")


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(xyz, vm, K, D, models=None, block=None, vis_thresh=0.25, cut_bound=0):
    """Every output of the package as device tensors: mapping, visible, min_depth, samples."""
    from gags_amd import depthsample as DS
    x, v, k, d = (t if torch.is_tensor(t) else dev(t) for t in (xyz, vm, K, D))
    kw = {} if models is None else dict(camera_models=models, radial_coeffs=block if torch.is_tensor(block) else dev(block))
    mapping, visible = DS.point_pixel_mapping(x, v, k, d, vis_thresh, cut_bound, **kw)
    samples, md = DS.depth_samples(x, v, k, d, vis_thresh, cut_bound, return_min_depth=True, **kw)
    assert torch.equal(md, DS.point_min_depth(x, v, k, d, vis_thresh, cut_bound, **kw))
    return {"mapping": mapping, "visible": visible, "min_depth": md, "samples": samples}


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def assert_same(got, want, what=""):
    for key in KEYS:
        assert got[key].dtype == want[key].dtype, (what, key)
        assert np.array_equal(got[key], want[key]), (what, key, int((got[key] != want[key]).sum()))


def entries(lib, new, xyz, vm, K, D, ids, block, vis_thresh, cut):
    """The C entries called directly: the N6 pair (new False) or the rig pair with cam_models = ids and radial_coeffs = block."""
    from gags_amd import _lib
    from gags_amd._lib import check, ptr
    n, (c, h, w) = xyz.shape[0], D.shape
    md = torch.empty(n, device="cuda")
    mapping = torch.empty(n, c, 2, dtype=torch.int32, device="cuda")
    visible = torch.empty(n, c, dtype=torch.uint8, device="cuda")
    samples = torch.empty(c, h, w, device="cuda")
    nb = (lib.gags_rig_depth_scratch_bytes if new else lib.gags_depthsample_scratch_bytes)(n, c, h, w)
    scratch = _lib.scratch(nb, xyz.device)
    head = (n, c, h, w, ptr(xyz), ptr(vm), ptr(K)) + ((ids, ptr(block)) if new else ()) + (ptr(D), vis_thresh, cut)
    fm, fs = (lib.gags_rig_depth_map, lib.gags_rig_depth_scatter) if new else (lib.gags_depthsample_map, lib.gags_depthsample_scatter)
    check(fm(*head, ptr(md), ptr(mapping), ptr(visible), ptr(scratch), nb, _lib.stream()), "map")
    check(fs(*head, ptr(md), ptr(samples), ptr(scratch), nb, _lib.stream()), "scatter")
    return {"mapping": mapping, "visible": visible, "min_depth": md, "samples": samples}


def five_cameras(w, h, models, coeffs, n=3000, seed=90):
    """A rig of len(models) cameras over the cone of points: xyz, viewmats, Ks, depths, the coefficient block."""
    xyz, vms = C.scene(w, h, seed, n, n_cams=len(models))
    Ks = np.stack([C.intrinsics(m, w, h) for m in models])
    depths = C.depth_maps(xyz, vms, Ks, models, coeffs, w, h, seed)
    block = np.stack([C.coeffs32(c) for c in coeffs])
    return xyz, vms, Ks, depths, block


def scatter_one(x, vm, K, D, kb, models, c, min_depth):
    """gags_rig_depth_scatter for camera c alone, fed the given min_depth [N]: samples [1, H, W]."""
    from gags_amd import _lib
    from gags_amd._lib import check, ptr
    lib = _lib.load()
    n, (h, w) = x.shape[0], D.shape[1:]
    samples = torch.empty(1, h, w, device="cuda")
    nb = lib.gags_rig_depth_scratch_bytes(n, 1, h, w)
    scratch = _lib.scratch(nb, x.device)
    ids = (ctypes.c_int32 * 1)(C.MODELS[models[c]])
    v1, k1, d1, b1 = vm[c:c + 1].contiguous(), K[c:c + 1].contiguous(), D[c:c + 1].contiguous(), kb[c:c + 1].contiguous()
    check(lib.gags_rig_depth_scatter(n, 1, h, w, ptr(x), ptr(v1), ptr(k1), ids, ptr(b1), ptr(d1), 0.25, 0, ptr(min_depth),
                                     ptr(samples), ptr(scratch), nb, _lib.stream()), "scatter")
    return samples


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cams", [1, 5])
@pytest.mark.parametrize("cut", [0, 3])
def test_all_pinhole_rigs_equal_the_n6_entries(n_cams, cut):
    """cam_models NULL and all zeros, with and without a coefficient block (which no pinhole camera reads): torch.equal to
    gags_depthsample_map / _scatter in all four outputs."""
    from gags_amd import _lib
    lib = _lib.load()
    xyz, vms, Ks, depths, _ = five_cameras(64, 48, ["pinhole"] * n_cams, [None] * n_cams)
    vm, K, D = dev(vms), dev(Ks), dev(depths)
    zeros = (ctypes.c_int32 * n_cams)(*([0] * n_cams))
    junk = torch.full((n_cams, 4), float("nan"), device="cuda")
    seen = 0
    for n in (0, 1, 255, 256, 257, 3000):
        x = dev(xyz[:n])
        old = entries(lib, False, x, vm, K, D, None, None, 0.25, cut)
        for ids, block in ((None, None), (zeros, None), (zeros, junk), (None, junk)):
            new = entries(lib, True, x, vm, K, D, ids, block, 0.25, cut)
            for key in KEYS:
                assert torch.equal(new[key], old[key]), (n, key, ids is None, block is None)
        seen += int(old["visible"].sum())
        assert n > 0 or not old["samples"].any()
    assert seen > 100


# 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", C.SIZES)
def test_ortho_equals_the_restatement_bit_for_bit(w, h):
    s = C.rig_scene("ortho", w, h)
    for cut in (0, 3):
        want = C.depth_sample(s["xyz"], s["viewmats"], s["Ks"], s["depths"], s["models"], cut_bound=cut)
        assert_same(host(run(s["xyz"], s["viewmats"], s["Ks"], s["depths"], s["models"], cut_bound=cut)), want, f"cut {cut}")
        assert 0.2 < want["visible"].mean() < 0.5
    # N6's edge rows under an axis-aligned ortho camera of 8 px per unit: u = 8 x + W / 2 exactly
    cx, cy = w / 2.0, h / 2.0
    rows = [((k + 0.5 - (cx - int(cx))) / 8, 0.0, z) for z in (1.5, 2.0) for k in range(-4, 4)]          # half-even ties
    rows += [((-0.5 - cx) / 8, 0.0, 2.0), ((w - 0.5 - cx) / 8, 0.0, 2.0), (0.0, (-0.5 - cy) / 8, 2.0), (0.0, (h - 0.5 - cy) / 8, 2.0)]
    rows += [(np.nan, 0.0, 2.0), (0.0, np.nan, 2.0), (0.0, 0.0, np.nan), (np.inf, 0.0, 2.0), (-np.inf, 0.0, 2.0), (0.0, 0.0, np.inf),
             (0.0, 0.0, -np.inf), (1e30, 0.0, 2.0), (0.0, 0.0, 0.0), (0.1, 0.1, -2.0),
             (0.25, 0.25, 2.5), (0.25, -0.25, 1.5), (0.25, 0.5, np.nextafter(F(2.5), F(3))), (0.5, -0.25, np.nextafter(F(1.5), F(0)))]
    near = [F(0.01), np.nextafter(F(0.01), F(0)), np.nextafter(F(0.01), F(1))]                             # zc at, below, above 0.01
    rows += [((5 - cx) / 8, (5 - cy) / 8, z) for z in near]
    xyz = np.array(rows, F)
    vm = np.stack([np.eye(4, dtype=F)] * 2)
    vm[1, :3, 3] = (0.125, -0.25, 0.5)
    K = np.stack([np.array([[8, 0, cx], [0, 8, cy], [0, 0, 1]], F), np.array([[10, 0, cx], [0, 10, cy], [0, 0, 1]], F)])
    D0 = np.full((h, w), 2.0, F)
    D0[:, : w // 4] = 1.5
    D0[h // 2, 3 * w // 4] = np.nan      # a NaN depth
    D0[0, :] = 0.0                       # a zero row
    D0[5, 5] = 0.01
    D = np.stack([D0, np.full((h, w), 2.5, F)])
    models = ["ortho", "ortho"]
    for cut in (0, 3):
        want = C.depth_sample(xyz, vm, K, D, models, cut_bound=cut)
        assert_same(host(run(xyz, vm, K, D, models, cut_bound=cut)), want, f"edges, cut {cut}")
        assert want["visible"].any() and not want["visible"].all()
    want = C.depth_sample(xyz, vm, K, D, models)
    assert list(want["visible"][-3:, 0]) == [True, False, True]      # the near plane decides, with an agreeing depth at the pixel
    u = xyz[:16, 0] * F(8) + F(cx)
    assert (u - np.floor(u) == 0.5).all()


# 3 ------------------------------------------------------------------------------------------------------------------------------
def check_against_float64(got, ref, what):
    """Outside the band visible and mapping are exact; min_depth for points with no camera in the band; samples at pixels no
    band point can land on."""
    band = ref["band"]
    assert band.mean() <= 0.02, what
    assert np.array_equal(got["visible"][~band], ref["visible"][~band]), what
    assert np.array_equal(got["mapping"][~band], ref["mapping"][~band]), what
    assert np.array_equal(got["min_depth"][ref["sure_points"]], ref["min_depth"][ref["sure_points"]]), what
    assert np.array_equal(got["samples"][ref["sure_pixels"]], ref["samples"][ref["sure_pixels"]]), what
    assert ref["sure_points"].mean() > 0.9 and ref["sure_pixels"].mean() > 0.9


@pytest.mark.parametrize("name", ["fisheye", "A", "B", "C"])
@pytest.mark.parametrize("w,h", C.SIZES)
def test_fisheye_against_the_float64_decision(name, w, h):
    s, ref = C.rig_scene(name, w, h), C.reference64(name, w, h)
    got = host(run(s["xyz"], s["viewmats"], s["Ks"], s["depths"], s["models"], s["coeff_block"]))
    check_against_float64(got, ref, (name, w, h))
    assert 0.2 < got["visible"].mean() < 0.5
    if name == "fisheye":   # zero coefficients are the plain fisheye, bit for bit
        zero = host(run(s["xyz"], s["viewmats"], s["Ks"], s["depths"], s["models"], np.zeros((3, 4), F)))
        assert_same(zero, got, "zero coefficients")
    if name == "C":         # the fold culls some points and keeps others
        folded = kept = 0
        for k in range(3):
            _, _, zc, dP = C.project64(s["xyz"], s["viewmats"][k], s["Ks"][k], "fisheye", "C")
            sure = ~ref["band"][:, k]
            assert not got["visible"][sure & (dP <= 0), k].any()
            folded += int((sure & (dP <= 0) & (zc >= 0.01)).sum())
            kept += int(got["visible"][:, k].sum())
        assert folded > 500 and kept > 500
        # the same scene without the cull would see points past the fold: the plain fisheye does
        plain = host(run(s["xyz"], s["viewmats"], s["Ks"], s["depths"], s["models"], None))
        assert not np.array_equal(plain["visible"], got["visible"])


# 4 ------------------------------------------------------------------------------------------------------------------------------
MIXED = (["pinhole", "ortho", "fisheye", "fisheye", "fisheye"], [None, None, None, "A", "C"])


@pytest.mark.parametrize("w,h", C.SIZES)
def test_mixed_rig_equals_its_cameras_one_by_one(w, h):
    models, coeffs = MIXED
    xyz, vms, Ks, depths, block = five_cameras(w, h, models, coeffs)
    x, vm, K, D, kb = dev(xyz), dev(vms), dev(Ks), dev(depths), dev(block)
    whole = run(x, vm, K, D, models, kb)
    md = torch.full_like(whole["min_depth"], float("inf"))
    for c in range(5):
        one = run(x, vm[c:c + 1], K[c:c + 1], D[c:c + 1], models[c:c + 1], kb[c:c + 1] if models[c] == "fisheye" else None)
        assert torch.equal(whole["mapping"][:, c], one["mapping"][:, 0]), c
        assert torch.equal(whole["visible"][:, c], one["visible"][:, 0]), c
        assert one["visible"].float().mean() > 0.05, c
        md = torch.minimum(md, one["min_depth"])
        # the sample map: the one-camera scatter of the rig's min depths (a map holds min_depth[winner], the min over ALL cameras)
        assert torch.equal(whole["samples"][c:c + 1], scatter_one(x, vm, K, D, kb, models, c, whole["min_depth"])), c
        assert torch.equal(whole["samples"][c] > 0, one["samples"][0] > 0), c
    assert torch.equal(whole["min_depth"], md)
    # the pinhole and ortho columns are the restatement's, bit for bit
    ref = C.depth_sample(xyz, vms, Ks, depths, models, coeffs)
    vis, mp = whole["visible"].cpu().numpy(), whole["mapping"].cpu().numpy()
    for c in (0, 1):
        assert np.array_equal(vis[:, c], ref["visible"][:, c]) and np.array_equal(mp[:, c], ref["mapping"][:, c]), c


# 5 ------------------------------------------------------------------------------------------------------------------------------
def test_65_cameras_cross_the_chunk():
    """64 cameras per launch: the ids and coefficients of the second chunk (camera 64, a fisheye with set A) and min_depth
    carried across the chunks."""
    w, h, n_cams = 8, 6, 65
    pattern = ["pinhole", "fisheye", "ortho"]
    models = [pattern[c % 3] for c in range(n_cams)]
    coeffs = [("A" if c % 2 == 0 else "B") if models[c] == "fisheye" else None for c in range(n_cams)]
    assert models[64] == "fisheye" and coeffs[64] == "A"
    focal = {"pinhole": 4.0, "ortho": 1.1, "fisheye": 3.0}
    xyz, vms = C.scene(w, h, 91, 2000, n_cams=n_cams)
    Ks = np.stack([np.array([[focal[m], 0, w / 2], [0, focal[m], h / 2], [0, 0, 1]], F) for m in models])
    depths = C.depth_maps(xyz, vms, Ks, models, coeffs, w, h, 91)
    block = np.stack([C.coeffs32(c) for c in coeffs])
    x, vm, K, D, kb = dev(xyz), dev(vms), dev(Ks), dev(depths), dev(block)
    whole = run(x, vm, K, D, models, kb)
    a = run(x, vm[:64], K[:64], D[:64], models[:64], kb[:64])
    b = run(x, vm[64:], K[64:], D[64:], models[64:], kb[64:])
    assert torch.equal(whole["mapping"], torch.cat([a["mapping"], b["mapping"]], 1))
    assert torch.equal(whole["visible"], torch.cat([a["visible"], b["visible"]], 1))
    assert torch.equal(whole["min_depth"], torch.minimum(a["min_depth"], b["min_depth"]))
    assert (b["min_depth"] < a["min_depth"]).any() and (a["min_depth"] < b["min_depth"]).any()
    assert torch.equal(whole["samples"] > 0, torch.cat([a["samples"], b["samples"]]) > 0)
    vis, mp, mdh = whole["visible"].cpu().numpy(), whole["mapping"].cpu().numpy(), whole["min_depth"].cpu().numpy()
    for c in (0, 63, 64):
        winner = np.full(h * w, -1, np.int64)
        idx = np.nonzero(vis[:, c])[0]
        np.maximum.at(winner, mp[idx, c, 0].astype(np.int64) * w + mp[idx, c, 1], idx)
        assert np.array_equal(whole["samples"][c].cpu().numpy(), np.where(winner >= 0, mdh[np.maximum(winner, 0)], F(0)).reshape(h, w))
    assert b["visible"].any() and not b["visible"].all()
    # camera 64 read ITS coefficients: without them, or with another camera's, it sees other points
    for other in (None, kb[61:62]):
        assert models[61] == "fisheye" and coeffs[61] == "B"
        assert not torch.equal(run(x, vm[64:], K[64:], D[64:], models[64:], other)["mapping"], b["mapping"])
    # the pinhole and ortho columns of both chunks are the restatement's
    ref = C.depth_sample(xyz, vms, Ks, depths, models, coeffs)
    exact = [c for c in range(n_cams) if models[c] != "fisheye"]
    assert np.array_equal(vis[:, exact], ref["visible"][:, exact]) and np.array_equal(mp[:, exact], ref["mapping"][:, exact])


# 6 ------------------------------------------------------------------------------------------------------------------------------
def test_collisions_under_a_fisheye_highest_index_wins_and_runs_are_bitwise_equal():
    rng = np.random.default_rng(3)
    n, w, h = 60_000, 33, 21
    xyz = np.stack([rng.uniform(-0.9, 0.9, n), rng.uniform(-0.6, 0.6, n), rng.uniform(2.0, 2.4, n)], 1).astype(F)
    vm = np.stack([np.eye(4, dtype=F)] * 2)
    vm[1, :3, 3] = (0.01, 0.02, 0.1)
    K = np.stack([np.array([[36, 0, w / 2], [0, 36, h / 2], [0, 0, 1]], F), np.array([[33, 0, w / 2], [0, 33, h / 2], [0, 0, 1]], F)])
    D = np.stack([np.full((h, w), 2.1, F), np.full((h, w), 2.0, F)])
    models, block = ["fisheye", "fisheye"], np.stack([C.coeffs32("A"), C.coeffs32(None)])
    a, b = host(run(xyz, vm, K, D, models, block)), host(run(xyz, vm, K, D, models, block))
    for key in KEYS:
        assert np.array_equal(a[key], b[key]), key
    for c in range(2):
        idx = np.nonzero(a["visible"][:, c])[0]
        px = a["mapping"][idx, c, 0].astype(np.int64) * w + a["mapping"][idx, c, 1]
        assert np.bincount(px).max() > 50
        winner = np.full(h * w, -1, np.int64)
        np.maximum.at(winner, px, idx)
        want = np.where(winner >= 0, a["min_depth"][np.maximum(winner, 0)], F(0)).reshape(h, w)
        assert np.array_equal(a["samples"][c], want), c


# 7 ------------------------------------------------------------------------------------------------------------------------------
def test_mixed_rig_on_a_side_stream_behind_late_producers():
    """The general path receives the stream: behind late producers on a side stream the mixed rig gives the bits of the null
    stream (the inputs hold another scene until the delayed copies land), and every streamed entry got the stream's handle."""
    import stream_harness as SH
    models, coeffs = MIXED
    real = dict(zip("xvkdb", five_cameras(64, 48, models, coeffs, n=700, seed=92)))
    decoy = dict(zip("xvkdb", five_cameras(64, 48, models, coeffs, n=700, seed=93)))
    want = run(real["x"], real["v"], real["k"], real["d"], models, real["b"])
    wrong = run(decoy["x"], decoy["v"], decoy["k"], decoy["d"], models, decoy["b"])
    assert not torch.equal(want["mapping"], wrong["mapping"])
    src = {k: dev(v) for k, v in real.items()}
    buf = {k: dev(v) for k, v in decoy.items()}
    stage = {k: v.clone() for k, v in buf.items()}
    torch.cuda.synchronize()
    stream = SH.concurrent_stream()
    with torch.cuda.stream(stream), SH.late_producers(stream) as calls:
        for k in stage:
            stage[k].copy_(src[k])
        for k in buf:
            buf[k].copy_(stage[k])
        got = run(buf["x"], buf["v"], buf["k"], buf["d"], models, buf["b"])
        got = {k: v.clone() for k, v in got.items()}
    stream.synchronize()
    torch.cuda.synchronize()
    for key in KEYS:
        assert torch.equal(got[key], want[key]), key
    names = {name for name, _ in calls}
    assert {"gags_rig_depth_map", "gags_rig_depth_scatter"} <= names and not any("depthsample" in nm for nm in names)
    assert SH.audit_streams(calls, stream) == []


# 8 ------------------------------------------------------------------------------------------------------------------------------
def scene_cameras():
    from gags_amd import synthetic as syn
    from gags_amd.scene import Camera
    w, h = 64, 48
    cams = []
    for k, kc in enumerate([C.COEFFS["zero"], C.COEFFS["A"], None, C.COEFFS["B"]]):
        if kc is None:
            cams.append(syn.make_camera(w, h, view=k, n_views=4))
            continue
        yaw = np.radians((k - 1.5) * 5.0)
        R = np.array([[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]])
        cams.append(Camera.from_opencv_fisheye((40.0, 40.0, w / 2, h / 2) + tuple(kc), R, np.zeros(3), w, h, uid=k))
    return cams, ["fisheye", "fisheye", "pinhole", "fisheye"]


def test_scene_end_to_end_on_fisheye_cameras():
    from gags_amd import depthsample as DS, prompts as PR, synthetic as syn
    from gags_amd.gaussian_renderer import render
    w, h = 64, 48
    model = syn.make_model(4000, 0, w, h, seed=1, device="cuda", scale0=syn.SCALE0 * 12)
    cams, models = scene_cameras()
    bg = torch.zeros(3, device="cuda")
    res = DS.depth_sample_scene(model, cams, return_mapping=True)
    for c, cam in enumerate(cams):
        assert torch.equal(res["depths"][c], render(cam, model, None, bg, feature_mode=False, render_mode="RGB+ED")["render"][3]), c
    vm, K, names, block, hw = DS.camera_rig(cams)
    assert names == models and hw == (h, w) and block.shape == (4, 4)
    ref = C.depth_sample64(model.get_xyz.cpu().numpy(), vm.cpu().numpy(), K.cpu().numpy(), res["depths"].cpu().numpy(), models,
                           [tuple(r) for r in block.cpu().numpy()])
    got = host({k: res[k] for k in KEYS})
    check_against_float64(got, ref, "scene")
    assert all(got["visible"][:, c].sum() > 50 for c in range(4)) and (got["samples"] > 0).any()
    for mode in ("depth", "mindepth", "pcd"):
        out = PR.prompt_scene(model, cams, mode, n_per_side=6, pcd_fraction=0.1, rng=random.Random(0))
        assert len(out["point_grids"]) == 4
        for layers in out["point_grids"]:
            for p in layers:
                p = p.cpu().numpy() if torch.is_tensor(p) else np.asarray(p)
                assert p.ndim == 2 and p.shape[1] == 2 and (p >= 0).all() and (p <= 1).all(), mode
                assert len(p) > 0 or mode == "pcd"
        assert sum(len(p) for layers in out["point_grids"] for p in layers) > 0
    # the same calls on an all-pinhole rig: the N6 functions fed from camera_matrices, bit for bit
    pin = [syn.make_camera(w, h, view=k, n_views=4) for k in range(4)]
    res = DS.depth_sample_scene(model, pin, return_mapping=True)
    vm, K, _ = DS.camera_matrices(pin)
    xyz = model.get_xyz
    assert torch.equal(res["depths"], DS.render_depths(model, pin, bg))
    mapping, visible = DS.point_pixel_mapping(xyz, vm, K, res["depths"])
    samples, md = DS.depth_samples(xyz, vm, K, res["depths"], return_min_depth=True)
    for a, b in ((res["mapping"], mapping), (res["visible"], visible), (res["samples"], samples), (res["min_depth"], md)):
        assert torch.equal(a, b)
    assert visible.any()
    grids = PR.prompt_scene(model, pin, "mindepth", n_per_side=6, rng=random.Random(5))["point_grids"]
    direct = PR.mindepth_point_grids(res["depths"], samples, 6, 0, 1, 4, random.Random(5))
    for g, (p, _) in zip(grids, direct):
        assert len(g) == len(p) and all(np.array_equal(x, y) for x, y in zip(g, p))
