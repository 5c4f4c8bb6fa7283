"""N6 on the GPU: depth_SAM's point-to-pixel min-depth mapping (gags_amd/depthsample.py, csrc/depthsample.hip) against the
reference's own depth_SAM.main (tests/golden/depthsample_vectors.npz) and against the float32 restatement
tests/depthsample_ref.py at the edges, at 1.5 M Gaussians x 16 cameras of 1080p and past 2^31 dense elements."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import depthsample_ref as R  # noqa: E402

Z = np.load(os.path.join(HERE, "golden", "depthsample_vectors.npz"))
F = np.float32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(xyz, vm, K, D, vis_thresh=0.25, cut_bound=0):
    """Every GPU output as numpy: mapping, visible, min_depth, samples."""
    from gags_amd import depthsample as DS
    x, v, k, d = dev(xyz), dev(vm), dev(K), dev(D)
    mapping, visible = DS.point_pixel_mapping(x, v, k, d, vis_thresh, cut_bound)
    samples, md = DS.depth_samples(x, v, k, d, vis_thresh, cut_bound, return_min_depth=True)
    md2 = DS.point_min_depth(x, v, k, d, vis_thresh, cut_bound)
    assert torch.equal(md, md2)
    return {"mapping": mapping.cpu().numpy(), "visible": visible.cpu().numpy(), "min_depth": md.cpu().numpy(),
            "samples": samples.cpu().numpy()}


def assert_same(got, want, what=""):
    for key in ("mapping", "visible", "min_depth", "samples"):
        assert got[key].dtype == want[key].dtype, (what, key)
        assert np.array_equal(got[key], want[key]), (what, key, int((got[key] != want[key]).sum()))


def axis_camera(tx=0.0, ty=0.0, tz=0.0, f=32.0, w=64, h=48, cx=None, cy=None):
    vm = np.eye(4, dtype=F)
    vm[:3, 3] = (tx, ty, tz)
    K = np.array([[f, 0, w / 2.0 if cx is None else cx], [0, f, h / 2.0 if cy is None else cy], [0, 0, 1]], F)
    return vm, K


@pytest.mark.parametrize("scene", ["even", "odd"])
def test_fixture_bit_exact(scene):
    got = run(Z[f"{scene}_xyz"], Z[f"{scene}_viewmats"], Z[f"{scene}_Ks"], Z[f"{scene}_depths"])
    want = {k: Z[f"{scene}_{k}"] for k in ("mapping", "visible", "min_depth", "samples")}
    assert_same(got, want, scene)
    assert np.isinf(got["min_depth"]).any()


@pytest.mark.parametrize("w,h", [(64, 48), (63, 47)])
def test_edges_against_the_restatement(w, h):
    rows = []
    for z in (1.5, 2.0, 2.5, 3.0):  # half-even ties: x = 0 at odd W is u = W / 2; x fx / z = k gives u = k + W / 2
        for k in range(-3, 4):
            rows.append((k * z / 32, 0.0, z))
    rows += [((w / 2 - 0.5) * 2 / 32, 0.0, 2.0), (-(w / 2 + 0.5) * 2 / 32, 0.0, 2.0),   # u = W - 0.5, u = -0.5
             (0.0, (h / 2 - 0.5) * 2 / 32, 2.0), (0.0, -(h / 2 + 0.5) * 2 / 32, 2.0)]
    rows += [(0.0, 0.0, 0.0), (0.5, 0.5, 0.0), (0.1, 0.1, -2.0), (0.0, 0.0, -1.0),         # zc = 0, zc < 0
             (np.nan, 0.0, 2.0), (0.0, np.nan, 2.0), (0.0, 0.0, np.nan), (np.inf, 0.0, 2.0), (0.0, 0.0, np.inf),
             (1.0, 0.0, 1e-9), (-1.0, 0.0, 1e-9), (0.0, 1.0, 1e-9),                           # |u| > 2^31
             (0.25, 0.25, 2.5), (0.25, -0.25, 1.5),                                         # |d - zc| = 0.25 d, d = 2
             (0.25, 0.5, np.nextafter(F(2.5), F(3))), (0.5, -0.25, np.nextafter(F(1.5), F(0)))]
    xyz = np.array(rows, F)
    vm0, K0 = axis_camera(w=w, h=h)
    vm1, K1 = axis_camera(0.125, -0.25, 0.5, f=40.0, w=w, h=h)
    D0 = np.full((h, w), 2.0, F)
    D0[:, : w // 4] = 1.5  # a band where the z = 1.5 points agree
    D0[h // 2, 3 * w // 4] = np.nan  # a NaN depth
    D0[0, :] = 0.0
    D1 = np.full((h, w), 2.5, F)
    vm, K, D = np.stack([vm0, vm1]), np.stack([K0, K1]), np.stack([D0, D1])
    for cut in (0, 3):
        want = R.depth_sample(xyz, vm, K, D, cut_bound=cut)
        assert_same(run(xyz, vm, K, D, cut_bound=cut), want, f"cut {cut}")
        assert want["visible"].any() and not want["visible"].all()
    # the ties occur: u = k + 0.5 exactly, and the occlusion test at equality on both sides
    with np.errstate(all="ignore"):
        u = (xyz[:, 0] * F(32)) / xyz[:, 2] + F(w / 2)
        assert (u - np.floor(u) == 0.5).sum() >= 4 or w % 2 == 0
    dd = np.abs(F(2.0) - xyz[:, 2])
    assert ((dd == F(0.25) * F(2.0)) & (xyz[:, 2] > 2)).any() and ((dd == F(0.5)) & (xyz[:, 2] < 2)).any()


def test_empty_single_camera_and_nothing_visible():
    from gags_amd import depthsample as DS
    vm, K = axis_camera()
    D = np.zeros((1, 48, 64), F)  # all-zero depth: nothing is visible
    xyz = np.random.default_rng(0).uniform(-1, 1, (500, 3)).astype(F)
    xyz[:, 2] += 3
    got = run(xyz, vm[None], K[None], D)
    assert not got["visible"].any() and (got["mapping"] == 0).all()
    assert np.isposinf(got["min_depth"]).all() and (got["samples"] == 0).all() and got["samples"].shape == (1, 48, 64)
    e = torch.empty(0, 3, device="cuda")
    mp, vis = DS.point_pixel_mapping(e, dev(vm[None]), dev(K[None]), dev(D))
    assert mp.shape == (0, 1, 2) and vis.shape == (0, 1)
    s, md = DS.depth_samples(e, dev(vm[None]), dev(K[None]), dev(D + 1), return_min_depth=True)
    assert md.shape == (0,) and s.shape == (1, 48, 64) and not s.any()


def test_division_is_correctly_rounded():
    """(xc fx) / zc == k + 0.5 exactly for odd, non-power-of-two zc: an approximate division lands a ulp off and rounds to
    the other integer for one parity of k."""
    w = 4096
    zs = np.array([3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23, 25, 27, 29, 31, 33, 99, 127, 255, 1001], F)
    ks = np.arange(0, 2000, dtype=F)
    zc = np.repeat(zs, len(ks))
    xc = zc * (np.tile(ks, len(zs)) + F(0.5))
    assert np.array_equal(xc / zc, np.tile(ks, len(zs)) + F(0.5))
    xyz = np.stack([xc, np.zeros_like(xc), zc], 1)
    vm, K = axis_camera(f=1.0, w=w, h=1, cx=0.0, cy=0.5)
    D = np.ones((1, 1, w), F)
    got = run(xyz, vm[None], K[None], D, vis_thresh=1e30)
    k = np.tile(ks, len(zs)).astype(np.int64)
    want_u = np.where(k % 2 == 0, k, k + 1)  # half to even
    assert got["visible"].all()
    assert np.array_equal(got["mapping"][:, 0, 1], want_u)
    assert_same(got, R.depth_sample(xyz, vm[None], K[None], D, vis_thresh=1e30))


def test_collisions_highest_index_wins_and_runs_are_bitwise_equal():
    rng = np.random.default_rng(3)
    n = 200_000
    xyz = np.stack([rng.uniform(-0.3, 0.3, n), rng.uniform(-0.2, 0.2, n), rng.uniform(2.0, 2.4, n)], 1).astype(F)
    vm, K = axis_camera(w=33, h=21)  # ~300 points per pixel
    vm2, K2 = axis_camera(0.01, 0.02, 0.1, f=30.0, w=33, h=21)
    D = np.stack([np.full((21, 33), 2.1, F), np.full((21, 33), 2.0, F)])
    vmm, KK = np.stack([vm, vm2]), np.stack([K, K2])
    a, b = run(xyz, vmm, KK, D), run(xyz, vmm, KK, D)
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    want = R.depth_sample(xyz, vmm, KK, D)
    assert_same(a, want, "collisions")
    per_pixel = np.bincount(want["mapping"][want["visible"][:, 0], 0, 0] * 33 + want["mapping"][want["visible"][:, 0], 0, 1])
    assert per_pixel.max() > 100


def test_scale_rendered_depths_1080p():
    """1.5 M Gaussians x 16 cameras at 1920 x 1080 with depths rendered by the project: every decision, min depth and (on
    four cameras) sample map equals the restatement; decisions that differ from a float64 projection all lie in the band
    and are below 1e-4 of all decisions."""
    from gags_amd import depthsample as DS
    from gags_amd import synthetic as syn
    model = syn.make_model(1_500_000, 0, 1920, 1080, seed=0, device="cuda", gen_device="cuda")
    cams = [syn.make_camera(1920, 1080, view=k, n_views=16) for k in range(16)]
    depths = DS.render_depths(model, cams, torch.zeros(3, device="cuda"))
    vm, K, hw = DS.camera_matrices(cams)
    assert hw == (1080, 1920)
    xyz = model.get_xyz.contiguous()
    mapping, visible = DS.point_pixel_mapping(xyz, vm, K, depths)
    pick = [0, 5, 10, 15]
    samples, md = DS.depth_samples(xyz, vm, K, depths, return_min_depth=True)
    X, VM, KK, D = (t.cpu().numpy() for t in (xyz, vm, K, depths))
    mapping, visible, md, samples = mapping.cpu().numpy(), visible.cpu().numpy(), md.cpu().numpy(), samples[pick].cpu().numpy()
    want = R.depth_sample(X, VM, KK, D, cams=pick)
    assert np.array_equal(visible, want["visible"])
    assert np.array_equal(mapping, want["mapping"])
    assert np.array_equal(md, want["min_depth"])
    assert np.array_equal(samples, want["samples"])
    assert 0.01 < visible.mean() < 0.99  # (the ED render hides most centres: ~4 % of the decisions are visible)
    diff = total = 0
    for c in range(16):
        vis64, v64, u64, band = R.decide64(X, VM[c], KK[c], D[c])
        d = (vis64 != visible[:, c]) | (vis64 & ((v64 != mapping[:, c, 0]) | (u64 != mapping[:, c, 1])))
        assert band[d].all(), c
        diff += int(d.sum())
        total += len(d)
    assert diff < 1e-4 * total, (diff, total)


def test_dense_offsets_past_2_31():
    """mapping [N, C, 2] with N C 2 > 2^31 int32 elements (4.2 M x 256 cameras of 32 x 32): rows sampled over the whole
    range, the last rows and the last cameras included, equal the restatement."""
    from gags_amd import depthsample as DS
    n, c, w, h = 4_200_000, 256, 32, 32
    assert n * c * 2 > 2 ** 31
    g = torch.Generator(device="cuda").manual_seed(5)
    xyz = torch.rand(n, 3, device="cuda", generator=g) * torch.tensor([2.0, 2.0, 10.0], device="cuda") + \
        torch.tensor([-1.0, -1.0, 2.0], device="cuda")
    yaw = np.linspace(-0.4, 0.4, c)
    vm = np.zeros((c, 4, 4), F)
    vm[:, 0, 0], vm[:, 0, 2], vm[:, 2, 0], vm[:, 2, 2] = np.cos(yaw), -np.sin(yaw), np.sin(yaw), np.cos(yaw)
    vm[:, 1, 1] = vm[:, 3, 3] = 1
    K = np.tile(np.array([[28.8, 0, 16], [0, 28.8, 16], [0, 0, 1]], F), (c, 1, 1))
    D = np.full((c, h, w), 7.0, F)
    D[:, ::3] = 4.0
    mapping, visible = DS.point_pixel_mapping(xyz, dev(vm), dev(K), dev(D), vis_thresh=0.5)
    rows = torch.cat([torch.randint(0, n, (3000,), device="cuda", generator=g), torch.arange(n - 64, n, device="cuda")])
    got_m, got_v = mapping[rows].cpu().numpy(), visible[rows].cpu().numpy()
    del mapping, visible
    want = R.depth_sample(xyz[rows].cpu().numpy(), vm, K, D, vis_thresh=0.5, cams=[])
    assert np.array_equal(got_v, want["visible"])
    assert np.array_equal(got_m, want["mapping"])
    assert want["visible"][-64:, -8:].any() and not want["visible"][-64:, -8:].all()


def test_depth_sample_scene_end_to_end(tmp_path):
    """depth_sample_scene (rendering its own depths) and save_depth_samples, compared file by file with the restatement on
    the same depths."""
    from gags_amd import depthsample as DS
    from gags_amd import synthetic as syn
    model = syn.make_model(20_000, 0, 63, 47, seed=1, device="cuda")
    cams = [syn.make_camera(63, 47, view=k, n_views=4) for k in range(4)]
    names = ["img1", "img10", "img2", "img3"]
    res = DS.depth_sample_scene(model, cams, names=names, return_mapping=True)
    assert torch.equal(res["depths"], DS.render_depths(model, cams, torch.zeros(3, device="cuda")))
    DS.save_depth_samples(str(tmp_path), names, res["samples"], res["min_depth"], res["visible"], res["mapping"])
    vm, K, _ = DS.camera_matrices(cams)
    want = R.depth_sample(model.get_xyz.cpu().numpy(), vm.cpu().numpy(), K.cpu().numpy(), res["depths"].cpu().numpy())
    for k, nm in enumerate(names):
        a = np.load(tmp_path / f"{nm}_depth_sample.npy")
        assert a.dtype == np.float32 and np.array_equal(a, want["samples"][k]), nm
    assert np.array_equal(np.load(tmp_path / "pcd_depth.npy"), want["min_depth"])
    assert np.array_equal(np.load(tmp_path / "pcd_pxl_mask.npy"), want["visible"])
    assert np.array_equal(np.load(tmp_path / "pcd_pxl_mapping.npy"), want["mapping"])
    assert want["visible"].any() and (want["samples"] > 0).any()
    # given depths, read back by name, give the same result
    for k, nm in enumerate(names):
        np.save(tmp_path / f"{nm}_depth.npy", res["depths"][k].cpu().numpy())
    again = DS.depth_sample_scene(model, cams, depths=DS.load_rendered_depths(str(tmp_path), names), names=names)
    assert torch.equal(again["samples"], res["samples"]) and torch.equal(again["min_depth"], res["min_depth"])
