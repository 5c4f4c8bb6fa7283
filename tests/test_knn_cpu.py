"""N9 without a GPU: the restatement of the 3-nearest-neighbour contract (tests/knn_ref.py) against float64 and a hand-checked
answer, the torch part of create_from_pcd, the points3D.ply round trip and nerfpp_norm against the reference's own results
(tests/golden/init_vectors.npz, written by tests/golden/make_golden_init.py), and the argument checks of the new entries.

The float32-against-float64 bound is derived, not measured: 8 x 2^-24 relative.  Each rounded difference carries half an ulp
(2^-24 relative), squaring doubles it (2), the square rounds (1), the two sums round (2), the sum of three and the division by
three round (3): 8 half-ulps to first order.  A k-th order statistic is monotone in its inputs, so the three smallest values
inherit the bound of the distances they are chosen from."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import knn_ref as K  # noqa: E402

Z = np.load(os.path.join(HERE, "golden", "init_vectors.npz"))
CONFIGS = [str(c) for c in Z["configs"]]
F32_BOUND = 8 * 2.0 ** -24
SIZES = {"min4": 4, "min5": 5, "wave63": 63, "wave64": 64, "wave65": 65, "box_m1": K.B - 1, "box": K.B, "box_p1": K.B + 1,
         "box_4p1": 4 * K.B + 1, "uniform": 1025, "lattice": 343, "two_clusters": 1004, "offset": 300, "plane": 200, "line": 100,
         "duplicates": 256, "presorted": 1025, "reversed": 1025}


def _ulps(a, b):
    """Distance in float32 ulps between two float32 arrays of one sign pattern."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def test_cases_are_the_ones_the_kernel_can_go_wrong_on():
    from gags_amd import knn
    assert K.B == knn.BOX
    assert {name: K.cloud(name).shape[0] for name in K.CASES} == SIZES
    for name in K.CASES:
        x = K.cloud(name)
        assert x.dtype == np.float32 and x.shape[1] == 3 and np.isfinite(x).all(), name
    assert np.ptp(K.cloud("plane"), axis=0).tolist().count(0.0) == 1 and np.ptp(K.cloud("line"), axis=0).tolist().count(0.0) == 2
    assert np.array_equal(K.cloud("reversed"), K.cloud("presorted")[::-1]) and (np.diff(K.cloud("presorted")[:, 0]) >= 0).all()
    assert np.array_equal(np.sort(K.cloud("presorted"), axis=0), np.sort(K.cloud("uniform"), axis=0))
    assert (K.expected("duplicates")[0] == 0).all()  # three copies of itself are every point's neighbours
    # the lattice's third neighbour is tied (six at the pitch for an inner point), and exactly the pitch squared
    assert np.count_nonzero(K.expected("lattice")[0] == np.float32(0.0625)) == 343
    # the triple's third neighbour is across the gap, the outlier's neighbours are far
    r = K.expected("two_clusters")[1]
    assert (r[-3:] > 1.0).all() and r[-4] > 1e5 and np.median(r[:500]) < 1e-5


@pytest.mark.parametrize("name", K.CASES)
def test_float32_restatement_is_within_the_derived_bound_of_float64(name):
    r32, r64 = K.expected(name)
    assert r32.dtype == np.float32 and r64.dtype == np.float64
    err = np.abs(r32.astype(np.float64) - r64)
    rel = float((err / np.where(r64 > 0, r64, 1.0)).max())
    print(f"\n{name}: float32 restatement within {rel:.3e} relative of float64 (bound {F32_BOUND:.3e}), smallest value {r64.min():.3e}")
    assert (err <= F32_BOUND * r64).all(), (name, rel)


def test_hand_checked_five_points():
    x = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, 3], [1, 2, 0]], np.float32)
    # squared distances: p0: 1 4 9 5; p1: 1 5 10 4; p2: 4 5 13 1; p3: 9 10 13 14; p4: 5 4 1 14
    want = np.array([10, 10, 10, 32, 10], np.float32) / np.float32(3)
    assert np.array_equal(K.dist2_f32(x), want)
    assert np.allclose(K.dist2_f64(x), np.array([10, 10, 10, 32, 10]) / 3.0, rtol=1e-15)
    # the neighbour is excluded by index, not by position: a duplicate is a neighbour at distance 0
    assert np.array_equal(K.dist2_f32(np.concatenate([x, x[:1]]))[[0, 5]], np.array([5, 5], np.float32) / np.float32(3))


def test_fixture_is_small_and_its_stub_is_the_float64_brute_force():
    assert os.path.getsize(os.path.join(HERE, "golden", "init_vectors.npz")) < 256 * 1024
    assert Z["points"].dtype == np.float32 and Z["points"].shape == (200, 3)
    assert np.array_equal(Z["dist2"], K.dist2_f64(Z["points"]).astype(np.float32))
    assert np.array_equal(np.rint(Z["colors"] * 255) / 255.0, Z["colors"])
    assert CONFIGS == ["sh3", "sh0_speedup", "sh3_sem512"]


@pytest.mark.parametrize("name", CONFIGS)
def test_init_tensors_equal_the_references_create_from_pcd(name):
    from gags_amd import scene
    shd, size, speedup, _ = Z[name + "_par"]
    points = torch.tensor(Z["points"]).float()
    colors = torch.tensor(Z["colors"]).float()
    t = scene._init_tensors(points, colors, torch.tensor(Z["dist2"]), int(shd), int(size), bool(speedup))
    n = points.shape[0]
    for attr, v in t.items():
        if v is not None:
            assert v.dtype == torch.float32 and v.is_contiguous(), attr
    shapes = {"_xyz": (n, 3), "_features_dc": (n, 1, 3), "_features_rest": (n, (int(shd) + 1) ** 2 - 1, 3), "_scaling": (n, 3),
              "_rotation": (n, 4), "_opacity": (n, 1), "max_radii2D": (n,)}
    for attr, shape in shapes.items():
        assert tuple(t[attr].shape) == shape, attr
        assert t[attr].shape == Z[name + ("_max_radii2D" if attr == "max_radii2D" else attr)].shape
    for attr in ("_xyz", "_features_rest", "_rotation", "max_radii2D"):
        assert np.array_equal(t[attr].numpy(), Z[name + ("_max_radii2D" if attr == "max_radii2D" else attr)]), attr
    if size:
        assert np.array_equal(t["_semantic_feature"].numpy(), Z[name + "_semantic_feature"])
        assert t["_semantic_feature"].shape[1] == (16 if speedup else 512)
    else:
        assert t["_semantic_feature"] is None and name + "_semantic_feature" not in Z.files
    assert np.array_equal(t["_features_dc"].numpy(), scene.RGB2SH(colors).numpy()[:, None, :])
    assert _ulps(t["_features_dc"].numpy(), Z[name + "_features_dc"]).max() <= 1
    assert _ulps(t["_opacity"].numpy(), Z[name + "_opacity"]).max() <= 1
    s = Z[name + "_scaling"]
    assert (np.abs(t["_scaling"].numpy() - s) <= 1e-6 + 1e-6 * np.abs(s)).all()
    want = np.log(np.sqrt(np.maximum(Z["dist2"].astype(np.float64), np.float64(np.float32(1e-7)))))
    assert np.allclose(s, np.repeat(want[:, None], 3, axis=1), rtol=1e-6, atol=1e-6)
    assert np.allclose(Z[name + "_opacity"], np.log(0.1 / 0.9), rtol=1e-6) and (Z[name + "_rotation"] == [1, 0, 0, 0]).all()


def test_rgb2sh_and_back_equal_the_references():
    from gags_amd import scene
    x = torch.tensor(Z["rgb2sh_in"])
    assert _ulps(scene.RGB2SH(x).numpy(), Z["rgb2sh_out"]).max() <= 1
    assert _ulps(scene.SH2RGB(x).numpy(), Z["sh2rgb_out"]).max() <= 1
    assert np.array_equal(scene.RGB2SH(Z["colors"]), (Z["colors"] - 0.5) / 0.28209479177387814)  # (numpy in, numpy out)


def test_point_cloud_ply_round_trip(tmp_path):
    from gags_amd import io_formats, scene
    rng = np.random.default_rng(5)
    xyz = (rng.standard_normal((37, 3)) * 100).astype(np.float32)
    rgb = rng.integers(0, 256, (37, 3))
    path = str(tmp_path / "sparse" / "0" / "points3D.ply")
    io_formats.write_point_cloud(path, xyz, rgb)
    raw = open(path, "rb").read()
    header = raw[:raw.index(b"end_header\n")].decode("ascii").splitlines()
    assert header[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 37"]
    props = [ln.split() for ln in header[3:]]
    assert [p[0] for p in props] == ["property"] * 9
    assert [p[2] for p in props] == [str(s) for s in Z["ply_names"]] and [p[1] for p in props] == [str(s) for s in Z["ply_types"]]
    assert len(raw) == raw.index(b"end_header\n") + len(b"end_header\n") + 37 * (6 * 4 + 3)
    pcd = io_formats.read_point_cloud(path)
    assert isinstance(pcd, scene.BasicPointCloud) and pcd._fields == ("points", "colors", "normals")
    assert pcd.points.dtype == np.float32 and np.array_equal(pcd.points, xyz)
    assert np.array_equal(pcd.colors, rgb / 255.0) and np.array_equal(np.rint(pcd.colors * 255), rgb)
    assert pcd.normals.shape == (37, 3) and not pcd.normals.any()
    with pytest.raises(ValueError):
        io_formats.write_point_cloud(path, xyz, rgb[:5])
    # float colours in 0 .. 255 are cast as the reference's assignment to a uchar field casts them
    io_formats.write_point_cloud(path, xyz, rgb + 0.75)
    assert np.array_equal(io_formats.read_point_cloud(path).colors, rgb / 255.0)


def test_nerfpp_norm_equals_the_references():
    from gags_amd import scene
    cams = [scene.Camera(R, T, 1.0, 0.8, 64, 48, device="cpu", uid=i) for i, (R, T) in enumerate(zip(Z["cam_R"], Z["cam_T"]))]
    norm = scene.nerfpp_norm(cams)
    assert sorted(norm) == ["radius", "translate"] and norm["translate"].shape == (3,)
    assert np.allclose(norm["translate"], Z["norm_translate"], rtol=1e-12, atol=1e-12)
    assert np.isclose(norm["radius"], float(Z["norm_radius"]), rtol=1e-12)
    centers = np.stack([-R @ T for R, T in zip(Z["cam_R"], Z["cam_T"])])  # C = -R T for the stored (transposed) R
    far = np.linalg.norm(centers - centers.mean(0), axis=1).max()
    assert np.isclose(norm["radius"], 1.1 * far, rtol=1e-5)  # (getWorld2View2 rounds the pose to float32)


def test_dist2_rejects_what_it_cannot_serve():
    import gags_amd
    from gags_amd import knn
    assert gags_amd.distCUDA2 is knn.dist2 and knn.distCUDA2 is knn.dist2
    with pytest.raises(ValueError):
        knn.dist2(torch.zeros(3, 3))
    with pytest.raises(ValueError):
        knn.dist2(torch.zeros(10, 2))
    with pytest.raises(ValueError):
        knn.dist2(torch.zeros(12))
    with pytest.raises(RuntimeError, match="no CPU path"):
        knn.dist2(torch.zeros(10, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        from gags_amd.scene import BasicPointCloud, GaussianModel
        GaussianModel(3).create_from_pcd(BasicPointCloud(Z["points"], Z["colors"], np.zeros((200, 3))), 1.0, device="cpu")


def test_c_entries_validate_without_launching():
    from gags_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    P = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.gags_abi_version() == 2
    for n in (-1, 0, 3, 1 << 31, 1 << 40):
        assert lib.gags_knn3_dist2_scratch_bytes(n) == 0
        assert lib.gags_knn3_dist2(n, P, P, P, 1 << 40, None) == -1
    nb = lib.gags_knn3_dist2_scratch_bytes(1000)
    assert nb % 256 == 0 and 1000 * 28 < nb < 1000 * 64 + 16 * 256
    big, small = lib.gags_knn3_dist2_scratch_bytes(1 << 20), lib.gags_knn3_dist2_scratch_bytes(1 << 19)
    assert 1.9 < big / small < 2.1  # linear in n
    assert lib.gags_knn3_dist2(1000, None, P, P, nb, None) == -1
    assert lib.gags_knn3_dist2(1000, P, None, P, nb, None) == -1
    assert lib.gags_knn3_dist2(1000, P, P, None, nb, None) == -1
    assert lib.gags_knn3_dist2(1000, P, P, P, nb - 1, None) == -3
    assert lib.gags_knn3_dist2_scratch_bytes((1 << 31) - 1) > 0
