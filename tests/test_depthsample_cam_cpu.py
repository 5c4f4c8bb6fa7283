"""N22 without a GPU (include/gags_next.h "N22"): the restatement tests/depthsample_cam_ref.py of the min-depth mapping under
camera models against closed forms and against N6's restatement, the conditions on the scenes the GPU tests use (the band where
float32 and float64 may disagree, and the margin of its two new widths), camera_rig and the new keyword arguments on the host,
and every argument check of the gags_rig_depth_* entries."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import depthsample_cam_ref as C  # noqa: E402
import depthsample_ref as R  # noqa: E402

F = np.float32
EINVAL, ESCRATCH = -1, -3
RIG = ("gags_rig_depth_scratch_bytes", "gags_rig_depth_map", "gags_rig_depth_scatter")
EYE = np.eye(4, dtype=F)


@pytest.fixture(scope="module")
def lib():
    from gags_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


# ---- the restatement ---------------------------------------------------------------------------------------------------------

def test_coefficient_sets_are_those_of_the_projection_tests():
    import fisheye_kb_ref as KB
    assert C.COEFFS == KB.COEFFS and float(C.EPS) == float(F(KB.EPS))
    from gags_amd import _lib
    assert C.MODELS == _lib.CAMERA_MODELS


def test_closed_forms():
    w, h = 64, 48
    on_axis = np.array([[0, 0, 1.0], [0, 0, 2.5], [0, 0, 4.0]], F)
    for model in C.MODELS:
        for kc in ([None, "A", "C"] if model == "fisheye" else [None]):
            K = C.intrinsics(model, w, h)
            u, v, zc, keep = C.project32(on_axis, EYE, K, model, kc)
            assert np.array_equal(u, np.full(3, w / 2, F)) and np.array_equal(v, np.full(3, h / 2, F)) and keep.all(), (model, kc)
    # a fisheye point at angle theta lands at radius f g(theta), g(theta) = theta P(theta^2)
    K = C.intrinsics("fisheye", w, h)
    for kc in (None, "A", "B", "C"):
        k = [float(x) for x in C.coeffs32(kc)]
        for deg in (5.0, 30.0, 60.0, 73.0):
            th = math.radians(deg)
            p = np.array([[2 * math.sin(th) * 0.6, 2 * math.sin(th) * 0.8, 2 * math.cos(th)]], F)
            u, v, _, keep = C.project32(p, EYE, K, "fisheye", kc)
            g = th * C.poly(k, th * th)[0]
            assert keep[0] and abs(math.hypot(u[0] - w / 2, v[0] - h / 2) - 24.0 * g) < 1e-4 * (1 + 24 * g), (kc, deg)
            u64, v64, _, _ = C.project64(p, EYE, K, "fisheye", kc)
            assert abs(u64[0] - u[0]) < 1e-4 and abs(v64[0] - v[0]) < 1e-4
    # the ortho pixel is independent of z
    K = C.intrinsics("ortho", w, h)
    pts = np.array([[0.7, -0.4, z] for z in (0.5, 1.0, 3.0, 50.0)], F)
    u, v, _, keep = C.project32(pts, EYE, K, "ortho")
    assert keep.all() and (u == u[0]).all() and (v == v[0]).all() and u[0] == F(0.7) * F(9) + F(32)
    # past the fold (set C: 74 degrees) or behind the near plane: outside, whatever the depth map holds
    D = np.full((h, w), 2.0, F)
    th = math.radians(80.0)
    past = np.array([[2 * math.sin(th), 0, 2 * math.cos(th)]], F)
    assert not C.project32(past, EYE, C.intrinsics("fisheye", w, h), "fisheye", "C")[3][0]
    assert C.project32(past, EYE, C.intrinsics("fisheye", w, h), "fisheye", "A")[3][0]
    near = np.array([[0, 0, 0.0099], [0, 0, 0.01], [0, 0, -1.0], [0, 0, np.nan]], F)
    for model in ("ortho", "fisheye"):
        K = C.intrinsics(model, w, h)
        assert list(C.project32(near, EYE, K, model)[3]) == [False, True, False, False]
        big = np.full((h, w), 1e-2, F)
        vis = C.decide(near, EYE, K, big, model, vis_thresh=10.0)[0]
        assert list(vis) == [False, True, False, False], model
        assert not C.decide64(near, EYE, K, big, model, vis_thresh=10.0)[0][[0, 2, 3]].any()
    assert not C.decide(past, EYE, C.intrinsics("fisheye", w, h), D, "fisheye", "C", vis_thresh=10.0)[0][0]
    assert C.decide(past, EYE, C.intrinsics("fisheye", w, h), D, "fisheye", "A", vis_thresh=10.0)[0][0]


@pytest.mark.parametrize("w,h", C.SIZES)
def test_all_pinhole_is_n6_and_zero_coefficients_are_the_plain_fisheye(w, h):
    s = C.rig_scene("pinhole", w, h)
    for cut in (0, 3):
        a = C.depth_sample(s["xyz"], s["viewmats"], s["Ks"], s["depths"], ["pinhole"] * 3, cut_bound=cut)
        b = R.depth_sample(s["xyz"], s["viewmats"], s["Ks"], s["depths"], cut_bound=cut)
        for key in b:
            assert a[key].dtype == b[key].dtype and np.array_equal(a[key], b[key]), key
    assert b["visible"].any()
    s = C.rig_scene("fisheye", w, h)
    a = C.depth_sample(s["xyz"], s["viewmats"], s["Ks"], s["depths"], s["models"], [None] * 3)
    b = C.depth_sample(s["xyz"], s["viewmats"], s["Ks"], s["depths"], s["models"], ["zero"] * 3)
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    # ... because P = P' = 1 exactly: k is theta / rho, the plain fisheye's
    xc, yc, zc = C.camera_space32(s["xyz"], s["viewmats"][0])
    k, dP = C.fisheye32(xc, yc, zc, "zero")
    with np.errstate(all="ignore"):
        rho = np.sqrt(xc * xc + yc * yc) + C.EPS
        assert np.array_equal(k, np.arctan2(rho, zc + C.EPS) / rho) and (dP == 1).all()


# ---- the scenes of the GPU tests --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(C.RIGS))
@pytest.mark.parametrize("w,h", C.SIZES)
def test_scene_conditions(name, w, h):
    """At most 2 % of the (point, camera) pairs lie in the band (the float64 reference alone shows 0.3 - 0.6 %), both decisions
    occur, the float32 restatement differs from float64 only inside the band, and set C folds inside the image."""
    s, r = C.rig_scene(name, w, h), C.reference64(name, w, h)
    share = r["band"].mean()
    print(f"{name} {w}x{h}: band {share:.4f} visible {r['visible'].mean():.3f}")
    assert share <= 0.02
    assert 0.05 < r["visible"].mean() < 0.6
    assert r["sure_points"].mean() > 0.9 and r["sure_pixels"].mean() > 0.9
    y = C.depth_sample(s["xyz"], s["viewmats"], s["Ks"], s["depths"], s["models"], s["coeffs"])
    differ = (y["visible"] != r["visible"]) | (r["visible"] & (y["mapping"] != r["mapping"]).any(-1))
    assert r["band"][differ].all()
    if name == "C":
        folded = kept = 0
        for k in range(3):
            _, _, zc, dP = C.project64(s["xyz"], s["viewmats"][k], s["Ks"][k], "fisheye", "C")
            folded += int(((dP <= 0) & (zc >= 0.01)).sum())
            kept += int(((dP > 0) & (zc >= 0.01)).sum())
            assert not r["visible"][dP <= 0, k].any()
        assert folded > 0.1 * (folded + kept) and kept > 0.1 * (folded + kept)


def test_band_margin_of_the_two_new_culls():
    """The widths of the bands around the near plane and the fold against what they must cover: the largest difference between
    the float32 restatement and float64 of zc and of P'(t) over every scene (docs/LAB_NOTES.md "GAS under camera models (N22)":
    3.4e-7 and 3.5e-7).  Each width is at least 8 times that."""
    dz = dp = 0.0
    for name in C.RIGS:
        for w, h in C.SIZES:
            s = C.rig_scene(name, w, h)
            for k in range(3):
                xc, yc, zc = C.camera_space32(s["xyz"], s["viewmats"][k])
                _, _, zc64, dP64 = C.project64(s["xyz"], s["viewmats"][k], s["Ks"][k], s["models"][k], s["coeffs"][k])
                dz = max(dz, float(np.abs(zc.astype(np.float64) - zc64).max()))
                if s["models"][k] == "fisheye":
                    dp = max(dp, float(np.abs(C.fisheye32(xc, yc, zc, s["coeffs"][k])[1].astype(np.float64) - dP64).max()))
    print(f"max |zc32 - zc64| = {dz:.3e}, max |dP32 - dP64| = {dp:.3e}; bands {C.ZC_BAND:.1e}, {C.FOLD_BAND:.1e}")
    assert dz > 0 and dp > 0
    assert C.ZC_BAND >= 8 * dz and C.FOLD_BAND >= 8 * dp


# ---- camera_rig and the keyword arguments on the host ----------------------------------------------------------------------------

class Cam:
    def __init__(self, w=32, h=24, model=None, K=None, coeffs=None):
        self.FoVx = self.FoVy = 1.0
        self.image_width, self.image_height = w, h
        self.world_view_transform = torch.eye(4)
        if model is not None:
            self.camera_model = model
        if K is not None:
            self.K = K
        if coeffs is not None:
            self.radial_coeffs = coeffs


def test_camera_rig_on_the_host():
    from gags_amd import depthsample as DS
    Kf = np.array([[24.0, 0, 16], [0, 25.0, 12], [0, 0, 1]], F)
    Ko = np.array([[9.0, 0, 15], [0, 9.0, 11], [0, 0, 1]], F)
    cams = [Cam(), Cam(model="ortho", K=Ko), Cam(model="fisheye", K=Kf), Cam(model="fisheye", K=Kf, coeffs=C.COEFFS["A"])]
    vm, K, models, coeffs, hw = DS.camera_rig(cams, device="cpu")
    assert models == ["pinhole", "ortho", "fisheye", "fisheye"] and hw == (24, 32)
    assert vm.shape == (4, 4, 4) and vm.dtype == torch.float32 and K.shape == (4, 3, 3) and K.dtype == torch.float32
    assert np.array_equal(K[1].numpy(), Ko) and np.array_equal(K[2].numpy(), Kf)
    pin_vm, pin_K, pin_hw = DS.camera_matrices([Cam()], device="cpu")
    assert torch.equal(K[0], pin_K[0]) and torch.equal(vm[0], pin_vm[0]) and pin_hw == hw
    assert coeffs.shape == (4, 4) and coeffs.dtype == torch.float32
    assert not coeffs[:3].any() and np.array_equal(coeffs[3].numpy(), C.coeffs32("A"))
    assert DS.camera_rig(cams[:3], device="cpu")[3] is None           # no camera carries coefficients
    assert DS.camera_rig([Cam(), Cam()], device="cpu")[2] == ["pinhole", "pinhole"]
    with pytest.raises(ValueError, match="differ in size"):
        DS.camera_rig([Cam(32, 24), Cam(32, 25, model="fisheye", K=Kf)], device="cpu")
    with pytest.raises(ValueError, match="explicit K"):
        DS.camera_rig([Cam(), Cam(model="fisheye")], device="cpu")
    with pytest.raises(ValueError, match="explicit K"):
        DS.camera_rig([Cam(model="ortho")], device="cpu")
    with pytest.raises(ValueError, match="unknown camera_model"):
        DS.camera_rig([Cam(model="equirect", K=Kf)], device="cpu")
    with pytest.raises(ValueError, match="radial_coeffs"):
        DS.camera_rig([Cam(model="ortho", K=Ko, coeffs=C.COEFFS["A"])], device="cpu")
    with pytest.raises(ValueError):
        DS.camera_rig([])
    with pytest.raises(NotImplementedError, match="pinhole"):           # its three values cannot carry a model
        DS.camera_matrices(cams, device="cpu")
    # nothing inside the package goes through camera_matrices any more
    # (synthetic.camera_matrices is another function: one synthetic camera's viewmat and K)
    import ast
    import glob
    for path in glob.glob(os.path.join(os.path.dirname(ROOT), "gags_amd", "*.py")):
        for node in ast.walk(ast.parse(open(path).read())):
            if isinstance(node, ast.Call):
                f = node.func
                if isinstance(f, ast.Name):
                    assert f.id != "camera_matrices", path
                elif isinstance(f, ast.Attribute) and f.attr == "camera_matrices":
                    assert isinstance(f.value, ast.Name) and f.value.id == "syn", path


def test_keyword_arguments_raise_on_plain_values():
    """ValueError before any tensor's device is looked at: the tensors here are on the CPU, which would raise RuntimeError."""
    from gags_amd import depthsample as DS
    x, vm, K, D = torch.zeros(4, 3), torch.eye(4).repeat(2, 1, 1), torch.eye(3).repeat(2, 1, 1), torch.ones(2, 8, 8)
    kb = torch.zeros(2, 4)
    for fn in (DS.point_pixel_mapping, DS.point_min_depth, DS.depth_samples):
        bad = [dict(camera_models=["pinhole", "equirect"]), dict(camera_models=["pinhole", 2]), dict(camera_models="fisheye"),
               dict(camera_models=["fisheye"]), dict(camera_models=["fisheye"] * 3),
               dict(camera_models=["pinhole", "ortho"], radial_coeffs=kb), dict(radial_coeffs=kb),
               dict(camera_models=["fisheye", "ortho"], radial_coeffs=torch.zeros(2, 3)),
               dict(camera_models=["fisheye", "ortho"], radial_coeffs=torch.zeros(4)),
               dict(camera_models=["fisheye", "ortho"], radial_coeffs=torch.zeros(2, 4, dtype=torch.float64)),
               dict(camera_models=["fisheye", "ortho"], radial_coeffs=[[0.0] * 4] * 2)]
        for kw in bad:
            with pytest.raises(ValueError):
                fn(x, vm, K, D, **kw)
        for kw in (dict(camera_models=["fisheye", "ortho"], radial_coeffs=kb), dict(camera_models=("pinhole", "pinhole")), {}):
            with pytest.raises(RuntimeError, match="no CPU path"):   # valid: on to the device check
                fn(x, vm, K, D, **kw)


# ---- the C entries -----------------------------------------------------------------------------------------------------------

def test_rig_entries_are_declared_exported_and_typed(lib):
    import re
    from gags_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(os.path.dirname(ROOT), "include", "gags_next.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(gags_rig_depth_\w+)\s*\(", src)) == set(RIG)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in RIG:
        assert hasattr(raw, name) and name in _lib.SIGNATURES, name
    old_m, old_s = _lib.SIGNATURES["gags_depthsample_map"][1], _lib.SIGNATURES["gags_depthsample_scatter"][1]
    new_m, new_s = _lib.SIGNATURES["gags_rig_depth_map"][1], _lib.SIGNATURES["gags_rig_depth_scatter"][1]
    # the N6 argument lists with cam_models and radial_coeffs behind Ks
    assert new_m == old_m[:7] + [ctypes.c_void_p] * 2 + old_m[7:] and new_s == old_s[:7] + [ctypes.c_void_p] * 2 + old_s[7:]
    assert lib.gags_abi_version() == 2


def test_rig_scratch_bytes(lib):
    al = lambda x: (x + 255) // 256 * 256  # noqa: E731
    for args in ((1, 1, 1, 1), (1000, 3, 32, 40), (999, 17, 33, 41), (1000, 300, 1080, 1920), (1_500_000, 65, 6, 8)):
        old, new = lib.gags_depthsample_scratch_bytes(*args), lib.gags_rig_depth_scratch_bytes(*args)
        assert new >= old > 0, args
        assert new == old - al(64 * args[1]) + al(96 * args[1]), args   # a 96-byte camera block where N6 has 64 bytes
    # the function's own fixture (tools/record_scratch_bytes.py LATER): the table of the N6 size function, every row recorded,
    # every value the library's, and every value the arithmetic above applied to the N6 fixture's row of the same arguments
    import json
    sys.path.insert(0, os.path.join(os.path.dirname(ROOT), "tools"))
    import record_scratch_bytes as rec
    name, rows = rec.LATER["gags_rig_depth_scratch_bytes"]
    assert "gags_rig_depth_scratch_bytes" not in rec.functions() and "gags_depthsample_scratch_bytes" in rec.functions()
    with open(os.path.join(ROOT, "golden", name)) as f:
        golden = json.load(f)
    with open(os.path.join(ROOT, "golden", "scratch_bytes.json")) as f:
        n6 = {tuple(r["args"]): r["value"] for r in json.load(f) if r["fn"] == "gags_depthsample_scratch_bytes"}
    assert {(r["fn"], tuple(r["args"])) for r in golden} == {("gags_rig_depth_scratch_bytes", tuple(a)) for a in rows}
    assert set(n6) == {tuple(a) for a in rows} and any(r["value"] > 0 for r in golden)
    for r in golden:
        a = tuple(r["args"])
        assert int(lib.gags_rig_depth_scratch_bytes(*a)) == r["value"], a
        assert r["value"] == (0 if n6[a] == 0 else n6[a] - al(64 * a[1]) + al(96 * a[1])), a
    assert lib.gags_rig_depth_scratch_bytes(0, 2, 32, 32) == 0
    for bad in ((-1, 2, 32, 32), (10, 0, 32, 32), (10, 2, 0, 32), (10, 2, 32, -1), (10, 2, 1 << 16, 1 << 15), ((1 << 31) - 1, 2, 8, 8)):
        assert lib.gags_rig_depth_scratch_bytes(*bad) == 0, bad


def test_rig_map_and_scatter_argument_checks(lib):
    P = ctypes.c_void_p(256)  # never dereferenced: every call below returns before a launch
    nb = lib.gags_rig_depth_scratch_bytes(1000, 3, 32, 40)
    fm, fs = lib.gags_rig_depth_map, lib.gags_rig_depth_scatter
    ids = (ctypes.c_int32 * 3)(0, 1, 2)
    for models, coeffs in ((None, None), (ids, None), (ids, P), (None, P)):
        ok_m = [1000, 3, 32, 40, P, P, P, models, coeffs, P, 0.25, 0, P, None, None, P, nb, None]
        ok_s = [1000, 3, 32, 40, P, P, P, models, coeffs, P, 0.25, 0, P, P, P, nb, None]

        def call(f, ok, **kw):
            a = list(ok)
            for i, v in kw.items():
                a[int(i[1:])] = v
            return f(*a)
        for f, ok in ((fm, ok_m), (fs, ok_s)):
            assert call(f, ok, a0=-1) == EINVAL                       # negative n
            assert call(f, ok, a0=(1 << 31) - 1) == EINVAL            # point indices are int32
            assert call(f, ok, a1=0) == EINVAL and call(f, ok, a1=-2) == EINVAL
            assert call(f, ok, a2=0) == EINVAL and call(f, ok, a3=0) == EINVAL
            assert call(f, ok, a2=1 << 16, a3=1 << 15) == EINVAL     # h w >= 2^31
            assert call(f, ok, a11=-1) == EINVAL                      # negative cut_bound
            for unknown in ((0, 3, 0), (-1, 0, 0), (0, 0, 1 << 20)):  # a model id outside the three, wherever it stands
                assert call(f, ok, a7=(ctypes.c_int32 * 3)(*unknown)) == EINVAL, unknown
        for i in (4, 5, 6, 9, 12, 15):                               # xyz, viewmats, Ks, depths, min_depth, scratch
            assert call(fm, ok_m, **{f"a{i}": None}) == EINVAL, i
        for i in (4, 5, 6, 9, 12, 13, 14):                           # ... min_depth, samples, scratch
            assert call(fs, ok_s, **{f"a{i}": None}) == EINVAL, i
        assert call(fm, ok_m, a16=nb - 1) == ESCRATCH
        assert call(fs, ok_s, a15=nb - 1) == ESCRATCH
        # the scratch of the N6 entries is too small for these, whatever the rig
        assert call(fm, ok_m, a16=lib.gags_depthsample_scratch_bytes(1000, 3, 32, 40)) == ESCRATCH
        # n == 0: the map is a no-op, with every pointer NULL
        assert fm(0, 3, 32, 40, None, None, None, models, None, None, 0.25, 0, None, None, None, None, 0, None) == 0
    bad_ids = (ctypes.c_int32 * 3)(0, 7, 0)
    assert fm(0, 3, 32, 40, None, None, None, bad_ids, None, None, 0.25, 0, None, None, None, None, 0, None) == EINVAL
    assert fs(0, 3, 32, 40, None, None, None, None, None, None, 0.25, 0, None, None, None, 0, None) == EINVAL  # samples NULL
