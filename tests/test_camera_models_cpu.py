"""Camera models (N20) without a GPU: the restatement of tests/camera_models_ref.py against closed forms, the declared fisheye
Jacobian against the true Jacobian of the map, the kernel's per-Gaussian backward formula (numpy, by hand) against float64
autograd, the C ABI of the two new entries, and the host logic around them (rasterization(), scene.Camera, render(),
depthsample.camera_matrices)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import camera_models_ref as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _one(model, mean, scale, K, w=200, h=200, eps2d=0.3, quat=(1.0, 0.0, 0.0, 0.0), **cull):
    """One Gaussian under an identity pose, float64: (pr, dec)."""
    s = dict(means=np.array([mean], np.float64), quats=np.array([quat], np.float64),
             scales=np.array([scale if np.ndim(scale) else [scale] * 3], np.float64), viewmat=np.eye(4), K=np.asarray(K, np.float64))
    pr, dec, _ = cm.run(model, s, w, h, F64, eps2d=eps2d, **cull)
    return pr, dec


def _K(fx, fy, cx, cy):
    return [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]


def _cov(pr, eps2d=0.0):
    s00, s01, s11 = (float(v[0]) for v in pr["cov"])
    return np.array([[s00 + eps2d, s01], [s01, s11 + eps2d]])


# -- the restatement against closed forms -------------------------------------------------------------------------------------

@pytest.mark.parametrize("theta,phi,r", [(math.pi / 4, 0.0, math.sqrt(2.0)), (0.3, 1.1, 5.0), (1.2, -2.0, 0.7), (1.5, 3.0, 11.0),
                                         (math.pi / 4, 0.0, 40.0)])
def test_fisheye_lands_at_f_theta_at_any_distance(theta, phi, r):
    fx, fy, cx, cy = 100.0, 80.0, 150.0, 120.0
    mean = [r * math.sin(theta) * math.cos(phi), r * math.sin(theta) * math.sin(phi), r * math.cos(theta)]
    pr, _ = _one("fisheye", mean, 0.01, _K(fx, fy, cx, cy), w=400, h=400)
    got = pr["means2d"][0].numpy()
    np.testing.assert_allclose(got, [cx + fx * theta * math.cos(phi), cy + fy * theta * math.sin(phi)], rtol=0, atol=2e-5)
    if phi == 0.0 and theta == math.pi / 4:     # (1, 0, 1) with fx = 100: cx + 78.5398
        assert abs(got[0] - (cx + 78.5398)) < 1e-4


@pytest.mark.parametrize("theta,phi,r,s", [(0.5, 0.0, 4.0, 0.05), (1.1, 0.9, 7.0, 0.2), (1.45, -2.4, 3.0, 0.1)])
def test_fisheye_isotropic_gaussian_has_radial_and_tangential_eigenvalues(theta, phi, r, s):
    """cov2d of an isotropic Gaussian of scale s at distance r: (f s / r)^2 along the radius, (f s theta / rho)^2 across it."""
    f = 90.0
    mean = [r * math.sin(theta) * math.cos(phi), r * math.sin(theta) * math.sin(phi), r * math.cos(theta)]
    pr, _ = _one("fisheye", mean, s, _K(f, f, 200, 200), w=400, h=400, quat=(0.3, -0.5, 0.2, 0.7))
    ev = np.sort(np.linalg.eigvalsh(_cov(pr)))
    rho = r * math.sin(theta)
    want = np.sort([(f * s / r) ** 2, (f * s * theta / rho) ** 2])
    np.testing.assert_allclose(ev, want, rtol=2e-5)   # (the closed form against the true Jacobian: 7.8e-6 relative)


def test_fisheye_on_the_axis_is_the_pinhole():
    fx, fy, z, s, eps2d = 100.0, 70.0, 4.0, 0.1, 0.3
    K = _K(fx, fy, 50, 40)
    pf, df = _one("fisheye", [0, 0, z], s, K, eps2d=eps2d)
    pp, dp = _one("pinhole", [0, 0, z], s, K, eps2d=eps2d)
    np.testing.assert_allclose(_cov(pf, eps2d), np.diag([(fx * s / z) ** 2 + eps2d, (fy * s / z) ** 2 + eps2d]), rtol=1e-6, atol=1e-12)
    np.testing.assert_allclose(_cov(pf, eps2d), _cov(pp, eps2d), rtol=1e-6, atol=1e-12)
    np.testing.assert_allclose(pf["means2d"].numpy(), pp["means2d"].numpy(), atol=1e-4)
    np.testing.assert_allclose(pf["J"][0].numpy(), [[fx / z, 0, 0], [0, fy / z, 0]], rtol=1e-6, atol=1e-12)
    assert df["radii"][0] == dp["radii"][0] > 0
    for v in pf.values():
        assert all(bool(torch.isfinite(t).all()) for t in (v if isinstance(v, tuple) else (v,)))


def test_ortho_does_not_depend_on_z():
    fx, fy, s, eps2d = 12.0, 9.0, 0.4, 0.3
    K = _K(fx, fy, 50, 40)
    res = [_one("ortho", [1.5, -0.7, z], s, K, eps2d=eps2d, quat=(0.9, 0.1, -0.3, 0.2)) for z in (2.0, 9.0)]
    for k in ("means2d", "conics", "comp"):
        assert torch.equal(res[0][0][k], res[1][0][k]), k
    assert res[0][1]["radii"][0] == res[1][1]["radii"][0] > 0 and res[0][1]["tiles"][0] == res[1][1]["tiles"][0]
    assert [float(r[0]["depths"][0]) for r in res] == [2.0, 9.0]
    np.testing.assert_allclose(res[0][0]["means2d"][0].numpy(), [fx * 1.5 + 50, fy * -0.7 + 40])
    np.testing.assert_allclose(_cov(res[0][0], eps2d), np.diag([(fx * s) ** 2 + eps2d, (fy * s) ** 2 + eps2d]), rtol=1e-12, atol=1e-12)


def test_fisheye_sees_what_the_pinhole_culls():
    """A Gaussian 80 degrees off axis: visible under the fisheye camera, culled under the pinhole camera with the same K."""
    th = math.radians(80.0)
    mean, K = [5 * math.sin(th), 0.0, 5 * math.cos(th)], _K(60.0, 60.0, 100, 100)
    _, df = _one("fisheye", mean, 0.1, K)
    _, dp = _one("pinhole", mean, 0.1, K)
    assert df["radii"][0] > 0 and dp["radii"][0] == 0


# -- the closed-form J against the true Jacobian ------------------------------------------------------------------------------

def test_fisheye_closed_form_jacobian_against_autograd_of_the_map():
    """For rho >= 0.02: within 1e-4 relative (Frobenius norm per point) of the Jacobian of the map.  Measured over these 5000
    points: 7.8e-6 at rho >= 0.029 -- the eps guards of the closed form."""
    rng = np.random.default_rng(0)
    n = 5000
    th, ph, r = rng.uniform(0.003, 1.54, n), rng.uniform(0, 2 * math.pi, n), rng.uniform(1.0, 12.0, n)
    p = torch.tensor(np.stack([r * np.sin(th) * np.cos(ph), r * np.sin(th) * np.sin(ph), r * np.cos(th)], 1), requires_grad=True)
    keep = (r * np.sin(th)) >= 0.02
    assert keep.sum() > 4500
    fx, fy, cx, cy = (torch.tensor(v, dtype=F64) for v in (100.0, 80.0, 10.0, 20.0))
    m = cm.true_map("fisheye", p, fx, fy, cx, cy)
    rows = [torch.autograd.grad(m[:, k].sum(), p, retain_graph=True)[0] for k in range(2)]
    Jt = torch.stack(rows, 1).numpy()
    x, y, z = p.detach().unbind(-1)
    _, _, J = cm.cam_map("fisheye", x, y, z, fx, fy, cx, cy, 100, 100)
    err = np.linalg.norm((J.numpy() - Jt).reshape(n, -1), axis=1) / np.linalg.norm(Jt.reshape(n, -1), axis=1)
    print(f"closed-form J vs autograd of the map: worst {err[keep].max():.2e} over {keep.sum()} points with rho >= 0.02")
    assert err[keep].max() <= 1e-4


def test_fisheye_jacobian_on_the_axis_is_finite():
    fx, fy = torch.tensor(100.0, dtype=F64), torch.tensor(80.0, dtype=F64)
    z = torch.tensor([0.5, 3.0, 40.0], dtype=F64)
    zero = torch.zeros_like(z)
    mx, my, J = cm.cam_map("fisheye", zero, zero, z, fx, fy, fx, fy, 100, 100)
    assert bool(torch.isfinite(J).all()) and torch.equal(mx, fx + zero) and torch.equal(my, fy + zero)
    want = torch.zeros(3, 2, 3, dtype=F64)
    want[:, 0, 0], want[:, 1, 1] = fx / z, fy / z
    np.testing.assert_allclose(J.numpy(), want.numpy(), rtol=1e-6, atol=1e-12)


# -- the kernel's per-Gaussian backward formula -------------------------------------------------------------------------------

def _truth_grads(model, s, w, h, cot, antialiased, **cull):
    pr, dec, L = cm.run(model, s, w, h, F64, grad=True, **cull)
    cm.project_loss(pr, dec["radii"], cot, antialiased=antialiased).backward()
    return dec, {k: v.grad.numpy() for k, v in L.items() if v.grad is not None}


@pytest.mark.parametrize("antialiased", [False, True])
@pytest.mark.parametrize("model", ["ortho", "fisheye"])
def test_backward_formula_against_float64_autograd(model, antialiased):
    """cam_bwd (and everything in front of it) restated by hand in numpy against autograd through the restatement: v_means and
    the twelve pose terms, classic and antialiased, with v_depths."""
    w, h, n = cm.KERNEL_W, cm.KERNEL_H, 400
    s = cm.model_scene(model, n, 0, w, h, cm.KERNEL_SEEDS[model])
    cot = cm.cotangents(n, 3)
    dec, g = _truth_grads(model, s, w, h, cot, antialiased, **cm.KERNEL_CULL)
    vis = dec["radii"] > 0
    assert 50 <= vis.sum() <= n - 50
    t = cm.bwd_terms(model, s, w, h, dec["radii"], cot["means2d"], cot["depths"], cot["conics"], cot["comp"],
                     antialiased=antialiased, eps2d=cm.KERNEL_CULL["eps2d"])
    e_m = np.linalg.norm(t["v_means"] - g["means"]) / np.linalg.norm(g["means"])
    e_p = np.linalg.norm(t["pose"].sum(0) - g["viewmat"][:3].reshape(-1)) / np.linalg.norm(g["viewmat"][:3])
    print(f"{model} aa={antialiased}: v_means {e_m:.2e}, pose {e_p:.2e}")
    assert e_m <= 1e-10 and e_p <= 1e-10
    assert np.all(t["v_means"][~vis] == 0) and np.all(g["viewmat"][3] == 0)


def test_backward_formula_on_the_fisheye_axis():
    """x = y = 0: every term of the hand-written backward is finite and equals autograd's (d rho taken as 0 there)."""
    s = dict(means=np.array([[0, 0, 3.0], [0, 0, 7.5]]), quats=np.array([[0.9, 0.1, -0.3, 0.2]] * 2), scales=np.array([[0.2, 0.1, 0.3]] * 2),
             viewmat=np.eye(4), K=np.array(_K(40.0, 35.0, 48.0, 30.0)))
    cot = cm.cotangents(2, 5)
    dec, g = _truth_grads("fisheye", s, 97, 61, cot, True)
    assert (dec["radii"] > 0).all()
    t = cm.bwd_terms("fisheye", s, 97, 61, dec["radii"], cot["means2d"], cot["depths"], cot["conics"], cot["comp"], antialiased=True)
    assert np.isfinite(t["v_means"]).all() and np.isfinite(t["pose"]).all() and np.isfinite(g["means"]).all()
    np.testing.assert_allclose(t["v_means"], g["means"], rtol=1e-9, atol=1e-12)


# -- the kernel-order restatement and the seeds of the GPU tests ----------------------------------------------------------------

def test_ortho_kernel_order_restatement_agrees_with_float64():
    w, h, n = cm.KERNEL_W, cm.KERNEL_H, 700
    s = cm.model_scene("ortho", n, 0, w, h, cm.KERNEL_SEEDS["ortho"])
    c = cm.KERNEL_CULL
    k = cm.ortho_kernel_order(s["means"], s["quats"], s["scales"], s["viewmat"], s["K"], w, h, c["eps2d"], c["near_plane"],
                              c["far_plane"], c["radius_clip"])
    pr, dec, _ = cm.run("ortho", s, w, h, F64, **c)
    o = cm.outputs(pr, dec)
    keep = ~dec["close"]
    assert np.array_equal(k["radii"][keep], dec["radii"][keep]) and np.array_equal(k["tiles"][keep], dec["tiles"][keep])
    both = keep & (dec["radii"] > 0)
    assert both.sum() >= 100
    for name in ("means2d", "depths", "conics", "comp"):
        assert np.linalg.norm(k[name][both] - o[name][both]) <= 2e-6 * np.linalg.norm(o[name][both]), name


@pytest.mark.parametrize("model", ["fisheye", "ortho"])
@pytest.mark.parametrize("eps2d", [0.3, 0.0])
def test_seeds_keep_the_float32_restatement_inside_the_exclusion_cap(model, eps2d):
    """The scenes of the GPU kernel tests: the float32 restatement's integers equal float64's outside the Gaussians float64
    puts within 1e-5 of a decision boundary, and those are at most 2 %; the scene has every kind of Gaussian the issue lists."""
    w, h, n = cm.KERNEL_W, cm.KERNEL_H, 700
    s = cm.model_scene(model, n, 0, w, h, cm.KERNEL_SEEDS[model])
    cull = dict(cm.KERNEL_CULL, eps2d=eps2d)
    pr, dec, _ = cm.run(model, s, w, h, F64, **cull)
    _, d32, _ = cm.run(model, s, w, h, torch.float32, **cull)
    keep = ~dec["close"]
    share = 1.0 - keep.mean()
    print(f"{model} eps2d={eps2d}: excluded {share:.2%}, visible {(dec['radii'] > 0).sum()}")
    assert share <= cm.MAX_EXCLUDED
    assert np.array_equal(d32["radii"][keep], dec["radii"][keep]) and np.array_equal(d32["tiles"][keep], dec["tiles"][keep])
    z = pr["depths"].numpy()
    vis = dec["radii"] > 0
    assert vis.sum() >= 100 and (z < 0).sum() >= 20 and ((z > 0) & (z < cull["near_plane"])).sum() >= 1
    _, d_noclip, _ = cm.run(model, s, w, h, F64, **dict(cull, radius_clip=0.0))
    assert ((d_noclip["radii"] > 0) & ~vis).sum() >= 5                      # below radius_clip
    if model == "fisheye":
        assert cm.off_axis_deg(s)[vis].max() > 80.0
    m2 = pr["means2d"].numpy()
    outside = (m2[:, 0] < 0) | (m2[:, 0] > w) | (m2[:, 1] < 0) | (m2[:, 1] > h)
    in_depth = (z > cull["near_plane"]) & (z < cull["far_plane"])
    assert (in_depth & outside).sum() >= 20 and (in_depth & outside & ~vis & (d_noclip["radii"] == 0)).sum() >= 5   # off-screen


# -- ABI ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from gags_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def _fwd_args(n, ptrs=None, w=16, h=16):
    p = [None] * 17 if ptrs is None else ptrs
    # means quats scales logit | modifier | viewmat K | w h | eps near far clip | radii m2 depths conics tiles opac qa sa grec comp | stream
    return (n, p[0], p[1], p[2], p[3], 1.0, p[4], p[5], w, h, 0.3, 0.01, 1e10, 0.0, *p[6:16], None)


def _bwd_args(n, ptrs=None, partials_bytes=0, w=16, h=16):
    p = [None] * 18 if ptrs is None else ptrs
    # means quats scales logit | modifier | viewmat K | w h eps | radii vm2 vdepth vcon vopac vcomp | vmeans vq vs vlogit vvm partials
    return (n, p[0], p[1], p[2], p[3], 1.0, p[4], p[5], w, h, 0.3, *p[6:18], partials_bytes, None)


def test_new_entries_are_declared_exported_and_bound(lib):
    from gags_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gags_raster.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("gags_project_fwd_cam", "gags_project_bwd_cam"):
        assert re.search(r"\b" + name + r"\s*\(", header) and hasattr(raw, name) and name in _lib.SIGNATURES
        decl = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", header, re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
    for const in ("GAGS_CAM_PINHOLE", "GAGS_CAM_ORTHO", "GAGS_CAM_FISHEYE", "GAGS_PROJ_RAW", "GAGS_PROJ_AA", "GAGS_PROJ_POSE"):
        assert int(re.search(r"#define\s+" + const + r"\s+(\d+)", header).group(1)) == getattr(_lib, const), const
    assert (_lib.GAGS_PROJ_RAW, _lib.GAGS_PROJ_AA) == (_lib.GAGS_POSE_RAW, _lib.GAGS_POSE_AA)
    assert _lib.CAMERA_MODELS == {"pinhole": 0, "ortho": 1, "fisheye": 2}


def test_new_entries_refuse_bad_arguments_before_any_launch(lib):
    from gags_amd import _lib
    EINVAL, OK = -1, 0
    buf = (ctypes.c_float * 4096)()
    P = ctypes.c_void_p(ctypes.addressof(buf))      # (a host address: never dereferenced, nothing is launched)
    allp17, allp18 = [P] * 17, [P] * 18
    for model in (-1, 3, 7):
        assert lib.gags_project_fwd_cam(model, 0, *_fwd_args(8, allp17)) == EINVAL
        assert lib.gags_project_bwd_cam(model, 0, *_bwd_args(8, allp18)) == EINVAL
    for model in (0, 1, 2):
        for flags in (4, 8, 16, -1):                  # (POSE is a backward flag)
            assert lib.gags_project_fwd_cam(model, flags, *_fwd_args(8, allp17)) == EINVAL
        for flags in (8, 16, 64, -1):
            assert lib.gags_project_bwd_cam(model, flags, *_bwd_args(8, allp18, 1 << 20)) == EINVAL
        for flags in (0, 1, 2, 3):
            assert lib.gags_project_fwd_cam(model, flags, *_fwd_args(-1, allp17)) == EINVAL
            assert lib.gags_project_fwd_cam(model, flags, *_fwd_args(8)) == EINVAL                  # null pointers
            assert lib.gags_project_fwd_cam(model, flags, *_fwd_args(8, allp17, w=0)) == EINVAL
            assert lib.gags_project_fwd_cam(model, flags, *_fwd_args(0)) == OK                      # n = 0: nothing to do
            for missing in (0, 1, 2, 4, 5, 6, 7, 8, 9, 10):
                assert lib.gags_project_fwd_cam(model, flags, *_fwd_args(8, [None if i == missing else P for i in range(17)])) == EINVAL
            if flags & 1:    # RAW reads the logits and writes the activated opacity
                for missing in (3, 11):
                    assert lib.gags_project_fwd_cam(model, flags, *_fwd_args(8, [None if i == missing else P for i in range(17)])) == EINVAL
            if flags & 2:    # AA writes the compensations
                assert lib.gags_project_fwd_cam(model, flags, *_fwd_args(8, [None if i == 15 else P for i in range(17)])) == EINVAL
            assert lib.gags_project_bwd_cam(model, flags, *_bwd_args(-1, allp18)) == EINVAL
            assert lib.gags_project_bwd_cam(model, flags, *_bwd_args(8)) == EINVAL
            assert lib.gags_project_bwd_cam(model, flags, *_bwd_args(0)) == OK
            for missing in (0, 1, 2, 4, 5, 6, 7, 9, 12, 13, 14):   # (without POSE v_means, v_quats, v_scales are required)
                assert lib.gags_project_bwd_cam(model, flags, *_bwd_args(8, [None if i == missing else P for i in range(18)])) == EINVAL
            pose = flags | _lib.GAGS_PROJ_POSE
            need = lib.gags_project_pose_partials(700) * 48
            assert need == 3 * 48
            assert lib.gags_project_bwd_cam(model, pose, *_bwd_args(700, allp18, need - 1)) == EINVAL    # a short partials buffer
            assert lib.gags_project_bwd_cam(model, pose, *_bwd_args(700, allp18, 0)) == EINVAL
            assert lib.gags_project_bwd_cam(model, pose, *_bwd_args(-1, allp18, need)) == EINVAL
            for missing in (16, 17):                                                                     # v_viewmat, partials
                assert lib.gags_project_bwd_cam(model, pose, *_bwd_args(700, [None if i == missing else P for i in range(18)], need)) == EINVAL
            for missing in (0, 4, 6, 7, 9):
                assert lib.gags_project_bwd_cam(model, pose, *_bwd_args(700, [None if i == missing else P for i in range(18)], need)) == EINVAL


# -- host logic -----------------------------------------------------------------------------------------------------------------

def _cpu_call(**kw):
    from gags_amd.rasterization import rasterization
    n = 4
    return rasterization(torch.zeros(n, 3), torch.ones(n, 4), torch.ones(n, 3), torch.ones(n), torch.ones(n, 3),
                         torch.eye(4)[None], torch.eye(3)[None], 16, 16, **kw)


def test_rasterization_checks_the_camera_model_before_the_tensors():
    for bad in ("spherical", "PINHOLE", "", None, 2):
        with pytest.raises(ValueError, match="camera_model"):
            _cpu_call(camera_model=bad)
    for ok in ("pinhole", "ortho", "fisheye"):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            _cpu_call(camera_model=ok)


def test_camera_takes_a_model_and_intrinsics():
    from gags_amd.scene import Camera
    K = np.array(_K(30.0, 32.0, 48.0, 30.0), np.float32)
    cam = Camera(np.eye(3), np.zeros(3), 1.0, 0.8, 97, 61, device="cpu", camera_model="fisheye", K=K)
    assert cam.camera_model == "fisheye" and np.array_equal(cam.K, K)
    cam = Camera(np.eye(3), np.zeros(3), 1.0, 0.8, 97, 61, device="cpu", K=torch.tensor(K))
    assert cam.camera_model == "pinhole" and np.array_equal(cam.K, K)
    plain = Camera(np.eye(3), np.zeros(3), 1.0, 0.8, 97, 61, device="cpu")
    assert plain.camera_model == "pinhole" and plain.K is None
    with pytest.raises(ValueError):
        Camera(np.eye(3), np.zeros(3), 1.0, 0.8, 97, 61, device="cpu", camera_model="spherical")
    with pytest.raises(ValueError):
        Camera(np.eye(3), np.zeros(3), 1.0, 0.8, 97, 61, device="cpu", K=np.eye(4))


class _Pc:
    get_xyz = torch.zeros(1, 3)


def test_render_wants_an_explicit_K_for_a_non_pinhole_camera():
    from gags_amd.gaussian_renderer import _intrinsics, render
    from gags_amd.scene import Camera
    for model in ("fisheye", "ortho"):
        cam = Camera(np.eye(3), np.zeros(3), 1.0, 0.8, 97, 61, device="cpu", camera_model=model)
        with pytest.raises(ValueError, match="explicit K"):
            render(cam, _Pc(), None, torch.zeros(3))
    # the intrinsics: an explicit K wins over the FoV, and the cache tells cameras apart that differ only in K
    cache, dev = {}, torch.device("cpu")
    Ka, Kb = np.array(_K(30.0, 32.0, 48.0, 30.0), np.float32), np.array(_K(30.0, 32.0, 48.5, 30.0), np.float32)
    mk = lambda **kw: Camera(np.eye(3), np.zeros(3), 1.0, 0.8, 97, 61, device="cpu", **kw)  # noqa: E731
    a, b, plain = mk(camera_model="fisheye", K=Ka), mk(camera_model="fisheye", K=Kb), mk()
    assert np.array_equal(_intrinsics(a, dev, cache).numpy(), Ka) and np.array_equal(_intrinsics(b, dev, cache).numpy(), Kb)
    assert np.array_equal(_intrinsics(mk(K=Ka), dev, cache).numpy(), Ka)
    fov = _intrinsics(plain, dev, cache).numpy()
    assert abs(fov[0, 0] - 97 / (2 * math.tan(0.5))) < 1e-3 and fov[0, 2] == 48.5
    assert _intrinsics(a, dev, cache) is _intrinsics(a, dev, cache) and len(cache) == 3

    class Reference:    # a camera of the reference: no camera_model, no K
        FoVx, FoVy, image_width, image_height = 1.0, 0.8, 97, 61
    assert np.array_equal(_intrinsics(Reference(), dev, cache).numpy(), fov)


def test_camera_matrices_refuses_non_pinhole_cameras():
    from gags_amd.depthsample import camera_matrices
    from gags_amd.scene import Camera
    K = np.array(_K(30.0, 32.0, 48.0, 30.0), np.float32)
    plain = Camera(np.eye(3), np.zeros(3), 1.0, 0.8, 97, 61, device="cpu")
    fish = Camera(np.eye(3), np.zeros(3), 1.0, 0.8, 97, 61, device="cpu", camera_model="fisheye", K=K)
    with pytest.raises(NotImplementedError, match="pinhole"):
        camera_matrices([plain, fish], device="cpu")
    vms, Ks, hw = camera_matrices([plain], device="cpu")
    assert vms.shape == (1, 4, 4) and Ks.shape == (1, 3, 3) and hw == (61, 97)
