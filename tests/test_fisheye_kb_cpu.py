"""The fisheye's distortion coefficients (N21) without a GPU: the declared Jacobian against the true Jacobian of the map, the
zero-coefficient case against N20's fisheye bit for bit, the kernel's hand-written backward (numpy) against float64 autograd,
the C ABI of GAGS_PROJ_KB, the host logic (rasterization(), scene.Camera, render()'s cache), and the seeds of the GPU tests."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import camera_models_ref as cm
import fisheye_kb_ref as kb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
W, H = cm.KERNEL_W, cm.KERNEL_H


def _K(fx, fy, cx, cy):
    return [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]


# -- the rule -------------------------------------------------------------------------------------------------------------------

def test_coefficient_sets_are_what_their_comments_say():
    """g' over 0 .. 88 degrees: A >= 0.66, B >= 0.86, C folds at 74 degrees (g' = 1 - 0.6 theta^2)."""
    th = np.linspace(0.0, math.radians(88.0), 20001)
    dg = {k: kb.poly(tuple(float(v) for v in kb.coeffs32(k)), th * th)[1] for k in "ABC"}
    print(f"min g' up to 88 degrees: A {dg['A'].min():.4f}, B {dg['B'].min():.4f}")
    assert abs(dg["A"].min() - 0.66) < 0.005 and abs(dg["B"].min() - 0.86) < 0.005
    fold = th[np.argmax(dg["C"] <= 0)]
    assert abs(math.degrees(fold) - math.degrees(math.sqrt(1 / 0.6))) < 0.01 and 73.5 < math.degrees(fold) < 74.5
    # set A moves a point 60 degrees off axis by 3.7 % of its image radius
    t = math.radians(60.0) ** 2
    assert abs(kb.poly(kb.COEFFS["A"], t)[0] - 1 + 0.037) < 5e-4


@pytest.mark.parametrize("name", ["A", "B"])
def test_closed_form_jacobian_against_autograd_of_the_map(name):
    """Float64, 2000 points up to 88 degrees off axis at distance 2 .. 12: J within 1e-6 relative (Frobenius norm per point) of
    the autograd Jacobian of the unguarded map.  The guards move J by at most about eps / rho^2 = 1e-7 / rho^2, so the points
    keep rho >= 0.4 (6e-7, inside the bound); measured here: 6.9e-8 (A), 6.6e-8 (B)."""
    rng = np.random.default_rng(7)
    n = 2000
    r = rng.uniform(2.0, 12.0, n)
    th = rng.uniform(np.arcsin(0.4 / r), math.radians(88.0))
    ph = rng.uniform(0, 2 * math.pi, n)
    assert math.degrees(th.max()) > 87.5 and (r * np.sin(th)).min() >= 0.4 - 1e-12
    p = torch.tensor(np.stack([r * np.sin(th) * np.cos(ph), r * np.sin(th) * np.sin(ph), r * np.cos(th)], 1), requires_grad=True)
    fx, fy, cx, cy = (torch.tensor(v, dtype=F64) for v in (100.0, 80.0, 10.0, 20.0))
    kc = kb._kc(name, fx)
    m = kb.true_map(kc, p, fx, fy, cx, cy)
    Jt = torch.stack([torch.autograd.grad(m[:, k].sum(), p, retain_graph=True)[0] for k in range(2)], 1).numpy()
    x, y, z = p.detach().unbind(-1)
    mx, my, J, dg = kb.cam_map(kc, x, y, z, fx, fy, cx, cy)
    err = np.linalg.norm((J.numpy() - Jt).reshape(n, -1), axis=1) / np.linalg.norm(Jt.reshape(n, -1), axis=1)
    print(f"set {name}: closed-form J vs autograd of the map, worst {err.max():.2e}")
    assert err.max() <= 1e-6
    assert float(dg.min()) > 0.6
    np.testing.assert_allclose(torch.stack([mx, my], -1).numpy(), m.detach().numpy(), rtol=0, atol=1e-5)


def test_zero_coefficients_are_the_plain_fisheye_bit_for_bit():
    """float32 on the CPU: P = P' = 1 exactly, and every output of the map is torch.equal to cm.cam_map("fisheye", ...)."""
    s = cm.model_scene("fisheye", 700, 0, W, H, cm.KERNEL_SEEDS["fisheye"])
    vm = torch.tensor(s["viewmat"])
    p = torch.tensor(s["means"]) @ vm[:3, :3].T + vm[:3, 3]
    p = torch.cat([p, torch.tensor([[0.0, 0.0, 3.0], [0.0, 0.0, 0.5]])])       # ... and the axis
    x, y, z = p.unbind(-1)
    K = torch.tensor(s["K"])
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    mx, my, J, dg = kb.cam_map(kb._kc("zero", z), x, y, z, fx, fy, cx, cy)
    wx, wy, wJ = cm.cam_map("fisheye", x, y, z, fx, fy, cx, cy, W, H)
    assert mx.dtype == torch.float32
    assert torch.equal(mx, wx) and torch.equal(my, wy) and torch.equal(J, wJ) and bool((dg == 1).all())
    pr, dec, _ = kb.run("zero", s, W, H, torch.float32, **cm.KERNEL_CULL)
    wr, wdec, _ = cm.run("fisheye", s, W, H, torch.float32, **cm.KERNEL_CULL)
    for k in ("means2d", "depths", "conics", "comp"):
        assert torch.equal(pr[k], wr[k]), k
    for k in ("radii", "tiles", "close"):
        assert np.array_equal(dec[k], wdec[k]), k


# -- the kernel's per-Gaussian backward formula -------------------------------------------------------------------------------

@pytest.mark.parametrize("antialiased", [False, True])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_backward_formula_against_float64_autograd(name, antialiased):
    """cam_bwd restated by hand in numpy against autograd through the restatement: v_means and the twelve pose terms, at the
    bound tests/test_camera_models_cpu.py holds cm.cam_bwd_np to (1e-10)."""
    n = 400
    s, cull = kb.kernel_scene(name)
    s = {k: (v[:n] if k in ("means", "quats", "scales") else v) for k, v in s.items()}
    cot = cm.cotangents(n, 3)
    pr, dec, L = kb.run(name, s, W, H, F64, grad=True, **cull)
    cm.project_loss(pr, dec["radii"], cot, antialiased=antialiased).backward()
    g = {k: v.grad.numpy() for k, v in L.items() if v.grad is not None}
    vis = dec["radii"] > 0
    assert 50 <= vis.sum() <= n - 50
    t = kb.bwd_terms(name, s, W, H, dec["radii"], cot["means2d"], cot["depths"], cot["conics"], cot["comp"],
                     antialiased=antialiased, eps2d=cull["eps2d"])
    e_m = np.linalg.norm(t["v_means"] - g["means"]) / np.linalg.norm(g["means"])
    e_p = np.linalg.norm(t["pose"].sum(0) - g["viewmat"][:3].reshape(-1)) / np.linalg.norm(g["viewmat"][:3])
    print(f"set {name} aa={antialiased}: v_means {e_m:.2e}, pose {e_p:.2e}")
    assert e_m <= 1e-10 and e_p <= 1e-10
    assert np.all(t["v_means"][~vis] == 0) and np.all(g["viewmat"][3] == 0)


def test_backward_formula_on_the_axis():
    """x = y = 0: every term of the hand-written backward is finite and equals autograd's (d rho taken as 0 there)."""
    s = dict(means=np.array([[0, 0, 3.0], [0, 0, 7.5]]), quats=np.array([[0.9, 0.1, -0.3, 0.2]] * 2), scales=np.array([[0.2, 0.1, 0.3]] * 2),
             viewmat=np.eye(4), K=np.array(_K(40.0, 35.0, 48.0, 30.0)))
    cot = cm.cotangents(2, 5)
    pr, dec, L = kb.run("A", s, 97, 61, F64, grad=True)
    cm.project_loss(pr, dec["radii"], cot, antialiased=True).backward()
    assert (dec["radii"] > 0).all()
    t = kb.bwd_terms("A", s, 97, 61, dec["radii"], cot["means2d"], cot["depths"], cot["conics"], cot["comp"], antialiased=True)
    assert np.isfinite(t["v_means"]).all() and np.isfinite(t["pose"]).all()
    np.testing.assert_allclose(t["v_means"], L["means"].grad.numpy(), rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(pr["means2d"].detach().numpy(), [[48.0, 30.0]] * 2, atol=1e-5)


# -- the seeds of the GPU tests ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_kernel_seeds_keep_the_float32_restatement_inside_the_exclusion_cap(name):
    """The scenes of tests/test_fisheye_kb_gpu.py: float64 puts at most 2 % of the Gaussians within NEAR_TOL of a decision
    boundary, the fold included, and outside them the float32 restatement takes the same integer decisions.  Set C has
    Gaussians on either side of its fold."""
    s, cull = kb.kernel_scene(name)
    pr, dec, _ = kb.run(name, s, W, H, F64, **cull)
    _, d32, _ = kb.run(name, s, W, H, torch.float32, **cull)
    keep = ~dec["close"]
    share = 1.0 - keep.mean()
    print(f"set {name}: excluded {share:.2%}, visible {(dec['radii'] > 0).sum()}, folded {dec['folded'].sum()}")
    assert share <= cm.MAX_EXCLUDED
    assert np.array_equal(d32["radii"][keep], dec["radii"][keep]) and np.array_equal(d32["tiles"][keep], dec["tiles"][keep])
    vis = dec["radii"] > 0
    ang = cm.off_axis_deg(s)
    assert vis.sum() >= 100
    if name == "C":
        assert (dec["folded"] & keep).sum() >= 50 and ang[vis].max() > 70.0 and ang[dec["folded"]].min() > 73.5
        assert not vis[dec["folded"]].any()
    else:
        assert dec["folded"].sum() == 0 and ang[vis].max() > 80.0
    sizes = (257, 700) if name == "C" else cm.KERNEL_SIZES
    for n in sizes:      # ... and every prefix the GPU tests cut from the scene
        assert dec["close"][:n].sum() <= cm.MAX_EXCLUDED * max(n, 1) or n < 63, n
    # the yardstick of the GPU tests is representative at every size: the float32 restatement's error on a prefix is at least
    # YARDSTICK_FLOOR of its error on the whole scene, for every quantity bounded by it (a seed chosen without this put a
    # single Gaussian with a float32 conic error of a third of the scene's in front: a bound of 3 x that measures luck)
    for raw in (False, True):
        full = kb.yardstick_errors(name, s, cull, 700, raw)
        for n in sizes:
            e = kb.yardstick_errors(name, s, cull, n, raw) if 0 < n < 700 else None
            for k in (e or {}):
                assert e[k] >= kb.YARDSTICK_FLOOR * full[k], (n, raw, k, e[k], full[k])


@pytest.mark.parametrize("case", kb.RASTER_CASES, ids=lambda c: f"D{c[2]}-set{c[8]}")
def test_raster_seeds_stay_inside_the_exclusion_cap(case):
    s = kb.raster_scene(case)
    _, dec, _ = kb.run(case[8], s, case[0], case[1], F64)
    assert dec["close"].mean() <= cm.MAX_EXCLUDED and (dec["radii"] > 0).sum() >= 100 and dec["folded"].sum() == 0
    assert 55.0 < cm.off_axis_deg(s)[dec["radii"] > 0].max() <= 70.5


# -- ABI ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from gags_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def _fwd_args(n, ptrs=None, w=16, h=16):
    p = [None] * 17 if ptrs is None else ptrs
    return (n, p[0], p[1], p[2], p[3], 1.0, p[4], p[5], w, h, 0.3, 0.01, 1e10, 0.0, *p[6:16], None)


def _bwd_args(n, ptrs=None, partials_bytes=0, w=16, h=16):
    p = [None] * 18 if ptrs is None else ptrs
    return (n, p[0], p[1], p[2], p[3], 1.0, p[4], p[5], w, h, 0.3, *p[6:18], partials_bytes, None)


def test_the_flag_is_declared_and_bound():
    from gags_amd import _lib
    header = open(os.path.join(ROOT, "include", "gags_raster.h")).read()
    assert int(re.search(r"#define\s+GAGS_PROJ_KB\s+(\d+)", header).group(1)) == _lib.GAGS_PROJ_KB == kb.KB == 32
    assert _lib.CAMERA_MODELS == cm.MODELS                       # a flag of the fisheye, not a fourth camera
    assert "GAGS_CAM_FISHEYE_KB" not in header


def test_the_flag_is_refused_or_accepted_before_any_launch(lib):
    """Nothing is launched: host addresses, never dereferenced."""
    EINVAL, OK = -1, 0
    buf = (ctypes.c_float * 4096)()
    P = ctypes.c_void_p(ctypes.addressof(buf))
    allp17, allp18 = [P] * 17, [P] * 18
    for model in (0, 1):           # the coefficients are the fisheye's
        for flags in (0, 1, 2, 3):
            assert lib.gags_project_fwd_cam(model, flags | kb.KB, *_fwd_args(8, allp17)) == EINVAL
            assert lib.gags_project_fwd_cam(model, flags | kb.KB, *_fwd_args(0)) == EINVAL
            for f in (flags, flags | 4):
                assert lib.gags_project_bwd_cam(model, f | kb.KB, *_bwd_args(8, allp18, 1 << 20)) == EINVAL
                assert lib.gags_project_bwd_cam(model, f | kb.KB, *_bwd_args(0, allp18, 1 << 20)) == EINVAL
    for flags in (0, 1, 2, 3):
        f = flags | kb.KB
        assert lib.gags_project_fwd_cam(2, f, *_fwd_args(-1, allp17)) == EINVAL
        assert lib.gags_project_fwd_cam(2, f, *_fwd_args(8)) == EINVAL                      # null pointers
        assert lib.gags_project_fwd_cam(2, f, *_fwd_args(8, [None if i == 5 else P for i in range(17)])) == EINVAL   # K
        assert lib.gags_project_fwd_cam(2, f, *_fwd_args(8, allp17, w=0)) == EINVAL
        assert lib.gags_project_fwd_cam(2, f, *_fwd_args(0)) == OK
        assert lib.gags_project_bwd_cam(2, f, *_bwd_args(-1, allp18)) == EINVAL
        assert lib.gags_project_bwd_cam(2, f, *_bwd_args(8)) == EINVAL
        assert lib.gags_project_bwd_cam(2, f, *_bwd_args(8, [None if i == 5 else P for i in range(18)])) == EINVAL
        assert lib.gags_project_bwd_cam(2, f, *_bwd_args(8, allp18, w=0)) == EINVAL
        assert lib.gags_project_bwd_cam(2, f, *_bwd_args(0)) == OK
        assert lib.gags_project_bwd_cam(2, f | 4, *_bwd_args(700, allp18, 3 * 48 - 1)) == EINVAL   # a short partials buffer
        for unknown in (8, 16, 64):
            assert lib.gags_project_fwd_cam(2, f | unknown, *_fwd_args(8, allp17)) == EINVAL
            assert lib.gags_project_bwd_cam(2, f | unknown, *_bwd_args(8, allp18, 1 << 20)) == EINVAL
        assert lib.gags_project_fwd_cam(2, f | 4, *_fwd_args(8, allp17)) == EINVAL              # (POSE is a backward flag)


# -- host logic -----------------------------------------------------------------------------------------------------------------

def _cpu_call(**kw):
    from gags_amd.rasterization import rasterization
    n = 4
    return rasterization(torch.zeros(n, 3), torch.ones(n, 4), torch.ones(n, 3), torch.ones(n), torch.ones(n, 3),
                         torch.eye(4)[None], torch.eye(3)[None], 16, 16, **kw)


def test_rasterization_checks_radial_coeffs_before_the_tensors():
    c = torch.zeros(4)
    for model in ("pinhole", "ortho"):
        with pytest.raises(ValueError, match="radial_coeffs"):
            _cpu_call(camera_model=model, radial_coeffs=c)
    with pytest.raises(ValueError, match="radial_coeffs"):
        _cpu_call(radial_coeffs=c)
    for bad in (torch.zeros(3), torch.zeros(2, 4), torch.zeros(4, 1), torch.zeros(4, dtype=F64), [0.0] * 4, (0.0, 0.0, 0.0, 0.0)):
        with pytest.raises(ValueError, match="radial_coeffs"):
            _cpu_call(camera_model="fisheye", radial_coeffs=bad)
    for ok in (c, c[None]):        # the plain values pass: the tensors are looked at next
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            _cpu_call(camera_model="fisheye", radial_coeffs=ok)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        _cpu_call(camera_model="fisheye", radial_coeffs=None)


def test_camera_takes_radial_coeffs_for_a_fisheye_only():
    from gags_amd.scene import Camera
    K = np.array(_K(30.0, 32.0, 48.0, 30.0), np.float32)
    mk = lambda **kw: Camera(np.eye(3), np.zeros(3), 1.0, 0.8, 97, 61, device="cpu", **kw)  # noqa: E731
    cam = mk(camera_model="fisheye", K=K, radial_coeffs=kb.COEFFS["A"])
    assert cam.radial_coeffs.dtype == np.float32 and cam.radial_coeffs.shape == (4,)
    assert np.array_equal(cam.radial_coeffs, kb.coeffs32("A"))
    assert np.array_equal(mk(camera_model="fisheye", K=K, radial_coeffs=torch.tensor([kb.COEFFS["B"]])).radial_coeffs, kb.coeffs32("B"))
    assert mk(camera_model="fisheye", K=K).radial_coeffs is None and mk().radial_coeffs is None
    for model in ("pinhole", "ortho"):
        with pytest.raises(ValueError, match="radial_coeffs"):
            mk(camera_model=model, K=K, radial_coeffs=kb.COEFFS["A"])
    with pytest.raises(ValueError, match="radial_coeffs"):
        mk(K=K, radial_coeffs=kb.COEFFS["A"])
    with pytest.raises(ValueError, match="radial_coeffs"):
        mk(camera_model="fisheye", K=K, radial_coeffs=(0.1, 0.2, 0.3))


def test_from_opencv_fisheye():
    from gags_amd.scene import Camera
    params = (30.0, 32.0, 48.0, 30.5) + kb.COEFFS["A"]
    R = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    cam = Camera.from_opencv_fisheye(params, R, np.array([0.1, 0.2, 0.3]), 97, 61, device="cpu", uid=5)
    assert cam.camera_model == "fisheye" and cam.uid == 5 and (cam.image_width, cam.image_height) == (97, 61)
    assert np.array_equal(cam.K, np.array(_K(30.0, 32.0, 48.0, 30.5), np.float32))
    assert np.array_equal(cam.radial_coeffs, kb.coeffs32("A"))
    same = Camera(R, np.array([0.1, 0.2, 0.3]), 1.0, 1.0, 97, 61, device="cpu")
    assert torch.equal(cam.world_view_transform, same.world_view_transform)
    for bad in (params[:4], params + (0.0,)):
        with pytest.raises(ValueError):
            Camera.from_opencv_fisheye(bad, R, np.zeros(3), 97, 61, device="cpu")


def test_render_cache_separates_cameras_that_differ_only_in_coefficients():
    from gags_amd.gaussian_renderer import _intrinsics, _intrinsics_kb
    from gags_amd.scene import Camera
    cache, dev = {}, torch.device("cpu")
    K = np.array(_K(30.0, 32.0, 48.0, 30.0), np.float32)
    mk = lambda **kw: Camera(np.eye(3), np.zeros(3), 1.0, 0.8, 97, 61, device="cpu", camera_model="fisheye", K=K, **kw)  # noqa: E731
    a, b = mk(radial_coeffs=kb.COEFFS["A"]), mk(radial_coeffs=kb.COEFFS["B"])
    Ka, ca = _intrinsics_kb(a, dev, cache)
    Kb, cb = _intrinsics_kb(b, dev, cache)
    assert len(cache) == 2 and np.array_equal(Ka.numpy(), K) and np.array_equal(Kb.numpy(), K)
    assert np.array_equal(ca.numpy(), kb.coeffs32("A")) and np.array_equal(cb.numpy(), kb.coeffs32("B"))
    # one resident block of 13 floats per camera: K and the coefficients are views of it, and a second call makes no new one
    assert ca.data_ptr() == Ka.data_ptr() + 36 and Ka.is_contiguous() and ca.is_contiguous()
    Ka2, ca2 = _intrinsics_kb(mk(radial_coeffs=kb.COEFFS["A"]), dev, cache)
    assert len(cache) == 2 and Ka2.data_ptr() == Ka.data_ptr() and ca2.data_ptr() == ca.data_ptr()
    # ... which rasterization() takes as the block, without a copy
    from gags_amd.rasterization import _kb_block
    blk = _kb_block(Ka[None][0], ca)
    assert blk.shape == (13,) and blk.data_ptr() == Ka.data_ptr() and np.array_equal(blk.numpy(), kb.block(K, "A"))
    apart = _kb_block(torch.tensor(K), torch.tensor(kb.coeffs32("B"))[None])
    assert np.array_equal(apart.numpy(), kb.block(K, "B"))
    # a camera without coefficients keeps its own entry and its nine floats
    plain = _intrinsics(mk(), dev, cache)
    assert len(cache) == 3 and plain.data_ptr() != Ka.data_ptr() and plain.shape == (3, 3)
