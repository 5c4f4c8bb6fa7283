"""N23 without a GPU: the float64 reference of tests/intrinsics_grad_ref.py against central differences, pose.IntrinsicsDelta,
the argument checks of gags_project_bwd_calib (nothing is launched), and header / binding agreement."""
import copy
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import camera_models_ref as cm
import fisheye_kb_ref as kb
import intrinsics_grad_ref as ig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = cm.KERNEL_W, cm.KERNEL_H
# the pinhole scene of the kernel-level tests (here and on the GPU): the first seed from 31 on whose float64 decisions under
# cm.KERNEL_CULL leave visible Gaussians past the tangent clamp on BOTH sides in x and in y (test_pinhole_scene_has_... pins it)
PINHOLE_SEED = 31
# central differences: step FD_STEP_K on fx, fy, cx, cy (pixels, 30 .. 90) and FD_STEP_C on k1 .. k4 (dimensionless, ~ 0.01; the
# loss's third derivative in k_j carries theta^(2j) three times over, theta up to 1.5, so their truncation error h^2 |f'''| / 6
# is the larger by far: 6e-7 of the normaliser at 1e-5, 6e-9 at 1e-6).  Round-off is 2^-52 |loss| / h with |loss| ~ 1e2 and
# normalisers of 1 .. 1e3: 1e-9 .. 1e-8 of the normaliser at these steps.  Both stay below 1e-8; the tolerance is ten times that.
FD_STEP_K, FD_STEP_C, FD_TOL = 1e-5, 1e-6, 1e-7


@pytest.fixture(scope="module")
def lib():
    from gags_amd import _lib
    return _lib.load()


def pinhole_scene(n=700, seed=PINHOLE_SEED):
    return cm.model_scene("pinhole", n, 0, W, H, seed), dict(cm.KERNEL_CULL)


def clamp_sides(s, radii):
    """Visible Gaussians past the pinhole's tangent clamp: (x positive side, x negative, y positive, y negative), float64."""
    vm, K = s["viewmat"].astype(np.float64), s["K"].astype(np.float64)
    p = s["means"].astype(np.float64) @ vm[:3, :3].T + vm[:3, 3]
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    xr, yr = p[:, 0] / p[:, 2], p[:, 1] / p[:, 2]
    vis = np.asarray(radii) > 0
    return (int((vis & (xr > (1.15 * W - cx) / fx)).sum()), int((vis & (xr < -(cx + 0.15 * W) / fx)).sum()),
            int((vis & (yr > (1.15 * H - cy) / fy)).sum()), int((vis & (yr < -(cy + 0.15 * H) / fy)).sum()))


def _case(variant, n):
    """(model, coeffs, scene cut to n, radii of the float64 decisions, cotangents)."""
    if variant == "pinhole":
        s, cull = pinhole_scene()
        model, coeffs = "pinhole", None
    elif variant == "ortho":
        s, cull = cm.model_scene("ortho", 700, 0, W, H, cm.KERNEL_SEEDS["ortho"]), dict(cm.KERNEL_CULL)
        model, coeffs = "ortho", None
    elif variant == "fisheye":
        s, cull = cm.model_scene("fisheye", 700, 0, W, H, cm.KERNEL_SEEDS["fisheye"]), dict(cm.KERNEL_CULL)
        model, coeffs = "fisheye", None
    else:
        s, cull = kb.kernel_scene("A")
        model, coeffs = "fisheye", "A"
    s = kb.cut(s, n)
    run = (lambda: kb.run(coeffs, s, W, H, torch.float64, **cull)) if coeffs else (lambda: cm.run(model, s, W, H, torch.float64, **cull))
    radii = run()[1]["radii"]
    return model, coeffs, s, radii, cm.cotangents(n, 7)


def test_pinhole_scene_has_visible_gaussians_past_the_clamp_on_both_sides():
    s, cull = pinhole_scene()
    radii = cm.run("pinhole", s, W, H, torch.float64, **cull)[1]["radii"]
    sides = clamp_sides(s, radii)
    print("visible past the clamp (x+, x-, y+, y-):", sides, "visible:", int((radii > 0).sum()))
    assert min(sides[:2]) >= 3 and min(sides[2:]) >= 3, sides


@pytest.mark.parametrize("antialiased", [False, True])
@pytest.mark.parametrize("variant", ["pinhole", "ortho", "fisheye", "fisheye_kb"])
def test_reference_against_central_differences(variant, antialiased):
    """The summed per-Gaussian autograd gradient (float64) against central differences of the loss with ONE shared set of
    intrinsics, on 48 Gaussians; pinhole: the clamp is active on visible Gaussians, so the v_cx term of the clamp (the limits
    move with cx) is in the comparison, and is asserted to be there."""
    n = 700 if variant == "pinhole" else 48
    model, coeffs, s, radii, cot = _case(variant, n)
    if variant == "pinhole":   # a handful: every visible Gaussian past the clamp and a few inside it
        vm, K = s["viewmat"].astype(np.float64), s["K"].astype(np.float64)
        p = s["means"].astype(np.float64) @ vm[:3, :3].T + vm[:3, 3]
        xr = p[:, 0] / p[:, 2]
        past = (radii > 0) & ((xr > (1.15 * W - K[0, 2]) / K[0, 0]) | (xr < -(K[0, 2] + 0.15 * W) / K[0, 0]))
        pick = np.concatenate([np.flatnonzero(past)[:6], np.flatnonzero((radii > 0) & ~past)[:10], np.flatnonzero(radii == 0)[:2]])
        assert past.sum() >= 2
        s = dict(s, **{k: s[k][pick] for k in ("means", "quats", "scales", "opacities")})
        radii, cot = radii[pick], {k: v[pick] for k, v in cot.items()}
    assert (radii > 0).sum() >= 5
    ref = ig.project_grads(model, coeffs, s, W, H, radii, cot, antialiased=antialiased)
    assert not ref["terms"][radii == 0].any()                       # (a culled Gaussian contributes exact zeros)
    x0 = ig.intrinsics_leaf(s["K"], coeffs, 1, torch.float64).detach().numpy()[0][:8 if coeffs else 4]
    f = lambda x: ig.project_loss_at(model, coeffs is not None, s, W, H, radii, cot, x, antialiased=antialiased)  # noqa: E731
    fd = ig.central_difference(f, x0, FD_STEP_K)
    if coeffs:
        fd[4:] = ig.central_difference(f, x0, FD_STEP_C)[4:]
    err = np.abs(fd - ref["sum"]) / ref["norm"]
    print(f"{variant} aa={antialiased}: |fd - autograd| / sum |term| per entry:", " ".join(f"{e:.1e}" for e in err))
    assert np.all(ref["norm"] > 0) and np.all(err <= FD_TOL), err
    if variant == "fisheye_kb":
        zero = ig.project_grads(model, "zero", s, W, H, radii, cot, antialiased=antialiased)
        assert np.all(np.abs(zero["sum"][4:]) > 0)                  # (the gradient at the plain fisheye starts a calibration)
    if variant == "pinhole":
        # inside the clamp the cx term is the means2d cotangent alone; past it the clamp's own term, vJ[0][2] / z, joins
        k = len(pick) - 2
        extra = np.abs(ref["terms"][:k, 2] - cot["means2d"][:k, 0].astype(np.float64)) / np.abs(ref["terms"][:k, 2])
        print("clamp term of v_cx as a share of the term, past the clamp:", extra[:past.sum()][:6], "inside:", extra[6:k].max())
        n_past = min(int(past.sum()), 6)
        assert np.all(extra[:n_past] > 1e-6) and np.all(extra[n_past:] < 1e-12)


# -- IntrinsicsDelta ---------------------------------------------------------------------------------------------------------------

def _camera(model="fisheye", coeffs=kb.COEFFS["A"], K=True):
    from gags_amd.scene import Camera
    Kmat = cm.intrinsics(model, W, H) if K else None
    return Camera(np.eye(3), np.zeros(3), 1.0, 0.8, W, H, device="cpu", camera_model=model, K=Kmat,
                  radial_coeffs=coeffs if model == "fisheye" else None)


def test_intrinsics_delta_at_zero_gives_the_cameras_values_bit_for_bit():
    from gags_amd.pose import IntrinsicsDelta
    intr = IntrinsicsDelta(3)
    assert [tuple(p.shape) for p in (intr.log_focal, intr.principal, intr.coeffs)] == [(3, 2), (3, 2), (3, 4)]
    assert all(not bool(p.any()) for p in intr.parameters()) and len(list(intr.parameters())) == 3
    for model, coeffs in (("fisheye", kb.COEFFS["A"]), ("fisheye", None), ("ortho", None), ("pinhole", None)):
        cam = _camera(model, coeffs)
        out = intr.camera(cam, 2)
        assert out is not cam and out.world_view_transform is cam.world_view_transform and out.image_width == cam.image_width
        assert out.K.shape == (3, 3) and out.K.dtype == torch.float32 and out.K.requires_grad
        assert np.array_equal(out.K.detach().numpy().view(np.uint32), np.asarray(cam.K, np.float32).view(np.uint32))
        if model == "fisheye":
            want = np.zeros(4, np.float32) if coeffs is None else np.asarray(coeffs, np.float32)
            assert out.radial_coeffs.shape == (4,) and out.radial_coeffs.requires_grad
            assert np.array_equal(out.radial_coeffs.detach().numpy().view(np.uint32), want.view(np.uint32))
        else:
            assert getattr(out, "radial_coeffs", None) is None
        assert cam.K is not out.K and isinstance(cam.K, np.ndarray)      # (the camera itself is untouched)
    # a pinhole camera without K: render()'s FoV -> K
    from gags_amd.gaussian_renderer import _intrinsics
    cam = _camera("pinhole", None, K=False)
    assert torch.equal(intr.camera(cam).K.detach(), _intrinsics(cam, torch.device("cpu"), {}))


def test_intrinsics_delta_values_gradients_and_groups():
    from gags_amd.pose import IntrinsicsDelta
    intr = IntrinsicsDelta(2)
    with torch.no_grad():
        intr.log_focal[1] = torch.tensor([0.02, -0.01])
        intr.principal[1] = torch.tensor([1.5, -2.0])
        intr.coeffs[1] = torch.tensor([0.01, 0.0, -0.002, 0.0])
    cam = _camera()
    K0 = torch.tensor(cam.K)
    out = intr.camera(cam, group=1)
    want = torch.tensor([[K0[0, 0] * np.exp(np.float32(0.02)), 0, K0[0, 2] + 1.5], [0, K0[1, 1] * np.exp(np.float32(-0.01)), K0[1, 2] - 2.0],
                         [0, 0, 1]])
    assert torch.allclose(out.K.detach(), want, rtol=1e-6, atol=0)
    assert torch.equal(out.K.detach()[[0, 1, 1, 2, 2, 2], [1, 0, 0, 0, 1, 2]], torch.tensor([0.0, 0, 0, 0, 0, 1]))
    assert torch.allclose(out.radial_coeffs.detach(), torch.tensor(kb.COEFFS["A"]) + intr.coeffs[1].detach(), rtol=1e-6, atol=0)
    (out.K * torch.arange(9.0).reshape(3, 3)).sum().backward(retain_graph=True)
    out.radial_coeffs.sum().backward()
    assert not bool(intr.log_focal.grad[0].any()) and not bool(intr.principal.grad[0].any()) and not bool(intr.coeffs.grad[0].any())
    assert torch.allclose(intr.log_focal.grad[1], torch.tensor([0.0, 4.0]) * out.K.detach()[[0, 1], [0, 1]])
    assert torch.equal(intr.principal.grad[1], torch.tensor([2.0, 5.0])) and torch.equal(intr.coeffs.grad[1], torch.ones(4))
    assert torch.equal(intr.camera(cam).K.detach(), K0)              # (group 0 is still at zero)


def test_intrinsics_delta_refuses_bad_arguments():
    from gags_amd.pose import IntrinsicsDelta
    with pytest.raises(ValueError):
        IntrinsicsDelta(0)
    intr = IntrinsicsDelta(2)
    cam = _camera()
    for group in (-1, 2):
        with pytest.raises(ValueError):
            intr.camera(cam, group)
    bad = copy.copy(cam)
    bad.K = np.eye(4, dtype=np.float32)
    with pytest.raises(ValueError):
        intr.camera(bad)
    bad = copy.copy(cam)
    bad.radial_coeffs = np.zeros(3, np.float32)
    with pytest.raises(ValueError):
        intr.camera(bad)
    with pytest.raises(ValueError):
        intr.camera(types.SimpleNamespace(camera_model="ortho", image_width=W, image_height=H, FoVx=1.0, FoVy=0.8))


def test_intrinsics_delta_composes_with_pose_delta():
    from gags_amd.pose import IntrinsicsDelta, PoseDelta
    intr, poses = IntrinsicsDelta(1), PoseDelta(2)
    cam = _camera()
    with torch.no_grad():
        poses.delta[1] = torch.tensor([0.1, -0.2, 0.05, 0.01, 0.02, -0.03])
        intr.log_focal[0, 0] = 0.03
    a = intr.camera(poses.camera(cam, 1), 0)
    b = poses.camera(intr.camera(cam, 0), 1)
    for c in (a, b):
        assert c.K.requires_grad and c.radial_coeffs.requires_grad and c.world_view_transform.requires_grad
    assert torch.equal(a.K, b.K) and torch.equal(a.radial_coeffs, b.radial_coeffs)
    assert torch.equal(a.world_view_transform, b.world_view_transform) and torch.equal(a.camera_center, b.camera_center)
    (a.K.sum() + a.world_view_transform.sum()).backward()
    assert bool(intr.log_focal.grad.any()) and bool(poses.delta.grad[1].any())


def test_render_refuses_a_malformed_trainable_camera_before_any_launch():
    """A trainable K / radial_coeffs of the wrong dtype, shape or device is a ValueError out of render()'s intrinsics step (the
    model's tensors here live on the CPU: nothing could be launched)."""
    from gags_amd import gaussian_renderer as GR
    dev = torch.device("cpu")
    cam = _camera()
    ok = copy.copy(cam)
    ok.K = torch.tensor(cam.K).requires_grad_(True)
    K, c = GR._intrinsics_trainable(ok, dev)
    assert K is ok.K and c.dtype == torch.float32 and tuple(c.shape) == (4,) and not c.requires_grad
    ok.radial_coeffs = torch.zeros(4, requires_grad=True)
    ok.K = cam.K
    K, c = GR._intrinsics_trainable(ok, dev)
    assert c is ok.radial_coeffs and tuple(K.shape) == (3, 3) and K.dtype == torch.float32
    for K, c in ((torch.eye(3, dtype=torch.float64, requires_grad=True), None), (torch.ones(9, requires_grad=True), None),
                 (torch.ones(3, 3, device="meta", requires_grad=True), None), (cam.K, torch.zeros(1, 4, requires_grad=True)),
                 (cam.K, torch.zeros(4, dtype=torch.float64, requires_grad=True))):
        bad = copy.copy(cam)
        bad.K, bad.radial_coeffs = K, c
        with pytest.raises(ValueError):
            GR._intrinsics_trainable(bad, dev)
    none = copy.copy(cam)
    none.K, none.radial_coeffs = None, torch.zeros(4, requires_grad=True)
    with pytest.raises(ValueError):
        GR._intrinsics_trainable(none, dev)


def test_table_ahead_counts_the_coefficients():
    from gags_amd.rasterization import _table_ahead
    t = lambda *shape, rg=False: torch.zeros(*shape, requires_grad=rg)  # noqa: E731
    base = (t(4, 3), t(4, 4), t(4, 3), t(4), t(4, 16), t(1, 4, 4), t(1, 3, 3), None, False, "RGB", False)
    assert _table_ahead(*base)[2] == (False,) * 5
    assert _table_ahead(*base, radial_coeffs=t(4))[2] == (False,) * 5
    assert _table_ahead(*base, radial_coeffs=t(4, rg=True))[2] == (True, True, False, False, False)
    assert _table_ahead(*base, True, t(4, rg=True))[2] == (True, True, False, True, False)       # (aa: the compensations)
    withK = base[:6] + (t(1, 3, 3, rg=True),) + base[7:]
    assert _table_ahead(*withK)[2] == (True, True, False, False, False)


# -- the C entries -----------------------------------------------------------------------------------------------------------------

def test_calib_entries_are_declared_exported_and_bound(lib):
    from gags_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gags_raster.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("gags_project_bwd_calib", "gags_project_calib_partials"):
        assert re.search(r"\b" + name + r"\s*\(", header) and hasattr(raw, name) and name in _lib.SIGNATURES
        decl = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", header, re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
    cam, calib = _lib.SIGNATURES["gags_project_bwd_cam"], _lib.SIGNATURES["gags_project_bwd_calib"]
    # gags_project_bwd_cam's list with v_K, v_coeffs behind v_viewmat
    assert calib[0] is cam[0] and calib[1] == cam[1][:24] + [ctypes.c_void_p, ctypes.c_void_p] + cam[1][24:]
    assert _lib.SIGNATURES["gags_project_calib_partials"] == (ctypes.c_int64, [ctypes.c_int])
    for const in ("GAGS_PROJ_RAW", "GAGS_PROJ_AA", "GAGS_PROJ_POSE", "GAGS_PROJ_KB", "GAGS_CALIB_PARTIAL_FLOATS"):
        assert int(re.search(r"#define\s+" + const + r"\s+(\d+)", header).group(1)) == getattr(_lib, const), const
    assert _lib.GAGS_CALIB_PARTIAL_FLOATS == 12 + 6 + 4
    assert lib.gags_abi_version() == 2
    assert [lib.gags_project_calib_partials(n) for n in (0, 1, 256, 257, 700)] == [1, 1, 1, 2, 3]


def _calib_args(n, ptrs=None, partials_bytes=0, w=16, h=16):
    p = [None] * 20 if ptrs is None else ptrs
    # means quats scales logit | modifier | viewmat K | w h eps | radii vm2 vdepth vcon vopac vcomp | vmeans vq vs vlogit vvm vK vcoeffs partials
    return (n, p[0], p[1], p[2], p[3], 1.0, p[4], p[5], w, h, 0.3, *p[6:20], partials_bytes, None)


def test_calib_entry_refuses_bad_arguments_before_any_launch(lib):
    """Every GAGS_EINVAL case of include/gags_raster.h returns on a machine without a GPU: nothing was launched (the pointers
    are host addresses and are never dereferenced).  The flag bits gags_project_bwd_cam refuses stay refused there."""
    from gags_amd import _lib
    EINVAL = -1
    POSE, KB = _lib.GAGS_PROJ_POSE, _lib.GAGS_PROJ_KB
    buf = (ctypes.c_float * 4096)()
    P = ctypes.c_void_p(ctypes.addressof(buf))
    allp = [P] * 20
    without = lambda *missing: [None if i in missing else P for i in range(20)]  # noqa: E731
    need = lib.gags_project_calib_partials(700) * _lib.GAGS_CALIB_PARTIAL_FLOATS * 4
    assert need == 3 * 88
    for model in (-1, 3, 7):
        assert lib.gags_project_bwd_calib(model, 0, *_calib_args(700, allp, need)) == EINVAL
    for model in (0, 1, 2):
        for flags in (8, 16, 64, 128, -1):
            assert lib.gags_project_bwd_calib(model, flags, *_calib_args(700, allp, need)) == EINVAL
            assert lib.gags_project_bwd_cam(model, flags, *_calib_args(700, allp, need)[:22], *_calib_args(700, allp, need)[24:]) == EINVAL
        for base in (0, 1, 2, 3):
            for flags in (base, base | POSE) + ((base | KB, base | KB | POSE) if model == 2 else ()):
                args = lambda n=700, p=allp, b=need, **kw: _calib_args(n, p, b, **kw)  # noqa: E731
                assert lib.gags_project_bwd_calib(model, flags, *args(n=-1)) == EINVAL
                assert lib.gags_project_bwd_calib(model, flags, *args(w=0)) == EINVAL
                assert lib.gags_project_bwd_calib(model, flags, *args(h=-3)) == EINVAL
                assert lib.gags_project_bwd_calib(model, flags, *args(b=need - 1)) == EINVAL       # a short partials buffer
                assert lib.gags_project_bwd_calib(model, flags, *args(b=3 * 48)) == EINVAL         # (the pose entry's size)
                assert lib.gags_project_bwd_calib(model, flags, *args(b=0)) == EINVAL
                assert lib.gags_project_bwd_calib(model, flags, *args(p=[None] * 20)) == EINVAL
                for missing in (0, 1, 2, 4, 5, 6, 7, 9, 17, 19):       # inputs, v_K, partials
                    assert lib.gags_project_bwd_calib(model, flags, *args(p=without(missing))) == EINVAL, (flags, missing)
                if flags & POSE:
                    assert lib.gags_project_bwd_calib(model, flags, *args(p=without(16))) == EINVAL    # v_viewmat
                if flags & KB:
                    assert lib.gags_project_bwd_calib(model, flags, *args(p=without(18))) == EINVAL    # v_coeffs
                if flags & 1:    # RAW writes the logit's gradient from the logits
                    assert lib.gags_project_bwd_calib(model, flags, *args(p=without(3))) == EINVAL
                # n = 0 with a NULL v_K or partials is refused as well: v_K is always written
                assert lib.gags_project_bwd_calib(model, flags, *args(n=0, p=without(17))) == EINVAL
                assert lib.gags_project_bwd_calib(model, flags, *args(n=0, p=without(19))) == EINVAL
        if model != 2:
            for flags in (KB, KB | 1, KB | POSE):
                assert lib.gags_project_bwd_calib(model, flags, *_calib_args(700, allp, need)) == EINVAL
