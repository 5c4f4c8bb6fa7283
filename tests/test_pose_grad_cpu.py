"""N17 without a GPU: the pose gradient's rule (tests/pose_ref.py) against central differences, the numpy restatement of the
kernel's per-Gaussian formula against autograd, PoseDelta, the new entries of the C ABI, and pose refinement on a tiny frozen
scene in float64 -- the reference the GPU test of the same case is measured against."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import pose_ref
from gags_amd import _lib as L
from helpers import GENERAL_CAMERAS, clamp_census, general_camera, general_scene

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
MULT = 30.0   # splat size of tests/test_general_camera_gpu.py: Gaussians beyond the tangent clamp stay on screen


def _cot(n, seed):
    rng = np.random.default_rng(seed)
    return dict(means2d=rng.standard_normal((n, 2)), depths=rng.standard_normal(n), conics=rng.standard_normal((n, 3)),
                comp=rng.standard_normal(n))


def _clamp_sets(s, vm, w, h):
    """Which Gaussians sit beyond the tangent clamp in x / in y under the pose vm (float64)."""
    K = s["K"].astype(np.float64)
    p = s["means"].astype(np.float64) @ vm[:3, :3].T + vm[:3, 3]
    xr, yr = p[:, 0] / p[:, 2], p[:, 1] / p[:, 2]
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    return ((xr > (w - cx) / fx + 0.15 * w / fx) | (xr < -(cx / fx + 0.15 * w / fx)),
            (yr > (h - cy) / fy + 0.15 * h / fy) | (yr < -(cy / fy + 0.15 * h / fy)))


def _central_differences(fn, vm, step):
    g = np.zeros((4, 4))
    for r in range(3):
        for c in range(4):
            d = np.zeros((4, 4))
            d[r, c] = step
            g[r, c] = (fn(vm + d) - fn(vm - d)) / (2 * step)
    return g


# Central differences in float64 with step 1e-6 on entries of size ~1..10: truncation ~ step^2 |f'''| and round-off
# ~ 2.2e-16 |loss| / step, both 1e-10 .. 1e-9 of the gradient here; a wrong term in the rule is an error of order 1.
FD_STEP, FD_TOL = 1e-6, 1e-6


@pytest.mark.parametrize("antialiased", [False, True])
@pytest.mark.parametrize("cam", list(GENERAL_CAMERAS))
def test_autograd_pose_gradient_against_central_differences(oracle, cam, antialiased):
    """Float64 autograd v_viewmat of pose_ref against central differences over the 12 entries, n = 60, with the oracle's radii and
    the blend decisions held fixed so that the function is smooth: the projection-only loss (random cotangents on means2d,
    depth, conics, compensation, masked to radii > 0) and the composited loss (through aa_ref.composite, with a background
    and a non-zero v_alpha).  No Gaussian crosses the tx / ty clamp within the step (asserted)."""
    w, h, n, seed = 48, 32, 60, 11
    s = general_scene(n, 3, w, h, seed, scale_mult=MULT, **general_camera(cam, w, h))
    radii, _, depths, _ = oracle.project_fwd(s["means"], s["quats"], s["scales"], s["viewmat"], s["K"], w, h)
    assert (radii > 0).sum() >= 20
    vm = s["viewmat"].astype(np.float64)
    base = _clamp_sets(s, vm, w, h)
    for r in range(3):
        for c in range(4):
            for sgn in (-1, 1):
                d = np.zeros((4, 4))
                d[r, c] = sgn * FD_STEP
                moved = _clamp_sets(s, vm + d, w, h)
                assert np.array_equal(moved[0], base[0]) and np.array_equal(moved[1], base[1])
    cot = _cot(n, seed)
    g = pose_ref.project_grads(s, w, h, radii, cot, antialiased=antialiased)["viewmat"]
    fd = _central_differences(lambda m: float(pose_ref.project_loss(s, w, h, radii, cot, antialiased=antialiased, viewmat=m)[0].detach()),
                              vm, FD_STEP)
    e = pose_ref.rel_err(g, fd)
    print(f"\n{cam} aa={antialiased} projection: autograd vs central differences {e:.2e}")
    assert e <= FD_TOL and np.all(g[3] == 0) and np.linalg.norm(g) > 0
    # composited
    rng = np.random.default_rng(seed + 1)
    v_out, v_alpha, bg = rng.standard_normal((h, w, 3)), rng.standard_normal((h, w)), np.full(3, 0.25)
    ref = pose_ref.full(s, w, h, s["colors"], bg, v_out, v_alpha, radii, depths, antialiased=antialiased)
    assert ref["n_blend"] > 100

    def loss(m):
        vmt = torch.tensor(m, dtype=torch.float64)
        out, alphas, _, _ = pose_ref.render(s, w, h, s["colors"], bg, radii, depths, viewmat=vmt, antialiased=antialiased,
                                            include=ref["include"])
        return float((out * torch.tensor(v_out)).sum() + (alphas * torch.tensor(v_alpha)).sum())
    fd = _central_differences(loss, vm, FD_STEP)
    e = pose_ref.rel_err(ref["g"]["viewmat"], fd)
    print(f"{cam} aa={antialiased} composited: autograd vs central differences {e:.2e}")
    assert e <= FD_TOL and np.all(ref["g"]["viewmat"][3] == 0)


@pytest.mark.parametrize("antialiased,with_depths", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("cam", list(GENERAL_CAMERAS))
def test_kernel_formula_restated_in_numpy_equals_autograd(oracle, cam, antialiased, with_depths):
    """The per-Gaussian terms the kernel adds (pose_ref.pose_terms, chain rule by hand), summed over N, against float64 autograd:
    equal to round-off.  Bound: 1e-12 x the cancellation of the sum (sum of the terms' norms / norm of the sum), i.e. some
    thousand float64 roundings per Gaussian.  n = 700 at the sizes of FULL_CASES, with >= 20 visible Gaussians beyond the clamp
    in x and in y, so that the clamped branch of the rule carries weight; culled Gaussians contribute exactly zero."""
    w, h, n, seed = 97, 61, 700, 21
    s = general_scene(n, 3, w, h, seed, scale_mult=MULT, **general_camera(cam, w, h))
    radii = oracle.project_fwd(s["means"], s["quats"], s["scales"], s["viewmat"], s["K"], w, h)[0]
    nx, ny, nvis, ncull = clamp_census(s, w, h, radii)
    assert nx >= 20 and ny >= 20 and nvis > 0 and ncull > 0, (nx, ny, nvis, ncull)
    cot = _cot(n, seed)
    if not with_depths:
        cot["depths"] = None
    g = pose_ref.project_grads(s, w, h, radii, cot, antialiased=antialiased)["viewmat"]
    terms = pose_ref.pose_terms(s, w, h, radii, cot["means2d"], cot["depths"], cot["conics"], cot["comp"], antialiased=antialiased)
    assert terms.shape == (n, 12) and np.all(terms[radii <= 0] == 0) and np.all(np.abs(terms[radii > 0]).sum(1) > 0)
    total = terms.sum(0)
    cond = np.linalg.norm(terms, axis=1).sum() / np.linalg.norm(total)
    e = pose_ref.rel_err(total, g[:3].reshape(12))
    print(f"\n{cam} aa={antialiased} depths={with_depths}: restatement vs autograd {e:.2e} (cancellation {cond:.1f})")
    assert e <= 1e-12 * cond
    if antialiased:   # the compensation's cotangent is part of it
        plain = pose_ref.pose_terms(s, w, h, radii, cot["means2d"], cot["depths"], cot["conics"], None, antialiased=True)
        assert pose_ref.rel_err(plain.sum(0), g[:3].reshape(12)) > 1e-6


# -- PoseDelta ---------------------------------------------------------------------------------------------------------------------

def _hat(o):
    z = torch.zeros((), dtype=o.dtype)
    return torch.stack([z, -o[2], o[1], o[2], z, -o[0], -o[1], o[0], z]).reshape(3, 3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_pose_delta_at_zero_is_the_identity_bit_for_bit(dtype):
    from gags_amd.pose import PoseDelta, so3_exp  # noqa: F401
    g = torch.Generator().manual_seed(3)
    vm = torch.randn(4, 4, generator=g, dtype=torch.float64).to(dtype) * 7.3
    pd = PoseDelta(3).to(dtype)
    assert pd.delta.shape == (3, 6) and not bool(pd.delta.any()) and [n for n, _ in pd.named_parameters()] == ["delta"]
    for idx in range(3):
        assert torch.equal(pd(vm, idx), vm)


def test_pose_delta_gradient_at_zero_matches_autograd_of_the_matrix_exponential():
    from gags_amd.pose import PoseDelta, so3_exp  # noqa: F401
    g = torch.Generator().manual_seed(4)
    vm = torch.randn(4, 4, generator=g, dtype=torch.float64)
    vm[3] = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64)
    W = torch.randn(4, 4, generator=g, dtype=torch.float64)
    pd = PoseDelta(2).double()
    (pd(vm, 1) * W).sum().backward()
    got = pd.delta.grad
    assert bool(torch.isfinite(got).all()) and not bool(got[0].any())
    d = torch.zeros(6, dtype=torch.float64, requires_grad=True)
    T = torch.cat([torch.cat([torch.linalg.matrix_exp(_hat(d[3:])), d[:3, None]], 1),
                   torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=torch.float64)], 0)
    v_viewmat = W   # d <W, out> / d out
    ((T @ vm) * W).sum().backward()
    assert torch.allclose(got[1], d.grad, rtol=1e-13, atol=1e-13)
    # d / d tau IS the translation column of the rasterizer's v_viewmat when the correction starts at zero
    assert torch.equal(got[1, :3], v_viewmat[:3, 3])


@pytest.mark.parametrize("norm", [1e-9, 1e-4, 1.0])
def test_pose_delta_rotation_stays_orthonormal(norm):
    from gags_amd.pose import PoseDelta, so3_exp  # noqa: F401
    axis = torch.tensor([0.3, -0.5, 0.8], dtype=torch.float64)
    o = (axis / axis.norm() * norm).requires_grad_(True)
    Rg = so3_exp(o)
    R = Rg.detach()
    assert float((R @ R.T - torch.eye(3, dtype=torch.float64)).abs().max()) <= 1e-12
    assert abs(float(torch.linalg.det(R)) - 1.0) <= 1e-12
    assert float((R - torch.linalg.matrix_exp(_hat(o.detach()))).abs().max()) <= 1e-12
    Rg.sum().backward()
    assert bool(torch.isfinite(o.grad).all())


def test_pose_delta_camera_is_a_shallow_copy_with_dependent_fields_recomputed():
    from gags_amd.pose import PoseDelta, so3_exp  # noqa: F401
    from gags_amd.scene import Camera
    cam = Camera(np.eye(3), np.array([0.1, -0.2, 3.0]), 0.9, 0.7, 48, 32, device="cpu")
    cam.projection_matrix = torch.randn(4, 4, generator=torch.Generator().manual_seed(1))
    cam.full_proj_transform = cam.world_view_transform @ cam.projection_matrix
    pd = PoseDelta(1)
    same = pd.camera(cam, 0)
    assert same is not cam and same.FoVx == cam.FoVx and same.image_width == 48
    assert torch.equal(same.world_view_transform, cam.world_view_transform)
    assert torch.allclose(same.camera_center, cam.camera_center, atol=1e-6)
    with torch.no_grad():
        pd.delta[0] = torch.tensor([0.5, 0.0, -0.25, 0.0, 0.3, 0.0])
    moved = pd.camera(cam, 0)
    w2c = moved.world_view_transform.T
    assert moved.world_view_transform.requires_grad and torch.equal(w2c, pd(cam.world_view_transform.T, 0))
    assert torch.allclose(w2c[:3, :3] @ moved.camera_center + w2c[:3, 3], torch.zeros(3), atol=1e-6)
    assert torch.allclose(moved.full_proj_transform, moved.world_view_transform @ cam.projection_matrix, atol=1e-6)
    assert torch.equal(cam.world_view_transform, same.world_view_transform.detach())   # the original is untouched


# -- the ABI -----------------------------------------------------------------------------------------------------------------------

NEW_ENTRIES = ("gags_project_pose_partials", "gags_project_bwd_pose", "gags_colsum_f32")


def test_new_entries_are_declared_typed_and_exported_and_refuse_bad_arguments_without_launching():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gags_raster.h")).read(), flags=re.S)
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in L.SIGNATURES, name
    assert not any(name.endswith("_scratch_bytes") for name in NEW_ENTRIES)
    for k, v in (("GAGS_POSE_RAW", 1), ("GAGS_POSE_AA", 2)):
        assert re.search(r"^#define\s+%s\s+%d\b" % (k, v), src, flags=re.M) and getattr(L, k) == v
    if not os.path.exists(L.LIB_PATH):
        L.build()
    lib = L.load()
    raw = ctypes.CDLL(L.LIB_PATH)
    assert all(hasattr(raw, name) for name in NEW_ENTRIES)
    assert lib.gags_abi_version() == 2
    # the union of the four backward entries' arguments + flags, v_viewmat, partials, partials_bytes
    assert len(L.SIGNATURES["gags_project_bwd_pose"][1]) == len(L.SIGNATURES["gags_project_bwd_raw_aa"][1]) + 5
    assert [lib.gags_project_pose_partials(n) for n in (0, 1, 256, 257, 70001)] == [1, 1, 1, 2, 274]
    buf = (ctypes.c_float * 4096)()
    P = ctypes.c_void_p(ctypes.addressof(buf))

    def pose(n, v_viewmat=P, partials=P, nbytes=None, flags=0, width=16):
        nbytes = lib.gags_project_pose_partials(max(n, 0)) * 48 if nbytes is None else nbytes
        return lib.gags_project_bwd_pose(flags, n, P, P, P, P, 1.0, P, P, width, 16, 0.3, P, P, P, P, P, P, P, P, P, P,
                                         v_viewmat, partials, nbytes, None)
    # every one of these returns before anything is launched (there is no GPU here: a launch would not return -1)
    for flags in (0, L.GAGS_POSE_RAW, L.GAGS_POSE_AA, L.GAGS_POSE_RAW | L.GAGS_POSE_AA):
        assert pose(-1, flags=flags) == -1
        assert pose(700, v_viewmat=None, flags=flags) == -1
        assert pose(700, partials=None, flags=flags) == -1
        assert pose(700, nbytes=3 * 48 - 1, flags=flags) == -1      # 700 Gaussians are 3 rows
        assert pose(700, nbytes=0, flags=flags) == -1
        assert pose(0, nbytes=47, flags=flags) == -1                # n = 0 still writes through one row's worth of checks
    assert pose(700, flags=4) == -1 and pose(700, width=0) == -1
    assert lib.gags_colsum_f32(-1, 3, P, 1.0, P, 3, None) == -1
    assert lib.gags_colsum_f32(8, 13, P, 1.0, P, 13, None) == -1    # k <= 12
    assert lib.gags_colsum_f32(8, 0, P, 1.0, P, 3, None) == -1
    assert lib.gags_colsum_f32(8, 3, P, 1.0, P, 2, None) == -1      # n_out < k
    assert lib.gags_colsum_f32(8, 3, P, 1.0, None, 3, None) == -1
    assert lib.gags_colsum_f32(8, 3, None, 1.0, P, 3, None) == -1


# -- refinement --------------------------------------------------------------------------------------------------------------------

REFINE_STEPS, REFINE_LR = 40, 0.01


@functools.lru_cache(maxsize=None)
def refinement_case():
    """A tiny frozen scene and a wrong first guess of its camera: n = 40, 48 x 32, D = 3; the true pose turned by 3 degrees
    about a skew axis and moved by 0.2 in the camera frame; the translation column of the world-to-camera matrix is then off by
    0.446, 6 % of the mean scene depth of 7 (translation_error measures that column).  The principal point is in the middle of
    the image, so that the same case runs through render() on the GPU (a Camera has it there)."""
    from gags_amd.pose import PoseDelta, so3_exp  # noqa: F401
    w, h, n = 48, 32, 40
    k = dict(general_camera("pitch_roll", w, h), cx=0.5 * w, cy=0.5 * h)
    s = general_scene(n, 3, w, h, 5, scale_mult=12.0, **k)
    vm_true = s["viewmat"].astype(np.float64)
    axis = np.array([0.5, -0.7, 0.5]) / np.linalg.norm([0.5, -0.7, 0.5])
    P = np.eye(4)
    P[:3, :3] = so3_exp(torch.tensor(axis * np.deg2rad(3.0))).numpy()
    P[:3, 3] = (0.12, -0.10, 0.12)
    assert abs(np.linalg.norm(P[:3, 3]) - 0.2) < 0.01
    return dict(s=s, w=w, h=h, n=n, k=k, vm_true=vm_true, vm0=P @ vm_true, bg=np.full(3, 0.25))


def translation_error(vm, vm_true):
    return float(np.linalg.norm(np.asarray(vm, np.float64)[:3, 3] - np.asarray(vm_true, np.float64)[:3, 3]))


def test_pose_refinement_in_float64_recovers_the_pose(oracle):
    """L1 to the image of the true pose, Adam (lr 0.01) on PoseDelta, 40 steps, everything in float64 through pose_ref.render
    with the fp32 oracle's radii and depth order at each step's pose.  The reference alone must reduce the loss and the
    translation error at least four-fold: the GPU test of the same case (tests/test_pose_grad_gpu.py) asks for two-fold.
    Recorded: loss 0.0214 -> 0.0008 (26.9-fold), translation error 0.446 -> 0.0272 (16.4-fold)."""
    from gags_amd.pose import PoseDelta, so3_exp  # noqa: F401
    c = refinement_case()
    s, w, h = c["s"], c["w"], c["h"]

    def image(vm):
        radii, _, depths, _ = oracle.project_fwd(s["means"], s["quats"], s["scales"], vm.detach().numpy().astype(np.float32),
                                                 s["K"], w, h)
        return pose_ref.render(s, w, h, s["colors"], c["bg"], radii, depths, viewmat=vm)[0]
    with torch.no_grad():
        gt = image(torch.tensor(c["vm_true"]))
    pd = PoseDelta(1).double()
    opt = torch.optim.Adam(pd.parameters(), lr=REFINE_LR)
    vm0 = torch.tensor(c["vm0"])
    losses, terr = [], []
    for _ in range(REFINE_STEPS + 1):
        vm = pd(vm0, 0)
        loss = (image(vm) - gt).abs().mean()
        losses.append(float(loss.detach()))
        terr.append(translation_error(vm.detach().numpy(), c["vm_true"]))
        opt.zero_grad()
        loss.backward()
        opt.step()
    print(f"\nfloat64 refinement: loss {losses[0]:.4f} -> {losses[-1]:.4f} ({losses[0] / losses[-1]:.1f}-fold), "
          f"translation error {terr[0]:.3f} -> {terr[-1]:.4f} ({terr[0] / terr[-1]:.1f}-fold)")
    assert losses[0] / losses[-1] >= 4.0 and terr[0] / terr[-1] >= 4.0
