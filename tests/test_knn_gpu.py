"""N9 on the GPU: gags_amd.knn.dist2 (csrc/knn.hip) against the restatement tests/knn_ref.py on the clouds it builds, and
GaussianModel.create_from_pcd against the reference's own result (tests/golden/init_vectors.npz).

Two contracts, tested apart so that a failure says which one broke:
  * BIT EQUALITY with the float32 brute force: the three smallest values of an exactly specified float32 expression do not
    depend on the order they are found in, so any exact traversal gives the same bits.
  * 1e-6 relative of the float64 brute force: the bound derived in tests/test_knn_cpu.py (8 x 2^-24 = 4.8e-7) with a factor
    of two of headroom.
create_from_pcd: positions, zero bands, rotations, the semantic feature and max_radii2D exactly; opacity and the SH band 0
within one float32 ulp (one division, one logarithm); the log-scales within 1e-6 + 1e-6 |s| of the fixture, whose distances
are the FLOAT64 brute force rounded to float32: dist2's 4.8e-7 halved by the square root, plus the logarithm's ulp."""
import os
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import knn_ref as K  # noqa: E402

DEV = torch.device("cuda", 0)
Z = np.load(os.path.join(HERE, "golden", "init_vectors.npz"))
CONFIGS = [str(c) for c in Z["configs"]]
# arguments/__init__.py:76-94
OPT = types.SimpleNamespace(iterations=30_000, position_lr_init=0.00016, position_lr_final=0.0000016, position_lr_delay_mult=0.01,
                            position_lr_max_steps=30_000, feature_lr=0.0025, opacity_lr=0.05, scaling_lr=0.005,
                            rotation_lr=0.001, semantic_feature_lr=0.001, percent_dense=0.01, lambda_dssim=0.2,
                            densification_interval=100, opacity_reset_interval=3000, densify_from_iter=500,
                            densify_until_iter=15_000, densify_grad_threshold=0.0002)


def _dist2(x):
    from gags_amd import knn
    return knn.dist2(torch.as_tensor(np.array(x) if isinstance(x, np.ndarray) else x).to(DEV))


def _ulps(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("name", K.CASES)
def test_bit_equal_to_the_float32_brute_force(name):
    got = _dist2(K.cloud(name))
    want = torch.from_numpy(K.expected(name)[0].copy()).to(DEV)
    assert got.dtype == torch.float32 and got.shape == want.shape
    bad = (got != want).nonzero().flatten()
    print(f"\n{name}: N = {got.shape[0]}, {bad.numel()} entries differ from the float32 restatement")
    assert torch.equal(got, want), (name, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())


@pytest.mark.parametrize("name", K.CASES)
def test_within_1e6_relative_of_the_float64_brute_force(name):
    got = _dist2(K.cloud(name)).cpu().numpy().astype(np.float64)
    r64 = K.expected(name)[1]
    err = np.abs(got - r64)
    rel = float((err / np.where(r64 > 0, r64, 1.0)).max())
    print(f"\n{name}: max relative error {rel:.3e} of float64 (bound 1e-6)")
    assert (err <= 1e-6 * r64).all(), (name, rel)


def test_repeatable_and_independent_of_the_inputs_layout_and_dtype():
    x = torch.from_numpy(K.cloud("box_4p1").copy()).to(DEV)
    first = _dist2(x)
    assert torch.equal(_dist2(x), first)
    assert torch.equal(_dist2(x.double()), first)                      # float32-representable float64: converted, same bits
    wide = torch.full((x.shape[0], 4), 7.0, device=DEV)
    wide[:, :3] = x
    view = wide[:, :3]                                                 # a [N, 3] view of [N, 4] rows: not contiguous
    assert not view.is_contiguous()
    assert torch.equal(_dist2(view), first)
    assert torch.equal(_dist2(wide[:, [0, 1, 2]]), first)              # the same columns by index
    assert torch.equal(_dist2(x.t().contiguous().t()), first)          # column-major
    assert torch.equal(_dist2(x.requires_grad_(True)), first) and not _dist2(x).requires_grad
    from gags_amd import distCUDA2
    assert torch.equal(distCUDA2(x), first)


def test_four_points_use_all_three_others():
    x = K.cloud("min4")
    want = np.empty(4, np.float32)
    for i in range(4):
        d = []
        for j in range(4):
            if j != i:
                dx, dy, dz = (x[j] - x[i]).astype(np.float32)
                d.append(np.float32(np.float32(dx * dx + dy * dy) + dz * dz))
        b0, b1, b2 = sorted(d)
        want[i] = np.float32(np.float32(b0 + b1) + b2) / np.float32(3)
    assert np.array_equal(_dist2(x).cpu().numpy(), want)


@pytest.mark.parametrize("name", CONFIGS)
def test_create_from_pcd_equals_the_references(name):
    from gags_amd.scene import BasicPointCloud, GaussianModel
    shd, size, speedup, lr_scale = Z[name + "_par"]
    pcd = BasicPointCloud(points=Z["points"], colors=Z["colors"], normals=np.zeros_like(Z["points"]))
    m = GaussianModel(int(shd))
    m._act_cache = {"stale": None}
    assert m.create_from_pcd(pcd, float(lr_scale), int(size), bool(speedup)) is m
    assert m.__dict__["_act_cache"] == {}  # invalidate_activations() was called
    assert m.active_sh_degree == int(Z[name + "_active_sh_degree"]) == 0 and m.spatial_lr_scale == float(Z[name + "_spatial_lr_scale"])
    attrs = ["_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity"] + (["_semantic_feature"] if size else [])
    got = {}
    for attr in attrs:
        p = getattr(m, attr)
        assert isinstance(p, torch.nn.Parameter) and p.requires_grad and p.is_cuda and p.dtype == torch.float32, attr
        assert p.is_contiguous() and tuple(p.shape) == Z[name + attr].shape, attr
        got[attr] = p.detach().cpu().numpy()
    if not size:
        assert m._semantic_feature is None
    assert not isinstance(m.max_radii2D, torch.nn.Parameter) and m.max_radii2D.is_cuda
    assert np.array_equal(m.max_radii2D.cpu().numpy(), Z[name + "_max_radii2D"])
    for attr in ("_xyz", "_features_rest", "_rotation") + (("_semantic_feature",) if size else ()):
        assert np.array_equal(got[attr], Z[name + attr]), attr
    for attr in ("_opacity", "_features_dc"):
        u = int(_ulps(got[attr], Z[name + attr]).max())
        print(f"\n{name}{attr}: {u} ulp from the fixture (bound 1)")
        assert u <= 1, attr
    s = Z[name + "_scaling"]
    err = np.abs(got["_scaling"] - s)
    print(f"\n{name}_scaling: max error {err.max():.3e} (bound 1e-6 + 1e-6 |s|, |s| up to {np.abs(s).max():.2f})")
    assert (err <= 1e-6 + 1e-6 * np.abs(s)).all()
    assert (got["_scaling"][:4] == got["_scaling"][0, 0]).all() and float(m.get_scaling.min()) > 3e-4  # four coincident points: the clamp at 1e-7


def test_the_rgb_stage_runs_on_a_model_created_here():
    """create_from_pcd -> training_setup_rgb(opt) -> three iterations of render, photometric loss, backward, statistics, step
    and densify_and_prune, with the reference's default optimisation parameters.  Asserted: finite gradients of the
    parameters' shapes, a finite loss, one length for every parameter, Adam moment and statistic after densification, and the
    fresh model's activated scales.  (The semantic feature is not rendered by the RGB pass: it may have no gradient.)  Not
    asserted: that the loss decreases."""
    from gags_amd import densify, knn, losses
    from gags_amd.gaussian_renderer import render
    from gags_amd.scene import BasicPointCloud, Camera, GaussianModel, focal2fov, nerfpp_norm
    x = K.cloud("uniform")[:200]
    colors = np.random.default_rng(77).random((200, 3))
    w, h = 64, 48
    # the cloud fills [0, 1)^3: a camera at (0.5, 0.5, -2) looking down +z sees all of it
    cam = Camera(np.eye(3), np.array([-0.5, -0.5, 2.0]), focal2fov(0.9 * w, w), focal2fov(0.9 * w, h), w, h, device=DEV)
    extent = float(nerfpp_norm([cam, Camera(np.eye(3), np.array([0.5, -0.5, 2.0]), 1.0, 1.0, w, h, device="cpu")])["radius"])
    assert extent > 0
    pc = GaussianModel(3).create_from_pcd(BasicPointCloud(x, colors, np.zeros_like(x)), extent)
    d2 = knn.dist2(torch.from_numpy(x.copy()).to(DEV))
    want = torch.sqrt(torch.clamp_min(d2, 1e-7))[:, None].expand(-1, 3)
    assert ((pc.get_scaling.detach() - want).abs() <= 1e-6 * want).all()
    opt = pc.training_setup_rgb(OPT)
    assert pc.spatial_lr_scale == extent
    assert [g["lr"] for g in opt.param_groups if g["name"] == "xyz"] == [OPT.position_lr_init * extent]
    bg = torch.zeros(3, device=DEV)
    gt = torch.rand(3, h, w, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    stored = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation", "_semantic_feature")
    for it in range(1, 4):
        pc.update_learning_rate(it)
        opt.zero_grad(set_to_none=True)
        pkg = render(cam, pc, None, bg, feature_mode=False)
        loss = losses.photometric_loss(pkg["render"], gt, OPT.lambda_dssim)
        loss.backward()
        assert bool(torch.isfinite(loss)), it
        for a in stored:
            p = getattr(pc, a)
            assert a == "_semantic_feature" or p.grad is not None, (it, a)
            if p.grad is not None:
                assert p.grad.shape == p.shape and bool(torch.isfinite(p.grad).all()), (it, a)
        densify.accumulate(pc, pkg)
        opt.step()
        pc.densify_and_prune(OPT.densify_grad_threshold, 0.005, extent, None, generator=torch.Generator(device=DEV).manual_seed(it))
        n = pc._xyz.shape[0]
        for a in stored:
            p = getattr(pc, a)
            assert p.shape[0] == n, (it, a)
            st = opt.state.get(p, {})
            assert all(st[k].shape == p.shape for k in ("exp_avg", "exp_avg_sq") if k in st), (it, a)
        assert pc.xyz_gradient_accum.shape == (n, 1) and pc.denom.shape == (n, 1) and pc.max_radii2D.shape == (n,)
    print(f"\n200 points -> {n} after three densifications, loss {float(loss.detach()):.4f}")
