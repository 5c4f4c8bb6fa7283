"""N7 (csrc/photometric.hip, gags_amd/losses.py: ssim, psnr, photometric_loss) on the GPU, against the reference's own float64
results (tests/golden/photometric_vectors.npz) and, at shapes the fixture does not hold, the float64 restatement
tests/photometric_ref.py evaluated on the host.

The rule for a fixture case: the distance to the reference's float64 result is at most
    max(4 x the distance of the reference's own float32 run for that case, the fixture's floor)
where the distance is |difference| for a scalar and max|difference| / max|float64 gradient| for a gradient, and the floors
(`floor_value`, `floor_grad`) are the largest float32 distances over the cases that are not `flat`.  The factor 4: the kernel
meets the same float32 roundings of its inputs and outputs in another order (11 + 11 taps against 121, partial sums in double);
one sample of the reference's error is not a bound on that.  For PSNR = -(10 / ln 10) ln(mse) an absolute difference d is a
relative difference d ln(10) / 10 of the mean squared error, and that relative difference is what the rule is applied to.
Every test prints the figures it asserts (pytest -s shows them)."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import photometric_ref as R  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]

Z = np.load(os.path.join(ROOT, "golden", "photometric_vectors.npz"))
SHAPES = [(3, 5, 7), (3, 16, 16), (3, 33, 17), (3, 47, 63), (1, 64, 48), (2, 3, 20, 24)]
KINDS = ("near", "rand", "flat")
CASES = [k + "_" + "x".join(map(str, s)) for k in KINDS for s in SHAPES]
FLOOR_V, FLOOR_G = float(Z["floor_value"]), float(Z["floor_grad"])
DEV = "cuda"
BIG = (3, 131, 197)  # 9 x 7 tiles of 16 x 32 per plane, neither size a multiple of a tile side


def pixel_major(t):
    """The same values as the channel-major view of pixel-major memory ([H,W,C] behind [C,H,W]: the rasterizer's layout)."""
    if t.dim() == 3:
        return t.permute(1, 2, 0).contiguous().permute(2, 0, 1)
    return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def grad_dist(g, g64):
    g64 = np.asarray(g64, dtype=np.float64)
    return float(np.abs(g.detach().double().cpu().numpy() - g64).max() / np.abs(g64).max())


def loss_and_grad(x, y, lam=0.2):
    from gags_amd import losses
    x = x.detach().requires_grad_(True)
    loss = losses.photometric_loss(x, y, lam)
    (g,) = torch.autograd.grad(loss, x)
    return loss.detach(), g


def case(name):
    return torch.from_numpy(Z[name + "_x"]).to(DEV), torch.from_numpy(Z[name + "_y"]).to(DEV)


@pytest.mark.parametrize("name", CASES)
def test_fixture_cases_both_layouts(name):
    x, y = case(name)
    l_c, g_c = loss_and_grad(x, y)
    xp = pixel_major(x)
    assert not xp.is_contiguous() or 1 in xp.shape[-3:]
    l_p, g_p = loss_and_grad(xp, y)
    assert l_c.dtype == torch.float32 and l_c.dim() == 0 and g_c.shape == x.shape and g_p.shape == x.shape
    assert torch.equal(l_c, l_p) and torch.equal(g_c, g_p)
    if x.dim() == 3:
        assert g_p.stride() == xp.stride()  # written in x's own layout
    dv, dv_ref = abs(float(l_c) - float(Z[name + "_loss64"])), abs(float(Z[name + "_loss32"]) - float(Z[name + "_loss64"]))
    dg, dg_ref = grad_dist(g_c, Z[name + "_grad64"]), grad_dist(torch.from_numpy(Z[name + "_grad32"]), Z[name + "_grad64"])
    print(f"\n{name}: value {dv:.2e} (reference float32 {dv_ref:.2e}, floor {FLOOR_V:.2e})  "
          f"gradient {dg:.2e} (reference float32 {dg_ref:.2e}, floor {FLOOR_G:.2e})")
    assert dv <= max(4 * dv_ref, FLOOR_V)
    assert dg <= max(4 * dg_ref, FLOOR_G)


@pytest.mark.parametrize("name", CASES)
def test_ssim_psnr_and_per_image_means(name):
    from gags_amd import losses
    x, y = case(name)
    for xx in (x, pixel_major(x)):
        s = losses.ssim(xx, y)
        ds, ds_ref = abs(float(s) - float(Z[name + "_ssim64"])), abs(float(Z[name + "_ssim32"]) - float(Z[name + "_ssim64"]))
        assert s.dim() == 0 and ds <= max(4 * ds_ref, FLOOR_V), (ds, ds_ref)
        p = losses.psnr(xx, y)
        assert p.shape == (x.shape[0], 1) and p.dtype == torch.float32
        k = math.log(10.0) / 10.0
        dp = float(np.abs(p.double().cpu().numpy() - Z[name + "_psnr64"]).max()) * k
        dp_ref = float(np.abs(Z[name + "_psnr32"].astype(np.float64) - Z[name + "_psnr64"]).max()) * k
        assert dp <= max(4 * dp_ref, FLOOR_V), (dp, dp_ref)
        if x.dim() == 4:
            sb = losses.ssim(xx, y, size_average=False)
            assert sb.shape == (x.shape[0],)
            db = float(np.abs(sb.double().cpu().numpy() - Z[name + "_ssimb64"]).max())
            db_ref = float(np.abs(Z[name + "_ssimb32"].astype(np.float64) - Z[name + "_ssimb64"]).max())
            assert db <= max(4 * db_ref, FLOOR_V), (db, db_ref)
        else:
            assert losses.ssim(xx, y, size_average=False).shape == (1,)
    print(f"\n{name}: ssim {ds:.2e} (reference float32 {ds_ref:.2e})  psnr as relative mse {dp:.2e} ({dp_ref:.2e})")


def test_per_image_ssim_gradient_and_ground_truth_refusal():
    """size_average=False sends one cotangent per image down the backward kernel; the ground truth is never differentiated."""
    from gags_amd import losses
    name = "near_2x3x20x24"
    x, y = case(name)
    wgt = torch.tensor([0.25, -1.5], device=DEV)
    xg = x.clone().requires_grad_(True)
    (g,) = torch.autograd.grad((losses.ssim(xg, y, size_average=False) * wgt).sum(), xg)
    xd = x.detach().double().cpu().requires_grad_(True)
    (g64,) = torch.autograd.grad((R.ssim(xd, y.cpu(), size_average=False) * wgt.double().cpu()).sum(), xd)
    d = grad_dist(g, g64.numpy())
    print(f"\nper-image ssim gradient {d:.2e}")
    assert d <= 4 * FLOOR_G
    with pytest.raises(RuntimeError):
        losses.photometric_loss(x, y.clone().requires_grad_(True))
    with pytest.raises(RuntimeError):
        losses.ssim(x, y.clone().requires_grad_(True))


@pytest.mark.parametrize("name", ["near_3x47x63", "near_2x3x20x24", "near_3x5x7"])
def test_identical_images(name):
    from gags_amd import losses
    _, y = case(name)
    scale = float(np.abs(Z[name + "_grad64"]).max())  # what a gradient of this loss at this size measures
    for img in (y.clone(), pixel_major(y)):
        loss, g = loss_and_grad(img, y)
        s = losses.ssim(img, y)
        print(f"\n{name}: 1 - ssim {abs(1 - float(s)):.2e}  loss {abs(float(loss)):.2e}  gradient / scale {float(g.abs().max()) / scale:.2e}")
        assert abs(float(s) - 1.0) <= FLOOR_V and abs(float(loss)) <= FLOOR_V
        assert float(g.abs().max()) <= FLOOR_G * scale
        assert torch.isinf(losses.psnr(img, y)).all()  # the reference's 20 log10(1 / sqrt(0))


@pytest.mark.parametrize("lam", [0.0, 1.0])
def test_lambda_zero_and_one_against_the_restatement(lam):
    x, y = case("near_3x33x17")
    l64, g64 = R.value_and_grad(R.photometric_loss, x.cpu(), y.cpu(), lam)
    for xx in (x, pixel_major(x)):
        loss, g = loss_and_grad(xx, y, lam)
        dv, dg = abs(float(loss) - float(l64)), grad_dist(g, g64.numpy())
        print(f"\nlambda {lam}: value {dv:.2e}  gradient {dg:.2e}")
        assert dv <= 4 * FLOOR_V and dg <= 4 * FLOOR_G
    if lam == 0.0:  # pure L1: the gradient is sign(x - y) / n, zeros where the fixture put the image on its target
        n = x.numel()
        assert torch.equal(g, torch.sign(x - y) * torch.tensor(1.0 / n, dtype=torch.float64).float().to(DEV))
        assert int((g == 0).sum()) >= 3


@functools.lru_cache(maxsize=None)
def big_case():
    g = torch.Generator().manual_seed(77)
    y = torch.rand(BIG, generator=g)
    x = (y + 0.05 * torch.randn(BIG, generator=g)).clamp(0.0, 1.0)
    x.view(-1)[::97] = y.view(-1)[::97]
    l64, g64 = R.value_and_grad(R.photometric_loss, x, y, 0.2)
    return x, y, float(l64), g64.numpy(), float(R.ssim(x, y)), R.psnr(x, y).numpy()


def test_many_tiles_in_both_directions():
    from gags_amd import _lib, losses
    x, y, l64, g64, s64, p64 = big_case()
    assert _lib.load().gags_photometric_partials(*BIG) == 3 * 9 * 7
    x, y = x.to(DEV), y.to(DEV)
    got = []
    for xx in (x, pixel_major(x)):
        loss, g = loss_and_grad(xx, y)
        dv, dg = abs(float(loss) - l64), grad_dist(g, g64)
        ds = abs(float(losses.ssim(xx, y)) - s64)
        dp = float(np.abs(losses.psnr(xx, y).double().cpu().numpy() - p64).max()) * math.log(10.0) / 10.0
        print(f"\n{BIG}: value {dv:.2e}  gradient {dg:.2e}  ssim {ds:.2e}  psnr as relative mse {dp:.2e}")
        assert dv <= 4 * FLOOR_V and ds <= 4 * FLOOR_V and dp <= 4 * FLOOR_V and dg <= 4 * FLOOR_G
        got.append((loss, g))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])


def test_two_runs_are_bit_identical():
    x, y = big_case()[:2]
    x, y = pixel_major(x.to(DEV)), y.to(DEV)
    l1, g1 = loss_and_grad(x, y)
    l2, g2 = loss_and_grad(x, y)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)


# ----------------------------------------------------------------------------------------------------------------------
# through the renderer
W, H, N = 64, 48, 500


def _scene(seed=3):
    from gags_amd import synthetic as syn
    pc = syn.make_model(N, 16, W, H, seed=seed, device=DEV, scale0=syn.SCALE0 * 24)
    cam = syn.make_camera(W, H, view=3, device=DEV)
    return pc, cam, torch.zeros(3, device=DEV)


def _target(pc, cam, bg):
    """The same scene rendered with perturbed SH coefficients: a contiguous [3,H,W] ground truth."""
    from gags_amd.gaussian_renderer import render
    g = torch.Generator(device=DEV).manual_seed(11)
    dc = pc._features_dc.detach().clone()
    with torch.no_grad():
        pc._features_dc += 0.5 * torch.randn(dc.shape, device=DEV, generator=g)
        gt = render(cam, pc, None, bg, feature_mode=False)["render"].detach().clamp(0.0, 1.0).contiguous()
        pc._features_dc.copy_(dc)
    return gt


STORED = ("_xyz", "_scaling", "_rotation", "_opacity", "_features_dc", "_features_rest")


def test_render_feeds_the_loss_without_a_copy():
    from gags_amd import losses
    from gags_amd.gaussian_renderer import render
    pc, cam, bg = _scene()
    gt = _target(pc, cam, bg)
    for name in STORED:
        getattr(pc, name).requires_grad_(True)
    img = render(cam, pc, None, bg, feature_mode=False)["render"]
    assert tuple(img.shape) == (3, H, W) and not img.is_contiguous() and img.permute(1, 2, 0).is_contiguous()
    loss = losses.photometric_loss(img, gt)
    (g_view,) = torch.autograd.grad(loss, img, retain_graph=True)
    assert g_view.permute(1, 2, 0).is_contiguous()  # the gradient the rasterizer receives lies as its output does
    clone = img.detach().contiguous().requires_grad_(True)
    loss_c = losses.photometric_loss(clone, gt)
    (g_clone,) = torch.autograd.grad(loss_c, clone)
    assert torch.equal(loss.detach(), loss_c.detach()) and torch.equal(g_view, g_clone)
    assert float(g_view.abs().max()) > 0
    loss.backward()
    for name in STORED:
        g = getattr(pc, name).grad
        assert g is not None and bool(torch.isfinite(g).all()), name
        assert float(g.abs().max()) > 0, name


def test_twenty_adam_steps_on_the_dc_colours_lower_the_loss():
    """A smoke test of the sign and the scale of the gradient, not a convergence claim."""
    from gags_amd import losses
    from gags_amd.gaussian_renderer import render
    from gags_amd.optim import FeatureAdam
    pc, cam, bg = _scene()
    gt = _target(pc, cam, bg)
    pc._features_dc.requires_grad_(True)
    opt = FeatureAdam([pc._features_dc], lr=0.02, eps=1e-15)

    def loss_now():
        return losses.photometric_loss(render(cam, pc, None, bg, feature_mode=False)["render"], gt)
    with torch.no_grad():
        before = float(loss_now())
    for _ in range(20):
        opt.zero_grad(set_to_none=True)
        loss_now().backward()
        opt.step()
    with torch.no_grad():
        after = float(loss_now())
    print(f"\nloss {before:.6f} -> {after:.6f}")
    assert math.isfinite(after) and after < before
