"""N24 on the GPU: the bilateral grid kernels (csrc/bilagrid.hip) against the float64 CPU reference tests/bilagrid_ref.py.

The yardstick of every comparison is the float32 torch composition of the same inputs run on the GPU (grid_sample and
element-wise operators, differentiated by autograd): the kernel's max abs error may be at most 4 x the composition's, with a
floor of 8 float32 ulps of the reference's largest magnitude (bilagrid_ref.bound).  Shapes: images smaller than the grid (empty
and one-pixel supports), 70 x 130 (several pixels per cell, many workgroups); grids 2x2x2, 5x3x4 and 16x16x8; both input
layouts and a non-contiguous cotangent.  Every figure is printed before it is asserted (pytest -s).
"""
import functools

import pytest
import torch

import bilagrid_ref as R
import photometric_ref as PR
import test_streams_gpu as TS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
IMAGES = [(1, 1), (1, 2), (3, 5), (17, 33), (70, 130)]
GRIDS = [(2, 2, 2), (4, 3, 5), (8, 16, 16)]   # (L, Gh, Gw)
LAYOUTS = ["view", "planar", "hwc", "planar_strided_cotangent"]


@functools.lru_cache(maxsize=None)
def _reference(h, w, L, gh, gw, spread=0.3):
    """Inputs (float32, CPU) and the float64 results of one (image, grid): computed once, shared, never written."""
    rgb = R.make_image(h, w, L, seed=7 * h + w)
    grid = R.make_grid(L, gh, gw, seed=L + gh + gw, spread=spread)
    v_out = R.make_cotangent(h, w, seed=h + w)
    out = R.slice_tent(grid.double(), rgb.double())
    v_grid, v_rgb, guide = R.grads_tent(grid.double(), rgb.double(), v_out.double())
    hit = R.reached(grid.shape, rgb.double())
    assert bool((v_grid[:, ~hit] == 0).all())   # the reference's gradient at unreached nodes is exactly 0
    return dict(rgb=rgb, grid=grid, v_out=v_out, out=out, v_grid=v_grid, v_rgb=v_rgb, guide=guide, hit=hit, kind=R.edge_kind(rgb))


@functools.lru_cache(maxsize=None)
def _yardstick(h, w, L, gh, gw):
    """Max abs errors (forward, v_grid, v_rgb) of the float32 composition on the GPU against the float64 reference."""
    ref = _reference(h, w, L, gh, gw)
    out, v_grid, v_rgb = R.value_and_grads(R.slice_grid_sample, ref["grid"].to(DEV), ref["rgb"].to(DEV), ref["v_out"].to(DEV))
    return tuple(float((a.cpu().double() - ref[k]).abs().max()) for a, k in ((out, "out"), (v_grid, "v_grid"), (v_rgb, "v_rgb")))


def _laid_out(layout, rgb_hwc, v_hwc):
    """(rgb as handed to slice, a function that lays the cotangent out for backward) on the GPU."""
    rgb_hwc, v_hwc = rgb_hwc.to(DEV), v_hwc.to(DEV)
    h, w, _ = rgb_hwc.shape
    if layout == "hwc":
        return rgb_hwc.contiguous(), v_hwc.contiguous()
    if layout == "view":                                      # what render() returns: [H,W,3] memory seen as [3,H,W]
        return rgb_hwc.contiguous().permute(2, 0, 1), v_hwc.contiguous().permute(2, 0, 1)
    rgb = rgb_hwc.permute(2, 0, 1).contiguous()               # a contiguous [3,H,W]
    if layout == "planar":
        return rgb, v_hwc.permute(2, 0, 1).contiguous()
    wide = torch.full((3, h + 1, 2 * w + 3), float("nan"), device=DEV)   # every second column of rows 1.. of a wider buffer
    v = wide[:, 1:, 1:2 * w + 1:2]
    v.copy_(v_hwc.permute(2, 0, 1))
    assert not v.is_contiguous() and tuple(v.shape) == (3, h, w)
    return rgb, v


def _as_hwc(t, layout):
    return t if layout == "hwc" else t.permute(1, 2, 0)


def _check(name, got, ref, yard):
    err = float((got.detach().cpu().double() - ref).abs().max())
    b = R.bound(yard, ref)
    print(f"  {name}: max abs error {err:.3e}, composition {yard:.3e} (ratio {err / yard if yard > 0 else float('inf'):.2f}), bound {b:.3e}")
    assert err <= b, (name, err, yard, b)


# (a [3,5,3] tensor is read as [3,H,W]: slice() cannot be handed the 3 x 5 image as [H,W,3], every other combination is here)
IMAGE_LAYOUTS = [(h, w, layout) for (h, w) in IMAGES for layout in LAYOUTS if not (h == 3 and layout == "hwc")]


@pytest.mark.parametrize("L,gh,gw", GRIDS)
@pytest.mark.parametrize("h,w,layout", IMAGE_LAYOUTS)
def test_slice_forward_and_backward_against_float64(h, w, L, gh, gw, layout):
    from gags_amd import bilagrid as B
    ref = _reference(h, w, L, gh, gw)
    yard = _yardstick(h, w, L, gh, gw)
    rgb, v = _laid_out(layout, ref["rgb"], ref["v_out"])
    grid = ref["grid"].to(DEV).requires_grad_(True)
    rgb.requires_grad_(True)
    out = B.slice(grid, rgb)
    assert out.shape == rgb.shape and _as_hwc(out, layout).is_contiguous()   # the input's logical shape over [H,W,3] memory
    print(f"\n{h}x{w} image, {gw}x{gh}x{L} grid, {layout}:")
    _check("forward", _as_hwc(out, layout), ref["out"], yard[0])
    v_grid, v_rgb = torch.autograd.grad(out, (grid, rgb), v, retain_graph=True)
    assert v_rgb.shape == rgb.shape and _as_hwc(v_rgb, layout).is_contiguous() and v_grid.is_contiguous()
    _check("v_grid", v_grid, ref["v_grid"], yard[1])      # every node, reached or not
    _check("v_rgb", _as_hwc(v_rgb, layout), ref["v_rgb"], yard[2])   # every pixel, the edge pixels included
    # nodes no pixel reaches are written, as exact zeros
    miss = ~ref["hit"].to(DEV)
    assert bool((v_grid[:, miss] == 0).all()) and not bool(torch.signbit(v_grid[:, miss]).any())
    if (h * w < 8 * 16 * 16) and (L, gh, gw) == (8, 16, 16):
        assert int(miss.sum()) > 0
    # deterministic: a second backward gives the same bits; each gradient alone is the same as both together
    again, again_rgb = torch.autograd.grad(out, (grid, rgb), v, retain_graph=True)
    assert torch.equal(again, v_grid) and torch.equal(again_rgb, v_rgb)
    (only_grid,) = torch.autograd.grad(out, (grid,), v, retain_graph=True)
    (only_rgb,) = torch.autograd.grad(out, (rgb,), v)
    assert torch.equal(only_grid, v_grid) and torch.equal(only_rgb, v_rgb)


@pytest.mark.parametrize("L,gh,gw", GRIDS)
@pytest.mark.parametrize("h,w", [(3, 5), (17, 33)])
def test_guide_gradient_is_exactly_zero_on_clamped_and_black_pixels(h, w, L, gh, gw):
    """A grid whose colour columns are zero and whose bias varies: the affine part of v_rgb vanishes exactly, what is left is
    the gradient through the luminance.  It is exactly 0 on the pixels with gray < 0, gray > 1 and on exact black, and
    nowhere else."""
    from gags_amd import bilagrid as B
    ref = _reference(h, w, L, gh, gw)
    grid = ref["grid"].clone().reshape(3, 4, L, gh, gw)
    grid[:, :3] = 0.0
    grid = grid.reshape(12, L, gh, gw)
    kind = ref["kind"]
    assert {1, 2, 3} <= set(kind.reshape(-1).tolist())
    want = R.grads_tent(grid.double(), ref["rgb"].double(), ref["v_out"].double())
    assert torch.equal(want[1], want[2])                       # (the reference's v_rgb IS its guide term here)
    rgb = ref["rgb"].to(DEV).permute(2, 0, 1).requires_grad_(True)   # (the [3,H,W] view: a [3,5,3] tensor would be read as one)
    B.slice(grid.to(DEV), rgb).backward(ref["v_out"].to(DEV).permute(2, 0, 1))
    g = rgb.grad.permute(1, 2, 0).cpu()
    assert bool((g[kind > 0] == 0).all())
    assert bool((g[kind == 0] != 0).any(-1).all())
    _, _, yard = R.value_and_grads(R.slice_grid_sample, grid.to(DEV), ref["rgb"].to(DEV), ref["v_out"].to(DEV))
    _check("guide", g, want[2], float((yard.cpu().double() - want[2]).abs().max()))


@pytest.mark.parametrize("L,gh,gw", [(2, 2, 2), (8, 16, 16)])
@pytest.mark.parametrize("b", [1, 3])
def test_total_variation_against_float64(b, L, gh, gw):
    from gags_amd import bilagrid as B
    g = torch.Generator().manual_seed(b + L)
    grids = torch.randn(b, 12, L, gh, gw, generator=g)
    g64 = grids.double().requires_grad_(True)
    want = R.tv_ref(g64)
    (want * 1.7).backward()
    g32 = grids.to(DEV).requires_grad_(True)
    comp = R.tv_ref(g32)
    (comp * 1.7).backward()
    mine_in = grids.to(DEV).requires_grad_(True)
    mine = B.total_variation_loss(mine_in)
    assert mine.shape == () and mine.dtype == torch.float32
    (mine * 1.7).backward()
    print(f"\nTV, B={b}, {gw}x{gh}x{L}:")
    _check("value", mine.reshape(1), want.detach().reshape(1), float((comp.detach().cpu().double() - want.detach()).abs()))
    _check("gradient", mine_in.grad, g64.grad, float((g32.grad.cpu().double() - g64.grad).abs().max()))
    again = grids.to(DEV).requires_grad_(True)
    B.total_variation_loss(again).backward(torch.tensor(1.7, device=DEV))
    assert torch.equal(again.grad, mine_in.grad)
    const = torch.full((b, 12, L, gh, gw), 0.37, device=DEV)
    assert float(B.total_variation_loss(const)) == 0.0


LOOP_STEPS, LOOP_LR, LOOP_IDX = 10, 40.0, 1


def test_a_short_sgd_loop_follows_the_float64_loop():
    """BilateralGrid(3), 10 plain-SGD steps on a 12 x 20 image against the image corrected by a known smooth grid.  The
    learning rate was chosen on the float64 reference alone: the Hessian of the mean squared error in a node's entries is at
    most (2 / 720) x (the node's summed squared weights, a few pixels' worth) ~ 1e-2, so 40 is well inside 2 / that; the
    reference loop's loss falls monotonically (asserted below).  Only slab LOOP_IDX moves."""
    from gags_amd.bilagrid import BilateralGrid
    h, w = 12, 20
    rgb = R.make_image(h, w, 8, seed=12)
    target = R.slice_tent(R.smooth_grid(8, 16, 16).double(), rgb.double()).float()
    start = BilateralGrid(3).grids.detach().clone()
    want = R.sgd_loop_ref(start.double(), LOOP_IDX, rgb.double(), target.double(), LOOP_LR, LOOP_STEPS)
    loss = lambda g: float(((R.slice_tent(g[LOOP_IDX], rgb.double()) - target.double()) ** 2).mean())  # noqa: E731
    trail = [loss(R.sgd_loop_ref(start.double(), LOOP_IDX, rgb.double(), target.double(), LOOP_LR, k)) for k in (0, 3, 6, 10)]
    assert all(b < a for a, b in zip(trail, trail[1:])) and trail[-1] < 0.7 * trail[0], trail

    def run(slicer):
        grids = torch.nn.Parameter(start.to(DEV).clone())
        opt = torch.optim.SGD([grids], lr=LOOP_LR)
        x, t = rgb.to(DEV), target.to(DEV)
        for _ in range(LOOP_STEPS):
            opt.zero_grad(set_to_none=True)
            ((slicer(grids[LOOP_IDX], x) - t) ** 2).mean().backward()
            opt.step()
        return grids.detach().cpu()

    model = BilateralGrid(3).to(DEV)
    opt = torch.optim.SGD(model.parameters(), lr=LOOP_LR)
    x, t = rgb.to(DEV), target.to(DEV)
    for _ in range(LOOP_STEPS):
        opt.zero_grad(set_to_none=True)
        ((model(x, LOOP_IDX) - t) ** 2).mean().backward()
        opt.step()
    mine = model.grids.detach().cpu()
    comp = run(R.slice_grid_sample)
    print(f"\nloop: reference loss {trail[0]:.3e} -> {trail[-1]:.3e}")
    _check("grids after the loop", mine[LOOP_IDX], want[LOOP_IDX], float((comp[LOOP_IDX].double() - want[LOOP_IDX]).abs().max()))
    assert float((mine[LOOP_IDX] - start[LOOP_IDX]).abs().max()) > 1e-3
    for other in (0, 2):
        assert torch.equal(mine[other], start[other]) and torch.equal(want[other].float(), start[other])


# -- render() with a grid ----------------------------------------------------------------------------------------------------------

W_R, H_R, N_R = 64, 48, 500


def _scene(seed=3):
    from gags_amd import synthetic as syn
    pc = syn.make_model(N_R, 16, W_R, H_R, seed=seed, device=DEV, scale0=syn.SCALE0 * 24)
    cam = syn.make_camera(W_R, H_R, view=2, device=DEV)
    assert cam.uid == 2
    _trainable(pc)
    return pc, cam


def _trainable(pc):
    for t in (pc._xyz, pc._features_dc, pc._features_rest, pc._scaling, pc._rotation, pc._opacity):
        t.requires_grad_(True)


def _zero_grads(pc):
    for t in (pc._xyz, pc._features_dc, pc._features_rest, pc._scaling, pc._rotation, pc._opacity):
        t.grad = None


def test_render_with_a_bilateral_grid():
    """"render_raw" is the render of the call without a grid, bit for bit; "render" is slice() of it; photometric_loss on it
    fills grids.grad (slab uid only) and sends the scene the cotangent the float64 reference sends -- measured where it enters
    the rasterizer (deterministic) and on the colour gradients behind it (the rasterizer's narrow backward adds with float
    atomics, in the kernel's run, in the composition's and in the reference's alike)."""
    from gags_amd import bilagrid as B, losses
    from gags_amd.gaussian_renderer import render
    pc, cam = _scene()
    bg = torch.zeros(3, device=DEV)
    gt = torch.rand(3, H_R, W_R, generator=torch.Generator().manual_seed(8)).to(DEV)
    model = B.BilateralGrid(4).to(DEV)
    with torch.no_grad():
        model.grids.add_(0.2 * torch.randn(model.grids.shape, generator=torch.Generator().manual_seed(9)).to(DEV))
    plain = render(cam, pc, None, bg, feature_mode=False)
    assert "render_raw" not in plain
    pkg = render(cam, pc, None, bg, feature_mode=False, bilateral_grid=model)
    assert set(pkg) == set(plain) | {"render_raw"}
    assert torch.equal(pkg["render_raw"], plain["render"]) and pkg["render_raw"].stride() == plain["render"].stride()
    assert torch.equal(pkg["render"], B.slice(model.grids[cam.uid], plain["render"].detach()))
    assert pkg["render"].shape == (3, H_R, W_R) and pkg["render"].permute(1, 2, 0).is_contiguous()
    assert losses._photo_view(pkg["render"])[0] is pkg["render"]          # photometric_loss reads it where it lies: no copy
    raw32 = plain["render"].detach().permute(1, 2, 0).cpu()
    assert int((R.edge_kind(raw32) == 3).sum()) > 0                      # (pixels no Gaussian reaches: exact black)

    # the kernels
    pkg["render_raw"].retain_grad()
    losses.photometric_loss(pkg["render"], gt).backward()
    v_raw = pkg["render_raw"].grad.permute(1, 2, 0).cpu()
    mine = dict(grids=model.grids.grad.cpu(), v_raw=v_raw, dc=pc._features_dc.grad.cpu().clone(),
                rest=pc._features_rest.grad.cpu().clone())
    assert all(bool((mine["grids"][k] == 0).all()) for k in (0, 1, 3)) and float(mine["grids"][cam.uid].abs().max()) > 0

    # the float64 reference from the raw render: slice, photometric loss, and the rule's backward
    grid64 = model.grids.detach()[cam.uid].cpu().double()
    out64 = R.slice_tent(grid64, raw32.double())
    _, v_out64 = PR.value_and_grad(PR.photometric_loss, out64.permute(2, 0, 1), gt.cpu(), 0.2)
    v_grid64, v_raw64, _ = R.grads_tent(grid64, raw32.double(), v_out64.permute(1, 2, 0))
    _zero_grads(pc)
    again = render(cam, pc, None, bg, feature_mode=False)
    again["render"].backward(v_raw64.float().to(DEV).permute(2, 0, 1))
    want = dict(grids=v_grid64, v_raw=v_raw64, dc=pc._features_dc.grad.cpu().double(), rest=pc._features_rest.grad.cpu().double())

    # the float32 composition
    _zero_grads(pc)
    g32 = model.grids.detach().clone().requires_grad_(True)
    comp_pkg = render(cam, pc, None, bg, feature_mode=False)
    comp_pkg["render"].retain_grad()
    comp_out = R.slice_grid_sample(g32[cam.uid], comp_pkg["render"].permute(1, 2, 0)).permute(2, 0, 1)
    losses.photometric_loss(comp_out, gt).backward()
    comp = dict(grids=g32.grad[cam.uid].cpu(), v_raw=comp_pkg["render"].grad.permute(1, 2, 0).cpu(),
                dc=pc._features_dc.grad.cpu(), rest=pc._features_rest.grad.cpu())
    print()
    _check("render", pkg["render"].permute(1, 2, 0), out64, float((comp_out.detach().permute(1, 2, 0).cpu().double() - out64).abs().max()))
    _check("grids.grad", mine["grids"][cam.uid], want["grids"], float((comp["grids"].double() - want["grids"]).abs().max()))
    for k in ("v_raw", "dc", "rest"):
        assert float(want[k].abs().max()) > 0
        _check(k, mine[k], want[k], float((comp[k].double() - want[k]).abs().max()))


# -- stream order ------------------------------------------------------------------------------------------------------------------

def _stream_inputs(seed):
    t = TS._model_inputs(N_R, 16, W_R, H_R, 24)(seed)
    g = torch.Generator().manual_seed(seed + 2)
    t["gt"] = torch.rand(3, H_R, W_R, generator=g)
    t["grids"] = (torch.eye(4)[:3].reshape(1, 12, 1, 1, 1) + 0.2 * torch.randn(3, 12, 8, 16, 16, generator=g)).contiguous()
    t["image"] = R.make_image(17, 33, 8, seed=seed)
    t["v_out"] = R.make_cotangent(17, 33, seed=seed)
    return t


def _stream_run(dev):
    """render() with a grid, the photometric loss and the TV term, backward; then slice() on its own, both gradients."""
    from gags_amd import bilagrid as B, losses, synthetic as syn
    from gags_amd.gaussian_renderer import render
    from gags_amd.rasterization import RasterContext
    pc = TS._model_on(dev)
    _trainable(pc)
    cam = syn.make_camera(W_R, H_R, view=2, device=DEV)
    model = B.BilateralGrid(3)
    model.grids = torch.nn.Parameter(dev["grids"])
    pkg = render(cam, pc, None, torch.zeros(3, device=DEV), feature_mode=False, bilateral_grid=model, context=RasterContext())
    pkg["render_raw"].retain_grad()
    tv = model.tv_loss()
    (losses.photometric_loss(pkg["render"], dev["gt"]) + 10.0 * tv).backward()
    res = {"render": pkg["render"], "render_raw": pkg["render_raw"], "v_raw": pkg["render_raw"].grad, "tv": tv.detach().reshape(1),
           "grids.grad": model.grids.grad}
    image = dev["image"].detach().requires_grad_(True)
    grid = dev["grids"][0].detach().requires_grad_(True)
    out = B.slice(grid, image)
    out.backward(dev["v_out"])
    res.update(out=out, v_image=image.grad, v_grid=grid.grad)
    return {k: TS._host(v) for k, v in res.items()}


# The case joins the cases of tests/test_streams_gpu.py, whose last test accounts for every streamed entry the package names:
# the four gags_bilagrid_* entries that launch are reached on a side stream here.
STREAM_CASE = "render_bilateral_grid_and_tv"
TS.CASES[STREAM_CASE] = TS.Case(_stream_inputs, _stream_run)


def test_side_stream_behind_late_producers_equals_the_default_stream(oracle):
    """The case above on a side stream behind late producers (tests/stream_harness.py), decoy inputs in memory until the delayed
    copies land: every output and gradient torch.equal to the run on the default stream (none of them passes through the
    rasterizer's atomic backward), every streamed entry called with the side stream's handle."""
    TS.test_side_stream_behind_late_producers_equals_the_default_stream(oracle, STREAM_CASE)
    assert {"gags_bilagrid_slice_fwd", "gags_bilagrid_slice_bwd", "gags_bilagrid_tv_fwd", "gags_bilagrid_tv_bwd"} <= TS.RECORDED[STREAM_CASE]
    ref = TS._reference(STREAM_CASE)[0]
    assert all(float(ref[k].abs().max()) > 0 for k in ("v_raw", "grids.grad", "v_image", "v_grid", "tv"))
