"""The fisheye's distortion coefficients (N21) on the GPU: gags_project_fwd_cam / gags_project_bwd_cam with GAGS_PROJ_KB at the
lane, wave and workgroup edges, through rasterization() and through render().  Truth is the float64 restatement of
tests/fisheye_kb_ref.py (autograd); the bound on a float is min(F64_CAP, F64_MARGIN x the error of a float32 yardstick against
the same float64) -- at kernel level the float32 CPU restatement, through rasterization() the project's pinhole path on the same
scene and K.  Integers are exact except for Gaussians float64 puts within 1e-5 of a decision boundary, the fold (g' = 0)
included (at most 2 %; tests/test_fisheye_kb_cpu.py pins the seeds).  The harness around the two entries is
tests/test_camera_models_gpu.py's: with GAGS_PROJ_KB in `flags` and the 13-float block as the scene's K it calls them as they are."""
import functools
import math

import numpy as np
import pytest
import torch

import aa_ref
import camera_models_ref as cm
import fisheye_kb_ref as kb
import test_camera_models_gpu as tcm
from helpers import rel_l2, spy_entries, to_dev
from test_general_camera_gpu import F64_CAP, F64_MARGIN

pytestmark = pytest.mark.gpu

F64 = torch.float64
W, H = cm.KERNEL_W, cm.KERNEL_H
RAW, AA, POSE, KB = 1, 2, 4, kb.KB
FLOATS = ("means2d", "depths", "conics", "comp")


def _bound(e32):
    return min(F64_CAP, F64_MARGIN * e32)


@functools.lru_cache(maxsize=None)
def _kscene(name):
    return kb.kernel_scene(name)


def _with_block(s, name):
    """The scene as the harness hands it to the entries: K = the 13 floats."""
    return dict(s, K=kb.block(s["K"], name))


def k_fwd(name, flags, s, cull, **kw):
    return tcm.k_fwd("fisheye", flags | KB, _with_block(s, name), cull, **kw)


def k_bwd(name, flags, s, cull, radii, cot, **kw):
    return tcm.k_bwd("fisheye", flags | KB, _with_block(s, name), cull, radii, cot, **kw)


def _truth(name, s, cull, flags, dtype, cot=None, radii=None):
    """The restatement in `dtype` on the CPU: (outputs dict, decisions, gradients dict | None)."""
    raw = bool(flags & RAW)
    pr, dec, L = kb.run(name, s, W, H, dtype, raw=raw, grad=cot is not None, **cull)
    o = cm.outputs(pr, dec)
    if raw:
        vis = dec["radii"] > 0
        op = L["opac_act"].detach().numpy()
        o["opac"] = op * np.where(vis, o["comp"], 0) if flags & AA else op
    g = None
    if cot is not None:
        n = s["means"].shape[0]
        c = {k: v[:n] for k, v in cot.items()}
        cm.project_loss(pr, radii, c, antialiased=bool(flags & AA), opac_act=L.get("opac_act")).backward()
        g = {k: (L[k].grad.numpy() if L[k].grad is not None else np.zeros(tuple(L[k].shape))) for k in L if k != "opac_act"}
    return o, dec, g


# -- (a) zero coefficients -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", (257, 700))
def test_zero_coefficients_with_the_flag_are_the_plain_fisheye(n):
    """k1 .. k4 = 0 behind GAGS_PROJ_KB against the call without the flag, same entry pair: torch.equal on every output of the
    forward (flags 0, AA, RAW, RAW | AA; RAW with quats_act, scales_act and the record table) and of the backward, with POSE
    (v_viewmat included) and without."""
    s0, cull = _kscene("A")
    s = tcm._cut(s0, n)
    cot = cm.cotangents(n, 8)
    for flags in (0, AA, RAW, RAW | AA):
        got, plain = k_fwd("zero", flags, s, cull, extras=True), tcm.k_fwd("fisheye", flags, s, cull, extras=True)
        assert int((plain["radii"] > 0).sum()) >= 80
        for k in plain:
            assert (got[k] is None) == (plain[k] is None), k
            if plain[k] is not None:
                assert torch.equal(got[k], plain[k]), (k, flags)
        for fl in (flags, flags | POSE):
            g, gp = k_bwd("zero", fl, s, cull, plain["radii"], cot), tcm.k_bwd("fisheye", fl, s, cull, plain["radii"], cot)
            for k in gp:
                assert (g[k] is None) == (gp[k] is None), k
                if gp[k] is not None:
                    assert torch.equal(g[k], gp[k]), (k, fl)
                    assert bool(torch.isfinite(g[k]).all()) and bool(g[k].any()), (k, fl)


# -- (b), (c), (d) against float64 -------------------------------------------------------------------------------------------------

def _forward_case(name, n):
    s0, cull = _kscene(name)
    s = tcm._cut(s0, n)
    got = None
    for flags in (0, AA, RAW, RAW | AA):
        got = k_fwd(name, flags, s, cull)
        o64, dec, _ = _truth(name, s, cull, flags, F64)
        o32, d32, _ = _truth(name, s, cull, flags, torch.float32)
        keep = tcm._check_ints(got, dec, f"set {name} n={n} flags={flags}")
        both = keep & (dec["radii"] > 0) & (d32["radii"] > 0)
        culled = got["radii"].cpu().numpy() == 0
        for k in [k for k in FLOATS if k != "comp" or flags & AA] + (["opac"] if flags & RAW else []):
            a = got[k].cpu().numpy()
            if k != "opac":
                assert np.all(a[culled] == 0), k
            elif flags & AA:
                assert np.all(a[culled] == 0), k
            if both.sum() == 0:
                continue
            rows = both if k != "opac" or flags & AA else np.ones(n, bool)
            e, e32 = rel_l2(a[rows], o64[k][rows]), rel_l2(o32[k][rows], o64[k][rows])
            print(f"kb fwd set {name} n={n} flags={flags} {k}: HIP {e:.2e} fp32 restatement {e32:.2e} ratio {e / max(e32, 1e-30):.2f}")
            assert e <= _bound(e32), (k, flags, e, e32)
    return s, got, dec


def _backward_case(name, n):
    s0, cull = _kscene(name)
    s = tcm._cut(s0, n)
    cot = cm.cotangents(700, 2)
    for flags in (0, AA, RAW, RAW | AA):
        fwd = k_fwd(name, flags, s, cull)
        _, dec, _ = _truth(name, s, cull, flags, F64)
        keep = tcm._check_ints(fwd, dec, f"set {name} n={n}")
        radii = fwd["radii"]
        rn = radii.cpu().numpy()
        g = k_bwd(name, flags, s, cull, radii, cot)
        gp = k_bwd(name, flags | POSE, s, cull, radii, cot)
        for k in ("means", "quats", "scales") + (("opacities",) if flags & RAW else ()):
            assert torch.equal(g[k], gp[k]), (k, flags)
            if k != "opacities" or flags & AA:
                assert not bool(g[k][radii <= 0].any()), (k, flags)
                assert not bool(g[k][to_dev(dec["folded"] & keep)].any()), (k, flags)      # (past the fold)
        assert bool((gp["viewmat"][3] == 0).all())
        if n == 0:
            assert not bool(gp["viewmat"].any())
            continue
        _, _, g64 = _truth(name, s, cull, flags, F64, cot, rn)
        _, _, g32 = _truth(name, s, cull, flags, torch.float32, cot, rn)
        if not (rn > 0).any():
            continue
        for k in ("means", "quats", "scales", "viewmat") + (("opacities",) if flags & RAW else ()):
            a = gp[k].cpu().numpy()
            e, e32 = rel_l2(a, g64[k]), rel_l2(g32[k], g64[k])
            print(f"kb bwd set {name} n={n} flags={flags} {k}: HIP {e:.2e} fp32 autograd {e32:.2e} ratio {e / max(e32, 1e-30):.2f}")
            assert e <= _bound(e32), (k, flags, e, e32)


@pytest.mark.parametrize("n", cm.KERNEL_SIZES)
@pytest.mark.parametrize("name", ["A", "B"])
def test_forward_against_float64(name, n):
    """RAW x AA, Gaussians up to 88 degrees off axis: floats within min(F64_CAP, F64_MARGIN x e32) of float64, e32 the float32
    CPU restatement's own error on the case; integers exact outside the near-boundary set; culled rows zero.
    Measured on an MI355X: see docs/LAB_NOTES.md "Fisheye distortion (N21)"."""
    s, got, _ = _forward_case(name, n)
    if n == 700:
        assert cm.off_axis_deg(s)[got["radii"].cpu().numpy() > 0].max() > 80.0


@pytest.mark.parametrize("n", cm.KERNEL_SIZES)
@pytest.mark.parametrize("name", ["A", "B"])
def test_backward_against_float64_autograd(name, n):
    """RAW x AA x POSE: every gradient and v_viewmat within min(F64_CAP, F64_MARGIN x e32) of float64 autograd through the
    restatement (e32: the same autograd in float32 on the CPU); culled rows exactly zero, row 3 of v_viewmat zero, without POSE
    the same bits as with it.  The radii are the kernel's own, accepted by the forward rule."""
    _backward_case(name, n)


@pytest.mark.parametrize("n", (257, 700))
def test_past_the_fold_is_culled(n):
    """Set C folds at 74 degrees: every Gaussian float64 puts past the fold (outside NEAR_TOL) has radius 0, zero outputs and
    zero gradients; the others meet the forward and the backward bounds."""
    s, got, dec = _forward_case("C", n)
    past = dec["folded"] & ~dec["close"]
    assert past.sum() >= 30 and (dec["radii"] > 0).sum() >= 60
    ang = cm.off_axis_deg(s)
    assert ang[past].min() > 73.5 and ang[past].max() < 88.5
    idx = to_dev(past)
    for k in ("radii", "tiles", "means2d", "depths", "conics", "comp"):
        assert not bool(got[k][idx].any()), k          # (the last flags of the case: RAW | AA)
    assert not bool(got["opac"][idx].any())
    # without the coefficients the same Gaussians are on screen: it is the fold that culls them
    plain = tcm.k_fwd("fisheye", 0, s, _kscene("C")[1])
    assert int((plain["radii"][idx] > 0).sum()) >= 10
    _backward_case("C", n)


# -- (e) through rasterization() ---------------------------------------------------------------------------------------------------

def _gpu_full(name, s, w, h, colors, bg, v_out, v_alpha, *, raw, aa, mode, sh, pose):
    from gags_amd.rasterization import rasterization
    if raw:
        p = s["raw"]
        L = dict(means=p["xyz"].cuda(), quats=p["rotation"].cuda(), scales=p["scaling_log"].cuda(), opacities=p["opacity_logit"].cuda())
    else:
        L = dict(means=to_dev(s["means"]), quats=to_dev(s["quats"]), scales=to_dev(s["scales"]), opacities=to_dev(s["opacities"]))
    L["colors"] = to_dev(colors)
    L["viewmat"] = to_dev(s["viewmat"])[None]
    for k, t in L.items():
        t.requires_grad_(k != "viewmat" or pose)
    out, alphas, info = rasterization(L["means"], L["quats"], L["scales"], L["opacities"], L["colors"], L["viewmat"],
                                      to_dev(s["K"])[None], w, h, backgrounds=to_dev(bg)[None], sh_degree=sh, render_mode=mode,
                                      raw_params=raw, rasterize_mode="antialiased" if aa else "classic", camera_model="fisheye",
                                      radial_coeffs=to_dev(kb.coeffs32(name))[None])
    info["means2d"].retain_grad()
    ((out[0] * to_dev(v_out)).sum() + (alphas[0, ..., 0] * to_dev(v_alpha)).sum()).backward()
    torch.cuda.synchronize()
    g = {k: t.grad for k, t in L.items() if t.grad is not None}
    g = {k: (t[0] if k == "viewmat" else t.reshape(-1) if k == "opacities" else t).cpu().numpy() for k, t in g.items()}
    g["means2d"] = info["means2d"].grad[0].cpu().numpy()
    return out[0].detach().cpu().numpy(), alphas[0, ..., 0].detach().cpu().numpy(), info, g


def _ref_full(name, s, w, h, colors, bg, v_out, v_alpha, radii, depths, *, raw, aa, mode, sh, dev="cuda"):
    """float64: the restatement -> aa_ref.composite and oracle.dense_ref.sh_colors, integer decisions from the kernel's radii
    and a stable depth order (tests/test_camera_models_gpu.py::_ref_full with this file's projection)."""
    from oracle import dense_ref

    def tm(a, rg=False):
        return torch.tensor(np.asarray(a), dtype=F64, device=dev, requires_grad=rg)
    n = s["means"].shape[0]
    pr, _, L = kb.run(name, s, w, h, F64, raw=raw, grad=True, dev=dev)
    m2 = pr["means2d"]
    m2.retain_grad()
    vis = torch.as_tensor(np.asarray(radii) > 0, device=dev)
    O = L["opac_act"] if raw else tm(s["opacities"], True)
    op = O * torch.where(vis, pr["comp"], torch.zeros_like(pr["comp"])) if aa else O
    C = tm(colors, True)
    cols = C if sh is None else dense_ref.sh_colors(sh, C, L["means"], torch.inverse(L["viewmat"])[:3, 3])
    bgt = tm(bg)
    if mode in ("RGB+D", "RGB+ED"):
        cols = torch.cat([cols, pr["depths"][:, None]], dim=1)
        bgt = torch.cat([bgt, torch.zeros(1, dtype=F64, device=dev)])
    order = np.lexsort((np.arange(n), np.asarray(depths)))
    out, alphas, _ = aa_ref.composite(m2, pr["conics"], op, cols, bgt, w, h, radii, order)
    if mode == "RGB+ED":
        out = torch.cat([out[..., :-1], out[..., -1:] / alphas[..., None].clamp(min=1e-10)], dim=-1)
    ((out * tm(v_out)).sum() + (alphas * tm(v_alpha)).sum()).backward()
    g = dict(means=L["means"].grad, quats=L["quats"].grad, scales=L["scales"].grad, colors=C.grad, means2d=m2.grad,
             opacities=L["opacities"].grad if raw else O.grad, viewmat=L["viewmat"].grad)
    return out.detach().cpu().numpy(), {k: v.cpu().numpy() for k, v in g.items()}


@pytest.mark.parametrize("case", kb.RASTER_CASES, ids=lambda c: f"D{c[2]}-{'raw' if c[3] else 'plain'}-{'aa' if c[4] else 'classic'}-{c[5]}-sh{c[6]}-set{c[8]}")
def test_rasterization_against_float64(case):
    """~700 Gaussians, visible ones up to 70 degrees off axis: D = 16 with raw_params and antialiasing, and sh_degree = 3 with
    RGB+ED and viewmats requiring grad; the render and every gradient.  Bound per quantity: min(F64_CAP, F64_MARGIN x e_pin),
    e_pin the pinhole path's error against float64 on the same scene and K through tests/test_camera_models_gpu.py's harness.
    Measured on an MI355X: see docs/LAB_NOTES.md "Fisheye distortion (N21)"."""
    w, h, d, raw, aa, mode, sh, seed, name = case
    s = kb.raster_scene(case)
    colors = s["sh"] if sh is not None else s["colors"]
    d0 = colors.shape[1] if sh is None else 3
    bg = np.full(d0, 0.25, np.float32)
    rng = np.random.default_rng(seed)
    v_out = rng.standard_normal((h, w, d0 + (mode != "RGB"))).astype(np.float32)
    v_alpha = rng.standard_normal((h, w)).astype(np.float32)
    kw = dict(raw=raw, aa=aa, mode=mode, sh=sh)
    # the model under test
    out, _, info, g = _gpu_full(name, s, w, h, colors, bg, v_out, v_alpha, pose=sh is not None, **kw)
    assert info["camera_model"] == "fisheye" and np.array_equal(info["radial_coeffs"].cpu().numpy().reshape(4), kb.coeffs32(name))
    radii, depths = info["radii"][0].cpu().numpy(), info["depths"][0].detach().cpu().numpy()
    _, dec, _ = kb.run(name, s, w, h, F64)
    keep = ~dec["close"]
    assert (~keep).sum() <= cm.MAX_EXCLUDED * keep.size
    np.testing.assert_array_equal(radii[keep], dec["radii"][keep])
    r_out, rg = _ref_full(name, s, w, h, colors, bg, v_out, v_alpha, radii, depths, **kw)
    # the yardstick: the pinhole path on the same scene and K
    p_out, _, p_info, pg = tcm._gpu_full("pinhole", s, w, h, colors, bg, v_out, v_alpha, pose=sh is not None, **kw)
    p_radii, p_depths = p_info["radii"][0].cpu().numpy(), p_info["depths"][0].detach().cpu().numpy()
    pr_out, prg = tcm._ref_full("pinhole", s, w, h, colors, bg, v_out, v_alpha, p_radii, p_depths, **kw)
    assert (radii > 0).sum() >= 100 and (p_radii > 0).sum() >= 20
    assert 55.0 < cm.off_axis_deg(s)[radii > 0].max() <= 70.5
    keys = ["out"] + [k for k in ("colors", "opacities", "means2d", "means", "quats", "scales", "viewmat") if k in g]
    assert ("viewmat" in keys) == (sh is not None) and len(keys) >= 7
    for k in keys:
        e = rel_l2(out, r_out) if k == "out" else rel_l2(g[k], rg[k])
        e_pin = rel_l2(p_out, pr_out) if k == "out" else rel_l2(pg[k], prg[k])
        print(f"kb raster {case} {k}: {e:.2e} pinhole {e_pin:.2e} ratio {e / max(e_pin, 1e-30):.2f}")
        assert e <= _bound(e_pin), (k, e, e_pin)
    culled = radii == 0
    for k in ("means", "quats", "scales", "means2d"):
        assert np.all(g[k][culled] == 0), k


# -- (f) known answers -------------------------------------------------------------------------------------------------------------

def test_known_answers():
    """A Gaussian on the axis lands on (cx, cy) exactly; centres at angle theta0 in the x-z plane land at cx + fx g(theta0)
    (float64 by hand), within the kernel-level bound against the float32 CPU restatement's error on the same points."""
    from gags_amd.rasterization import rasterization
    fx, fy, cx, cy = 100.0, 80.0, 150.0, 120.0
    K = to_dev(np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32))[None]
    th = np.radians(np.array([0.0, 5.0, 15.0, 25.0, 35.0, 45.0, 52.0, 60.0, 66.0, 72.0, 78.0, 83.0, 86.0]))
    r = np.linspace(2.0, 9.0, th.size)
    means = np.stack([r * np.sin(th), np.zeros_like(th), r * np.cos(th)], 1).astype(np.float32)
    n = th.size
    for name in ("A", "B"):
        c32 = kb.coeffs32(name)
        _, _, info = rasterization(to_dev(means), to_dev(np.array([[1.0, 0, 0, 0]] * n, np.float32)), to_dev(np.full((n, 3), 0.05, np.float32)),
                                   to_dev(np.full(n, 0.5, np.float32)), to_dev(np.ones((n, 1), np.float32)),
                                   torch.eye(4, device="cuda")[None], K, 330, 240, camera_model="fisheye", radial_coeffs=to_dev(c32))
        got = info["means2d"][0].cpu().numpy()
        assert bool((info["radii"] > 0).all())
        assert got[0, 0] == cx and np.all(got[:, 1] == cy)             # x = 0 / y = 0: fx * 0 * k + cx
        # by hand, float64, from the float32 centres the kernel was given
        x, z = means[:, 0].astype(np.float64), means[:, 2].astype(np.float64)
        t0 = np.arctan2(x, z)
        k1, k2, k3, k4 = (float(v) for v in c32)
        g0 = t0 * (1 + k1 * t0 ** 2 + k2 * t0 ** 4 + k3 * t0 ** 6 + k4 * t0 ** 8)
        want = np.stack([cx + fx * g0, np.full(n, cy)], 1)
        p32 = torch.tensor(means)
        m32x, m32y, _, _ = kb.cam_map(kb._kc(name, p32), p32[:, 0], p32[:, 1], p32[:, 2], *(torch.tensor(v) for v in (fx, fy, cx, cy)))
        e, e32 = rel_l2(got[1:], want[1:]), rel_l2(torch.stack([m32x, m32y], 1).numpy()[1:], want[1:])
        print(f"kb known answer set {name}: HIP {e:.2e} fp32 restatement {e32:.2e} ratio {e / max(e32, 1e-30):.2f}")
        assert e <= _bound(e32), (e, e32)
        if name == "A":       # 60 degrees off axis: 3.7 % of the image radius inwards of the ideal lens
            assert abs((got[7, 0] - cx) / (fx * th[7]) - (1 - 0.037)) < 1e-3


def test_render_with_a_distorted_fisheye_camera():
    """scene.Camera(camera_model="fisheye", K=, radial_coeffs=) through render(): torch.equal, forward, to rasterization()
    called directly; the 13-float block stays resident in the context's k_cache: one entry, the same memory on every call."""
    from gags_amd.gaussian_renderer import render
    from gags_amd.rasterization import RasterContext, rasterization
    from gags_amd.scene import Camera, GaussianModel
    w, h, n, d = 97, 61, 700, 16
    s = cm.model_scene("fisheye", n, d, w, h, 71, max_deg=70.0)
    R, C = s["R"], s["C"]
    cam = Camera(R, -R.T @ C, 1.0, 0.8, w, h, device="cuda", camera_model="fisheye", K=s["K"], radial_coeffs=kb.COEFFS["A"])
    other = Camera.from_opencv_fisheye((s["K"][0, 0], s["K"][1, 1], s["K"][0, 2], s["K"][1, 2]) + kb.COEFFS["B"], R, -R.T @ C, w, h)
    p = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in s["raw"].items()}
    pc = GaussianModel.from_tensors(p["xyz"], p["scaling_log"], p["rotation"], p["opacity_logit"], p["features_dc"],
                                    p["features_rest"], p["semantic_feature"])
    ctx = RasterContext()
    bg = torch.ones(3, device="cuda")
    with torch.no_grad(), spy_entries("gags_project_fwd_cam") as calls:
        pkg = render(cam, pc, None, bg, feature_mode=True, context=ctx)
        again = render(cam, pc, None, bg, feature_mode=True, context=ctx)
        pkg_b = render(other, pc, None, bg, feature_mode=True, context=ctx)
        vm = cam.world_view_transform.T[None].contiguous()
        out, _, info = rasterization(pc._xyz, pc._rotation, pc._scaling, pc._opacity.squeeze(-1), pc._semantic_feature, vm,
                                     to_dev(s["K"])[None], w, h, backgrounds=torch.ones(1, d, device="cuda"), raw_params=True,
                                     camera_model="fisheye", radial_coeffs=to_dev(kb.coeffs32("A")))
    assert pkg["info"]["camera_model"] == "fisheye" and int(pkg["visibility_filter"].sum()) >= 100
    assert torch.equal(pkg["render"], out[0].permute(2, 0, 1)) and torch.equal(pkg["radii"], info["radii"][0])
    assert torch.equal(pkg["viewspace_points"], info["means2d"]) and torch.equal(again["render"], pkg["render"])
    assert torch.equal(pkg["info"]["radial_coeffs"].reshape(4), to_dev(kb.coeffs32("A")))
    assert not torch.equal(pkg_b["viewspace_points"], pkg["viewspace_points"])      # (the coefficients are part of the key)
    assert len(ctx.k_cache) == 2
    blocks = {k: v for k, v in ctx.k_cache.items() if k[0] == "KB"}
    assert len(blocks) == 2 and all(v.shape == (13,) for v in blocks.values())
    assert len(calls) == 4 and all(a[1] & KB for _, a in calls)
    k_ptr = [a[9].value for _, a in calls]
    assert k_ptr[0] == k_ptr[1] and k_ptr[0] in {v.data_ptr() for v in blocks.values()} and k_ptr[2] != k_ptr[0]
    # ... and differs from the same camera without its coefficients
    ideal = Camera(R, -R.T @ C, 1.0, 0.8, w, h, device="cuda", camera_model="fisheye", K=s["K"])
    with torch.no_grad():
        assert not torch.equal(render(ideal, pc, None, bg, feature_mode=True, context=ctx)["viewspace_points"], pkg["viewspace_points"])


# -- (g) nothing moved -------------------------------------------------------------------------------------------------------------

def test_without_coefficients_nothing_moved():
    """radial_coeffs=None: the recorded calls of the entry pair carry no GAGS_PROJ_KB and the caller's own nine-float K, and
    every output and gradient is torch.equal to the call without the argument and to the entry called directly without the
    flag; with coefficients the flag is there and K is another, 13-float tensor."""
    from gags_amd.rasterization import rasterization
    w, h, n, d = W, H, 700, 16
    s = cm.model_scene("fisheye", n, d, w, h, 72, max_deg=75.0)
    v = to_dev(np.random.default_rng(0).standard_normal((h, w, d)).astype(np.float32))
    Ks = to_dev(s["K"])[None]
    assert Ks.numel() == 9
    res = []
    for kw in ({}, dict(radial_coeffs=None), dict(radial_coeffs=to_dev(kb.coeffs32("A")))):
        L = [to_dev(s[k]).requires_grad_(True) for k in ("means", "quats", "scales", "opacities", "colors")]
        vm = to_dev(s["viewmat"])[None].requires_grad_(True)
        with spy_entries("gags_project_fwd_cam", "gags_project_bwd_cam") as calls:
            out, alphas, info = rasterization(*L, vm, Ks, w, h, camera_model="fisheye", **kw)
            (out[0] * v).sum().backward()
        assert [c[0] for c in calls] == ["gags_project_fwd_cam", "gags_project_bwd_cam"]
        res.append(dict(calls=calls, info=info,
                        t=[out, alphas, info["radii"], info["means2d"], info["conics"], info["depths"], info["tiles_per_gauss"], vm.grad]
                        + [t.grad for t in L]))
    for r in res[:2]:
        assert r["info"]["radial_coeffs"] is None
        for name, a in r["calls"]:
            assert a[0] == 2 and not (a[1] & KB) and a[9].value == Ks.data_ptr(), name
        assert r["calls"][0][1][1] == 0 and r["calls"][1][1][1] == POSE
    for name, a in res[2]["calls"]:
        assert a[0] == 2 and (a[1] & KB) and a[9].value != Ks.data_ptr(), name
    assert int((res[0]["info"]["radii"] > 0).sum()) >= 100
    for a, b in zip(res[0]["t"], res[1]["t"]):
        assert torch.equal(a, b)
    assert not torch.equal(res[2]["t"][3], res[0]["t"][3])
    # the entry itself, without the flag, on the same inputs
    cull = dict(eps2d=0.3, near_plane=0.01, far_plane=1e10, radius_clip=0.0)
    direct = tcm.k_fwd("fisheye", 0, s, cull)
    for k, t in (("radii", 2), ("means2d", 3), ("conics", 4), ("depths", 5), ("tiles", 6)):
        assert torch.equal(direct[k], res[1]["t"][t][0]), k
