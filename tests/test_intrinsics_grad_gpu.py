"""N23 on the GPU: Ks.grad and radial_coeffs.grad from gags_project_bwd_calib to render(), against the float64 reference of
tests/intrinsics_grad_ref.py.

Error of an entry (fx, fy, cx, cy, k1 .. k4): |got - ref64| / sum_i |term_i|, the per-Gaussian terms from float64 autograd with
every Gaussian its own copy of the intrinsics; a case's error is the largest over its entries.  Yardstick: the same
computation in float32 on the CPU.  A handful of numbers per case makes a per-case ratio noisy, so the yardstick is POOLED --
the maximum over the cases of the same test and camera variant -- and the bound is min(F64_CAP, F64_MARGIN x pooled) with the
constants of tests/test_general_camera_gpu.py; a pooled yardstick above the cap would mean the inputs are wrong, and is
refused.  Every case prints the HIP error, its own yardstick, the pooled one and the bound before it asserts; the figures
measured on an MI355X are in docs/LAB_NOTES.md, "Intrinsics gradients (N23)"."""
import copy
import functools

import numpy as np
import pytest
import torch

import camera_models_ref as cm
import fisheye_kb_ref as kb
import intrinsics_grad_ref as ig
import test_camera_models_gpu as tcm
import test_streams_gpu as TS
from helpers import rel_l2, spy_entries, to_dev
from test_general_camera_gpu import F64_CAP, F64_MARGIN
from test_intrinsics_grad_cpu import clamp_sides, pinhole_scene

pytestmark = pytest.mark.gpu

F64 = torch.float64
W, H = cm.KERNEL_W, cm.KERNEL_H
RAW, AA, POSE, KB = 1, 2, 4, kb.KB
# variant -> (camera model, coefficient set or None)
VARIANTS = {"pinhole": ("pinhole", None), "ortho": ("ortho", None), "fisheye": ("fisheye", None), "fisheye_kbA": ("fisheye", "A"),
            "fisheye_kbB": ("fisheye", "B"), "fisheye_kb0": ("fisheye", "zero")}
KERNEL_NS = (1, 63, 64, 65, 255, 256, 257, 700)    # lane, wave and workgroup edges; 257 and 700: two and three partial rows
ALL_FLAGS_NS = (257, 700)                          # RAW x AA at these; the others run plain and RAW | AA
KERNEL_CASES = [(n, raw, aa) for n in KERNEL_NS for raw in (False, True) for aa in (False, True)
                if n in ALL_FLAGS_NS or raw == aa]


def _bound(pooled):
    return min(F64_CAP, F64_MARGIN * pooled)


def _report(label, e, y, pooled):
    print(f"{label}: HIP {e:.3e}, float32 CPU {y:.3e}, pooled {pooled:.3e}, ratio to pooled {e / max(pooled, 1e-300):.2f}, "
          f"bound {_bound(pooled):.3e}")


# -- 1. the entry directly ---------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _variant_scene(variant):
    """(scene of 700 with K = the block the entries read, culling parameters, index of the first visible Gaussian)."""
    model, coeffs = VARIANTS[variant]
    if model == "pinhole":
        s, cull = pinhole_scene()
    elif coeffs in ("A", "B"):
        s, cull = kb.kernel_scene(coeffs)
    else:
        s, cull = cm.model_scene(model, 700, 0, W, H, cm.KERNEL_SEEDS[model]), dict(cm.KERNEL_CULL)
    radii = _forward(variant, s, cull, 0)["radii"].cpu().numpy()
    return s, cull, int(np.flatnonzero(radii > 0)[0])


def _entry_scene(variant, s):
    """The scene as the harness hands it to the entries: with coefficients K is the 13-float block."""
    coeffs = VARIANTS[variant][1]
    return s if coeffs is None else dict(s, K=kb.block(s["K"], coeffs))


def _forward(variant, s, cull, flags):
    model, coeffs = VARIANTS[variant]
    return tcm.k_fwd(model, flags | (KB if coeffs is not None else 0), _entry_scene(variant, s), cull)


def _cut(variant, n):
    s, cull, first = _variant_scene(variant)
    return tcm._cut(s, n, start=first if n == 1 else 0), cull      # (n = 1: a Gaussian on screen)


def calib_entry(variant, flags, s, cull, radii, cot, *, outputs=True, fill=7.0):
    """gags_project_bwd_calib on pre-filled outputs: dict(means, quats, scales, opacities | None, viewmat | None, K [9],
    coeffs [4] | None) of GPU tensors.  outputs=False: the scene gradients are passed as NULL."""
    from gags_amd import _lib
    from gags_amd._lib import check, ptr
    lib = _lib.load()
    model, coeffs = VARIANTS[variant]
    flags |= KB if coeffs is not None else 0
    s = _entry_scene(variant, s)
    means, quats, scales, logit = tcm._inputs(s, flags)
    n = means.shape[0]
    raw, aa, pose = bool(flags & RAW), bool(flags & AA), bool(flags & POSE)
    full = lambda *shape: torch.full(shape, fill, device="cuda")  # noqa: E731
    g = dict(means=full(n, 3) if outputs else None, quats=full(n, 4) if outputs else None, scales=full(n, 3) if outputs else None,
             opacities=full(n) if (raw and outputs) else None, viewmat=full(4, 4) if pose else None, K=full(9),
             coeffs=full(4) if coeffs is not None else None)
    rows = lib.gags_project_calib_partials(n)
    partials = full(rows, _lib.GAGS_CALIB_PARTIAL_FLOATS)
    v_opac = to_dev(cot["opacities"][:n]) if raw else None
    v_comp = to_dev(cot["comp"][:n]) if (aa and not raw) else None
    vm, K = to_dev(s["viewmat"]), to_dev(s["K"])      # (held here: a temporary's memory would be reused before the launch)
    v_m2, v_z, v_con = to_dev(cot["means2d"][:n]), to_dev(cot["depths"][:n]), to_dev(cot["conics"][:n])
    check(lib.gags_project_bwd_calib(cm.MODELS[model], flags, n, ptr(means), ptr(quats), ptr(scales), ptr(logit), 1.0, ptr(vm), ptr(K),
                                     W, H, cull["eps2d"], ptr(radii), ptr(v_m2), ptr(v_z), ptr(v_con), ptr(v_opac), ptr(v_comp),
                                     ptr(g["means"]), ptr(g["quats"]), ptr(g["scales"]), ptr(g["opacities"]), ptr(g["viewmat"]),
                                     ptr(g["K"]), ptr(g["coeffs"]), ptr(partials), partials.numel() * 4, _lib.stream()),
          "gags_project_bwd_calib")
    torch.cuda.synchronize()
    return g


def _got(g):
    return ig.from_kernel(g["K"].cpu().numpy(), None if g["coeffs"] is None else g["coeffs"].cpu().numpy())


@functools.lru_cache(maxsize=None)
def _kernel_refs(variant):
    """float64 and float32 (both on the CPU) per-Gaussian autograd for every case of test 1 of one variant, the loss masked to
    the HIP forward's radii > 0: computed once, never modified.  ({(n, raw, aa): (ref64, yardstick, radii)}, pooled)."""
    model, coeffs = VARIANTS[variant]
    refs = {}
    for n, raw, aa in KERNEL_CASES:
        s, cull = _cut(variant, n)
        radii = _forward(variant, s, cull, (RAW if raw else 0) | (AA if aa else 0))["radii"].cpu().numpy()
        cot = cm.cotangents(700, 9)
        kw = dict(antialiased=aa, raw=raw, eps2d=cull["eps2d"])
        r64 = ig.project_grads(model, coeffs, s, W, H, radii, cot, **kw)
        r32 = ig.project_grads(model, coeffs, s, W, H, radii, cot, dtype=torch.float32, **kw)
        refs[(n, raw, aa)] = (r64, float(ig.entry_errors(r32["sum"], r64).max()), radii)
    pooled = max(v[1] for v in refs.values())
    assert 0 < pooled <= F64_CAP, (variant, pooled)      # (above the cap: the inputs are wrong, not the cap)
    return refs, pooled


def test_pinhole_scene_reaches_past_the_clamp_on_both_sides():
    s, cull, _ = _variant_scene("pinhole")
    radii = _forward("pinhole", s, cull, 0)["radii"].cpu().numpy()
    sides = clamp_sides(s, radii)
    print("visible past the clamp (x+, x-, y+, y-):", sides, "visible:", int((radii > 0).sum()))
    assert min(sides) >= 3, sides


@pytest.mark.parametrize("n,raw,aa", KERNEL_CASES)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_calib_entry_against_float64_and_the_existing_entry(variant, n, raw, aa):
    """gags_project_bwd_calib behind the HIP forward, random cotangents, against float64 per-Gaussian autograd.  Per case:
    v_means, v_quats, v_scales and v_logit are torch.equal to gags_project_bwd_cam's, with POSE v_viewmat is torch.equal to the
    pose kernel's; two calls (and a call with the scene outputs NULL, and one without POSE) give v_K and v_coeffs the same bits;
    the five constant entries of v_K are exactly zero; with all-zero coefficients v_coeffs is not zero.
    Measured on an MI355X (docs/LAB_NOTES.md, "Intrinsics gradients (N23)"): HIP error 6.3e-9 .. 1.2e-6 over the 120 cases, the
    float32 yardsticks 3.7e-9 .. 2.0e-6, pooled per variant 4.5e-7 .. 2.0e-6, worst HIP / pooled 1.16 (bound: 3)."""
    model, coeffs = VARIANTS[variant]
    refs, pooled = _kernel_refs(variant)
    r64, y, radii_np = refs[(n, raw, aa)]
    s, cull = _cut(variant, n)
    cot = cm.cotangents(700, 9)
    radii = to_dev(radii_np)
    flags = (RAW if raw else 0) | (AA if aa else 0)
    nvis = int((radii_np > 0).sum())
    assert nvis >= 1 and (n - nvis >= 1 or n < 63), (nvis, n)
    g = calib_entry(variant, flags | POSE, s, cull, radii, cot)
    old = tcm.k_bwd(model, flags | POSE | (KB if coeffs is not None else 0), _entry_scene(variant, s), cull, radii, cot)
    for k in ("means", "quats", "scales", "opacities", "viewmat"):
        assert (g[k] is None and old[k] is None) or torch.equal(g[k], old[k]), k
    for other in (calib_entry(variant, flags | POSE, s, cull, radii, cot, fill=-5.0),
                  calib_entry(variant, flags | POSE, s, cull, radii, cot, outputs=False, fill=11.0),
                  calib_entry(variant, flags, s, cull, radii, cot, fill=3.0)):
        assert torch.equal(other["K"], g["K"]) and (coeffs is None or torch.equal(other["coeffs"], g["coeffs"]))
    plain = calib_entry(variant, flags, s, cull, radii, cot, fill=3.0)
    assert plain["viewmat"] is None
    for k in ("means", "quats", "scales", "opacities"):
        assert (plain[k] is None and old[k] is None) or torch.equal(plain[k], old[k]), k
    vK = g["K"].cpu().numpy()
    assert np.all(vK[[1, 3, 6, 7, 8]] == 0) and np.all(np.isfinite(vK)) and np.all(vK[[0, 2, 4, 5]] != 0)
    if coeffs is not None:
        assert bool(torch.isfinite(g["coeffs"]).all()) and bool((g["coeffs"] != 0).all())
    errs = ig.entry_errors(_got(g), r64)
    print()
    print("   per entry:", " ".join(f"{k}={e:.1e}" for k, e in zip(ig.ENTRIES, errs)))
    _report(f"calib {variant} n={n} raw={raw} aa={aa} ({nvis} visible)", float(errs.max()), y, pooled)
    assert errs.max() <= _bound(pooled)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_calib_entry_with_everything_culled_and_with_no_gaussians(variant):
    model, coeffs = VARIANTS[variant]
    s, cull, _ = _variant_scene(variant)
    cull = dict(cull, near_plane=1e9, far_plane=2e9)      # every Gaussian is nearer than the near plane
    cot = cm.cotangents(700, 9)
    for flags in (0, RAW | AA):
        radii = _forward(variant, s, cull, flags)["radii"]
        assert not bool(radii.any())
        g = calib_entry(variant, flags | POSE, s, cull, radii, cot)
        assert not bool(g["K"].any()) and not bool(g["viewmat"].any()) and (coeffs is None or not bool(g["coeffs"].any()))
        assert all(not bool(g[k].any()) for k in ("means", "quats", "scales"))
        e = calib_entry(variant, flags | POSE, tcm._cut(s, 0), cull, radii[:0].contiguous(), {k: v[:0] for k, v in cot.items()})
        assert not bool(e["K"].any()) and not bool(e["viewmat"].any()) and (coeffs is None or not bool(e["coeffs"].any()))
        e = calib_entry(variant, flags, tcm._cut(s, 0), cull, radii[:0].contiguous(), {k: v[:0] for k, v in cot.items()})
        assert not bool(e["K"].any()) and (coeffs is None or not bool(e["coeffs"].any()))


# -- 2. through rasterization() ----------------------------------------------------------------------------------------------------

# (variant, w, h, D, raw_params, antialiased, render_mode, sh_degree, seed): kb.RASTER_CASES and a pinhole and an ortho case of
# the same size
def _from_kb(c):
    return ("fisheye_kb" + c[8],) + tuple(c[:8])


RASTER_CASES = [_from_kb(c) for c in kb.RASTER_CASES] + [("pinhole", 97, 61, 16, False, False, "RGB", None, 63),
                                                         ("ortho", 97, 61, 16, True, True, "RGB+ED", None, 64)]
RASTER_IDS = [f"{c[0]}-D{c[3]}-{'raw' if c[4] else 'plain'}-{'aa' if c[5] else 'classic'}-{c[6]}-sh{c[7]}" for c in RASTER_CASES]


@functools.lru_cache(maxsize=None)
def _raster_inputs(case):
    variant, w, h, d, raw, aa, mode, sh, seed = case
    model, coeffs = VARIANTS[variant]
    if coeffs is not None:
        s = kb.raster_scene(case[1:] + (coeffs,))
    elif model == "pinhole":
        s = cm.model_scene(model, 700, d, w, h, seed, scale_mult=30.0)
    else:
        s = cm.model_scene(model, 700, d, w, h, seed, max_deg=75.0)
    colors = s["sh"] if sh is not None else s["colors"]
    d0 = colors.shape[1] if sh is None else 3
    rng = np.random.default_rng(seed)
    v_out = rng.standard_normal((h, w, d0 + (mode != "RGB"))).astype(np.float32)
    v_alpha = rng.standard_normal((h, w)).astype(np.float32)
    return s, colors, np.full(d0, 0.25, np.float32), v_out, v_alpha


def _raster_run(case, *, camera=True, scene=True, pose=None, coeff_shape=(4,), backward=True):
    """rasterization() on a case: dict(out, alphas, info, K = Ks.grad, coeffs = radial_coeffs.grad, vm = viewmats.grad, g = the
    scene gradients, calls = the projection entries called, in order)."""
    from gags_amd.rasterization import rasterization
    variant, w, h, d, raw, aa, mode, sh, seed = case
    model, coeffs = VARIANTS[variant]
    s, colors, bg, v_out, v_alpha = _raster_inputs(case)
    if raw:
        p = s["raw"]
        L = dict(means=p["xyz"].cuda(), quats=p["rotation"].cuda(), scales=p["scaling_log"].cuda(), opacities=p["opacity_logit"].cuda())
    else:
        L = dict(means=to_dev(s["means"]), quats=to_dev(s["quats"]), scales=to_dev(s["scales"]), opacities=to_dev(s["opacities"]))
    L["colors"] = to_dev(colors)
    for t in L.values():
        t.requires_grad_(scene)
    vm = to_dev(s["viewmat"])[None].requires_grad_(scene if pose is None else pose)
    Ks = to_dev(s["K"])[None].requires_grad_(camera)
    rc = None if coeffs is None else to_dev(kb.coeffs32(coeffs)).reshape(coeff_shape).requires_grad_(camera)
    with spy_entries("gags_project_fwd_cam", "gags_project_bwd_cam", "gags_project_bwd_calib", "gags_project_bwd_pose") as calls:
        out, alphas, info = rasterization(L["means"], L["quats"], L["scales"], L["opacities"], L["colors"], vm, Ks, w, h,
                                          backgrounds=to_dev(bg)[None], sh_degree=sh, render_mode=mode, raw_params=raw,
                                          rasterize_mode="antialiased" if aa else "classic", camera_model=model, radial_coeffs=rc)
        if backward:
            ((out[0] * to_dev(v_out)).sum() + (alphas[0, ..., 0] * to_dev(v_alpha)).sum()).backward()
    torch.cuda.synchronize()
    return dict(out=out[0].detach(), alphas=alphas[0, ..., 0].detach(), info=info, K=Ks.grad, coeffs=None if rc is None else rc.grad,
                vm=vm.grad, g={k: t.grad for k, t in L.items() if t.grad is not None}, calls=[c[0] for c in calls],
                flags=[c[1][1] for c in calls])


@functools.lru_cache(maxsize=None)
def _raster_refs():
    """Per case of RASTER_CASES: float64 on the device and float32 on the CPU (with the float64 run's blend decisions), radii and
    depth order from the HIP forward: computed once, never modified.  ({case: (ref64, yardstick, radii)}, pooled)."""
    refs = {}
    for case in RASTER_CASES:
        variant, w, h, d, raw, aa, mode, sh, seed = case
        model, coeffs = VARIANTS[variant]
        s, colors, bg, v_out, v_alpha = _raster_inputs(case)
        with torch.no_grad():
            info = _raster_run(case, camera=False, scene=False, backward=False)["info"]
        radii, depths = info["radii"][0].cpu().numpy(), info["depths"][0].cpu().numpy()
        kw = dict(raw=raw, antialiased=aa, render_mode=mode, sh_degree=sh)
        r64 = ig.full(model, coeffs, s, w, h, colors, bg, v_out, v_alpha, radii, depths, dev="cuda", **kw)
        r32 = ig.full(model, coeffs, s, w, h, colors, bg, v_out, v_alpha, radii, depths, dtype=torch.float32,
                      include=r64["include"].cpu(), **kw)
        refs[case] = (r64, float(ig.entry_errors(r32["sum"], r64).max()), radii)
    pooled = max(v[1] for v in refs.values())
    assert 0 < pooled <= F64_CAP, pooled
    return refs, pooled


def _check_camera_gradient(case, r, label):
    refs, pooled = _raster_refs()
    r64, y, radii = refs[case]
    coeffs = VARIANTS[case[0]][1]
    assert (radii > 0).sum() >= 100
    np.testing.assert_array_equal(r["info"]["radii"][0].cpu().numpy(), radii)
    assert rel_l2(r["out"].cpu().numpy(), r64["out"]) < 1e-5          # (the same render: the decisions agree)
    assert r["K"].shape == (1, 3, 3) and r["K"].dtype == torch.float32
    vK = r["K"][0].reshape(9).cpu().numpy()
    assert np.all(vK[[1, 3, 6, 7, 8]] == 0)
    errs = ig.entry_errors(ig.from_kernel(vK, None if coeffs is None else r["coeffs"].reshape(4).cpu().numpy()), r64)
    print()
    print("   per entry:", " ".join(f"{k}={e:.1e}" for k, e in zip(ig.ENTRIES, errs)))
    _report(f"rasterization() {label}", float(errs.max()), y, pooled)
    assert errs.max() <= _bound(pooled)
    return r64


@pytest.mark.parametrize("case", RASTER_CASES, ids=RASTER_IDS)
def test_camera_gradients_through_rasterization(case):
    """Ks.grad [1,3,3] and radial_coeffs.grad against float64 autograd of the oracle-style composition (projection, SH colours,
    depth channel, composite, ED division) -- antialiased with raw_params at D = 16, RGB+ED with sh_degree = 3, a pinhole and an
    antialiased orthographic RGB+ED case -- with K, the coefficients, viewmats and the scene all requiring grad, and again with
    the camera alone (scene and pose frozen: no scene tensor gets a gradient).
    Measured on an MI355X (docs/LAB_NOTES.md, "Intrinsics gradients (N23)"): HIP error 9.7e-8 .. 1.9e-6, float32 yardsticks
    1.2e-7 .. 8.3e-7, pooled 8.3e-7, bound 2.5e-6; the worst, 2.28 x pooled, is the SH case on the float-atomic backward."""
    coeffs = VARIANTS[case[0]][1]
    for shape in ((4,), (1, 4)) if coeffs is not None else ((4,),):
        r = _raster_run(case, coeff_shape=shape)
        assert r["calls"] == ["gags_project_fwd_cam", "gags_project_bwd_calib"] and r["flags"][1] & POSE
        assert bool(r["flags"][1] & KB) == (coeffs is not None)
        if coeffs is not None:
            assert tuple(r["coeffs"].shape) == shape
        _check_camera_gradient(case, r, f"{case[0]} everything, coefficients {list(shape)}")
    assert len(r["g"]) == 5 and r["vm"] is not None
    only = _raster_run(case, scene=False)
    assert only["g"] == {} and only["vm"] is None and torch.equal(only["out"], r["out"])
    assert only["calls"] == ["gags_project_fwd_cam", "gags_project_bwd_calib"] and not (only["flags"][1] & POSE)
    _check_camera_gradient(case, only, f"{case[0]} camera alone")


@pytest.mark.parametrize("case", [RASTER_CASES[0], RASTER_CASES[2]], ids=[RASTER_IDS[0], RASTER_IDS[2]])
def test_without_a_trainable_camera_nothing_moved(case):
    """With nothing of the camera requiring grad the projection entries called are exactly gags_project_fwd_cam and
    gags_project_bwd_cam; the render, viewmats.grad and every scene gradient are torch.equal between that call and the call
    with Ks (and radial_coeffs) requiring grad (D = 16: no float atomics on the way)."""
    plain, cam = _raster_run(case, camera=False), _raster_run(case)
    assert plain["calls"] == ["gags_project_fwd_cam", "gags_project_bwd_cam"] and plain["K"] is None and plain["coeffs"] is None
    assert cam["calls"] == ["gags_project_fwd_cam", "gags_project_bwd_calib"] and cam["K"] is not None
    assert torch.equal(plain["out"], cam["out"]) and torch.equal(plain["alphas"], cam["alphas"])
    assert torch.equal(plain["vm"], cam["vm"]) and set(plain["g"]) == set(cam["g"]) and len(plain["g"]) == 5
    for k in plain["g"]:
        assert torch.equal(plain["g"][k], cam["g"][k]), k
    frozen = _raster_run(case, camera=False, scene=True, pose=False)
    assert frozen["calls"] == ["gags_project_fwd_cam", "gags_project_bwd_cam"] and not (frozen["flags"][1] & POSE)


# -- 3. render() and IntrinsicsDelta -----------------------------------------------------------------------------------------------

def _model_and_camera(seed=71, n=300, coeffs="A", d=16):
    from gags_amd.scene import Camera, GaussianModel
    w, h = 97, 61
    s = cm.model_scene("fisheye", n, d, w, h, seed, max_deg=70.0)
    R, C = s["R"], s["C"]
    cam = Camera(R, -R.T @ C, 1.0, 0.8, w, h, device="cuda", camera_model="fisheye", K=s["K"], radial_coeffs=kb.COEFFS[coeffs])
    p = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in s["raw"].items()}
    pc = GaussianModel.from_tensors(p["xyz"], p["scaling_log"], p["rotation"], p["opacity_logit"], p["features_dc"],
                                    p["features_rest"], p["semantic_feature"])
    return s, pc, cam


def test_render_hands_a_trainable_camera_through():
    """render() with IntrinsicsDelta.camera: the gradient reaches log_focal, principal and coeffs, equals the chain rule applied
    to rasterization()'s Ks.grad / radial_coeffs.grad of the same call made directly, and the trainable camera leaves no entry
    in the context's k_cache (the plain camera leaves one)."""
    from gags_amd.gaussian_renderer import render
    from gags_amd.pose import IntrinsicsDelta
    from gags_amd.rasterization import RasterContext, rasterization
    s, pc, cam = _model_and_camera()
    for t in (pc._xyz, pc._rotation, pc._scaling, pc._opacity, pc._semantic_feature):
        t.requires_grad_(False)
    intr = IntrinsicsDelta(2).cuda()
    ctx = RasterContext()
    bg = torch.ones(3, device="cuda")
    v = to_dev(np.random.default_rng(5).standard_normal((16, 61, 97)).astype(np.float32))
    with spy_entries("gags_project_fwd_cam", "gags_project_bwd_cam", "gags_project_bwd_calib") as calls:
        pkg = render(intr.camera(cam, 1), pc, None, bg, feature_mode=True, context=ctx)
        (pkg["render"] * v).sum().backward()
    assert [c[0] for c in calls] == ["gags_project_fwd_cam", "gags_project_bwd_calib"] and len(ctx.k_cache) == 0
    assert int(pkg["visibility_filter"].sum()) >= 30
    for p in (intr.log_focal, intr.principal, intr.coeffs):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool((p.grad[1] != 0).all()) and not bool(p.grad[0].any())
    with torch.no_grad():
        plain = render(cam, pc, None, bg, feature_mode=True, context=ctx)
    assert len(ctx.k_cache) == 1 and torch.equal(plain["render"], pkg["render"])      # (at zero: the camera's own values)
    # the same call made directly
    Ks = to_dev(s["K"])[None].requires_grad_(True)
    rc = to_dev(kb.coeffs32("A")).requires_grad_(True)
    out, _, _ = rasterization(pc._xyz, pc._rotation, pc._scaling, pc._opacity.squeeze(-1), pc._semantic_feature,
                              cam.world_view_transform.T[None].contiguous(), Ks, 97, 61, backgrounds=torch.ones(1, 16, device="cuda"),
                              raw_params=True, camera_model="fisheye", radial_coeffs=rc)
    (out[0].permute(2, 0, 1) * v).sum().backward()
    assert torch.equal(out[0].permute(2, 0, 1), pkg["render"])
    K = to_dev(s["K"])
    assert torch.equal(intr.log_focal.grad[1], torch.stack([Ks.grad[0, 0, 0] * K[0, 0], Ks.grad[0, 1, 1] * K[1, 1]]))
    assert torch.equal(intr.principal.grad[1], torch.stack([Ks.grad[0, 0, 2], Ks.grad[0, 1, 2]]))
    assert torch.equal(intr.coeffs.grad[1], rc.grad)


def test_render_refuses_a_trainable_camera_on_the_wrong_device_before_any_launch():
    from gags_amd.gaussian_renderer import render
    s, pc, cam = _model_and_camera()
    bad = copy.copy(cam)
    bad.K = torch.tensor(s["K"], requires_grad=True)      # (on the CPU)
    with spy_entries("gags_project_fwd_cam") as calls, pytest.raises(ValueError):
        render(bad, pc, None, torch.ones(3, device="cuda"), feature_mode=True)
    assert not calls


RECOVER_STEPS, RECOVER_LR = 60, 2e-3


def test_intrinsics_refinement_recovers_focal_length_and_k1():
    """A 97 x 61 fisheye view of 300 Gaussians rendered with the true (K, k) is the target; the start has fx, fy 2 % too long
    and k1 0.01 too large; 60 Adam steps on an IntrinsicsDelta alone (scene and pose frozen).  The loss falls below a tenth of
    its start and |fx - fx_true| and |k1 - k1_true| both shrink: conditions on direction, not measured tolerances.  The
    learning rate was chosen on the float64 CPU reference of the same scene and schedule before any GPU run (loss 2141-fold
    down, |fx - true| 0.582 -> 0.032, |k1 - true| 0.0100 -> 0.0014); measured on an MI355X: the same figures."""
    from gags_amd.gaussian_renderer import render
    from gags_amd.pose import IntrinsicsDelta
    s, pc, cam_true = _model_and_camera()
    for t in (pc._xyz, pc._rotation, pc._scaling, pc._opacity, pc._semantic_feature):
        t.requires_grad_(False)
    bg = torch.zeros(3, device="cuda")
    with torch.no_grad():
        gt = render(cam_true, pc, None, bg, feature_mode=True)["render"].clone()
    cam0 = copy.copy(cam_true)
    cam0.K = cam_true.K.copy()
    cam0.K[0, 0] *= 1.02
    cam0.K[1, 1] *= 1.02
    cam0.radial_coeffs = cam_true.radial_coeffs + np.array([0.01, 0, 0, 0], np.float32)
    fx_true, k1_true = float(cam_true.K[0, 0]), float(cam_true.radial_coeffs[0])
    intr = IntrinsicsDelta(1).cuda()
    opt = torch.optim.Adam(intr.parameters(), lr=RECOVER_LR)
    losses, fx_err, k1_err = [], [], []
    for _ in range(RECOVER_STEPS + 1):
        cam = intr.camera(cam0, 0)
        loss = ((render(cam, pc, None, bg, feature_mode=True)["render"] - gt) ** 2).mean()
        losses.append(float(loss.detach()))
        fx_err.append(abs(float(cam.K[0, 0].detach()) - fx_true))
        k1_err.append(abs(float(cam.radial_coeffs[0].detach()) - k1_true))
        opt.zero_grad()
        loss.backward()
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in intr.parameters())
        opt.step()
    print(f"\nrefinement: loss {losses[0]:.3e} -> {losses[-1]:.3e} ({losses[0] / losses[-1]:.1f}-fold), "
          f"|fx - true| {fx_err[0]:.3f} -> {fx_err[-1]:.4f}, |k1 - true| {k1_err[0]:.4f} -> {k1_err[-1]:.5f}")
    assert losses[-1] < 0.1 * losses[0] and fx_err[-1] < fx_err[0] and k1_err[-1] < k1_err[0]


# -- 4. stream order ---------------------------------------------------------------------------------------------------------------

def _stream_inputs(seed):
    t = TS._raster_inputs(32, 97, 61)(seed)
    t["coeffs"] = torch.tensor(kb.coeffs32("A" if seed == TS.REAL_SEED else "B"))
    return t


def _stream_run(dev):
    """rasterization() of a fisheye with coefficients; K, the coefficients, the pose and the means require grad."""
    from gags_amd.rasterization import RasterContext, rasterization
    leaf = {k: dev[k].detach().requires_grad_(True) for k in ("means", "K", "coeffs", "viewmat0")}
    out, alphas, info = rasterization(leaf["means"], dev["quats"], dev["scales"], dev["opacities"], dev["colors"], leaf["viewmat0"][None],
                                      leaf["K"][None], 97, 61, backgrounds=dev["bg"][None], context=RasterContext(),
                                      camera_model="fisheye", radial_coeffs=leaf["coeffs"])
    ((out[0] * dev["v_out0"]).sum() + (alphas[0, ..., 0] * dev["v_alpha0"]).sum()).backward()
    res = {"out": out, "alphas": alphas, "radii": info["radii"]}
    res.update({f"grad.{k}": t.grad for k, t in leaf.items()})
    return {k: TS._host(v) for k, v in res.items()}


# The case joins the cases of tests/test_streams_gpu.py, whose last test accounts for every streamed entry the package names:
# gags_project_bwd_calib is reached on a side stream here.
STREAM_CASE = "raster_fisheye_intrinsics"
TS.CASES[STREAM_CASE] = TS.Case(_stream_inputs, _stream_run)


def test_side_stream_behind_late_producers_equals_the_default_stream(oracle):
    """The case above on a side stream behind late producers (tests/stream_harness.py), decoy inputs in memory until the delayed
    copies land: every output and gradient torch.equal to the run on the default stream, every streamed entry called with the
    side stream's handle, gags_project_bwd_calib among them."""
    TS.test_side_stream_behind_late_producers_equals_the_default_stream(oracle, STREAM_CASE)
    assert "gags_project_bwd_calib" in TS.RECORDED[STREAM_CASE]
    assert float(TS._reference(STREAM_CASE)[0]["grad.K"].abs().max()) > 0 and float(TS._reference(STREAM_CASE)[0]["grad.coeffs"].abs().max()) > 0
