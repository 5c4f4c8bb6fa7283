"""N16 on the GPU: rasterize_mode="antialiased" and absgrad=True, from the kernels to render() and the densification
statistics, against the float64 restatement of tests/aa_ref.py.  Scenes: helpers.general_scene under the four GENERAL_CAMERAS at
the sizes and seeds of tests/test_general_camera_gpu.py::FULL_CASES, splat size scale_mult = 10, where every case has at least 20
visible Gaussians with comp < 0.5, in [0.5, 0.9) and >= 0.9 (asserted).  Bounds are tied to yardsticks computed on the same
case -- a float32 CPU evaluation of aa_ref, or the fp32 oracle's own float64 error -- and every test prints HIP error,
yardstick and ratio before it asserts."""
import functools

import numpy as np
import pytest
import torch

import aa_ref
from helpers import general_camera, general_scene, rel_l2, scene_arrays, to_dev
from test_antialias_absgrad_cpu import hand_absgrad
from test_general_camera_gpu import F64_CAP, F64_MARGIN, FULL_CASES, _cotangents, oracle_full
from test_parity_gpu import GRAD_TOL

pytestmark = pytest.mark.gpu

MULT = 10.0
CAMS = {c[0]: (c[1], c[2], c[3], c[5]) for c in FULL_CASES}   # camera -> (w, h, n, seed)
ACT = ("means", "quats", "scales", "opacities", "colors")
BG = 0.25


def _scene(cam, d):
    w, h, n, seed = CAMS[cam]
    return general_scene(n, d, w, h, seed, scale_mult=MULT, **general_camera(cam, w, h)), w, h, n, seed


def _run(s, w, h, d, *, mode="classic", absgrad=False, flags=0, grad=True, v=None, opacities=None, leaves=ACT):
    """rasterization() on a scene's arrays with background BG: dict(out, alphas, info, g = gradients (torch, on the device),
    absgrad).  v = (v_out, v_alpha) numpy cotangents; without them no backward."""
    from gags_amd.rasterization import rasterization
    L = dict(means=to_dev(s["means"]), quats=to_dev(s["quats"]), scales=to_dev(s["scales"]),
             opacities=to_dev(s["opacities"]) if opacities is None else opacities.detach().clone(), colors=to_dev(s["colors"][:, :d]))
    for k, t in L.items():
        t.requires_grad_(grad and k in leaves)
    with torch.set_grad_enabled(grad):
        out, alphas, info = rasterization(L["means"], L["quats"], L["scales"], L["opacities"], L["colors"], to_dev(s["viewmat"])[None],
                                          to_dev(s["K"])[None], w, h, backgrounds=to_dev(np.full(d, BG, np.float32))[None],
                                          rasterize_mode=mode, absgrad=absgrad, raster_flags=flags)
    r = dict(out=out[0].detach(), alphas=alphas[0, ..., 0].detach(), info=info, g=None, absgrad=None, leaves=L)
    if v is not None:
        if info["means2d"].requires_grad:
            info["means2d"].retain_grad()
        ((out[0] * to_dev(v[0])).sum() + (alphas[0, ..., 0] * to_dev(v[1])).sum()).backward()
        r["g"] = {k: t.grad for k, t in L.items() if t.grad is not None}
        if info["means2d"].grad is not None:
            r["g"]["means2d"] = info["means2d"].grad[0]
        r["absgrad"] = getattr(info["means2d"], "absgrad", None)
    torch.cuda.synchronize()
    return r


@functools.lru_cache(maxsize=None)
def _reference(oracle, cam, d, antialiased, f32=True):
    """One case through float64 (on the GPU), and through float32 on the CPU with the float64 run's blend decisions: computed
    once per (camera, D, mode) and shared, never modified.  The integer decisions come from the fp32 oracle, which in
    antialiased mode is called with opacities * comp."""
    s, w, h, n, seed = _scene(cam, d)
    v = _cotangents(seed, h, w, d)
    bg = np.full(d, BG, np.float32)
    radii = oracle.project_fwd(s["means"], s["quats"], s["scales"], s["viewmat"], s["K"], w, h)[0]
    t64 = lambda a: torch.tensor(a, dtype=torch.float64)
    comp64 = aa_ref.project(t64(s["means"]), t64(s["quats"]), t64(s["scales"]), t64(s["viewmat"]), t64(s["K"]), w, h, radii=radii)[3]
    t32 = lambda a: torch.tensor(a, dtype=torch.float32)
    comp32 = aa_ref.project(t32(s["means"]), t32(s["quats"]), t32(s["scales"]), t32(s["viewmat"]), t32(s["K"]), w, h, radii=radii)[3]
    op = (torch.tensor(s["opacities"]) * comp32).numpy() if antialiased else s["opacities"]
    oi = oracle.rasterization(s["means"], s["quats"], s["scales"], op, s["colors"], s["viewmat"], s["K"], bg, w, h)[2]
    assert np.array_equal(oi["radii"], radii)
    r64 = aa_ref.full(s, w, h, s["colors"], bg, v[0], v[1], radii, oi["depths"], antialiased=antialiased, dev="cuda")
    assert r64["n_blend"] == oi["n_blend"], (r64["n_blend"], oi["n_blend"])
    r32 = None
    if f32:
        r32 = aa_ref.full(s, w, h, s["colors"], bg, v[0], v[1], radii, oi["depths"], antialiased=antialiased, dtype=torch.float32,
                          include=r64["include"].cpu())
    order = np.lexsort((np.arange(n), oi["depths"]))
    blended = np.zeros(n, bool)
    blended[order] = r64["include"].any(0).cpu().numpy()
    return dict(s=s, w=w, h=h, n=n, v=v, radii=radii, comp64=comp64.numpy(), comp32=comp32.numpy(), r64=r64, r32=r32, blended=blended)


def _census(comp, radii):
    vis = np.asarray(radii) > 0
    bands = (int((vis & (comp < 0.5)).sum()), int((vis & (comp >= 0.5) & (comp < 0.9)).sum()), int((vis & (comp >= 0.9)).sum()))
    assert min(bands) >= 20, bands
    return bands


# -- 1. compensations -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cam", list(CAMS))
def test_compensations_against_float64(oracle, cam):
    """info["compensations"] against the float64 restatement, bound = 4 x the error of a float32 CPU evaluation of the same rule
    on the case (the kernel orders its sums differently).  Exactly 0 where the Gaussian is culled.  Measured on an MI355X
    (rel-L2 against float64, HIP / float32 CPU, ratio): pp_outside 9.49e-8 / 9.38e-8, 1.01; behind 8.44e-8 / 8.02e-8, 1.05;
    upside_down 9.42e-8 / 9.06e-8, 1.04; pitch_roll 9.97e-8 / 9.69e-8, 1.03 (docs/LAB_NOTES.md, "Antialiased mode and absgrad
    (N16)")."""
    c = _reference(oracle, cam, 16, True, f32=False)
    bands = _census(c["comp64"], c["radii"])
    r = _run(c["s"], c["w"], c["h"], 16, mode="antialiased", grad=False)
    comp = r["info"]["compensations"]
    assert comp.shape == (1, c["n"]) and comp.dtype == torch.float32
    comp = comp[0].cpu().numpy()
    radii = r["info"]["radii"][0].cpu().numpy()
    np.testing.assert_array_equal(radii, c["radii"])
    e, y = rel_l2(comp, c["comp64"]), rel_l2(c["comp32"], c["comp64"])
    print(f"\ncompensations {cam}: census {bands}, HIP {e:.3e}, float32 CPU {y:.3e}, ratio {e / y:.2f}")
    assert e <= 4 * y
    assert np.all(comp[radii == 0] == 0) and np.all(comp[radii > 0] > 0) and np.all(comp <= 1)
    np.testing.assert_array_equal(r["info"]["opacities"][0].cpu().numpy(), c["s"]["opacities"] * comp)


# -- 2. the forward is the classic forward on compensated opacities ---------------------------------------------------------------

@pytest.mark.parametrize("cam,d", [("pp_outside", 3), ("pitch_roll", 16), ("behind", 128)])
def test_antialiased_forward_is_the_classic_forward_on_compensated_opacities(cam, d):
    s, w, h, n, seed = _scene(cam, max(d, 16))
    a = _run(s, w, h, d, mode="antialiased", grad=False)
    assert a["info"]["compensations"] is not None
    b = _run(s, w, h, d, grad=False, opacities=to_dev(s["opacities"]) * a["info"]["compensations"][0])
    assert b["info"]["compensations"] is None
    for k in ("out", "alphas"):
        assert torch.equal(a[k], b[k]), k
    for k in ("last_ids", "isect_ids", "flatten_ids", "radii", "means2d", "conics", "depths", "tiles_per_gauss", "opacities"):
        assert torch.equal(a["info"][k], b["info"][k]), k
    plain = _run(s, w, h, d, grad=False)
    assert not torch.equal(plain["out"], a["out"])
    for k in ("radii", "means2d", "conics", "depths", "tiles_per_gauss", "isect_ids", "flatten_ids"):   # the blurred covariance decides
        assert torch.equal(plain["info"][k], a["info"][k]), k


def _model_and_camera(w, h, n, d, seed, view=2):
    from gags_amd import synthetic as syn
    pc = syn.make_model(n, d, w, h, seed=seed, device="cuda", scale0=syn.SCALE0 * MULT)
    return pc, syn.make_camera(w, h, view=view, device="cuda"), scene_arrays(n, d, w, h, seed=seed, view=view, scale_mult=MULT)


def test_render_on_raw_parameters_equals_the_activated_call_bit_for_bit():
    from gags_amd.gaussian_renderer import _intrinsics, render
    from gags_amd.rasterization import rasterization
    w, h, n, d = 97, 61, 700, 16
    pc, cam, s = _model_and_camera(w, h, n, d, 31)
    bg = torch.full((3,), BG, device="cuda")
    with torch.no_grad():
        pkg = render(cam, pc, None, bg, rasterize_mode="antialiased")
        out, alphas, info = rasterization(pc.get_xyz, pc.get_rotation, pc.get_scaling, pc.get_opacity.squeeze(-1),
                                          pc.get_semantic_feature, cam.world_view_transform.transpose(0, 1)[None],
                                          _intrinsics(cam, "cuda", {})[None], w, h,
                                          backgrounds=bg[0].repeat(d)[None], rasterize_mode="antialiased")
    assert torch.equal(pkg["render"], out[0].permute(2, 0, 1)) and torch.equal(pkg["alphas"], alphas[0, ..., 0])
    for k in ("compensations", "opacities", "radii", "last_ids", "flatten_ids"):
        assert torch.equal(pkg["info"][k], info[k]), k
    comp = info["compensations"][0]
    assert int(((comp > 0) & (comp < 0.5)).sum()) >= 20 and int((comp >= 0.9).sum()) >= 20


# -- 3. gradients in antialiased mode ---------------------------------------------------------------------------------------------

def _check_f64(label, got, r64, r32, keys):
    worst = 0.0
    for k in keys:
        e, y = rel_l2(got[k].cpu().numpy(), r64[k]), rel_l2(r32[k], r64[k])
        print(f"{label} {k}: HIP {e:.3e}, float32 CPU {y:.3e}, ratio {e / y:.2f}, bound {min(F64_CAP, F64_MARGIN * y):.3e}")
        worst = max(worst, e / y)
    for k in keys:
        e, y = rel_l2(got[k].cpu().numpy(), r64[k]), rel_l2(r32[k], r64[k])
        assert e <= min(F64_CAP, F64_MARGIN * y), (label, k, e, y)
    return worst


@pytest.mark.parametrize("cam,d", [("pp_outside", 16), ("pitch_roll", 16), ("behind", 128), ("upside_down", 128), ("pp_outside", 3)])
def test_antialiased_gradients_against_float64(oracle, cam, d):
    """means, quats, scales, opacities, colours (and means2d) with a background and a non-zero v_alpha; D = 16 and 128 take the
    matrix-core geometry pass, D = 3 the VALU kernel.  Yardstick per gradient: a float32 CPU autograd run through aa_ref with
    the float64 run's blend decisions; bound min(F64_CAP, F64_MARGIN x that).  Culled rows are exactly zero.  Measured on an
    MI355X: HIP errors 2.8e-6 .. 7.7e-6, ratio HIP / yardstick 0.92 .. 1.01 over all gradients of the five cases, worst 1.01
    (docs/LAB_NOTES.md, "Antialiased mode and absgrad (N16)")."""
    c = _reference(oracle, cam, d, True)
    _census(c["comp64"], c["radii"])
    r = _run(c["s"], c["w"], c["h"], d, mode="antialiased", v=c["v"])
    print()
    assert rel_l2(r["out"].cpu().numpy(), c["r64"]["out"]) < 1e-5
    worst = _check_f64(f"{cam} D={d}", r["g"], c["r64"]["g"], c["r32"]["g"], ACT + ("means2d",))
    print(f"worst ratio {worst:.2f}")
    culled = torch.as_tensor(c["radii"] == 0, device="cuda")
    for k in ACT + ("means2d",):
        assert bool((r["g"][k][culled] == 0).all()), k


def test_antialiased_gradients_through_render_on_raw_parameters(oracle):
    """The same through render() on a GaussianModel: gradients of _xyz, _scaling, _rotation, _opacity against float64 autograd
    through the getters and aa_ref; yardstick and bound as above.  Measured: HIP 1.2e-6 .. 2.3e-6, ratios 0.97 .. 1.01."""
    from gags_amd.gaussian_renderer import render
    w, h, n, d = 97, 61, 700, 16
    pc, cam, s = _model_and_camera(w, h, n, d, 31)
    for a in ("_xyz", "_scaling", "_rotation", "_opacity", "_semantic_feature"):
        getattr(pc, a).requires_grad_(True)
    v = _cotangents(31, h, w, d)
    bgv = np.full(d, BG, np.float32)
    pkg = render(cam, pc, None, torch.full((3,), BG, device="cuda"), rasterize_mode="antialiased")
    ((pkg["render"].permute(1, 2, 0) * to_dev(v[0])).sum() + (pkg["alphas"] * to_dev(v[1])).sum()).backward()
    comp = pkg["info"]["compensations"][0].cpu().numpy()
    oi = oracle.rasterization(s["means"], s["quats"], s["scales"], s["opacities"] * comp, s["colors"], s["viewmat"], s["K"], bgv, w, h)[2]
    np.testing.assert_array_equal(oi["radii"], pkg["radii"].cpu().numpy())
    r64 = aa_ref.full(s, w, h, s["colors"], bgv, v[0], v[1], oi["radii"], oi["depths"], antialiased=True, dev="cuda", raw=True)
    assert r64["n_blend"] == oi["n_blend"]
    r32 = aa_ref.full(s, w, h, s["colors"], bgv, v[0], v[1], oi["radii"], oi["depths"], antialiased=True, dtype=torch.float32,
                      include=r64["include"].cpu(), raw=True)
    got = {a: getattr(pc, a).grad.reshape(r64["g"][a].shape) for a in ("_xyz", "_scaling", "_rotation", "_opacity")}
    print()
    worst = _check_f64("render()", got, r64["g"], r32["g"], tuple(got))
    print(f"worst ratio {worst:.2f}")
    culled = pkg["radii"] == 0
    assert int(culled.sum()) > 0
    for a, g in got.items():
        assert bool((g[culled] == 0).all()), a


# -- 4. classic mode untouched ----------------------------------------------------------------------------------------------------

def test_classic_mode_is_deterministic_and_has_no_compensations():
    s, w, h, n, seed = _scene("pitch_roll", 16)
    v = _cotangents(seed, h, w, 16)
    a, b = _run(s, w, h, 16, v=v), _run(s, w, h, 16, v=v)
    assert a["info"]["compensations"] is None and a["absgrad"] is None and not hasattr(a["info"]["means2d"], "absgrad")
    assert torch.equal(a["out"], b["out"]) and torch.equal(a["alphas"], b["alphas"])
    for k in a["g"]:
        assert torch.equal(a["g"][k], b["g"][k]), k


# -- 5. absgrad against float64 ---------------------------------------------------------------------------------------------------

def _f32mfma():
    from gags_amd import _lib
    return _lib.GAGS_BWD_F32MFMA


@functools.lru_cache(maxsize=None)
def _oracle_means2d_error(oracle, cam, d):
    """The fp32 oracle's float64 error of the SIGNED v_means2d on the case: the established yardstick of this gradient."""
    c = _reference(oracle, cam, d, False, f32=False)
    og = oracle_full(oracle, c["s"], c["w"], c["h"], c["s"]["colors"], np.full(d, BG, np.float32), c["v"][0], c["v"][1])[3]
    return rel_l2(og["means2d"], c["r64"]["g"]["means2d"]), og


@pytest.mark.parametrize("cam,d,f32mfma", [("upside_down", 3, False), ("pitch_roll", 20, False), ("pp_outside", 16, False),
                                           ("behind", 128, False), ("behind", 128, True), ("upside_down", 264, False)])
def test_absgrad_against_float64(oracle, cam, d, f32mfma):
    """D = 3 (VALU, 4-channel kernel), 20 (VALU, 32-channel kernel, one chunk), 16 and 128 (geometry pass), 128 with
    GAGS_BWD_F32MFMA, 264 (two dot passes).  Bound: min(1e-4, 3 x the oracle's float64 error of the signed v_means2d on the
    case); absgrad >= |grad| elementwise; rows of Gaussians that blended nowhere are exactly zero.  Measured on an MI355X
    (rel-L2 against float64: HIP absgrad / the oracle's signed v_means2d, ratio): D=3 1.64e-6 / 6.97e-6, 0.24; D=20 1.16e-6 /
    6.38e-6, 0.18; D=16 1.35e-6 / 6.94e-6, 0.19; D=128 1.26e-6 / 5.59e-6, 0.22 (the same with GAGS_BWD_F32MFMA); D=264 1.72e-6 /
    6.74e-6, 0.26 -- no cancellation, so well inside the signed gradient's error (docs/LAB_NOTES.md, "Antialiased mode and
    absgrad (N16)")."""
    from gags_amd import rasterization as R
    c = _reference(oracle, cam, d, False, f32=False)
    y, _ = _oracle_means2d_error(oracle, cam, d)
    r = _run(c["s"], c["w"], c["h"], d, absgrad=True, v=c["v"], flags=_f32mfma() if f32mfma else 0)
    route = R._route(c["n"], d, False, (True,) * 5, _f32mfma() if f32mfma else 0, False, absgrad=True)
    assert route.bwd == ("valu" if d in (3, 20) else "staged+geom")
    ab = r["absgrad"]
    assert ab is not None and ab.shape == (1, c["n"], 2) and ab.dtype == torch.float32
    ab = ab[0].cpu().numpy()
    e = rel_l2(ab, c["r64"]["g"]["absgrad"])
    es = rel_l2(r["g"]["means2d"].cpu().numpy(), c["r64"]["g"]["means2d"])
    print(f"\nabsgrad {cam} D={d}{' f32mfma' if f32mfma else ''}: HIP {e:.3e}, oracle (signed) {y:.3e}, ratio {e / y:.2f}; "
          f"HIP signed {es:.3e}")
    assert e <= min(1e-4, 3 * y)
    g = np.abs(r["g"]["means2d"].cpu().numpy())
    assert np.all(ab >= g - 1e-6 * ab.max())
    assert c["blended"].sum() > 50 and (~c["blended"]).sum() > 50
    assert np.all(ab[~c["blended"]] == 0) and np.all(ab[c["blended"]].sum(1) > 0)
    assert ab.sum() > g.sum()   # opposite signs cancel in the signed sum


# -- 6. absgrad changes nothing else ----------------------------------------------------------------------------------------------

def test_absgrad_changes_nothing_else_on_the_geometry_route():
    s, w, h, n, seed = _scene("pp_outside", 16)
    v = _cotangents(seed, h, w, 16)
    a, b = _run(s, w, h, 16, v=v), _run(s, w, h, 16, v=v, absgrad=True)
    assert a["absgrad"] is None and b["absgrad"] is not None
    assert torch.equal(a["out"], b["out"]) and torch.equal(a["alphas"], b["alphas"])
    assert set(a["g"]) == set(b["g"]) == set(ACT + ("means2d",))
    for k in a["g"]:
        assert torch.equal(a["g"][k], b["g"][k]), k


def test_absgrad_leaves_the_signed_gradients_of_the_valu_route_within_the_oracle_bound(oracle):
    cam, d = "upside_down", 3
    c = _reference(oracle, cam, d, False, f32=False)
    og = _oracle_means2d_error(oracle, cam, d)[1]
    r = _run(c["s"], c["w"], c["h"], d, absgrad=True, v=c["v"])
    e = {k: rel_l2(r["g"][k].cpu().numpy(), og[k]) for k in ACT + ("means2d",)}
    print("\nVALU route with absgrad, signed gradients vs the oracle:", {k: f"{x:.2e}" for k, x in e.items()})
    assert e["colors"] <= GRAD_TOL
    for k in ("opacities", "means2d", "means", "quats", "scales"):
        assert e[k] <= 1e-4, (k, e)


# -- 7. known answer --------------------------------------------------------------------------------------------------------------

def test_known_answer_one_centred_gaussian():
    """One isotropic Gaussian centred on the pixel-grid centre of a 16x16 image, D = 3, a uniform cotangent: the signed
    screen-space gradient cancels, absgrad is the float64 hand sum."""
    f, z, sig = 20.0, 4.0, 0.6
    s = dict(means=np.array([[0, 0, z]], np.float32), quats=np.array([[1, 0, 0, 0]], np.float32),
             scales=np.full((1, 3), sig, np.float32), opacities=np.array([0.8], np.float32),
             colors=np.array([[0.9, 0.2, 0.5]], np.float32), viewmat=np.eye(4, dtype=np.float32),
             K=np.array([[f, 0, 8], [0, f, 8], [0, 0, 1]], np.float32))
    v_c, v_a = np.array([0.7, -0.4, 1.1], np.float32), np.float32(0.35)
    v = (np.broadcast_to(v_c, (16, 16, 3)).copy(), np.full((16, 16), v_a, np.float32))
    r = _run(s, 16, 16, 3, absgrad=True, v=v)
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    _, _, con, _ = aa_ref.project(t(s["means"]), t(s["quats"]), t(s["scales"]), t(s["viewmat"]), t(s["K"]), 16, 16)
    _, want = hand_absgrad((8.0, 8.0), con[0].tolist(), float(s["opacities"][0]), s["colors"][0].astype(np.float64),
                           np.full(3, BG), v_c.astype(np.float64), float(v_a))
    ab, g = r["absgrad"][0, 0].cpu().numpy(), r["g"]["means2d"][0].cpu().numpy()
    print(f"\nknown answer: absgrad {ab}, hand sum {want}, signed {g}")
    assert np.all(want > 0.1)
    assert np.all(np.abs(g) <= 1e-5 * ab)
    np.testing.assert_allclose(ab, want, rtol=1e-5)


# -- 8. lifetime ------------------------------------------------------------------------------------------------------------------

def test_absgrad_is_overwritten_by_each_backward():
    from gags_amd.rasterization import rasterization
    s, w, h, n, seed = _scene("pitch_roll", 16)
    v1, v2 = _cotangents(seed, h, w, 16), _cotangents(seed + 1, h, w, 16)
    L = [to_dev(s[k]).requires_grad_(True) for k in ("means", "quats", "scales", "opacities")] + [to_dev(s["colors"]).requires_grad_(True)]
    out, alphas, info = rasterization(*L, to_dev(s["viewmat"])[None], to_dev(s["K"])[None], w, h, absgrad=True)
    m2 = info["means2d"]
    m2.retain_grad()
    assert not hasattr(m2, "absgrad")
    ((out[0] * to_dev(v1[0])).sum() + (alphas[0, ..., 0] * to_dev(v1[1])).sum()).backward(retain_graph=True)
    first, g1 = m2.absgrad.clone(), m2.grad.clone()
    ((out[0] * to_dev(v2[0])).sum() + (alphas[0, ..., 0] * to_dev(v2[1])).sum()).backward()
    fresh = _run_nobg(s, w, h, v2)
    assert torch.equal(m2.absgrad, fresh.absgrad) and not torch.equal(m2.absgrad, first)
    assert torch.equal(m2.grad, g1 + fresh.grad)   # (.grad accumulates, as autograd does; .absgrad does not)


def _run_nobg(s, w, h, v):
    from gags_amd.rasterization import rasterization
    L = [to_dev(s[k]).requires_grad_(True) for k in ("means", "quats", "scales", "opacities")] + [to_dev(s["colors"]).requires_grad_(True)]
    out, alphas, info = rasterization(*L, to_dev(s["viewmat"])[None], to_dev(s["K"])[None], w, h, absgrad=True)
    info["means2d"].retain_grad()
    ((out[0] * to_dev(v[0])).sum() + (alphas[0, ..., 0] * to_dev(v[1])).sum()).backward()
    return info["means2d"]


@pytest.mark.parametrize("d", [3, 16])
def test_absgrad_of_an_empty_view_and_of_no_gaussians(d):
    from gags_amd.rasterization import rasterization
    s, w, h, n, seed = _scene("pitch_roll", 16)
    away = s["viewmat"].copy()
    away[:3] *= -1.0   # the camera turned away: every Gaussian behind it
    for nn, vm in ((n, away), (0, s["viewmat"])):
        L = [to_dev(s[k][:nn]).requires_grad_(True) for k in ("means", "quats", "scales", "opacities")]
        L.append(to_dev(np.ascontiguousarray(s["colors"][:nn, :d])).requires_grad_(True))
        out, alphas, info = rasterization(*L, to_dev(vm)[None], to_dev(s["K"])[None], w, h, absgrad=True,
                                          rasterize_mode="antialiased", backgrounds=torch.full((1, d), BG, device="cuda"))
        assert info["n_isects"] == 0 and info["compensations"].shape == (1, nn) and not bool(info["compensations"].any())
        (out.sum() + alphas.sum()).backward()
        ab = info["means2d"].absgrad
        assert ab.shape == (1, nn, 2) and ab.dtype == torch.float32 and not bool(ab.any())
        assert all(t.grad is not None and t.grad.shape == t.shape and not bool(t.grad.any()) for t in L)


# -- 9. both options through render() and the densification statistics -------------------------------------------------------------

def test_render_with_both_options_feeds_the_densification_statistics():
    import types
    from gags_amd import densify, losses
    from gags_amd.gaussian_renderer import render
    w, h, n = 64, 48, 500
    pc, cam, _ = _model_and_camera(w, h, n, 16, 3, view=3)
    args = types.SimpleNamespace(percent_dense=0.01, position_lr_init=0.00016, position_lr_final=0.0000016,
                                 position_lr_delay_mult=0.01, position_lr_max_steps=30000, feature_lr=0.0025, opacity_lr=0.05,
                                 scaling_lr=0.005, rotation_lr=0.001, semantic_feature_lr=0.001)
    pc.training_setup_rgb(args)
    bg = torch.zeros(3, device="cuda")
    gt = torch.rand(3, h, w, device="cuda", generator=torch.Generator(device="cuda").manual_seed(11))
    pkg = render(cam, pc, None, bg, feature_mode=False, rasterize_mode="antialiased", absgrad=True)
    plain = render(cam, pc, None, bg, feature_mode=False, rasterize_mode="antialiased")
    with pytest.raises(RuntimeError, match="absgrad"):
        densify.accumulate(pc, plain, absgrad=True)
    losses.photometric_loss(pkg["render"], gt).backward()
    vp = pkg["viewspace_points"]
    assert vp.absgrad.shape == vp.grad.shape == (1, n, 2) and pkg["info"]["compensations"].shape == (1, n)
    densify.accumulate(pc, pkg, absgrad=True)
    accum, denom = pc.xyz_gradient_accum.clone(), pc.denom.clone()
    want, signed = (types.SimpleNamespace(_xyz=pc._xyz) for _ in range(2))
    densify.stats(want, vp.absgrad.clone(), pkg["radii"], None, None, w, h)
    densify.stats(signed, vp.grad.clone(), pkg["radii"], None, None, w, h)
    assert torch.equal(accum, want.xyz_gradient_accum) and torch.equal(denom, want.denom)
    assert torch.equal(denom, signed.denom) and not torch.equal(accum, signed.xyz_gradient_accum)
    assert bool((accum >= signed.xyz_gradient_accum * (1 - 1e-5)).all()) and float(accum.sum()) > float(signed.xyz_gradient_accum.sum())
    # the model's own method reads the same tensor
    twin = types.SimpleNamespace(_xyz=pc._xyz)
    type(pc).add_densification_stats(twin, vp, pkg["radii"] > 0, w, h, absgrad=True)
    assert torch.equal(twin.xyz_gradient_accum, accum)
    pc.densify_and_prune(0.0002, 0.005, 5.0, None, generator=torch.Generator(device="cuda").manual_seed(4))
    m = pc._xyz.shape[0]
    assert m != n
    for a in ("_xyz", "_scaling", "_rotation", "_opacity", "_features_dc", "_features_rest"):
        assert getattr(pc, a).shape[0] == m, a
    assert pc.xyz_gradient_accum.shape == (m, 1) and pc.denom.shape == (m, 1) and pc.max_radii2D.shape == (m,)
    for grp in pc.optimizer.param_groups:
        p = grp["params"][0]
        st = pc.optimizer.state.get(p)
        assert p.shape[0] == m and (not st or st["exp_avg"].shape == p.shape), grp["name"]
    again = render(cam, pc, None, bg, feature_mode=False, rasterize_mode="antialiased", absgrad=True)
    losses.photometric_loss(again["render"], gt).backward()
    assert again["viewspace_points"].absgrad.shape == (1, m, 2)


# -- 10. errors -------------------------------------------------------------------------------------------------------------------

def test_absgrad_at_a_width_the_valu_route_cannot_serve_raises_before_any_launch():
    from gags_amd import _lib
    s, w, h, n, seed = _scene("pitch_roll", 40)
    launched = []
    real = _lib.load

    def spy():
        launched.append(1)
        return real()
    for d in (36, 40):   # (40: the geometry pass serves it)
        _lib.load = spy
        try:
            if d == 36:
                with pytest.raises(NotImplementedError, match="absgrad"):
                    _run(s, w, h, d, absgrad=True, v=None)
                assert not launched
            else:
                assert _run(s, w, h, d, absgrad=True, v=_cotangents(seed, h, w, d))["absgrad"] is not None
        finally:
            _lib.load = real
    assert _run(s, w, h, 36, absgrad=True, grad=False)["absgrad"] is None   # no geometry gradient: nothing to refuse, nothing set
