"""HIP path under general cameras: arbitrary pose (yaw, pitch and roll, camera centre |C| up to ~10), fx != fy, principal
point off-centre and outside the image, Gaussians beyond the tangent clamp of the projection (so that the backward's clamped
branch carries gradient), non-default near / far / radius_clip / eps2d, the depth render modes with geometry gradients, SH
colours seen from far away from the origin, raw parameters and render().  Against the CPU oracle at the bounds of
tests/test_parity_gpu.py, and against float64 autograd through oracle/dense_ref.py (run on the GPU in float64) at bounds
tied to the oracle's own float64 error on the same case.  Scenes and cameras are those of tests/test_general_camera_cpu.py,
where the oracle itself is pinned to float64."""
import functools

import numpy as np
import pytest
import torch

from helpers import check_forward, clamp_census, general_camera, general_scene, rel_l2, to_dev
from test_general_camera_cpu import CULLING, depth_tie_inputs, quarter_turn_case, quarter_turn_expected
from test_parity_gpu import GRAD_TOL, _check_indices

pytestmark = pytest.mark.gpu

MULT = 30.0      # splat size at which >= 20 visible Gaussians sit beyond the clamp in x and in y (asserted per case)
GEOM = ("opacities", "means2d", "means", "quats", "scales")


def _gpu(s, w, h, colors, bg, *, need_geom=False, v_out=None, v_alpha=None, render_mode="RGB", sh_degree=None, flags=0,
         grad=True, **cull):
    """rasterization() on the scene's arrays; returns (out [H,W,D'], alpha [H,W], info, gradients or None).  (test_parity_gpu's
    _run_gpu passes no culling parameters and cannot run without grad, which the depth and culling tests here need.)"""
    from gags_amd.rasterization import rasterization
    L = dict(means=to_dev(s["means"]), quats=to_dev(s["quats"]), scales=to_dev(s["scales"]), opacities=to_dev(s["opacities"]),
             colors=to_dev(colors))
    if grad:
        for k, t in L.items():
            t.requires_grad_(k == "colors" or need_geom)
    with torch.set_grad_enabled(grad):
        out, alphas, info = rasterization(L["means"], L["quats"], L["scales"], L["opacities"], L["colors"],
                                          to_dev(s["viewmat"])[None], to_dev(s["K"])[None], w, h,
                                          backgrounds=None if bg is None else to_dev(bg)[None], sh_degree=sh_degree,
                                          render_mode=render_mode, raster_flags=flags, **cull)
    grads = None
    if v_out is not None:
        loss = (out[0] * to_dev(v_out)).sum()
        if v_alpha is not None:
            loss = loss + (alphas[0, ..., 0] * to_dev(v_alpha)).sum()
        if need_geom:
            info["means2d"].retain_grad()
        loss.backward()
        grads = {k: t.grad.cpu().numpy() for k, t in L.items() if t.grad is not None}
        if need_geom:
            grads["means2d"] = info["means2d"].grad[0].cpu().numpy()
    torch.cuda.synchronize()
    return out[0].detach().cpu().numpy(), alphas[0, ..., 0].detach().cpu().numpy(), info, grads


def _exact(s, w, h, colors, bg, **kw):
    """The render through GAGS_FWD_EXACT where the default forward is the 16-bit matrix-core one (D >= 128), else None."""
    from gags_amd import _lib
    if colors.shape[-1] < 128:
        return None
    return _gpu(s, w, h, colors, bg, flags=_lib.GAGS_FWD_EXACT, grad=False, **kw)[0]


def _scene(cam, w, h, n, d, seed):
    return general_scene(n, d, w, h, seed, scale_mult=MULT, **general_camera(cam, w, h))


def _cotangents(seed, h, w, d):
    rng = np.random.default_rng(seed + 100)
    return rng.standard_normal((h, w, d)).astype(np.float32), rng.standard_normal((h, w)).astype(np.float32)


def oracle_full(oracle, s, w, h, colors, bg, v_out, v_alpha, render_mode="RGB", sh_degree=None, **cull):
    """Oracle forward and every gradient.  Depth modes: the depth channel's colour gradient is v_depths of project_bwd; the
    ED division out = acc / max(alpha, 1e-10) is differentiated by hand in front of raster_bwd."""
    okw = dict(eps2d=cull.get("eps2d", 0.3), near=cull.get("near_plane", 0.01), far=cull.get("far_plane", 1e10),
               radius_clip=cull.get("radius_clip", 0.0))
    out, alpha, oi = oracle.rasterization(s["means"], s["quats"], s["scales"], s["opacities"], colors, s["viewmat"], s["K"], bg,
                                          w, h, render_mode=render_mode, sh_degree=sh_degree, **okw)
    v_o, v_a = v_out.copy(), v_alpha.copy()
    if render_mode in ("ED", "RGB+ED"):
        den = np.maximum(alpha, np.float32(1e-10))
        v_ed = v_out[..., -1]
        v_o[..., -1] = v_ed / den
        v_a = v_a + np.where(alpha > 1e-10, -v_ed * out[..., -1] / den, 0.0).astype(np.float32)   # out_ed = acc / alpha
    vc, vo, vm2, vcon = oracle.raster_bwd(oi["means2d"], oi["conics"], s["opacities"], oi["colors"], oi["backgrounds"], w, h,
                                          oi["isect_offsets"], oi["flatten_ids"], alpha, oi["last_ids"], v_o, v_a)
    depth = render_mode != "RGB"
    vM, vQ, vS = oracle.project_bwd(s["means"], s["quats"], s["scales"], s["viewmat"], s["K"], w, h, oi["radii"], vm2,
                                    vc[:, -1].copy() if depth else None, vcon, eps2d=okw["eps2d"])
    g = dict(opacities=vo, means2d=vm2, means=vM, quats=vQ, scales=vS)
    if render_mode in ("RGB", "RGB+D", "RGB+ED") and sh_degree is None:
        g["colors"] = vc[:, :colors.shape[1]]
    return out, alpha, oi, g


def dense_full(s, w, h, colors, bg, v_out, v_alpha, oi, render_mode="RGB", sh_degree=None, eps2d=0.3, dev="cuda"):
    """float64 autograd through dense_ref on the same scene (integer decisions -- radii, depth order -- from the oracle):
    every gradient, the view-direction term of the SH colours and the ED division (stated in float64) included."""
    from oracle import dense_ref as dr

    def tm(a, rg=False):
        return torch.tensor(np.asarray(a), dtype=torch.float64, device=dev, requires_grad=rg)

    n = s["means"].shape[0]
    M, Q, S, O, C = tm(s["means"], True), tm(s["quats"], True), tm(s["scales"], True), tm(s["opacities"], True), tm(colors, True)
    vm = tm(s["viewmat"])
    m2, z, con = dr.project(M, Q, S, vm, tm(s["K"]), w, h, eps2d=eps2d)
    m2.retain_grad()
    cols = dr.sh_colors(sh_degree, C, M, torch.inverse(vm)[:3, 3]) if sh_degree is not None else C
    bgt = None if bg is None else tm(bg)
    if render_mode in ("RGB+D", "RGB+ED"):
        cols = torch.cat([cols, z[:, None]], dim=1)
        bgt = None if bgt is None else torch.cat([bgt, torch.zeros(1, dtype=torch.float64, device=dev)])
    elif render_mode in ("D", "ED"):
        cols = z[:, None]
        bgt = None if bgt is None else torch.zeros(1, dtype=torch.float64, device=dev)
    order = np.lexsort((np.arange(n), oi["depths"]))
    o2, a2, _, ninc = dr.composite(m2, con, O, cols, bgt, w, h, oi["radii"], order)
    assert ninc == oi["n_blend"], (ninc, oi["n_blend"])
    if render_mode in ("ED", "RGB+ED"):
        o2 = torch.cat([o2[..., :-1], o2[..., -1:] / a2[..., None].clamp(min=1e-10)], dim=-1)
    ((o2 * tm(v_out)).sum() + (a2 * tm(v_alpha)).sum()).backward()
    g = dict(opacities=O.grad, means2d=m2.grad, means=M.grad, quats=Q.grad, scales=S.grad)
    if C.grad is not None:
        g["colors"] = C.grad
    return o2.detach().cpu().numpy(), {k: v.cpu().numpy() for k, v in g.items()}


def _assert_clamp_census(s, w, h, radii):
    nx, ny, nvis, ncull = clamp_census(s, w, h, radii)
    assert nx >= 20 and ny >= 20 and nvis > 0 and ncull > 0, (nx, ny, nvis, ncull)


# -- forward and colour gradient ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cam,w,h,n,d,seed,bgv", [
    ("pitch_roll", 97, 61, 1500, 3, 0, 1.0),       # ragged image, VALU width
    ("behind", 130, 100, 1500, 16, 1, 0.0),        # narrowest matrix-core width
    ("pp_outside", 150, 110, 1500, 48, 2, 0.4),    # principal point outside the image; ragged last slice
    ("upside_down", 97, 61, 1200, 128, 3, None),   # one 128-channel slice, ragged image, no background
    ("pitch_roll", 176, 130, 2000, 256, 4, 0.3),   # two 128-channel slices
])
def test_forward_and_colour_grad(oracle, cam, w, h, n, d, seed, bgv):
    s = _scene(cam, w, h, n, d, seed)
    bg = None if bgv is None else np.full(d, bgv, np.float32)
    v_out, _ = _cotangents(seed, h, w, d)
    o_out, o_alpha, oinfo = oracle.rasterization(s["means"], s["quats"], s["scales"], s["opacities"], s["colors"],
                                                 s["viewmat"], s["K"], bg, w, h)
    _assert_clamp_census(s, w, h, oinfo["radii"])
    out, alpha, info, grads = _gpu(s, w, h, s["colors"], bg, v_out=v_out)
    _check_indices(info, oinfo)
    np.testing.assert_array_equal(alpha, o_alpha)
    check_forward(out, o_out, _exact(s, w, h, s["colors"], bg))
    o_vc, _, _, _ = oracle.raster_bwd(oinfo["means2d"], oinfo["conics"], s["opacities"], s["colors"], bg, w, h,
                                      oinfo["isect_offsets"], oinfo["flatten_ids"], o_alpha, oinfo["last_ids"],
                                      v_out, None, colors_only=True)
    o_vf = oracle.raster_bwd_colors_fwdorder(oinfo["means2d"], oinfo["conics"], s["opacities"], d, w, h,
                                             oinfo["isect_offsets"], oinfo["flatten_ids"], v_out, n)
    e = min(rel_l2(grads["colors"], o_vc), rel_l2(grads["colors"], o_vf))   # as tests/test_parity_gpu.py: either order of T
    print(f"colour gradient vs the oracle: {e:.2e}")
    assert e <= GRAD_TOL
    assert np.all(grads["colors"][oinfo["radii"] == 0] == 0)


# -- full backward: against the oracle and against float64 ---------------------------------------------------------------------

FULL_CASES = [("pp_outside", 97, 61, 700, 16, 21), ("behind", 104, 72, 700, 128, 122),
              ("upside_down", 97, 61, 700, 128, 23), ("pitch_roll", 104, 72, 700, 16, 124)]


@functools.lru_cache(maxsize=None)
def _full_case(oracle, cam, w, h, n, d, seed, render_mode="RGB", sh_degree=None):
    """One scene through the GPU, the oracle and float64, computed once for the tests that share it."""
    s = _scene(cam, w, h, n, 3 if render_mode != "RGB" or sh_degree is not None else d, seed)
    colors = s["sh"] if sh_degree is not None else s["colors"]
    d0 = 3 if sh_degree is not None else colors.shape[1]
    bg = np.full(d0, 0.25, np.float32)
    d_out = {"RGB": d0, "RGB+D": d0 + 1, "RGB+ED": d0 + 1, "D": 1, "ED": 1}[render_mode]
    v_out, v_alpha = _cotangents(seed, h, w, d_out)
    out, alpha, info, g = _gpu(s, w, h, colors, bg, need_geom=True, v_out=v_out, v_alpha=v_alpha, render_mode=render_mode,
                               sh_degree=sh_degree)
    o_out, o_alpha, oi, og = oracle_full(oracle, s, w, h, colors, bg, v_out, v_alpha, render_mode=render_mode,
                                         sh_degree=sh_degree)
    r_out, rg = dense_full(s, w, h, colors, bg, v_out, v_alpha, oi, render_mode=render_mode, sh_degree=sh_degree)
    return dict(s=s, colors=colors, bg=bg, out=out, alpha=alpha, info=info, g=g, o_out=o_out, o_alpha=o_alpha, oi=oi, og=og,
                r_out=r_out, rg=rg)


@pytest.mark.parametrize("cam,w,h,n,d,seed", FULL_CASES)
def test_full_backward_against_the_oracle(oracle, cam, w, h, n, d, seed):
    """Every gradient at the bounds of tests/test_parity_gpu.py::test_full_backward, on both geometry routes (D = 16: VALU,
    D = 128: matrix cores), with >= 20 visible Gaussians beyond the clamp in x and in y."""
    c = _full_case(oracle, cam, w, h, n, d, seed)
    _assert_clamp_census(c["s"], w, h, c["oi"]["radii"])
    _check_indices(c["info"], c["oi"])
    np.testing.assert_array_equal(c["alpha"], c["o_alpha"])
    check_forward(c["out"], c["o_out"], _exact(c["s"], w, h, c["colors"], c["bg"]))
    e = {k: rel_l2(c["g"][k], c["og"][k]) for k in ("colors",) + GEOM}
    print("vs the oracle:", {k: f"{v:.2e}" for k, v in e.items()})
    assert e["colors"] <= GRAD_TOL
    for k in GEOM:
        assert e[k] <= 1e-4, (k, e)
    culled = c["oi"]["radii"] == 0
    for k in ("colors",) + GEOM:
        assert np.all(c["g"][k][culled] == 0), k


# Margin of the float64 bounds below: the kernels sum in another order than the oracle, so their float64 error is not the
# oracle's.  Measured on an MI355X, HIP error / oracle error per gradient: 0.15-1.04 on the full-backward cases (the matrix-core
# route and the forward-order weights are mostly closer to float64 than the oracle's back-to-front T), 0.97-1.02 on the depth
# cases; margin = 3 x the worst ratio.  The resulting bounds are 4e-6 .. 1.9e-5.
F64_MARGIN = 3.0
F64_CAP = 1e-4   # what the project already allows against the oracle: never exceeded


def _check_against_float64(c, keys, label):
    e = {k: rel_l2(c["g"][k], c["rg"][k]) for k in keys}
    eo = {k: rel_l2(c["og"][k], c["rg"][k]) for k in keys if k in c["og"]}
    print(f"{label} vs float64: HIP", {k: f"{v:.2e}" for k, v in e.items()}, "oracle", {k: f"{v:.2e}" for k, v in eo.items()},
          "ratio", {k: f"{e[k] / eo[k]:.2f}" for k in eo})
    for k in keys:
        if k in eo:
            assert e[k] <= min(F64_CAP, F64_MARGIN * eo[k]), (k, e[k], eo[k])
    return e, eo


@pytest.mark.parametrize("cam,w,h,n,d,seed", FULL_CASES)
def test_full_backward_against_float64(oracle, cam, w, h, n, d, seed):
    """The same cases against float64 autograd through dense_ref.  Bound per gradient: the oracle's own float64 error on the
    case times F64_MARGIN, never above 1e-4.  Measured (rel-L2 against float64, HIP / oracle; worst gradient of each case):
    pp_outside D=16 4.1e-6 / 4.4e-6, behind D=128 3.5e-6 / 3.7e-6, upside_down D=128 4.0e-6 / 4.1e-6, pitch_roll D=16
    2.8e-6 / 6.3e-6; worst ratio over all gradients 1.04 (v_quats, pp_outside)."""
    c = _full_case(oracle, cam, w, h, n, d, seed)
    assert rel_l2(c["o_out"], c["r_out"]) < 1e-5
    _check_against_float64(c, ("colors",) + GEOM, f"{cam} D={d}")


# -- depth --------------------------------------------------------------------------------------------------------------------

DEPTH_CASES = [("pitch_roll", 97, 61, 700, 31, "RGB+D"), ("behind", 104, 72, 700, 232, "RGB+ED"),
               ("pp_outside", 97, 61, 700, 33, "D"), ("upside_down", 104, 72, 700, 34, "ED")]


@pytest.mark.parametrize("cam,w,h,n,seed,mode", DEPTH_CASES)
def test_depth_modes_values_and_geometry_gradients(oracle, cam, w, h, n, seed, mode):
    """The depth render modes with every geometry leaf requiring grad (v_depths -> project_bwd -> v_means): colour channels
    and the accumulated depth bit-exact against the oracle, the expected depth at rtol 1e-6, and the means / quaternion /
    scale / opacity gradients against float64 autograd through dense_ref with the ED division stated in float64.  The
    no-grad route (gags_ed_normalize in place) against the autograd route: one fp32 division each.
    Measured (rel-L2 against float64, HIP / oracle; worst gradient of each case): RGB+D 5.6e-6 / 5.6e-6, RGB+ED 2.2e-6 / 2.2e-6,
    D 4.5e-6 / 4.4e-6, ED 2.7e-6 / 2.7e-6; worst ratio 1.02.  Bound: the oracle's error times F64_MARGIN, at most 1e-4."""
    c = _full_case(oracle, cam, w, h, n, 3, seed, render_mode=mode)
    _assert_clamp_census(c["s"], w, h, c["oi"]["radii"])
    _check_indices(c["info"], c["oi"])
    out, o_out = c["out"], c["o_out"]
    assert out.shape == o_out.shape == (h, w, {"RGB+D": 4, "RGB+ED": 4, "D": 1, "ED": 1}[mode])
    np.testing.assert_array_equal(out[..., :-1], o_out[..., :-1])
    if mode in ("RGB+D", "D"):
        np.testing.assert_array_equal(out[..., -1], o_out[..., -1])
    else:
        np.testing.assert_allclose(out[..., -1], o_out[..., -1], rtol=1e-6, atol=0)
    assert np.abs(out[..., -1]).max() > 1.0                       # depths of 2..12 were rendered
    nograd = _gpu(c["s"], w, h, c["colors"], c["bg"], render_mode=mode, grad=False)[0]
    np.testing.assert_array_equal(nograd[..., :-1], out[..., :-1])
    np.testing.assert_allclose(nograd[..., -1], out[..., -1], rtol=1e-6, atol=0)
    assert np.linalg.norm(c["g"]["means"]) > 0
    _check_against_float64(c, ("means", "quats", "scales", "opacities"), f"{cam} {mode}")
    culled = c["oi"]["radii"] == 0
    for k in ("means", "quats", "scales", "opacities"):
        assert np.all(c["g"][k][culled] == 0), k


# -- SH -----------------------------------------------------------------------------------------------------------------------

# Measured on an MI355X against float64: v_means 2.3e-6 / 1.7e-6 / 2.5e-6, v_coeffs 2.1e-6 / 1.2e-6 / 1.6e-6 on the three cases
# below; bound = 3 x the worst, below the 1e-4 the project allows against the oracle.
SH_TOL = 8e-6


@pytest.mark.parametrize("cam,w,h,n,seed,deg", [("pitch_roll", 97, 61, 700, 741, 3), ("behind", 104, 72, 700, 142, 1),
                                                ("pp_outside", 97, 61, 700, 43, 3)])
def test_sh_gradients_with_the_camera_far_from_the_origin(oracle, cam, w, h, n, seed, deg):
    """sh_degree with means requiring grad and campos = inverse(viewmat)[:3, 3] at |C| > 7: the full means gradient
    (projection term plus view-direction term) and the coefficient gradient against float64 autograd through
    dense_ref.sh_colors -> dense_ref.composite.  Measured: see SH_TOL; the direction term is 4.6 %, 1.3 % and 4.7 % of the means
    gradient on the three cases, 6000, 2000 and 6000 times the bound."""
    c = _full_case(oracle, cam, w, h, n, 3, seed, sh_degree=deg)
    s = c["s"]
    assert np.linalg.norm(np.linalg.inv(s["viewmat"].astype(np.float64))[:3, 3]) > 7.0
    np.testing.assert_array_equal(c["alpha"], c["o_alpha"])
    assert rel_l2(c["out"], c["o_out"]) <= 1e-6                  # as tests/test_parity_gpu.py::test_render_modes_and_sh
    assert rel_l2(c["out"], c["r_out"]) <= 1e-5
    # the direction term is a visible share of the means gradient: the projection term alone (the oracle's v_means) misses it
    share = rel_l2(c["og"]["means"], c["rg"]["means"])
    e_m, e_c = rel_l2(c["g"]["means"], c["rg"]["means"]), rel_l2(c["g"]["colors"], c["rg"]["colors"])
    print(f"{cam} SH degree {deg} vs float64: v_means {e_m:.2e} (direction term is {share:.1%} of it), v_coeffs {e_c:.2e}")
    assert share > 1e-3
    assert e_m <= SH_TOL and e_c <= SH_TOL
    k_used = (deg + 1) ** 2
    assert np.all(c["g"]["colors"][:, k_used:] == 0) and np.abs(c["g"]["colors"][:, :k_used]).max() > 0


# -- culling parameters -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case,d", list(zip(CULLING, (16, 128, 3, 128))), ids=lambda v: v[0] if isinstance(v, tuple) else str(v))
def test_non_default_culling_parameters(oracle, case, d):
    """near_plane / far_plane / radius_clip / eps2d (eps2d = 0 included) through rasterization(): indices and forward
    bit-exact against the oracle, gradients inside the oracle bounds, culled Gaussians exactly zero in every gradient."""
    cam, seed, eps2d, near, far, clip = case
    w, h, n = 97, 61, 700
    cull = dict(near_plane=near, far_plane=far, radius_clip=clip, eps2d=eps2d)
    s = _scene(cam, w, h, n, d, seed)
    bg = np.full(d, 0.25, np.float32)
    v_out, v_alpha = _cotangents(seed, h, w, d)
    o_out, o_alpha, oi, og = oracle_full(oracle, s, w, h, s["colors"], bg, v_out, v_alpha, **cull)
    _, _, oi_default = oracle.rasterization(s["means"], s["quats"], s["scales"], s["opacities"], s["colors"], s["viewmat"],
                                            s["K"], bg, w, h)
    vis = oi["radii"] > 0
    assert vis.sum() >= 50 and (~vis).sum() >= 50
    assert not np.array_equal(oi["conics"], oi_default["conics"]) or not np.array_equal(oi["radii"], oi_default["radii"])
    out, alpha, info, g = _gpu(s, w, h, s["colors"], bg, need_geom=True, v_out=v_out, v_alpha=v_alpha, **cull)
    _check_indices(info, oi)
    np.testing.assert_array_equal(alpha, o_alpha)
    check_forward(out, o_out, _exact(s, w, h, s["colors"], bg, **cull))
    e = {k: rel_l2(g[k], og[k]) for k in ("colors",) + GEOM}
    print("vs the oracle:", {k: f"{v:.2e}" for k, v in e.items()})
    assert e["colors"] <= GRAD_TOL
    for k in GEOM:
        assert e[k] <= 1e-4, (k, e)
    for k in ("colors",) + GEOM:
        assert np.all(g[k][~vis] == 0), k


def test_depth_ties_and_quarter_turn_known_answers():
    """The hand-worked cases of tests/test_general_camera_cpu.py on the GPU: z == near and z == far are kept, one ulp outside
    is culled; a Gaussian seen through exact quarter turns with a dyadic translation lands where it must."""
    from gags_amd.rasterization import rasterization
    means, vm, near, far, want = depth_tie_inputs()
    n = len(means)
    K = np.array([[40, 0, 16], [0, 40, 16], [0, 0, 1]], np.float32)
    args = (to_dev(means), to_dev(np.array([[1, 0, 0, 0]] * n, np.float32)), to_dev(np.full((n, 3), 0.05, np.float32)),
            to_dev(np.full(n, 0.5, np.float32)), to_dev(np.ones((n, 1), np.float32)), to_dev(vm)[None], to_dev(K)[None], 32, 32)
    _, _, info = rasterization(*args, near_plane=near, far_plane=far)
    assert (info["radii"][0] > 0).tolist() == want
    assert info["depths"][0].tolist() == [near, far, 0.0, 0.0]
    _, _, info = rasterization(*args)
    assert bool((info["radii"][0] > 0).all())
    for axis in "xyz":
        (mean, quat, scale, vm, K, w, h), pc, var, pix = quarter_turn_case(axis)
        _, _, info = rasterization(to_dev(mean), to_dev(quat), to_dev(scale), to_dev(np.array([0.5], np.float32)),
                                   to_dev(np.ones((1, 1), np.float32)), to_dev(vm)[None], to_dev(K)[None], w, h)
        _, want_z, want_con = quarter_turn_expected(pc, var)
        assert int(info["radii"][0, 0]) > 0 and float(info["depths"][0, 0]) == want_z
        assert tuple(info["means2d"][0, 0].tolist()) == pix
        np.testing.assert_allclose(info["conics"][0, 0].cpu().numpy(), want_con, rtol=2e-6, atol=1e-9)


# -- raw parameters -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("modifier,cam", [(1.0, "pp_outside"), (0.7, "behind")])
def test_raw_parameters_under_a_general_camera(oracle, modifier, cam):
    """raw_params=True (gags_project_fwd_raw / gags_project_bwd_raw) under a general camera: every output that
    test_raw_parameter_projection_is_bit_identical_to_the_getters compares is bit-identical to the activated-parameter call
    (and to the oracle), and the gradients of the STORED parameters agree with autograd through torch's getters as in
    test_raw_parameter_projection_gradients_match_autograd_through_the_getters."""
    from gags_amd import _lib
    from gags_amd.rasterization import _Project, _ProjectRaw, rasterization
    w, h, n, d = 150, 110, 2000, 32
    s = _scene(cam, w, h, n, d, 51)
    p = s["raw"]
    vm, Kd = to_dev(s["viewmat"]), to_dev(s["K"])
    xyz, rot, slog, logit = (p[k].cuda() for k in ("xyz", "rotation", "scaling_log", "opacity_logit"))
    q_act, s_act, o_act = torch.nn.functional.normalize(rot), torch.exp(slog) * modifier, torch.sigmoid(logit)
    cfg = (w, h, 0.3, 0.01, 1e10, 0.0)
    want = _Project.apply(xyz, q_act, s_act, vm, Kd, *cfg)
    got = _ProjectRaw.apply(xyz, rot, slog, logit, vm, Kd, *cfg, modifier, True)
    for a, b, name in zip(got[:5], want, ("radii", "means2d", "depths", "conics", "tiles_per_gauss")):
        assert torch.equal(a, b), name
    assert torch.equal(got[5], o_act.reshape(-1))
    rec = torch.zeros(n, 8, device="cuda")
    _lib.check(_lib.load().gags_pack_isects(n, 1, _lib.ptr(torch.zeros(1, dtype=torch.int32, device="cuda")), _lib.ptr(want[1]),
                                            _lib.ptr(want[3]), _lib.ptr(o_act.reshape(-1).contiguous()), _lib.ptr(want[0]),
                                            _lib.ptr(rec), None, None), "gags_pack_isects")
    vis = want[0] > 0
    assert torch.equal(got[6][vis], rec[vis])
    o_radii, o_m2d, o_depths, o_conics = oracle.project_fwd(xyz.cpu().numpy(), q_act.cpu().numpy(), s_act.cpu().numpy(),
                                                            s["viewmat"], s["K"], w, h)
    _assert_clamp_census(s, w, h, o_radii)
    np.testing.assert_array_equal(got[0].cpu().numpy(), o_radii)
    np.testing.assert_array_equal(got[1].cpu().numpy(), o_m2d)
    np.testing.assert_array_equal(got[2].cpu().numpy(), o_depths)
    np.testing.assert_array_equal(got[3].cpu().numpy(), o_conics)
    # gradients of the stored parameters: kernels' own getter backward against torch's
    bg = to_dev(np.full(d, 0.5, np.float32))[None]
    v_out, v_alpha = _cotangents(51, h, w, d)
    res = {}
    for raw in (True, False):
        L = [t.detach().clone().requires_grad_(True) for t in (xyz, rot, slog, logit)]
        feats = p["semantic_feature"].cuda().requires_grad_(True)
        if raw:
            a = (L[0], L[1], L[2], L[3])
        else:
            a = (L[0], torch.nn.functional.normalize(L[1]), torch.exp(L[2]) * modifier, torch.sigmoid(L[3]).squeeze(-1))
        out, alphas, info = rasterization(*a, feats, vm[None], Kd[None], w, h, backgrounds=bg, raw_params=raw,
                                          scaling_modifier=modifier if raw else 1.0)
        info["means2d"].retain_grad()
        ((out[0] * to_dev(v_out)).sum() + (alphas[0, ..., 0] * to_dev(v_alpha)).sum()).backward()
        res[raw] = (out.detach().clone(), feats.grad.clone(), [t.grad.clone() for t in L], info["means2d"].grad.clone())
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])
    assert torch.equal(res[True][3], res[False][3])
    for a, b, name in zip(res[True][2], res[False][2], ("xyz", "rotation", "scaling", "opacity")):
        assert a.shape == b.shape and float(b.abs().max()) > 0, name
        assert rel_l2(a.cpu().numpy(), b.cpu().numpy()) <= 1e-6, name


# -- render() -----------------------------------------------------------------------------------------------------------------

def test_render_with_a_camera_built_from_a_general_pose(oracle):
    """gaussian_renderer.render() with a scene.Camera built from a general R, T (pitch and roll non-zero, T non-zero, fx != fy):
    the render and the feature gradient against the oracle fed with syn.camera_matrices(cam)."""
    from gags_amd import synthetic as syn
    from gags_amd.gaussian_renderer import render
    from gags_amd.scene import Camera, GaussianModel, focal2fov
    w, h, n, d = 130, 100, 1500, 16
    k = dict(general_camera("upside_down", w, h), cx=0.5 * w, cy=0.5 * h)     # (a Camera has its principal point in the middle)
    s = general_scene(n, d, w, h, 61, scale_mult=MULT, **k)
    R, C = s["R"], s["C"]
    T = -R.T @ C
    assert np.abs(T).min() > 0.1 and min(abs(a) for a in k["ypr"][1:]) > 0.1
    cam = Camera(R, T, focal2fov(k["fx"], w), focal2fov(k["fy"], h), w, h, device="cuda")
    vm, K = syn.camera_matrices(cam)
    assert np.abs(vm.cpu().numpy() - s["viewmat"]).max() < 1e-5 and abs(K[0, 0] - k["fx"]) < 1e-3 and abs(K[1, 1] - k["fy"]) < 1e-3
    p = {key: (v.cuda() if torch.is_tensor(v) else v) for key, v in s["raw"].items()}
    pc = GaussianModel.from_tensors(p["xyz"], p["scaling_log"], p["rotation"], p["opacity_logit"], p["features_dc"],
                                    p["features_rest"], p["semantic_feature"])
    pc.training_setup()
    bg = torch.tensor([1.0, 1.0, 1.0], device="cuda")
    pkg = render(cam, pc, None, bg, feature_mode=True)
    G = syn.make_cotangent(d, h, w, seed=1).cuda()
    (pkg["render"] * G).sum().backward()
    o_out, o_alpha, oinfo = oracle.rasterization(
        pc.get_xyz.detach().cpu().numpy(), pc.get_rotation.detach().cpu().numpy(),
        pc.get_scaling.detach().cpu().numpy(), pc.get_opacity.detach().cpu().numpy().reshape(-1),
        pc.get_semantic_feature.detach().cpu().numpy(), vm.cpu().numpy(), K, np.ones(d, np.float32), w, h)
    _assert_clamp_census(dict(s, viewmat=vm.cpu().numpy(), K=K), w, h, oinfo["radii"])
    np.testing.assert_array_equal(pkg["radii"].cpu().numpy(), oinfo["radii"])
    _check_indices(pkg["info"], oinfo)
    np.testing.assert_array_equal(pkg["alphas"].detach().cpu().numpy(), o_alpha)
    np.testing.assert_array_equal(pkg["render"].permute(1, 2, 0).detach().cpu().numpy(), o_out)
    o_vc, _, _, _ = oracle.raster_bwd(oinfo["means2d"], oinfo["conics"], oinfo["opacities"], oinfo["colors"],
                                      np.ones(d, np.float32), w, h, oinfo["isect_offsets"], oinfo["flatten_ids"],
                                      o_alpha, oinfo["last_ids"], G.permute(1, 2, 0).cpu().numpy(), None, colors_only=True)
    o_vf = oracle.raster_bwd_colors_fwdorder(oinfo["means2d"], oinfo["conics"], oinfo["opacities"], d, w, h,
                                             oinfo["isect_offsets"], oinfo["flatten_ids"], G.permute(1, 2, 0).cpu().numpy(), n)
    g = pc._semantic_feature.grad.cpu().numpy()
    assert min(rel_l2(g, o_vc), rel_l2(g, o_vf)) <= GRAD_TOL
