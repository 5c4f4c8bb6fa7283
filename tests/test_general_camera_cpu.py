"""CPU tests of the oracle under general cameras: arbitrary pose (yaw, pitch and roll, camera centre away from the origin),
fx != fy, principal point off-centre and outside the image, Gaussians beyond the tangent clamp of the projection, and
non-default culling parameters.  The oracle (oracle/gags_oracle.c) against the dense float64 autograd restatement
(oracle/dense_ref.py) at the bounds of tests/test_oracle_cpu.py::test_oracle_matches_dense_float64, plus known answers
that follow by hand.  Every case asserts that its inputs still exercise the edge it is there for."""
import math

import numpy as np
import pytest
import torch

from helpers import clamp_census, general_camera, general_scene, rel_l2

# name of GENERAL_CAMERAS, W, H, N, D, seed, scale_mult
CASES = [
    ("pitch_roll", 64, 48, 700, 5, 40, 30.0),
    ("behind", 72, 40, 700, 16, 61, 30.0),
    ("pp_outside", 64, 48, 700, 1, 2, 30.0),   # principal point left of the image (cx = -0.15 W), spread 1.9
    ("upside_down", 72, 40, 700, 3, 3, 30.0),
]


def tm(a, rg=False):
    return torch.tensor(np.asarray(a), dtype=torch.float64, requires_grad=rg)


def check_scene_exercises_the_clamp(s, w, h, radii):
    nx, ny, nvis, ncull = clamp_census(s, w, h, radii)
    assert nx >= 20 and ny >= 20, (nx, ny)
    assert nvis > 0 and ncull > 0, (nvis, ncull)
    return nx, ny, nvis, ncull


def oracle_and_dense(oracle, s, w, h, seed, render_mode="RGB", eps2d=0.3, near=0.01, far=1e10, radius_clip=0.0, colors=None,
                     sh_degree=None):
    """The oracle's forward and full backward next to float64 autograd through dense_ref on one scene.  Returns
    (errors dict, oracle info, visible mask).  RGB+D / D put the depth channel into the dense colours as cat(colours, z);
    v_depths is the last column of the oracle's colour gradient."""
    from oracle import dense_ref as dr
    n = s["means"].shape[0]
    colors = s["colors"] if colors is None else colors
    d0 = 3 if sh_degree is not None else colors.shape[1]
    bg = np.full(d0, 0.3, np.float32)
    out, alphas, info = oracle.rasterization(s["means"], s["quats"], s["scales"], s["opacities"], colors, s["viewmat"], s["K"],
                                             bg, w, h, render_mode=render_mode, sh_degree=sh_degree, eps2d=eps2d, near=near,
                                             far=far, radius_clip=radius_clip)
    d = out.shape[-1]
    rng = np.random.default_rng(seed)
    v_out = rng.standard_normal((h, w, d)).astype(np.float32)
    v_a = rng.standard_normal((h, w)).astype(np.float32)
    vc, vo, vm2, vcon = oracle.raster_bwd(info["means2d"], info["conics"], s["opacities"], info["colors"], info["backgrounds"],
                                          w, h, info["isect_offsets"], info["flatten_ids"], alphas, info["last_ids"], v_out, v_a)
    depth = render_mode in ("RGB+D", "D")
    v_depths = vc[:, -1].copy() if depth else None
    vM, vQ, vS = oracle.project_bwd(s["means"], s["quats"], s["scales"], s["viewmat"], s["K"], w, h, info["radii"], vm2,
                                    v_depths, vcon, eps2d=eps2d)

    M, Q, S, O = tm(s["means"], True), tm(s["quats"], True), tm(s["scales"], True), tm(s["opacities"], True)
    C = tm(colors, True)
    m2, z, con = dr.project(M, Q, S, tm(s["viewmat"]), tm(s["K"]), w, h, eps2d=eps2d)
    m2.retain_grad(); con.retain_grad()
    if sh_degree is not None:
        campos = torch.inverse(tm(s["viewmat"]))[:3, 3]
        cols = dr.sh_colors(sh_degree, C, M.detach(), campos)
    else:
        cols = C
    if render_mode == "RGB+D":
        cols = torch.cat([cols, z[:, None]], dim=1)
    elif render_mode == "D":
        cols = z[:, None]
    order = np.lexsort((np.arange(n), info["depths"]))
    o2, a2, last2, ninc = dr.composite(m2, con, O, cols, tm(info["backgrounds"]), w, h, info["radii"], order)
    vis = info["radii"] > 0
    e = dict(means2d_abs=float(np.abs(m2.detach().numpy()[vis] - info["means2d"][vis]).max()),
             conics=rel_l2(info["conics"][vis], con.detach().numpy()[vis]),
             depths=rel_l2(info["depths"][vis], z.detach().numpy()[vis]),
             ninc=(ninc, info["n_blend"]),
             render=rel_l2(out, o2.detach().numpy()),
             alpha_abs=float(np.abs(alphas - a2.detach().numpy()).max()))
    ((o2 * tm(v_out)).sum() + (a2 * tm(v_a)).sum()).backward()
    if render_mode != "D":
        e["v_colors"] = rel_l2(vc[:, :d0], C.grad.numpy()) if sh_degree is None else None
    e.update(v_opacities=rel_l2(vo, O.grad.numpy()), v_means2d=rel_l2(vm2, m2.grad.numpy()),
             v_conics=rel_l2(vcon, con.grad.numpy()), v_means=rel_l2(vM, M.grad.numpy()),
             v_quats=rel_l2(vQ, Q.grad.numpy()), v_scales=rel_l2(vS, S.grad.numpy()))
    return e, info, vis


def assert_oracle_bounds(e):
    """Everything test_oracle_matches_dense_float64 asserts, at its bounds."""
    assert e["means2d_abs"] < 1e-4, e
    assert e["conics"] < 1e-5, e
    assert e["ninc"][0] == e["ninc"][1], e
    assert e["render"] < 1e-5, e
    assert e["alpha_abs"] < 1e-5, e
    for k in ("v_colors", "v_opacities", "v_means2d", "v_conics", "v_means", "v_quats", "v_scales"):
        if e.get(k) is not None:
            assert e[k] < 1e-5, (k, e)


@pytest.mark.parametrize("cam,w,h,n,d,seed,mult", CASES)
def test_oracle_matches_dense_float64_under_general_cameras(oracle, cam, w, h, n, d, seed, mult):
    s = general_scene(n, d, w, h, seed, scale_mult=mult, **general_camera(cam, w, h))
    e, info, vis = oracle_and_dense(oracle, s, w, h, seed)
    check_scene_exercises_the_clamp(s, w, h, info["radii"])
    print(cam, e)
    assert_oracle_bounds(e)


def test_case_table_covers_the_edges_it_names():
    cams = {c[0]: general_camera(c[0], c[1], c[2]) for c in CASES}
    assert len(CASES) >= 4
    assert any(k["cx"] < 0 or k["cx"] > c[1] for c, k in zip(CASES, cams.values()))       # principal point outside the image
    assert any(k["spread"] >= 1.6 for k in cams.values())
    for k in cams.values():
        assert abs(k["fx"] / k["fy"] - 1.0) > 0.1 and np.linalg.norm(k["centre"]) > 5.0
        assert min(abs(a) for a in k["ypr"]) > 0.1                                          # yaw, pitch and roll all at work


@pytest.mark.parametrize("cam,w,h,n,d,seed,mult,mode", [("pitch_roll", 64, 48, 700, 3, 44, 30.0, "RGB+D"),
                                                        ("pp_outside", 64, 48, 700, 3, 5, 30.0, "RGB+D"),
                                                        ("behind", 72, 40, 700, 3, 6, 30.0, "D")])
def test_depth_channel_gradient_matches_dense_float64(oracle, cam, w, h, n, d, seed, mult, mode):
    """RGB+D and D: the depth channel is cat(colours, z) in the dense reference; v_depths (the oracle's colour gradient of
    that channel) enters project_bwd, and v_means / v_quats / v_scales are held to 1e-5."""
    s = general_scene(n, d, w, h, seed, scale_mult=mult, **general_camera(cam, w, h))
    e, info, vis = oracle_and_dense(oracle, s, w, h, seed, render_mode=mode)
    check_scene_exercises_the_clamp(s, w, h, info["radii"])
    print(cam, mode, e)
    assert e["depths"] < 1e-6
    assert_oracle_bounds(e)


@pytest.mark.parametrize("cam,seed", [("pitch_roll", 7), ("behind", 48)])
def test_sh_degree_3_render_with_the_camera_far_from_the_origin(oracle, cam, seed):
    """campos = inverse(viewmat)[:3, 3] is |C| > 7 from the origin: the oracle's SH render against dense_ref.sh_colors
    composited in float64."""
    w, h, n = 64, 48, 700
    s = general_scene(n, 3, w, h, seed, scale_mult=30.0, **general_camera(cam, w, h))
    campos = np.linalg.inv(s["viewmat"].astype(np.float64))[:3, 3]
    assert np.abs(campos - s["C"]).max() < 1e-5 and np.linalg.norm(campos) > 7.0
    e, info, vis = oracle_and_dense(oracle, s, w, h, seed, colors=s["sh"], sh_degree=3)
    check_scene_exercises_the_clamp(s, w, h, info["radii"])
    print(cam, e)
    assert e["ninc"][0] == e["ninc"][1]
    assert e["render"] < 1e-5 and e["alpha_abs"] < 1e-5


def visible_float64(s, w, h, eps2d, near, far, radius_clip, rel=1e-4):
    """The culling rule of SURVEY A2-A5 restated in float64: (visible, decided).  `decided` is False where a float64 value
    sits within `rel` (relative) of the threshold it is compared with, so that fp32 may legitimately land on the other
    side: z against near / far, 3 sqrt(lambda) against the integers (the ceil), the radius against radius_clip, and
    means2d -/+ radius against the image edges."""
    from oracle import dense_ref as dr
    with torch.no_grad():
        m2, z, con = dr.project(tm(s["means"]), tm(s["quats"]), tm(s["scales"]), tm(s["viewmat"]), tm(s["K"]), w, h, eps2d=eps2d)
    m2, z, con = m2.numpy(), z.numpy(), con.numpy()
    with np.errstate(all="ignore"):
        detc = con[:, 0] * con[:, 2] - con[:, 1] ** 2
        s00, s01, s11 = con[:, 2] / detc, -con[:, 1] / detc, con[:, 0] / detc       # cov2d (blurred) back from the conic
        det = s00 * s11 - s01 * s01
        hb = 0.5 * (s00 + s11)
        rf = 3.0 * np.sqrt(hb + np.sqrt(np.maximum(0.01, hb * hb - det)))
        radius = np.ceil(rf)
        in_z = (z >= near) & (z <= far)
        on = ~((m2[:, 0] + radius <= 0) | (m2[:, 0] - radius >= w) | (m2[:, 1] + radius <= 0) | (m2[:, 1] - radius >= h))
        vis = in_z & (det > 0) & (radius > radius_clip) & on

        def close(a, b):
            return np.abs(a - b) <= rel * np.maximum(np.abs(a), np.abs(b))

        shaky = close(z, near) | close(z, far)
        shaky |= in_z & close(rf, np.round(rf))                  # the ceil (and with it radius > radius_clip)
        for c, size in ((m2[:, 0], float(w)), (m2[:, 1], float(h))):
            big = np.maximum(np.abs(c), radius)                  # a sum of two terms against an edge: relative to the larger
            shaky |= in_z & ((np.abs(c + radius) <= rel * big) | (np.abs(c - radius - size) <= rel * np.maximum(big, size)))
    return vis, ~shaky, z, radius


CULLING = [  # camera, seed, eps2d, near, far, radius_clip
    ("pitch_roll", 50, 0.0, 0.01, 1e10, 0.0),
    ("behind", 11, 0.3, 4.0, 9.0, 0.0),
    ("pp_outside", 12, 0.1, 3.0, 1e10, 6.0),
    ("upside_down", 13, 0.0, 2.5, 10.5, 4.0),
]


@pytest.mark.parametrize("cam,seed,eps2d,near,far,clip", CULLING)
def test_non_default_culling_parameters(oracle, cam, seed, eps2d, near, far, clip):
    """near / far / radius_clip / eps2d through oracle.rasterization and project_bwd: the visible set against the float64
    restatement of the rule (leaving out at most 1 % of the Gaussians, those within 1e-4 relative of a threshold), values and
    gradients against dense float64 at the usual bounds."""
    w, h, n = 64, 48, 700
    s = general_scene(n, 4, w, h, seed, scale_mult=30.0, **general_camera(cam, w, h))
    e, info, vis = oracle_and_dense(oracle, s, w, h, seed, eps2d=eps2d, near=near, far=far, radius_clip=clip)
    vis64, decided, z, radius = visible_float64(s, w, h, eps2d, near, far, clip)
    assert (~decided).sum() <= n // 100, int((~decided).sum())
    np.testing.assert_array_equal(vis[decided], vis64[decided])
    both = vis & vis64 & decided
    np.testing.assert_array_equal(info["radii"][both], radius[both].astype(np.int32))
    zv = info["depths"][vis]
    assert zv.min() >= near and zv.max() <= far and info["radii"][vis].min() > clip
    # each parameter decides something in its case: the default rule would keep Gaussians that this one culls
    d_vis, _, _, _ = visible_float64(s, w, h, eps2d, 0.01, 1e10, 0.0)
    if (near, far, clip) != (0.01, 1e10, 0.0):
        assert (d_vis & ~vis64).sum() >= 20
    assert vis.sum() >= 50 and (~vis).sum() >= 50
    print(cam, e, int(vis.sum()))
    assert_oracle_bounds(e)


def test_eps2d_changes_the_conic_as_stated(oracle):
    """eps2d = 0 on an isotropic on-axis Gaussian: conic = 1 / (f s / z)^2 exactly as without blur; eps2d = 0.7 adds 0.7."""
    w = h = 33
    fx, sc, z = 40.0, 0.05, 2.0
    for eps in (0.0, 0.7):
        out, alpha, info = oracle.rasterization(np.array([[0, 0, z]], np.float32), np.array([[1, 0, 0, 0]], np.float32),
                                                np.full((1, 3), sc, np.float32), np.array([0.5], np.float32),
                                                np.ones((1, 1), np.float32), np.eye(4, dtype=np.float32),
                                                np.array([[fx, 0, 16.5], [0, fx, 16.5], [0, 0, 1]], np.float32), None, w, h,
                                                eps2d=eps)
        var = (fx * sc / z) ** 2 + eps
        np.testing.assert_allclose(info["conics"][0], [1 / var, 0, 1 / var], rtol=2e-6, atol=1e-7)
        assert info["radii"][0] == math.ceil(3 * math.sqrt(var + math.sqrt(0.01)))  # isotropic: hb^2 - det = 0 < 0.01


# -- known answers ----------------------------------------------------------------------------------------------------------

def quarter_turn(axis):
    """World-to-camera rotation by exactly 90 degrees about one axis: entries 0 and +-1 only."""
    return {"x": np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32),
            "y": np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]], np.float32),
            "z": np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float32)}[axis]


def quarter_turn_case(axis):
    """One axis-aligned Gaussian at (1, 0.5, 2) with scales (0.25, 0.5, 0.125) seen through a quarter turn and a dyadic
    translation, with fx = 32, fy = 64, principal point (24, 40) in a 64 x 64 image.  Everything up to the conic's divisions is
    exact in fp32.  Returns (arguments of project_fwd, camera-space point, camera-space variances, pixel), the last three
    worked out by hand."""
    t, pc, var, pix = {
        # R p = (1, -2, 0.5); camera axes = world (x, -z, y)
        "x": ((-0.5, 2.25, 1.5), (0.5, 0.25, 2.0), (0.0625, 0.015625, 0.25), (32.0, 48.0)),
        # R p = (2, 0.5, -1); camera axes = world (z, y, -x)
        "y": ((-1.0, -0.25, 3.0), (1.0, 0.25, 2.0), (0.015625, 0.25, 0.0625), (40.0, 48.0)),
        # R p = (-0.5, 1, 2); camera axes = world (-y, x, z)
        "z": ((1.0, -0.5, 2.0), (0.5, 0.5, 4.0), (0.25, 0.0625, 0.015625), (28.0, 48.0)),
    }[axis]
    vm = np.eye(4, dtype=np.float32)
    vm[:3, :3], vm[:3, 3] = quarter_turn(axis), np.array(t, np.float32)
    K = np.array([[32, 0, 24], [0, 64, 40], [0, 0, 1]], np.float32)
    args = (np.array([[1.0, 0.5, 2.0]], np.float32), np.array([[1, 0, 0, 0]], np.float32),
            np.array([[0.25, 0.5, 0.125]], np.float32), vm, K, 64, 64)
    return args, pc, var, pix


def quarter_turn_expected(pc, var, eps2d=0.3, fx=32.0, fy=64.0, cx=24.0, cy=40.0):
    """means2d, depth, conic by hand (float64) for an axis-aligned covariance diag(var) at camera point pc, clamp inactive:
    J = [[fx/z, 0, -fx x/z^2], [0, fy/z, -fy y/z^2]]."""
    x, y, z = pc
    a = (fx / z) ** 2 * var[0] + (fx * x / z ** 2) ** 2 * var[2] + eps2d
    c = (fy / z) ** 2 * var[1] + (fy * y / z ** 2) ** 2 * var[2] + eps2d
    b = (fx * x / z ** 2) * (fy * y / z ** 2) * var[2]
    det = a * c - b * b
    return (fx * x / z + cx, fy * y / z + cy), z, (c / det, -b / det, a / det)


@pytest.mark.parametrize("axis", ["x", "y", "z"])
def test_quarter_turn_cameras_known_answer(oracle, axis):
    args, pc, var, pix = quarter_turn_case(axis)
    radii, m2, depths, con = oracle.project_fwd(*args)
    want_m2, want_z, want_con = quarter_turn_expected(pc, var)
    assert want_m2 == pix
    assert radii[0] > 0
    assert depths[0] == want_z and tuple(m2[0]) == pix            # exact: dyadic inputs, a permutation, a power-of-two z
    np.testing.assert_allclose(con[0], want_con, rtol=2e-6, atol=1e-9)


def depth_tie_inputs():
    """Identity rotation, z = mean_z + t_z exact in fp32.  near = 1.5, far = 6: Gaussians at z == near, z == far, one ulp
    below near and one ulp above far.  Returns (means, viewmat, near, far, expected visibility)."""
    near, far, tz = np.float32(1.5), np.float32(6.0), np.float32(0.5)
    zs = np.array([near, far, np.nextafter(near, np.float32(0)), np.nextafter(far, np.float32(10))], np.float32)
    means = np.zeros((4, 3), np.float32)
    means[:, 2] = zs - tz                                        # exact: zs - 0.5 keeps every bit at these magnitudes
    assert np.all(means[:, 2] + tz == zs)
    vm = np.eye(4, dtype=np.float32)
    vm[2, 3] = tz
    return means, vm, float(near), float(far), [True, True, False, False]


def test_depth_ties_near_and_far_are_kept_one_ulp_outside_is_culled(oracle):
    means, vm, near, far, want = depth_tie_inputs()
    n = len(means)
    K = np.array([[40, 0, 16], [0, 40, 16], [0, 0, 1]], np.float32)
    radii, m2, depths, con = oracle.project_fwd(means, np.array([[1, 0, 0, 0]] * n, np.float32), np.full((n, 3), 0.05, np.float32),
                                                vm, K, 32, 32, near=near, far=far)
    assert (radii > 0).tolist() == want
    assert depths[0] == np.float32(near) and depths[1] == np.float32(far)
    assert np.all(depths[2:] == 0) and np.all(m2[2:] == 0) and np.all(con[2:] == 0)
    # the same through the front-end
    _, _, info = oracle.rasterization(means, np.array([[1, 0, 0, 0]] * n, np.float32), np.full((n, 3), 0.05, np.float32),
                                      np.full(n, 0.5, np.float32), np.ones((n, 1), np.float32), vm, K, None, 32, 32,
                                      near=near, far=far)
    assert (info["radii"] > 0).tolist() == want
    # and with the defaults all four are visible: the planes decided
    assert (oracle.project_fwd(means, np.array([[1, 0, 0, 0]] * n, np.float32), np.full((n, 3), 0.05, np.float32), vm, K,
                               32, 32)[0] > 0).all()


def test_general_scene_builds_what_it_says():
    """viewmat = [R^T | -R^T C] with R orthonormal, camera centre where asked, and the Gaussians' pixel positions uniform over
    spread x the image about its centre, depths in z_range."""
    w, h, n = 64, 48, 4000
    k = general_camera("pp_outside", w, h)
    s = general_scene(n, 2, w, h, 3, scale_mult=1.0, **k)
    vm = s["viewmat"].astype(np.float64)
    assert np.abs(vm[:3, :3] @ vm[:3, :3].T - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(vm[:3, :3]) - 1) < 1e-6
    assert np.abs(np.linalg.inv(vm)[:3, 3] - np.asarray(k["centre"])).max() < 1e-5
    assert np.abs(vm[:3, :3] - vm[:3, :3].T).max() > 0.1                # a transposed viewmat is a different camera
    p = s["means"].astype(np.float64) @ vm[:3, :3].T + vm[:3, 3]
    u, v = k["fx"] * p[:, 0] / p[:, 2] + k["cx"], k["fy"] * p[:, 1] / p[:, 2] + k["cy"]
    sp = k["spread"]
    assert p[:, 2].min() > 1.99 and p[:, 2].max() < 12.01
    for q, size in ((u, w), (v, h)):
        lo, hi = 0.5 * size * (1 - sp), 0.5 * size * (1 + sp)
        assert q.min() > lo - 1e-3 * size and q.max() < hi + 1e-3 * size
        assert q.min() < lo + 0.01 * sp * size and q.max() > hi - 0.01 * sp * size
        assert abs(q.mean() - 0.5 * size) < 0.03 * sp * size
    assert set(s) >= {"means", "quats", "scales", "opacities", "colors", "sh", "viewmat", "K", "cam", "raw"}
    s2 = general_scene(n, 2, w, h, 3, scale_mult=1.0, **k)
    assert all(np.array_equal(s[a], s2[a]) for a in ("means", "quats", "scales", "opacities", "colors", "sh", "viewmat", "K"))
