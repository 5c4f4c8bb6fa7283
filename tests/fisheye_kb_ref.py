"""Reference for the fisheye's distortion coefficients (N21; include/gags_raster.h "GAGS_PROJ_KB" has the rule).  TEST
INFRASTRUCTURE ONLY, in the style of tests/camera_models_ref.py, from which it takes what does not depend on the camera's map
(decide, outputs, project_loss, the scenes and cotangents).

`cam_map` restates the rule in torch and follows the dtype of its inputs: float64 with autograd is the truth, float32 on the CPU
the yardstick; with zero coefficients its float32 values are cm.cam_map("fisheye")'s bit for bit.  `decide` adds the fold
(dg <= 0) to cm.decide's decisions and |dg| <= NEAR_TOL to its boundaries.  `cam_bwd_np` / `bwd_terms` restate the kernel's
hand-written backward in numpy float64, as cm.cam_bwd_np / cm.bwd_terms do for N20."""
import numpy as np
import torch

import aa_ref
import camera_models_ref as cm

EPS = cm.FISHEYE_EPS
KB = 32   # GAGS_PROJ_KB
# (k1, k2, k3, k4).  A: mild, g' >= 0.66 up to 88 degrees; B: g' >= 0.86; C folds (g' = 1 - 0.6 theta^2 = 0) at 74 degrees
COEFFS = {"A": (-0.0290, -0.0049, 0.0012, -0.0004), "B": (-0.04, 0.01, -0.003, 0.0005), "C": (-0.2, 0.0, 0.0, 0.0),
          "zero": (0.0, 0.0, 0.0, 0.0)}
# the scenes of the kernel-level GPU tests: cm.model_scene("fisheye", 700, 0, KERNEL_W, KERNEL_H, seed) under cm.KERNEL_CULL;
# tests/test_fisheye_kb_cpu.py pins them on the CPU, from the reference alone: at most MAX_EXCLUDED of the Gaussians near a
# decision boundary (the fold included), and a float32 yardstick that is representative at every size the GPU tests cut from the
# scene (`yardstick_errors`) -- the first seed from 21 on that meets both, per set
KERNEL_SEEDS = {"A": 42, "B": 29, "C": 22}
YARDSTICK_FLOOR = 0.5   # the float32 restatement's error on a prefix of a scene, as a share of its error on the whole scene
# through rasterization(): (w, h, D, raw_params, antialiased, render_mode, sh_degree, seed, coefficient set)
RASTER_CASES = [(97, 61, 16, True, True, "RGB", None, 61, "A"), (97, 61, 3, False, False, "RGB+ED", 3, 62, "B")]


def coeffs32(name_or_values):
    """The coefficients as the kernel sees them: float32 [4]."""
    v = COEFFS[name_or_values] if isinstance(name_or_values, str) else name_or_values
    return np.asarray(v, np.float32).reshape(4)


def block(K, kc):
    """The 13 floats behind GAGS_PROJ_KB: K row-major, then k1 .. k4."""
    return np.concatenate([np.asarray(K, np.float32).reshape(9), coeffs32(kc)])


def poly(kc, t):
    """(P(t), P'(t)) by Horner; kc: four scalars (or 0-d tensors) of t's dtype."""
    k1, k2, k3, k4 = kc
    return 1 + t * (k1 + t * (k2 + t * (k3 + t * k4))), 1 + t * (3 * k1 + t * (5 * k2 + t * (7 * k3 + t * (9 * k4))))


def ddg(kc, theta, t):
    k1, k2, k3, k4 = kc
    return theta * (6 * k1 + t * (20 * k2 + t * (42 * k3 + t * (72 * k4))))


def cam_map(kc, x, y, z, fx, fy, cx, cy):
    """(m2x, m2y, J [N,2,3], dg [N]) of a camera-space point: the declared arithmetic, in cm.cam_map("fisheye")'s order."""
    rho = cm._safe_sqrt(x * x + y * y) + EPS
    theta = torch.atan2(rho, z + EPS)
    g = theta * poly(kc, theta * theta)[0]
    x2, y2, xy = x * x + EPS, y * y, x * y
    s = x2 + y2
    l2 = s + z * z
    tb = torch.atan2(rho, z)
    Pb, dg = poly(kc, tb * tb)
    b = (tb * Pb) / rho / s
    a = dg * (z / (l2 * s))
    J = torch.stack([fx * (x2 * a + y2 * b), fx * xy * (a - b), -fx * x / l2 * dg,
                     fy * xy * (a - b), fy * (y2 * a + x2 * b), -fy * y / l2 * dg], -1)
    return fx * x * g / rho + cx, fy * y * g / rho + cy, J.reshape(-1, 2, 3), dg


def true_map(kc, p, fx, fy, cx, cy):
    """The map alone, [N,3] -> [N,2], without guards: autograd of it is the true Jacobian."""
    x, y, z = p.unbind(-1)
    rho = torch.sqrt(x * x + y * y)
    theta = torch.atan2(rho, z)
    k = theta * poly(kc, theta * theta)[0] / rho
    return torch.stack([fx * x * k + cx, fy * y * k + cy], -1)


def _kc(kc, like):
    return tuple(torch.as_tensor(coeffs32(kc)).to(dtype=like.dtype, device=like.device).unbind(0))


def project(kc, means, quats, scales, viewmat, K, width, height, eps2d=0.3):
    """cm.project's dict for the fisheye with coefficients kc, and dg [N]."""
    Rcw, t = viewmat[:3, :3], viewmat[:3, 3]
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    R = aa_ref.quat_to_rotmat(quats)
    M = R * scales[:, None, :]
    cov_c = Rcw @ (M @ M.transpose(1, 2)) @ Rcw.T
    p = means @ Rcw.T + t
    x, y, z = p.unbind(-1)
    m2x, m2y, J, dg = cam_map(_kc(kc, z), x, y, z, fx, fy, cx, cy)
    c2 = J @ cov_c @ J.transpose(1, 2)
    s00, s01, s11 = c2[:, 0, 0], c2[:, 0, 1], c2[:, 1, 1]
    a, c = s00 + eps2d, s11 + eps2d
    det = a * c - s01 * s01
    conics = torch.stack([c / det, -s01 / det, a / det], -1)
    return dict(means2d=torch.stack([m2x, m2y], -1), depths=z, conics=conics, comp=aa_ref.compensation(s00, s01, s11, eps2d),
                cov=(s00, s01, s11), p=p, J=J, dg=dg)


def decide(pr, width, height, eps2d=0.3, near=0.01, far=1e10, radius_clip=0.0):
    """cm.decide with the fold: a Gaussian with dg <= 0 (in pr's dtype) has radius and tile count 0; dg within NEAR_TOL of 0 is
    close.  A Gaussian past the fold is close only through the fold itself or near / far.  `folded`: in depth and dg <= 0."""
    dec = cm.decide(pr, width, height, eps2d=eps2d, near=near, far=far, radius_clip=radius_clip)
    z, dg = pr["depths"].detach().cpu().numpy(), pr["dg"].detach().cpu().numpy()
    dt = z.dtype.type
    in_depth = ~((z < dt(near)) | (z > dt(far)))
    fold = in_depth & (dg <= 0)
    near_fold = in_depth & cm._near(dg, 0.0)
    radii, tiles = dec["radii"].copy(), dec["tiles"].copy()
    radii[fold] = 0
    tiles[fold] = 0
    close = np.where(fold, cm._near(z, near) | cm._near(z, far), dec["close"]) | near_fold
    return dict(radii=radii, tiles=tiles, close=close, folded=fold)


def run(kc, s, width, height, dtype, *, raw=False, modifier=1.0, grad=False, dev="cpu", viewmat=None, **cull):
    """cm.run for the fisheye with coefficients kc: (pr, dec, leaves).  s["K"] is the [3,3] matrix."""
    def tm(a, rg=False):
        return torch.tensor(np.asarray(a), dtype=dtype, device=dev, requires_grad=rg)
    vm = tm(s["viewmat"] if viewmat is None else viewmat, grad)
    if raw:
        L = dict(means=tm(s["raw"]["xyz"], grad), quats=tm(s["raw"]["rotation"], grad), scales=tm(s["raw"]["scaling_log"], grad),
                 opacities=tm(s["raw"]["opacity_logit"].reshape(-1), grad))
        q, sc = torch.nn.functional.normalize(L["quats"]), torch.exp(L["scales"]) * modifier
        L["opac_act"] = torch.sigmoid(L["opacities"])
    else:
        L = dict(means=tm(s["means"], grad), quats=tm(s["quats"], grad), scales=tm(s["scales"], grad))
        q, sc = L["quats"], L["scales"]
    L["viewmat"] = vm
    eps2d = cull.get("eps2d", 0.3)
    pr = project(kc, L["means"], q, sc, vm, tm(s["K"]), width, height, eps2d=eps2d)
    dec = decide(pr, width, height, eps2d=eps2d, near=cull.get("near_plane", 0.01), far=cull.get("far_plane", 1e10),
                 radius_clip=cull.get("radius_clip", 0.0))
    return pr, dec, L


def cam_bwd_np(kc, fx, fy, x, y, z, vm2, vJ, v_depths):
    """cam_bwd<GAGS_CAM_FISHEYE_KB> of csrc/project.hip in numpy float64: (v_means2d [N,2], vJ [N,2,3]) -> vp [N,3]."""
    kc = tuple(float(v) for v in coeffs32(kc))
    n = x.shape[0]
    vd = np.zeros(n) if v_depths is None else np.asarray(v_depths, np.float64)
    r0 = np.sqrt(x * x + y * y)
    rho, zt = r0 + EPS, z + EPS
    theta = np.arctan2(rho, zt)
    P, dP = poly(kc, theta * theta)
    k = theta * P / rho
    x2, y2, xy = x * x + EPS, y * y, x * y
    s, z2 = x2 + y2, z * z
    l2 = s + z2
    tb = np.arctan2(rho, z)
    tt = tb * tb
    Pb, dg = poly(kc, tt)
    a0 = z / (l2 * s)
    b, a = tb * Pb / rho / s, dg * a0
    v_k = fx * x * vm2[:, 0] + fy * y * vm2[:, 1]
    vx, vy, vz = fx * k * vm2[:, 0], fy * k * vm2[:, 1], vd.copy()
    v_g = v_k / rho
    v_rho = -v_k * k / rho
    g00, g01, g02 = fx * vJ[:, 0, 0], fx * vJ[:, 0, 1], fx * vJ[:, 0, 2]
    g10, g11, g12 = fy * vJ[:, 1, 0], fy * vJ[:, 1, 1], fy * vJ[:, 1, 2]
    gx = g01 + g10
    v_x2, v_y2 = g00 * a + g11 * b, g00 * b + g11 * a
    v_a = g00 * x2 + g11 * y2 + gx * xy
    v_b = g00 * y2 + g11 * x2 - gx * xy
    v_xy = gx * (a - b)
    vx = vx - g02 / l2 * dg
    vy = vy - g12 / l2 * dg
    v_l2 = (g02 * x + g12 * y) / (l2 * l2) * dg
    v_dg = -(g02 * x + g12 * y) / l2
    vz = vz + v_a * dg / (l2 * s)
    v_l2 = v_l2 - v_a * a / l2
    v_s = -v_a * a / s
    v_dg = v_dg + v_a * a0
    v_gb = v_b / (rho * s)
    v_rho = v_rho - v_b * b / rho
    v_s = v_s - v_b * b / s
    v_tb = v_gb * dg + v_dg * ddg(kc, tb, tt)
    hb = rho * rho + z2
    v_rho = v_rho + v_tb * z / hb
    vz = vz - v_tb * rho / hb
    v_s = v_s + v_l2
    vz = vz + 2 * z * v_l2
    v_x2, v_y2 = v_x2 + v_s, v_y2 + v_s
    vx = vx + 2 * x * v_x2 + y * v_xy
    vy = vy + 2 * y * v_y2 + x * v_xy
    v_theta = v_g * dP
    ht = rho * rho + zt * zt
    v_rho = v_rho + v_theta * zt / ht
    vz = vz - v_theta * rho / ht
    safe = np.where(r0 > 0, r0, 1.0)
    vx = vx + np.where(r0 > 0, v_rho * x / safe, 0.0)
    vy = vy + np.where(r0 > 0, v_rho * y / safe, 0.0)
    return np.stack([vx, vy, vz], -1)


def bwd_terms(kc, s, width, height, radii, v_means2d, v_depths, v_conics, v_comp=None, *, antialiased=False, eps2d=0.3):
    """cm.bwd_terms for the fisheye with coefficients kc: dict(v_means [N,3], pose [N,12]); zero rows where radii <= 0."""
    f = lambda a: np.asarray(a, np.float64)  # noqa: E731
    mu, q, sc, vm, K = f(s["means"]), f(s["quats"]), f(s["scales"]), f(s["viewmat"]), f(s["K"])
    n = mu.shape[0]
    Rc, tc = vm[:3, :3], vm[:3, 3]
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    R = aa_ref.quat_to_rotmat(torch.tensor(q)).numpy()
    M = R * sc[:, None, :]
    A = Rc[None] @ (M @ M.transpose(0, 2, 1))
    Sc = A @ Rc.T[None]
    p = mu @ Rc.T + tc
    x, y, z = p.T
    t = lambda a: torch.tensor(a)  # noqa: E731
    _, _, J, _ = cam_map(_kc(kc, t(z)), t(x), t(y), t(z), t(fx), t(fy), t(cx), t(cy))
    J = J.numpy()
    c2 = J @ Sc @ J.transpose(0, 2, 1)
    s00o, s01, s11o = c2[:, 0, 0], c2[:, 0, 1], c2[:, 1, 1]
    s00, s11 = s00o + eps2d, s11o + eps2d
    det = s00 * s11 - s01 * s01
    ca, cb, cc = s11 / det, -s01 / det, s00 / det
    vcon = f(v_conics)
    X = np.stack([ca, cb, cb, cc], -1).reshape(n, 2, 2)
    Gx = np.stack([vcon[:, 0], 0.5 * vcon[:, 1], 0.5 * vcon[:, 1], vcon[:, 2]], -1).reshape(n, 2, 2)
    G = -(X @ Gx @ X)
    if antialiased and v_comp is not None:
        r = (s00o * s11o - s01 * s01) / det
        comp = np.sqrt(np.maximum(0.0, r))
        v_r = np.where(comp > 0, f(v_comp) / (2 * np.where(comp > 0, comp, 1.0)), 0.0)
        e = eps2d / det
        G[:, 0, 0] += v_r * ((1 - r) * ca - e)
        G[:, 1, 1] += v_r * ((1 - r) * cc - e)
        G[:, 0, 1] += v_r * (1 - r) * cb
        G[:, 1, 0] += v_r * (1 - r) * cb
    GSc = J.transpose(0, 2, 1) @ G @ J
    vJ = G @ J @ Sc.transpose(0, 2, 1) + G.transpose(0, 2, 1) @ J @ Sc
    vp = cam_bwd_np(kc, fx, fy, x, y, z, f(v_means2d), vJ, v_depths)
    vR = vp[:, :, None] * mu[:, None, :] + (GSc + GSc.transpose(0, 2, 1)) @ A
    pose = np.concatenate([vR, vp[:, :, None]], axis=2).reshape(n, 12)
    v_means = vp @ Rc
    cull = np.asarray(radii) <= 0
    pose[cull] = 0.0
    v_means[cull] = 0.0
    return dict(v_means=v_means, pose=pose)


def kernel_scene(name):
    """The kernel-level scene of coefficient set `name`: 700 Gaussians up to 88 degrees off axis, and the culling parameters."""
    return cm.model_scene("fisheye", 700, 0, cm.KERNEL_W, cm.KERNEL_H, KERNEL_SEEDS[name]), dict(cm.KERNEL_CULL)


def cut(s, n):
    """The first n Gaussians of a scene."""
    out = dict(s)
    for k in ("means", "quats", "scales", "opacities"):
        out[k] = s[k][:n]
    out["raw"] = {k: (v[:n] if torch.is_tensor(v) else v) for k, v in s["raw"].items()}
    return out


def yardstick_errors(name, s, cull, n, raw):
    """The float32 CPU restatement's own error (rel-L2 against float64) on the first n Gaussians of a scene, per quantity the
    GPU tests bound by it: the forward's floats over the rows both precisions see away from a boundary, and, under `g_`, the
    gradients of the antialiased loss with cm.cotangents(700, 2).  None when no such row exists.  The bound of the GPU tests is a
    multiple of these figures, so a scene serves only where they are representative: drawn from one or a few Gaussians, a
    float32 error can be many times below its value over the scene, and then bounds nothing but luck."""
    from helpers import rel_l2
    w, h = cm.KERNEL_W, cm.KERNEL_H
    s = cut(s, n)
    cot = {k: v[:n] for k, v in cm.cotangents(700, 2).items()}
    P = {dt: run(name, s, w, h, dt, raw=raw, grad=True, **cull) for dt in (torch.float64, torch.float32)}
    d64, d32 = P[torch.float64][1], P[torch.float32][1]
    both = ~d64["close"] & (d64["radii"] > 0) & (d32["radii"] > 0)
    if both.sum() == 0:
        return None
    o64, o32 = cm.outputs(P[torch.float64][0], d64), cm.outputs(P[torch.float32][0], d32)
    res = {k: rel_l2(o32[k][both], o64[k][both]) for k in ("means2d", "depths", "conics", "comp")}
    G = {}
    for dt, (pr, _, L) in P.items():
        cm.project_loss(pr, d64["radii"], cot, antialiased=True, opac_act=L.get("opac_act")).backward()
        G[dt] = {k: L[k].grad.numpy() for k in ("means", "quats", "scales", "viewmat")}
    for k in G[torch.float64]:
        res["g_" + k] = rel_l2(G[torch.float32][k], G[torch.float64][k])
    return res


def raster_scene(case):
    """The scene of a RASTER_CASES entry: visible Gaussians up to 70 degrees off axis (set C is not rendered here)."""
    w, h, d, _, _, _, sh, seed, _ = case
    return cm.model_scene("fisheye", 700, 3 if sh is not None else d, w, h, seed, max_deg=70.0)
