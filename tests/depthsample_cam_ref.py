"""The min-depth mapping under camera models (include/gags_next.h "N22") without the package: TEST INFRASTRUCTURE ONLY, in
the style of tests/depthsample_ref.py, whose pinhole functions it calls.  Does not import gags_amd.

`decide` / `depth_sample` restate the general decision in numpy float32 in the stated operation order (one rounding per
operation, no FMA, correctly rounded division).  For pinhole and ortho cameras that is the kernel bit for bit; for the fisheye
it is only a yardstick, because numpy's float32 arctan2 and the device's atan2f are different functions.

`decide64` / `depth_sample64` make the same decision from a float64 projection and mark the BAND in which float32 and float64
may disagree: N6's own widths (depthsample_ref.decide64: 1e-3 px from a half-integer, 1e-5 d around the depth test) and a
band around each of the two position culls, |zc - 0.01| <= ZC_BAND and |P'(t)| <= FOLD_BAND.  Both widths come from the
precision of float32: zc is a sum of four terms of magnitude <= 8 (ulp 4.8e-7 each, so a few 1e-6 at worst), P'(t) a Horner
form in t = theta^2 <= 2.5 with |k| <= 0.2 whose slope in theta is below 2 and whose theta carries the few-ulp error of
atan2f on top of that of (xc, yc, zc): again a few 1e-6.  tests/test_depthsample_cam_cpu.py measures the float32 restatement
against float64 on the scenes below and asserts that each width is at least 8 times the largest difference.

The scenes (`scene`): points in a cone up to 88 degrees off the z axis at distances 1 .. 4, three cameras with small random
rotations and translations, intrinsics per model (fisheye 24 px / rad, ortho 9 px / unit, pinhole f = 32); `depth_maps`: the zc
of the lowest-index point on each pixel times a factor drawn from {1, 1.2, 1.4, 0.7}, so that the depth test decides both
ways."""
import numpy as np

import depthsample_ref as R

F = np.float32
EPS = F(1e-7)          # GAGS_FISHEYE_EPS
NEAR = F(0.01)         # render()'s near plane
MODELS = {"pinhole": 0, "ortho": 1, "fisheye": 2}
ZC_BAND = 2e-5
FOLD_BAND = 2e-5
SIZES = ((64, 48), (63, 47))
FOCAL = {"pinhole": 32.0, "ortho": 9.0, "fisheye": 24.0}
# the coefficient sets A, B and C of tests/fisheye_kb_ref.py (which imports the package through tests/helpers.py, so they are
# repeated here; tests/test_depthsample_cam_cpu.py holds the two tables equal).  C folds at 74 degrees: 1 - 0.6 theta^2 = 0
COEFFS = {"A": (-0.0290, -0.0049, 0.0012, -0.0004), "B": (-0.04, 0.01, -0.003, 0.0005), "C": (-0.2, 0.0, 0.0, 0.0),
          "zero": (0.0, 0.0, 0.0, 0.0)}


def coeffs32(kc):
    """A camera's coefficients as the kernel sees them: float32 [4]; None = zero; a name = a set of COEFFS."""
    if kc is None:
        return np.zeros(4, F)
    return np.asarray(COEFFS[kc] if isinstance(kc, str) else kc, F).reshape(4)


def poly(kc, t):
    """(P(t), P'(t)) by Horner, in t's dtype."""
    k1, k2, k3, k4 = kc
    return 1 + t * (k1 + t * (k2 + t * (k3 + t * k4))), 1 + t * (3 * k1 + t * (5 * k2 + t * (7 * k3 + t * (9 * k4))))


def camera_space32(xyz, M):
    """Step 1 in float32: (xc, yc, zc)."""
    x, y, z = (np.ascontiguousarray(xyz[:, k], dtype=F) for k in range(3))
    M = np.asarray(M, F)
    with np.errstate(all="ignore"):
        return [((M[i, 0] * x + M[i, 1] * y) + M[i, 2] * z) + M[i, 3] for i in range(3)]


def fisheye32(xc, yc, zc, kc):
    """(k, P'(t)) of the fisheye in float32, in the rule's operation order."""
    k1, k2, k3, k4 = coeffs32(kc)
    with np.errstate(all="ignore"):
        rho = np.sqrt(xc * xc + yc * yc) + EPS
        theta = np.arctan2(rho, zc + EPS)
        t = theta * theta
        P = F(1) + t * (k1 + t * (k2 + t * (k3 + t * k4)))
        dP = F(1) + t * (F(3) * k1 + t * (F(5) * k2 + t * (F(7) * k3 + t * (F(9) * k4))))
        k = (theta * P) / rho
    assert k.dtype == F and dP.dtype == F
    return k, dP


def project32(xyz, M, K, model, kc=None):
    """(u, v, zc, keep) of one camera in float32, in the rule's operation order.  keep: the position culls (all True for a
    pinhole camera)."""
    K = np.asarray(K, F)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    xc, yc, zc = camera_space32(xyz, M)
    with np.errstate(all="ignore"):
        if model == "pinhole":
            return (xc * fx) / zc + cx, (yc * fy) / zc + cy, zc, np.ones(len(zc), bool)
        keep = zc >= NEAR
        if model == "ortho":
            return xc * fx + cx, yc * fy + cy, zc, keep
        assert model == "fisheye", model
        k, dP = fisheye32(xc, yc, zc, kc)
        return (fx * xc) * k + cx, (fy * yc) * k + cy, zc, keep & ~(dP <= 0)


def decide(xyz, M, K, depth, model="pinhole", kc=None, vis_thresh=0.25, cut_bound=0):
    """depthsample_ref.decide for a camera of any model: (visible, v, u, d)."""
    if model == "pinhole":
        return R.decide(xyz, M, K, depth, vis_thresh, cut_bound)
    u, v, zc, keep = project32(xyz, M, K, model, kc)
    h, w = depth.shape
    with np.errstate(all="ignore"):
        ur, vr = np.rint(u), np.rint(v)
        cut = F(cut_bound)
        inside = keep & (ur >= cut) & (ur < F(w) - cut) & (vr >= cut) & (vr < F(h) - cut)
        ui = np.where(inside, ur, 0).astype(np.int32)
        vi = np.where(inside, vr, 0).astype(np.int32)
        d = np.where(inside, depth[vi, ui], F(0)).astype(F)
        vis = inside & (np.abs(d - zc) <= F(vis_thresh) * d)
    return vis, vi, ui, d


def _assemble(per_camera, n, depths, cams):
    """depthsample_ref.depth_sample's outputs from per-camera (visible, v, u, d)."""
    c, h, w = depths.shape
    mapping = np.zeros((n, c, 2), np.int32)
    visible = np.zeros((n, c), bool)
    md = np.full(n, np.inf, F)
    for k, (vis, vi, ui, d) in enumerate(per_camera):
        mapping[vis, k, 0], mapping[vis, k, 1], visible[:, k] = vi[vis], ui[vis], vis
        md = np.where(vis, np.minimum(md, d.astype(F)), md)
    cams = range(c) if cams is None else cams
    samples = np.zeros((len(cams), h, w), F)
    winner = np.full((len(cams), h * w), -1, np.int64)
    idx = np.arange(n, dtype=np.int64)
    for j, k in enumerate(cams):
        vis = visible[:, k]
        np.maximum.at(winner[j], mapping[vis, k, 0].astype(np.int64) * w + mapping[vis, k, 1], idx[vis])
        samples[j] = np.where(winner[j] >= 0, md[np.maximum(winner[j], 0)], F(0)).reshape(h, w)
    return {"mapping": mapping, "visible": visible, "min_depth": md, "samples": samples, "winner": winner}


def depth_sample(xyz, viewmats, Ks, depths, models=None, coeffs=None, vis_thresh=0.25, cut_bound=0, cams=None):
    """depthsample_ref.depth_sample for a rig: models [C] names (None: all pinhole), coeffs [C] of coefficient sets or None."""
    c = depths.shape[0]
    models = ["pinhole"] * c if models is None else list(models)
    coeffs = [None] * c if coeffs is None else list(coeffs)
    per = [decide(xyz, viewmats[k], Ks[k], depths[k], models[k], coeffs[k], vis_thresh, cut_bound) for k in range(c)]
    out = _assemble(per, xyz.shape[0], depths, cams)
    del out["winner"]
    return out


def project64(xyz, M, K, model, kc=None):
    """(u, v, zc, dP) in float64 from the float32 inputs; dP = P'(t) for a fisheye, 1 otherwise."""
    p = np.asarray(xyz, np.float64)
    M, K = np.asarray(M, np.float64), np.asarray(K, np.float64)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    r = p @ M[:3, :3].T + M[:3, 3]
    xc, yc, zc = r.T
    one = np.ones(len(zc))
    with np.errstate(all="ignore"):
        if model == "pinhole":
            return xc * fx / zc + cx, yc * fy / zc + cy, zc, one
        if model == "ortho":
            return xc * fx + cx, yc * fy + cy, zc, one
        assert model == "fisheye", model
        kc = tuple(float(v) for v in coeffs32(kc))
        rho = np.sqrt(xc * xc + yc * yc) + float(EPS)
        theta = np.arctan2(rho, zc + float(EPS))
        P, dP = poly(kc, theta * theta)
        k = theta * P / rho
        return fx * xc * k + cx, fy * yc * k + cy, zc, dP


def decide64(xyz, M, K, depth, model="pinhole", kc=None, vis_thresh=0.25, cut_bound=0):
    """The decision from the float64 projection and the band where float32 may decide otherwise: (visible, v, u, band)."""
    u, v, zc, dP = project64(xyz, M, K, model, kc)
    h, w = depth.shape
    general = model != "pinhole"
    with np.errstate(all="ignore"):
        keep = (zc >= float(NEAR)) & ~(dP <= 0) if general else np.ones(len(zc), bool)
        ur, vr = np.rint(u), np.rint(v)
        inside = keep & (ur >= cut_bound) & (ur < w - cut_bound) & (vr >= cut_bound) & (vr < h - cut_bound)
        ui = np.where(inside, ur, 0).astype(np.int64)
        vi = np.where(inside, vr, 0).astype(np.int64)
        d = np.where(inside, depth[vi, ui], 0).astype(np.float64)
        vis = inside & (np.abs(d - zc) <= F(vis_thresh) * d)
        half = lambda t: np.abs(t - np.floor(t) - 0.5) < 1e-3  # noqa: E731
        band = half(u) | half(v) | (inside & (np.abs(np.abs(d - zc) - F(vis_thresh) * d) <= 1e-5 * np.abs(d)))
        if general:
            band |= np.abs(zc - float(NEAR)) <= ZC_BAND
            if model == "fisheye":
                band |= np.abs(dP) <= FOLD_BAND
    return vis, vi.astype(np.int32), ui.astype(np.int32), band


def depth_sample64(xyz, viewmats, Ks, depths, models, coeffs=None, vis_thresh=0.25, cut_bound=0):
    """The float64 decision for a rig, with what a comparison needs besides depth_sample's outputs:
      band [N, C]       where float32 may decide otherwise
      sure_points [N]   no camera has the point in its band: min_depth is exact
      sure_pixels [C, H, W]  no band point can land on the pixel (its 3 x 3 neighbourhood under the float64 projection, and any
                        pixel at all when its projection is not finite) and the pixel's winner, if any, is a sure point."""
    n, (c, h, w) = xyz.shape[0], depths.shape
    coeffs = [None] * c if coeffs is None else list(coeffs)
    per, band = [], np.zeros((n, c), bool)
    for k in range(c):
        vis, vi, ui, b = decide64(xyz, viewmats[k], Ks[k], depths[k], models[k], coeffs[k], vis_thresh, cut_bound)
        per.append((vis, vi, ui, depths[k][vi, ui]))
        band[:, k] = b
    out = _assemble(per, n, depths, None)
    sure_points = ~band.any(1)
    sure_pixels = np.ones((c, h, w), bool)
    for k in range(c):
        u, v, _, _ = project64(xyz, viewmats[k], Ks[k], models[k], coeffs[k])
        for i in np.nonzero(band[:, k])[0]:
            if not (np.isfinite(u[i]) and np.isfinite(v[i])):
                sure_pixels[k] = False
                break
            ui, vi = int(np.clip(np.rint(u[i]), -2, w + 1)), int(np.clip(np.rint(v[i]), -2, h + 1))
            sure_pixels[k, max(vi - 1, 0):max(vi + 2, 0), max(ui - 1, 0):max(ui + 2, 0)] = False
        win = out["winner"][k].reshape(h, w)
        sure_pixels[k] &= (win < 0) | sure_points[np.maximum(win, 0)]
    out.update(band=band, sure_points=sure_points, sure_pixels=sure_pixels)
    del out["winner"]
    return out


def intrinsics(model, w, h):
    f = FOCAL[model]
    return np.array([[f, 0, w / 2.0], [0, f, h / 2.0], [0, 0, 1]], F)


def scene(w, h, seed, n=3000, n_cams=3):
    """(xyz [n, 3], viewmats [n_cams, 4, 4]) float32: the cone of points and the cameras of the module docstring."""
    rng = np.random.default_rng(seed)
    ang = np.radians(88.0) * np.sqrt(rng.uniform(0, 1, n))
    phi = rng.uniform(0, 2 * np.pi, n)
    dist = rng.uniform(1.0, 4.0, n)
    xyz = np.stack([dist * np.sin(ang) * np.cos(phi), dist * np.sin(ang) * np.sin(phi), dist * np.cos(ang)], 1).astype(F)
    vms = np.zeros((n_cams, 4, 4), F)
    for k in range(n_cams):
        a, b, g = rng.uniform(-0.05, 0.05, 3)
        rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
        ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
        rz = np.array([[np.cos(g), -np.sin(g), 0], [np.sin(g), np.cos(g), 0], [0, 0, 1]])
        vms[k, :3, :3] = rx @ ry @ rz
        vms[k, :3, 3] = rng.uniform(-0.1, 0.1, 3)
        vms[k, 3, 3] = 1
    return xyz, vms


def depth_maps(xyz, viewmats, Ks, models, coeffs, w, h, seed):
    """[C, h, w] float32: per pixel the zc of the lowest-index point that lands on it (float64 projection, culls applied; 2.5
    where none does) times a factor drawn from {1, 1.2, 1.4, 0.7}."""
    rng = np.random.default_rng(seed + 1000)
    c = len(models)
    coeffs = [None] * c if coeffs is None else coeffs
    out = np.zeros((c, h, w), F)
    for k in range(c):
        u, v, zc, dP = project64(xyz, viewmats[k], Ks[k], models[k], coeffs[k])
        with np.errstate(all="ignore"):
            ur, vr = np.rint(u), np.rint(v)
            ok = (zc >= 0.01) & ~(dP <= 0) & (ur >= 0) & (ur < w) & (vr >= 0) & (vr < h)
        base = np.full(h * w, 2.5)
        idx = np.nonzero(ok)[0][::-1]  # (the lowest index is written last)
        base[vr[idx].astype(np.int64) * w + ur[idx].astype(np.int64)] = zc[idx]
        out[k] = (base.reshape(h, w) * rng.choice([1.0, 1.2, 1.4, 0.7], (h, w))).astype(F)
    return out


# the rigs of the tests: name -> (models, coefficient sets), three cameras each
RIGS = {
    "pinhole": (["pinhole"] * 3, [None] * 3),
    "ortho": (["ortho"] * 3, [None] * 3),
    "fisheye": (["fisheye"] * 3, [None] * 3),
    "A": (["fisheye"] * 3, ["A"] * 3),
    "B": (["fisheye"] * 3, ["B"] * 3),
    "C": (["fisheye"] * 3, ["C"] * 3),
}
SCENE_SEEDS = {"pinhole": 70, "ortho": 71, "fisheye": 72, "A": 73, "B": 74, "C": 75}
_CACHE = {}


def rig_scene(name, w, h, n=3000):
    """The scene of rig `name` at w x h, built once: dict of xyz, viewmats, Ks, depths, models, coeffs (names) and coeff_block
    [C, 4] float32 (None when the rig has no coefficients)."""
    key = (name, w, h, n)
    if key not in _CACHE:
        models, coeffs = RIGS[name]
        xyz, vms = scene(w, h, SCENE_SEEDS[name] + (w % 2), n)
        Ks = np.stack([intrinsics(m, w, h) for m in models])
        depths = depth_maps(xyz, vms, Ks, models, coeffs, w, h, SCENE_SEEDS[name])
        block = None if all(c is None for c in coeffs) else np.stack([coeffs32(c) for c in coeffs])
        _CACHE[key] = dict(xyz=xyz, viewmats=vms, Ks=Ks, depths=depths, models=list(models), coeffs=list(coeffs),
                           coeff_block=block)
    return _CACHE[key]


def reference64(name, w, h, n=3000):
    """depth_sample64 of rig_scene(name, w, h), computed once and shared (callers do not modify it)."""
    key = ("ref64", name, w, h, n)
    if key not in _CACHE:
        s = rig_scene(name, w, h, n)
        _CACHE[key] = depth_sample64(s["xyz"], s["viewmats"], s["Ks"], s["depths"], s["models"], s["coeffs"])
    return _CACHE[key]
