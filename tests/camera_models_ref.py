"""Reference for the camera models of N20 (include/gags_raster.h has the rules).  TEST INFRASTRUCTURE ONLY.

`project` is a torch restatement of the projection for "pinhole", "ortho" and "fisheye", with the antialiased
compensation as in tests/aa_ref.py.  Everything follows the dtype of its inputs: in float64 with autograd it is the truth, run
in float32 on the CPU it is the yardstick for fp32 error.  `decide` takes the integer decisions (cull, radius, tile count) from
a projection and says which Gaussians sit within 1e-5 of a decision boundary.  `ortho_kernel_order` restates the orthographic
forward in the kernel's operation order in numpy float32: no transcendental function on that path, so the kernel is compared bit for
bit.  `bwd_terms` is a numpy float64 restatement of the kernel's per-Gaussian backward (hand-written chain rule, no autograd):
the formula the kernel implements is checked on the CPU before any GPU run."""
import math

import numpy as np
import torch

import aa_ref
from helpers import _ypr_rotation, GENERAL_CAMERAS
from gags_amd import synthetic as syn

TILE = 16
FISHEYE_EPS = 1e-7
MODELS = {"pinhole": 0, "ortho": 1, "fisheye": 2}
NEAR_TOL = 1e-5   # a float64 value within NEAR_TOL * max(1, |v|) of a decision boundary: the Gaussian's integers are not compared
MAX_EXCLUDED = 0.02


def _safe_sqrt(q):
    """sqrt with derivative 0 at 0 (the declared derivative of rho at x = y = 0)."""
    pos = q > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, q, torch.ones_like(q))), torch.zeros_like(q))


def cam_map(model, x, y, z, fx, fy, cx, cy, width, height):
    """(m2x, m2y, J [N,2,3]) of a camera-space point under `model`: the declared arithmetic."""
    zero = torch.zeros_like(z)
    if model == "pinhole":
        tanx, tany = 0.5 * width / fx, 0.5 * height / fy
        lxp, lxn = (width - cx) / fx + 0.3 * tanx, cx / fx + 0.3 * tanx
        lyp, lyn = (height - cy) / fy + 0.3 * tany, cy / fy + 0.3 * tany
        rz = 1.0 / z
        tx = z * torch.minimum(lxp, torch.maximum(-lxn, x * rz))
        ty = z * torch.minimum(lyp, torch.maximum(-lyn, y * rz))
        J = torch.stack([fx * rz, zero, -fx * tx * rz * rz, zero, fy * rz, -fy * ty * rz * rz], -1)
        return fx * x * rz + cx, fy * y * rz + cy, J.reshape(-1, 2, 3)
    if model == "ortho":
        one = torch.ones_like(z)
        J = torch.stack([fx * one, zero, zero, zero, fy * one, zero], -1)
        return fx * x + cx, fy * y + cy, J.reshape(-1, 2, 3)
    assert model == "fisheye", model
    eps = FISHEYE_EPS
    rho = _safe_sqrt(x * x + y * y) + eps
    theta = torch.atan2(rho, z + eps)
    x2, y2, xy = x * x + eps, y * y, x * y
    s = x2 + y2
    l2 = s + z * z
    b = torch.atan2(rho, z) / rho / s
    a = z / (l2 * s)
    J = torch.stack([fx * (x2 * a + y2 * b), fx * xy * (a - b), -fx * x / l2,
                     fy * xy * (a - b), fy * (y2 * a + x2 * b), -fy * y / l2], -1)
    return fx * x * theta / rho + cx, fy * y * theta / rho + cy, J.reshape(-1, 2, 3)


def true_map(model, p, fx, fy, cx, cy):
    """The map alone, [N,3] -> [N,2], without guards (fisheye: theta = atan2(|xy|, z)): autograd of it is the true Jacobian."""
    x, y, z = p.unbind(-1)
    if model == "ortho":
        return torch.stack([fx * x + cx, fy * y + cy], -1)
    if model == "pinhole":
        return torch.stack([fx * x / z + cx, fy * y / z + cy], -1)
    rho = torch.sqrt(x * x + y * y)
    k = torch.atan2(rho, z) / rho
    return torch.stack([fx * x * k + cx, fy * y * k + cy], -1)


def project(model, means, quats, scales, viewmat, K, width, height, eps2d=0.3):
    """dict(means2d [N,2], depths [N], conics [N,3], comp [N], cov = (s00, s01, s11) before eps2d, p [N,3], J [N,2,3]), nothing
    culled."""
    Rcw, t = viewmat[:3, :3], viewmat[:3, 3]
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    R = aa_ref.quat_to_rotmat(quats)
    M = R * scales[:, None, :]
    cov_c = Rcw @ (M @ M.transpose(1, 2)) @ Rcw.T
    p = means @ Rcw.T + t
    x, y, z = p.unbind(-1)
    m2x, m2y, J = cam_map(model, x, y, z, fx, fy, cx, cy, width, height)
    c2 = J @ cov_c @ J.transpose(1, 2)
    s00, s01, s11 = c2[:, 0, 0], c2[:, 0, 1], c2[:, 1, 1]
    a, c = s00 + eps2d, s11 + eps2d
    det = a * c - s01 * s01
    conics = torch.stack([c / det, -s01 / det, a / det], -1)
    return dict(means2d=torch.stack([m2x, m2y], -1), depths=z, conics=conics, comp=aa_ref.compensation(s00, s01, s11, eps2d),
                cov=(s00, s01, s11), p=p, J=J)


def _near(v, boundary):
    return np.abs(v - boundary) <= NEAR_TOL * np.maximum(1.0, np.abs(v))


def decide(pr, width, height, eps2d=0.3, near=0.01, far=1e10, radius_clip=0.0):
    """The integer decisions of a projection `pr` (project's dict), taken in its dtype: dict(radii int32 [N], tiles int32 [N],
    close bool [N]).  close: a value that decides lies within NEAR_TOL * max(1, |v|) of its boundary (near / far, det > 0, the
    radius' integer, radius_clip, off-screen, a tile edge)."""
    f = lambda t: t.detach().cpu().numpy()  # noqa: E731
    z = f(pr["depths"])
    dt = z.dtype.type
    s00, s01, s11 = (f(v) for v in pr["cov"])
    m2 = f(pr["means2d"])
    n = z.shape[0]
    in_depth = ~((z < dt(near)) | (z > dt(far)))
    close = _near(z, near) | _near(z, far)
    S00, S11 = s00 + dt(eps2d), s11 + dt(eps2d)
    det = S00 * S11 - s01 * s01
    close |= in_depth & _near(det, 0.0)
    ok = in_depth & (det > 0)
    hb = dt(0.5) * (S00 + S11)
    with np.errstate(invalid="ignore"):
        rf = dt(3.0) * np.sqrt(hb + np.sqrt(np.maximum(dt(0.01), hb * hb - det)))
    rf = np.where(ok, rf, 0).astype(z.dtype)
    radius = np.ceil(rf)
    close |= ok & _near(rf, np.round(rf))
    fw, fh = dt(width), dt(height)
    mx, my = m2[:, 0], m2[:, 1]
    off = (radius <= dt(radius_clip)) | (mx + radius <= 0) | (mx - radius >= fw) | (my + radius <= 0) | (my - radius >= fh)
    close |= ok & (_near(mx + radius, 0.0) | _near(mx - radius, width) | _near(my + radius, 0.0) | _near(my - radius, height))
    vis = ok & ~off
    tile_w, tile_h = (width + TILE - 1) // TILE, (height + TILE - 1) // TILE
    tiles = np.zeros(n, np.int32)
    edges = []
    lo_hi = []
    for m, lim in ((mx, tile_w), (my, tile_h)):
        lo_f, hi_f = (m - radius) / dt(TILE), (m + radius) / dt(TILE)
        edges += [lo_f, hi_f]
        lo_hi.append((np.clip(np.floor(lo_f), 0, lim), np.clip(np.ceil(hi_f), 0, lim)))
    with np.errstate(invalid="ignore"):
        cnt = (lo_hi[1][1] - lo_hi[1][0]) * (lo_hi[0][1] - lo_hi[0][0])
    tiles[vis] = cnt[vis].astype(np.int32)
    for e in edges:
        close |= vis & _near(e, np.round(e))
    radii = np.where(vis, radius, 0).astype(np.int32)
    return dict(radii=radii, tiles=tiles, close=close)


def outputs(pr, dec):
    """What the kernel writes: numpy (means2d, depths, conics, comp) with culled rows zero."""
    vis = dec["radii"] > 0
    out = {}
    for k in ("means2d", "depths", "conics", "comp"):
        a = pr[k].detach().cpu().numpy().copy()
        a[~vis] = 0
        out[k] = a
    return out


def run(model, s, width, height, dtype, *, raw=False, modifier=1.0, grad=False, dev="cpu", viewmat=None, **cull):
    """project + decide on a scene dict in `dtype`: (pr, dec, leaves).  raw: the stored parameters s["raw"] through torch's
    getters (exp * modifier, F.normalize, sigmoid) in `dtype`; leaves then carries xyz, rotation, scaling_log, opacity_logit."""
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
    pr = project(model, L["means"], q, sc, vm, tm(s["K"]), width, height, eps2d=eps2d)
    dec = decide(pr, width, height, eps2d=eps2d, near=cull.get("near_plane", 0.01), far=cull.get("far_plane", 1e10),
                 radius_clip=cull.get("radius_clip", 0.0))
    return pr, dec, L


def project_loss(pr, radii, cot, *, antialiased, opac_act=None):
    """sum over Gaussians with radii > 0 of <cotangent, output>; cot = dict(means2d, depths | None, conics, comp | None (AA,
    activated parameters), opacities | None (raw: the cotangent of the -- compensated, with AA -- activated opacity))."""
    t = lambda a: torch.tensor(np.asarray(a), dtype=pr["depths"].dtype, device=pr["depths"].device)  # noqa: E731
    vis = torch.as_tensor(np.asarray(radii) > 0, device=pr["depths"].device)
    loss = (pr["means2d"] * t(cot["means2d"]))[vis].sum() + (pr["conics"] * t(cot["conics"]))[vis].sum()
    if cot.get("depths") is not None:
        loss = loss + (pr["depths"] * t(cot["depths"]))[vis].sum()
    if opac_act is not None and cot.get("opacities") is not None:
        if antialiased:   # a culled Gaussian's compensation is 0
            loss = loss + (opac_act * pr["comp"] * t(cot["opacities"]))[vis].sum()
        else:             # the opacity's gradient is not gated by radii
            loss = loss + (opac_act * t(cot["opacities"])).sum()
    elif antialiased and cot.get("comp") is not None:
        loss = loss + (pr["comp"] * t(cot["comp"]))[vis].sum()
    return loss


def ortho_kernel_order(means, quats, scales, viewmat, K, width, height, eps2d=0.3, near=0.01, far=1e10, radius_clip=0.0):
    """The orthographic forward in the kernel's operation order, numpy float32 on the CPU, one rounding per operation:
    dict(radii, tiles, means2d, depths, conics, comp) as the kernel writes them (culled rows zero).  quats / scales are the
    ACTIVATED parameters (for the RAW variants: torch's getters, which the kernel reproduces bit for bit).  numpy, not torch:
    torch.sqrt on float32 CPU tensors is not correctly rounded on every host (on the MI355X host 15 % of 1e5 values differed from
    numpy's by an ulp, which the determinant's cancellation turned into 1e-4 on the conics), numpy's is."""
    f = np.float32
    A32 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=f))  # noqa: E731
    means, q, sc, vm, K = A32(means), A32(quats), A32(scales), A32(viewmat), A32(K)
    eps2d, near, far, radius_clip = f(eps2d), f(near), f(far), f(radius_clip)
    one, two, three, half = f(1), f(2), f(3), f(0.5)
    px, py, pz = means[:, 0], means[:, 1], means[:, 2]
    Rc, tc = vm[:3, :3], vm[:3, 3]
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    x, y, z = (((Rc[r, 0] * px + Rc[r, 1] * py) + Rc[r, 2] * pz) + tc[r] for r in range(3))
    qw, qx, qy, qz = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    inv_norm = one / np.sqrt(((qx * qx + qy * qy) + qz * qz) + qw * qw)
    qw, qx, qy, qz = qw * inv_norm, qx * inv_norm, qy * inv_norm, qz * inv_norm
    x2, y2, z2, xy, xz, yz, wx, wy, wz = qx * qx, qy * qy, qz * qz, qx * qy, qx * qz, qy * qz, qw * qx, qw * qy, qw * qz
    R = [[one - two * (y2 + z2), two * (xy - wz), two * (xz + wy)],
         [two * (xy + wz), one - two * (x2 + z2), two * (yz - wx)],
         [two * (xz - wy), two * (yz + wx), one - two * (x2 + y2)]]
    M = [[R[r][c] * sc[:, c] for c in range(3)] for r in range(3)]
    C = [[(M[r][0] * M[c][0] + M[r][1] * M[c][1]) + M[r][2] * M[c][2] for c in range(3)] for r in range(3)]   # (symmetric)
    A = [[(Rc[r, 0] * C[0][c] + Rc[r, 1] * C[1][c]) + Rc[r, 2] * C[2][c] for c in range(3)] for r in range(3)]
    V = [[(A[r][0] * Rc[c, 0] + A[r][1] * Rc[c, 1]) + A[r][2] * Rc[c, 2] for c in range(3)] for r in range(3)]
    v00, v01, v02, v11, v12, v22 = V[0][0], V[0][1], V[0][2], V[1][1], V[1][2], V[2][2]
    zero = np.zeros_like(z)
    j00, j02, j11, j12 = fx + zero, zero, fy + zero, zero
    b00, b01, b02 = j00 * v00 + j02 * v02, j00 * v01 + j02 * v12, j00 * v02 + j02 * v22
    b11, b12 = j11 * v11 + j12 * v12, j11 * v12 + j12 * v22
    s00o, s01, s11o = b00 * j00 + b02 * j02, b01 * j11 + b02 * j12, b11 * j11 + b12 * j12
    m2x, m2y = fx * x + cx, fy * y + cy
    det_o = s00o * s11o - s01 * s01
    s00, s11 = s00o + eps2d, s11o + eps2d
    det = s00 * s11 - s01 * s01
    with np.errstate(all="ignore"):
        inv_det = one / det
        hb = half * (s00 + s11)
        v1 = hb + np.sqrt(np.maximum(f(0.01), hb * hb - det))
        radius = np.ceil(three * np.sqrt(v1))
        fw, fh = f(width), f(height)
        off = (radius <= radius_clip) | (m2x + radius <= 0) | (m2x - radius >= fw) | (m2y + radius <= 0) | (m2y - radius >= fh)
        vis = ~((z < near) | (z > far)) & (det > 0) & ~off
        tile_w, tile_h = f((width + TILE - 1) // TILE), f((height + TILE - 1) // TILE)
        tr, tx, ty = radius / f(TILE), m2x / f(TILE), m2y / f(TILE)
        x0, x1 = np.minimum(np.maximum(np.floor(tx - tr), 0), tile_w), np.minimum(np.maximum(np.ceil(tx + tr), 0), tile_w)
        y0, y1 = np.minimum(np.maximum(np.floor(ty - tr), 0), tile_h), np.minimum(np.maximum(np.ceil(ty + tr), 0), tile_h)
        comp = np.sqrt(np.maximum(f(0), det_o / det))
        Z = lambda t: np.where(vis, t, f(0)).astype(f)  # noqa: E731
        out = dict(radii=Z(radius).astype(np.int32), tiles=Z((y1 - y0) * (x1 - x0)).astype(np.int32),
                   means2d=np.stack([Z(m2x), Z(m2y)], -1), depths=Z(z),
                   conics=np.stack([Z(s11 * inv_det), Z(-s01 * inv_det), Z(s00 * inv_det)], -1), comp=Z(comp))
    assert all(v.dtype in (np.float32, np.int32) for v in out.values())
    return out


def cam_bwd_np(model, fx, fy, x, y, z, vm2, vJ, v_depths):
    """cam_bwd of csrc/project.hip for "ortho" and "fisheye" in numpy float64: (v_means2d [N,2], vJ [N,2,3]) -> vp [N,3]."""
    n = x.shape[0]
    vd = np.zeros(n) if v_depths is None else np.asarray(v_depths, np.float64)
    if model == "ortho":
        return np.stack([fx * vm2[:, 0], fy * vm2[:, 1], vd], -1)
    assert model == "fisheye"
    eps = FISHEYE_EPS
    r0 = np.sqrt(x * x + y * y)
    rho, zt = r0 + eps, z + eps
    theta = np.arctan2(rho, zt)
    k = theta / rho
    x2, y2, xy = x * x + eps, y * y, x * y
    s, z2 = x2 + y2, z * z
    l2 = s + z2
    tb = np.arctan2(rho, z)
    b, a = tb / rho / s, z / (l2 * s)
    v_k = fx * x * vm2[:, 0] + fy * y * vm2[:, 1]
    vx, vy, vz = fx * k * vm2[:, 0], fy * k * vm2[:, 1], vd.copy()
    v_theta = v_k / rho
    v_rho = -v_k * k / rho
    g00, g01, g02 = fx * vJ[:, 0, 0], fx * vJ[:, 0, 1], fx * vJ[:, 0, 2]
    g10, g11, g12 = fy * vJ[:, 1, 0], fy * vJ[:, 1, 1], fy * vJ[:, 1, 2]
    gx = g01 + g10
    v_x2, v_y2 = g00 * a + g11 * b, g00 * b + g11 * a
    v_a = g00 * x2 + g11 * y2 + gx * xy
    v_b = g00 * y2 + g11 * x2 - gx * xy
    v_xy = gx * (a - b)
    vx = vx - g02 / l2
    vy = vy - g12 / l2
    v_l2 = (g02 * x + g12 * y) / (l2 * l2)
    vz = vz + v_a / (l2 * s)
    v_l2 = v_l2 - v_a * a / l2
    v_s = -v_a * a / s
    v_tb = v_b / (rho * s)
    v_rho = v_rho - v_b * b / rho
    v_s = v_s - v_b * b / s
    hb = rho * rho + z2
    v_rho = v_rho + v_tb * z / hb
    vz = vz - v_tb * rho / hb
    v_s = v_s + v_l2
    vz = vz + 2 * z * v_l2
    v_x2, v_y2 = v_x2 + v_s, v_y2 + v_s
    vx = vx + 2 * x * v_x2 + y * v_xy
    vy = vy + 2 * y * v_y2 + x * v_xy
    ht = rho * rho + zt * zt
    v_rho = v_rho + v_theta * zt / ht
    vz = vz - v_theta * rho / ht
    safe = np.where(r0 > 0, r0, 1.0)
    vx = vx + np.where(r0 > 0, v_rho * x / safe, 0.0)
    vy = vy + np.where(r0 > 0, v_rho * y / safe, 0.0)
    return np.stack([vx, vy, vz], -1)


def bwd_terms(model, s, width, height, radii, v_means2d, v_depths, v_conics, v_comp=None, *, antialiased=False, eps2d=0.3):
    """What project_bwd_kernel<.., CAM> computes per Gaussian up to the camera-space cotangents, in numpy float64 by hand:
    dict(v_means [N,3] = Rcw^T vp, pose [N,12] as tests/pose_ref.py::pose_terms lays it out); zero rows where radii <= 0."""
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
    _, _, J = cam_map(model, t(x), t(y), t(z), t(fx), t(fy), t(cx), t(cy), width, height)
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
    vp = cam_bwd_np(model, fx, fy, x, y, z, f(v_means2d), vJ, v_depths)
    vR = vp[:, :, None] * mu[:, None, :] + (GSc + GSc.transpose(0, 2, 1)) @ A
    pose = np.concatenate([vR, vp[:, :, None]], axis=2).reshape(n, 12)
    v_means = vp @ Rc
    cull = np.asarray(radii) <= 0
    pose[cull] = 0.0
    v_means[cull] = 0.0
    return dict(v_means=v_means, pose=pose)


# -- scenes ---------------------------------------------------------------------------------------------------------------------

def intrinsics(model, width, height):
    """A K for `model` at an image size: fx != fy, principal point off-centre.  fisheye: 88 degrees off axis lands inside the
    image's width (fx = 0.30 W pixels per radian); ortho: the image spans about 9 x 8 H/W world units."""
    if model == "fisheye":
        fx, fy = 0.30 * width, 0.33 * width
    elif model == "ortho":
        fx, fy = width / 9.0, width / 8.0
    else:
        fx, fy = 0.94 * width, 0.70 * width
    return np.array([[fx, 0, 0.48 * width], [0, fy, 0.53 * height], [0, 0, 1]], np.float32)


def model_scene(model, n, d, width, height, seed, cam="pitch_roll", max_deg=88.0, scale_mult=60.0, behind=0.08):
    """A scene dict (as helpers.general_scene's) laid out for `model` in front of a general pose (GENERAL_CAMERAS[cam]'s yaw,
    pitch, roll and centre).  fisheye: off-axis angle uniform in [0, max_deg], any azimuth, distance 2..12; ortho: x, y uniform
    over 1.5 x the image's world extent, z in 0..12.5 (dense near 0); scales log-uniform over one decade below scale_mult x synthetic.SCALE0.
    `behind`: the share of Gaussians put behind the camera.  Gaussians outside
    the image follow from the layout (the image is wider than high; ortho: the 1.5)."""
    c = GENERAL_CAMERAS[cam]
    R = _ypr_rotation(*c["ypr"])
    C = np.asarray(c["centre"], np.float64)
    vm = np.eye(4)
    vm[:3, :3] = R.T
    vm[:3, 3] = -R.T @ C
    K = intrinsics(model, width, height)
    p = syn.make_gaussians(n, d, width, height, seed=seed, scale0=syn.SCALE0 * scale_mult)
    g = torch.Generator(device="cpu")
    g.manual_seed(seed + 104729)
    u = torch.rand(n, 5, generator=g, dtype=torch.float64).numpy()
    back = u[:, 3] < behind
    # sizes over one decade, so that some Gaussians fall below a radius_clip of a few pixels
    p["scaling_log"] = p["scaling_log"] - torch.from_numpy(math.log(10.0) * u[:, 4:5]).float()
    dist = 2.0 + 10.0 * u[:, 2]
    if model == "fisheye":
        th = np.where(back, np.radians(95.0 + 80.0 * u[:, 0]), np.radians(max_deg) * u[:, 0])
        ph = 2 * math.pi * u[:, 1]
        pc = dist[:, None] * np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], 1)
    else:
        fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
        px = 0.5 * width + (u[:, 0] - 0.5) * 1.5 * width
        py = 0.5 * height + (u[:, 1] - 0.5) * 1.5 * height
        z = np.where(back, -dist, 12.5 * u[:, 2] ** 2 if model == "ortho" else dist)
        if model == "ortho":
            pc = np.stack([(px - cx) / fx, (py - cy) / fy, z], 1)
        else:
            pc = np.stack([(px - cx) / fx * z, (py - cy) / fy * z, z], 1)
    p["xyz"] = torch.from_numpy((pc @ R.T + C).astype(np.float32))
    return dict(means=p["xyz"].numpy(), quats=torch.nn.functional.normalize(p["rotation"]).numpy(),
                scales=p["scaling_log"].exp().numpy(), opacities=torch.sigmoid(p["opacity_logit"]).reshape(-1).numpy(),
                colors=None if d == 0 else p["semantic_feature"].numpy(),
                sh=torch.cat([p["features_dc"], p["features_rest"]], dim=1).numpy(),
                viewmat=vm.astype(np.float32), K=K, raw=p, R=R, C=C)


def off_axis_deg(s):
    """Off-axis angle of every Gaussian's centre in the camera frame, degrees."""
    vm = s["viewmat"].astype(np.float64)
    p = s["means"].astype(np.float64) @ vm[:3, :3].T + vm[:3, 3]
    return np.degrees(np.arctan2(np.hypot(p[:, 0], p[:, 1]), p[:, 2]))


def cotangents(n, seed):
    rng = np.random.default_rng(seed + 500)
    return dict(means2d=rng.standard_normal((n, 2)).astype(np.float32), depths=rng.standard_normal(n).astype(np.float32),
                conics=rng.standard_normal((n, 3)).astype(np.float32), comp=rng.standard_normal(n).astype(np.float32),
                opacities=rng.standard_normal(n).astype(np.float32))


# kernel-level cases shared by the CPU and the GPU tests: (model, seed, culling parameters)
KERNEL_SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 700)
KERNEL_CULL = dict(eps2d=0.3, near_plane=0.2, far_plane=11.0, radius_clip=3.0)   # (88 degrees off axis at distance 12: z = 0.42)
KERNEL_W, KERNEL_H = 97, 61
KERNEL_SEEDS = {"fisheye": 11, "ortho": 12}
