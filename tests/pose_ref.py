"""Reference for the camera pose gradient of N17.  TEST INFRASTRUCTURE ONLY.

`full` is tests/aa_ref.py's project + composite (+ oracle/dense_ref.py's sh_colors, the depth channel and the ED division, as
tests/test_general_camera_gpu.py::dense_full states them) with `viewmat` as a LEAF: torch differentiates the whole render with
respect to the 4 x 4.  Everything follows `dtype`, so the same code run in float32 on the CPU is the yardstick the GPU tests
measure the kernels against.  The integer decisions come from elsewhere, as in N16: radii and depth order from the fp32 oracle,
the blend set from the float64 run (`include`).

`pose_terms` is a numpy float64 restatement of what project_bwd_kernel<.., POSE> adds per Gaussian: hand-written chain rule,
no autograd, so that the formula the kernel implements is checked on the CPU before any GPU run."""
import numpy as np
import torch

import aa_ref
from oracle import dense_ref


def project_loss(s, w, h, radii, cot, *, antialiased, dtype=torch.float64, dev="cpu", eps2d=0.3, viewmat=None):
    """Projection only: sum over Gaussians with radii > 0 of <cotangent, output> for cot = dict(means2d [N,2], depths [N] or
    None, conics [N,3], comp [N] or None).  Returns (loss, leaves) with leaves = dict(viewmat, means, quats, scales)."""
    def tm(a, rg=False):
        return torch.tensor(np.asarray(a), dtype=dtype, device=dev, requires_grad=rg)
    L = dict(viewmat=tm(s["viewmat"] if viewmat is None else viewmat, True), means=tm(s["means"], True),
             quats=tm(s["quats"], True), scales=tm(s["scales"], True))
    m2, z, con, comp = aa_ref.project(L["means"], L["quats"], L["scales"], L["viewmat"], tm(s["K"]), w, h, eps2d=eps2d, radii=radii)
    vis = torch.as_tensor(np.asarray(radii) > 0, device=dev)
    loss = (m2 * tm(cot["means2d"]))[vis].sum() + (con * tm(cot["conics"]))[vis].sum()
    if cot.get("depths") is not None:
        loss = loss + (z * tm(cot["depths"]))[vis].sum()
    if antialiased and cot.get("comp") is not None:
        loss = loss + (comp * tm(cot["comp"]))[vis].sum()
    return loss, L


def project_grads(s, w, h, radii, cot, **kw):
    """d project_loss / d (viewmat [4,4], means, quats, scales), numpy."""
    loss, L = project_loss(s, w, h, radii, cot, **kw)
    loss.backward()
    return {k: t.grad.detach().cpu().numpy() for k, t in L.items()}


def render(s, w, h, colors, bg, radii, depths, *, viewmat, antialiased=False, render_mode="RGB", sh_degree=None,
           dtype=torch.float64, dev="cpu", include=None, eps2d=0.3, detach_campos=False, scene_grad=False):
    """One scene rendered in `dtype` with `viewmat` (a torch tensor, leaf or not) as the pose: (out [H,W,D'], alphas [H,W], aux,
    leaves).  colors: [N,D], or the SH coefficients [N,K,3] with sh_degree.  detach_campos: the SH view direction is cut off
    the pose (what a renderer without the campos gradient computes)."""
    def tm(a, rg=False):
        return torch.tensor(np.asarray(a), dtype=dtype, device=dev, requires_grad=rg)
    n = s["means"].shape[0]
    L = dict(means=tm(s["means"], scene_grad), quats=tm(s["quats"], scene_grad), scales=tm(s["scales"], scene_grad),
             opacities=tm(s["opacities"], scene_grad), colors=tm(colors, scene_grad))
    m2, z, con, comp = aa_ref.project(L["means"], L["quats"], L["scales"], viewmat, tm(s["K"]), w, h, eps2d=eps2d, radii=radii)
    op = L["opacities"] * comp if antialiased else L["opacities"]
    cols = L["colors"]
    if sh_degree is not None:
        campos = torch.inverse(viewmat)[:3, 3]
        cols = dense_ref.sh_colors(sh_degree, cols, L["means"], campos.detach() if detach_campos else campos)
    bgt = None if bg is None else tm(bg)
    if render_mode in ("RGB+D", "RGB+ED"):
        cols = torch.cat([cols, z[:, None]], dim=1)
        bgt = None if bgt is None else torch.cat([bgt, torch.zeros(1, dtype=dtype, device=dev)])
    elif render_mode in ("D", "ED"):
        cols = z[:, None]
        bgt = None if bgt is None else torch.zeros(1, dtype=dtype, device=dev)
    order = np.lexsort((np.arange(n), np.asarray(depths)))
    out, alphas, aux = aa_ref.composite(m2, con, op, cols, bgt, w, h, radii, order, include=include)
    if render_mode in ("ED", "RGB+ED"):
        out = torch.cat([out[..., :-1], out[..., -1:] / alphas[..., None].clamp(min=1e-10)], dim=-1)
    return out, alphas, aux, L


def full(s, w, h, colors, bg, v_out, v_alpha, radii, depths, *, dtype=torch.float64, dev="cpu", viewmat=None, **kw):
    """render + backward of <v_out, out> + <v_alpha, alphas>: dict(out, alphas, include, n_blend, g = dict(viewmat [4,4] and --
    scene_grad -- means, quats, scales, opacities, colors)), numpy."""
    vm = torch.tensor(np.asarray(s["viewmat"] if viewmat is None else viewmat), dtype=dtype, device=dev, requires_grad=True)
    out, alphas, aux, L = render(s, w, h, colors, bg, radii, depths, viewmat=vm, dtype=dtype, dev=dev, **kw)
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype, device=dev)  # noqa: E731
    ((out * t(v_out)).sum() + (alphas * t(v_alpha)).sum()).backward()
    g = dict(viewmat=vm.grad)
    g.update({k: v.grad for k, v in L.items() if v.grad is not None})
    return dict(out=out.detach().cpu().numpy(), alphas=alphas.detach().cpu().numpy(), include=aux["include"],
                n_blend=aux["n_blend"], g={k: v.detach().cpu().numpy() for k, v in g.items()})


def pose_terms(s, w, h, radii, v_means2d, v_depths, v_conics, v_comp=None, *, antialiased=False, eps2d=0.3):
    """What project_bwd_kernel<.., POSE> adds per Gaussian, restated in numpy float64: [N,12], entry 4 r + c the term of
    viewmat[r][c] (c = 3: the translation), zero rows where radii <= 0.
        v_t[r] = vp[r],   v_Rcw[r][c] = vp[r] mu[c] + sum_k (GSc[r][k] + GSc[k][r]) A[k][c],   A = Rcw Sigma
    with vp the cotangent of the camera-space point and GSc that of the camera-space covariance (both by hand below)."""
    f = lambda a: np.asarray(a, np.float64)  # noqa: E731
    mu, q, sc, vm, K = f(s["means"]), f(s["quats"]), f(s["scales"]), f(s["viewmat"]), f(s["K"])
    n = mu.shape[0]
    Rc, tc = vm[:3, :3], vm[:3, 3]
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    qw, qx, qy, qz = q.T
    R = np.stack([1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qw * qz), 2 * (qx * qz + qw * qy),
                  2 * (qx * qy + qw * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qw * qx),
                  2 * (qx * qz - qw * qy), 2 * (qy * qz + qw * qx), 1 - 2 * (qx * qx + qy * qy)], -1).reshape(n, 3, 3)
    M = R * sc[:, None, :]
    S3 = M @ M.transpose(0, 2, 1)
    A = Rc[None] @ S3
    Sc = A @ Rc.T[None]
    p = mu @ Rc.T + tc
    x, y, z = p.T
    rz = 1.0 / z
    rz2, rz3 = rz * rz, rz * rz * rz
    tanx, tany = 0.5 * w / fx, 0.5 * h / fy
    lxp, lxn = (w - cx) / fx + 0.3 * tanx, cx / fx + 0.3 * tanx
    lyp, lyn = (h - cy) / fy + 0.3 * tany, cy / fy + 0.3 * tany
    xr, yr = x * rz, y * rz
    x_in, y_in = (xr <= lxp) & (xr >= -lxn), (yr <= lyp) & (yr >= -lyn)
    tx, ty = z * np.clip(xr, -lxn, lxp), z * np.clip(yr, -lyn, lyp)
    J = np.zeros((n, 2, 3))
    J[:, 0, 0], J[:, 0, 2], J[:, 1, 1], J[:, 1, 2] = fx * rz, -fx * tx * rz2, fy * rz, -fy * ty * rz2
    c2 = J @ Sc @ J.transpose(0, 2, 1)
    s00o, s01, s11o = c2[:, 0, 0], c2[:, 0, 1], c2[:, 1, 1]
    s00, s11 = s00o + eps2d, s11o + eps2d
    det = s00 * s11 - s01 * s01
    ca, cb, cc = s11 / det, -s01 / det, s00 / det
    vcon = f(v_conics)
    X = np.stack([ca, cb, cb, cc], -1).reshape(n, 2, 2)
    Gx = np.stack([vcon[:, 0], 0.5 * vcon[:, 1], 0.5 * vcon[:, 1], vcon[:, 2]], -1).reshape(n, 2, 2)
    G = -(X @ Gx @ X)                                     # conic = inverse(cov2d): G = -X Gx X
    if antialiased and v_comp is not None:
        r = (s00o * s11o - s01 * s01) / det
        comp = np.sqrt(np.maximum(0.0, r))
        v_r = np.where(comp > 0, f(v_comp) / (2 * np.where(comp > 0, comp, 1.0)), 0.0)
        e = eps2d / det
        G[:, 0, 0] += v_r * ((1 - r) * ca - e)
        G[:, 1, 1] += v_r * ((1 - r) * cc - e)
        G[:, 0, 1] += v_r * (1 - r) * cb
        G[:, 1, 0] += v_r * (1 - r) * cb
    GSc = J.transpose(0, 2, 1) @ G @ J                    # cov2d = J Sc J^T
    vJ = G @ J @ Sc.transpose(0, 2, 1) + G.transpose(0, 2, 1) @ J @ Sc
    vm2 = f(v_means2d)
    vp = np.zeros((n, 3))
    vp[:, 0] = fx * rz * vm2[:, 0]
    vp[:, 1] = fy * rz * vm2[:, 1]
    vp[:, 2] = -(fx * x * vm2[:, 0] + fy * y * vm2[:, 1]) * rz2
    if v_depths is not None:
        vp[:, 2] += f(v_depths)
    # J[0][2] = -fx tx / z^2 with tx = x inside the clamp, = z * limit outside (then a function of z alone)
    vp[:, 0] += np.where(x_in, -fx * rz2 * vJ[:, 0, 2], 0.0)
    vp[:, 2] += np.where(x_in, 0.0, -fx * rz3 * vJ[:, 0, 2] * tx)
    vp[:, 1] += np.where(y_in, -fy * rz2 * vJ[:, 1, 2], 0.0)
    vp[:, 2] += np.where(y_in, 0.0, -fy * rz3 * vJ[:, 1, 2] * ty)
    vp[:, 2] += -fx * rz2 * vJ[:, 0, 0] - fy * rz2 * vJ[:, 1, 1] + 2 * fx * tx * rz3 * vJ[:, 0, 2] + 2 * fy * ty * rz3 * vJ[:, 1, 2]
    vR = vp[:, :, None] * mu[:, None, :] + (GSc + GSc.transpose(0, 2, 1)) @ A
    out = np.concatenate([vR, vp[:, :, None]], axis=2).reshape(n, 12)
    out[np.asarray(radii) <= 0] = 0.0
    return out


def rel_err(got, ref):
    """|| got - ref || / || ref || over all entries (the 12, or 16, numbers of a pose gradient)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))
