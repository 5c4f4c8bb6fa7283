"""Reference for the intrinsics' gradients of N23 (include/gags_raster.h, "gags_project_bwd_calib", has the
rule).  TEST INFRASTRUCTURE ONLY.

The truth is float64 autograd through the declared forward: tests/camera_models_ref.py::cam_map for "pinhole", "ortho" and
"fisheye", tests/fisheye_kb_ref.py::cam_map with coefficients.  Every Gaussian gets ITS OWN copy of (fx, fy, cx, cy, k1 .. k4)
as a leaf [N,8], so that one backward gives the per-Gaussian terms: their sum over N is the reference, the sum of their
absolute values the normaliser.  error(got) = |got - ref64| / sum_i |term_i| per entry: cancellation among random cotangents
cannot inflate it and a small entry cannot hide behind a large one.  Everything follows `dtype`; the same code in float32 on
the CPU is the yardstick.

`project_grads` is the projection alone under cm.project_loss (the kernel-level tests); `full` the oracle-style composition
the pose tests use -- projection, SH colours, depth channel, aa_ref.composite, ED division -- with the integer decisions
(radii, depth order) handed in and the blend set of the float64 run."""
import numpy as np
import torch

import aa_ref
import camera_models_ref as cm
import fisheye_kb_ref as kb
from oracle import dense_ref

ENTRIES = ("fx", "fy", "cx", "cy", "k1", "k2", "k3", "k4")


def intrinsics_leaf(K, coeffs, n, dtype, dev="cpu"):
    """[N,8] leaf: every row (fx, fy, cx, cy, k1 .. k4) from K [3,3] and coeffs [4] (None: zeros, and the plain model is used)."""
    K = np.asarray(K, np.float32).reshape(3, 3)
    c = np.zeros(4, np.float32) if coeffs is None else kb.coeffs32(coeffs)
    row = np.concatenate([[K[0, 0], K[1, 1], K[0, 2], K[1, 2]], c]).astype(np.float32)
    return torch.tensor(np.repeat(row[None], n, 0), dtype=dtype, device=dev, requires_grad=True)


def project(model, with_coeffs, means, quats, scales, viewmat, P, width, height, eps2d=0.3):
    """cm.project's dict with per-Gaussian intrinsics P [N,8]; with_coeffs: the fisheye of N21 (kb.cam_map) on P[:, 4:]."""
    Rcw, t = viewmat[:3, :3], viewmat[:3, 3]
    fx, fy, cx, cy = P[:, 0], P[:, 1], P[:, 2], P[:, 3]
    R = aa_ref.quat_to_rotmat(quats)
    M = R * scales[:, None, :]
    cov_c = Rcw @ (M @ M.transpose(1, 2)) @ Rcw.T
    p = means @ Rcw.T + t
    x, y, z = p.unbind(-1)
    if with_coeffs:
        assert model == "fisheye"
        m2x, m2y, J, _ = kb.cam_map(tuple(P[:, 4 + j] for j in range(4)), x, y, z, fx, fy, cx, cy)
    else:
        m2x, m2y, J = cm.cam_map(model, x, y, z, fx, fy, cx, cy, width, height)
    c2 = J @ cov_c @ J.transpose(1, 2)
    s00, s01, s11 = c2[:, 0, 0], c2[:, 0, 1], c2[:, 1, 1]
    a, c = s00 + eps2d, s11 + eps2d
    det = a * c - s01 * s01
    conics = torch.stack([c / det, -s01 / det, a / det], -1)
    return dict(means2d=torch.stack([m2x, m2y], -1), depths=z, conics=conics, comp=aa_ref.compensation(s00, s01, s11, eps2d),
                cov=(s00, s01, s11), p=p, J=J)


def _leaves(s, dtype, dev, raw, modifier=1.0, grad=False):
    def tm(a, rg=False):
        return torch.tensor(np.asarray(a), dtype=dtype, device=dev, requires_grad=rg)
    if raw:
        L = dict(means=tm(s["raw"]["xyz"], grad), quats=tm(s["raw"]["rotation"], grad), scales=tm(s["raw"]["scaling_log"], grad),
                 opacities=tm(s["raw"]["opacity_logit"].reshape(-1), grad))
        q, sc, op = torch.nn.functional.normalize(L["quats"]), torch.exp(L["scales"]) * modifier, torch.sigmoid(L["opacities"])
    else:
        L = dict(means=tm(s["means"], grad), quats=tm(s["quats"], grad), scales=tm(s["scales"], grad),
                 opacities=tm(s["opacities"], grad))
        q, sc, op = L["quats"], L["scales"], L["opacities"]
    L["viewmat"] = tm(s["viewmat"], grad)
    return L, q, sc, op


def _result(P, with_coeffs, L=None):
    terms = P.grad.detach().cpu().numpy().astype(np.float64)
    if not with_coeffs:
        terms = terms[:, :4]
    res = dict(terms=terms, sum=terms.sum(0), norm=np.abs(terms).sum(0))
    if L is not None:
        res["g"] = {k: v.grad.detach().cpu().numpy() for k, v in L.items() if v.grad is not None}
    return res


def project_grads(model, coeffs, s, width, height, radii, cot, *, antialiased, raw=False, dtype=torch.float64, dev="cpu",
                  eps2d=0.3):
    """d cm.project_loss / d the per-Gaussian intrinsics: dict(terms [N,4 or 8], sum, norm), columns in ENTRIES' order.  The
    loss runs over the Gaussians with radii > 0 (the HIP forward's): a culled Gaussian's row is exactly zero."""
    L, q, sc, op = _leaves(s, dtype, dev, raw)
    n = L["means"].shape[0]
    P = intrinsics_leaf(s["K"], coeffs, n, dtype, dev)
    pr = project(model, coeffs is not None, L["means"], q, sc, L["viewmat"], P, width, height, eps2d=eps2d)
    c = {k: (None if v is None else v[:n]) for k, v in cot.items()}
    loss = cm.project_loss(pr, radii, c, antialiased=antialiased, opac_act=op if raw else None)
    loss.backward()
    return _result(P, coeffs is not None)


def project_loss_at(model, with_coeffs, s, width, height, radii, cot, x, *, antialiased, raw=False, eps2d=0.3):
    """cm.project_loss in float64 with ONE shared set of intrinsics x = (fx, fy, cx, cy[, k1 .. k4]): the function whose
    central differences the summed per-Gaussian gradient is checked against."""
    with torch.no_grad():
        L, q, sc, op = _leaves(s, torch.float64, "cpu", raw)
        n = L["means"].shape[0]
        row = np.concatenate([np.asarray(x, np.float64), np.zeros(8 - len(x))])
        P = torch.tensor(np.repeat(row[None], n, 0), dtype=torch.float64)
        pr = project(model, with_coeffs, L["means"], q, sc, L["viewmat"], P, width, height, eps2d=eps2d)
        c = {k: (None if v is None else v[:n]) for k, v in cot.items()}
        return float(cm.project_loss(pr, radii, c, antialiased=antialiased, opac_act=op if raw else None))


def full(model, coeffs, s, width, height, colors, bg, v_out, v_alpha, radii, depths, *, raw=False, antialiased=False,
         render_mode="RGB", sh_degree=None, dtype=torch.float64, dev="cpu", include=None, scene_grad=True):
    """The whole render differentiated with respect to the per-Gaussian intrinsics (and, scene_grad, the scene and the pose):
    dict(terms, sum, norm, g, out, include)."""
    def tm(a, rg=False):
        return torch.tensor(np.asarray(a), dtype=dtype, device=dev, requires_grad=rg)
    L, q, sc, op = _leaves(s, dtype, dev, raw, grad=scene_grad)
    n = L["means"].shape[0]
    P = intrinsics_leaf(s["K"], coeffs, n, dtype, dev)
    pr = project(model, coeffs is not None, L["means"], q, sc, L["viewmat"], P, width, height)
    vis = torch.as_tensor(np.asarray(radii) > 0, device=dev)
    if antialiased:
        op = op * torch.where(vis, pr["comp"], torch.zeros_like(pr["comp"]))
    C = tm(colors, scene_grad)
    cols = C if sh_degree is None else dense_ref.sh_colors(sh_degree, C, L["means"], torch.inverse(L["viewmat"])[:3, 3])
    bgt = tm(bg)
    if render_mode in ("RGB+D", "RGB+ED"):
        cols = torch.cat([cols, pr["depths"][:, None]], dim=1)
        bgt = torch.cat([bgt, torch.zeros(1, dtype=dtype, device=dev)])
    order = np.lexsort((np.arange(n), np.asarray(depths)))
    out, alphas, aux = aa_ref.composite(pr["means2d"], pr["conics"], op, cols, bgt, width, height, radii, order, include=include)
    if render_mode == "RGB+ED":
        out = torch.cat([out[..., :-1], out[..., -1:] / alphas[..., None].clamp(min=1e-10)], dim=-1)
    ((out * tm(v_out)).sum() + (alphas * tm(v_alpha)).sum()).backward()
    res = _result(P, coeffs is not None, dict(L, colors=C))
    res.update(out=out.detach().cpu().numpy(), include=aux["include"])
    return res


def from_kernel(v_K, v_coeffs=None):
    """The kernel's v_K [9] (row-major 3 x 3) and v_coeffs [4] in ENTRIES' order."""
    k = np.asarray(v_K, np.float64).reshape(9)
    head = np.array([k[0], k[4], k[2], k[5]])
    return head if v_coeffs is None else np.concatenate([head, np.asarray(v_coeffs, np.float64).reshape(4)])


def entry_errors(got, ref):
    """|got - ref64| / sum_i |term_i| per entry (0 where no Gaussian contributes anything to the entry: then got must be 0)."""
    got = np.asarray(got, np.float64)
    d = np.abs(got - ref["sum"])
    return np.where(ref["norm"] > 0, d / np.where(ref["norm"] > 0, ref["norm"], 1.0), np.where(d == 0, 0.0, np.inf))


def central_difference(f, x0, h):
    """(f(x0 + h e_k) - f(x0 - h e_k)) / 2 h for every k of the flat float64 vector x0."""
    x0 = np.asarray(x0, np.float64)
    out = np.zeros_like(x0)
    for k in range(x0.size):
        e = np.zeros_like(x0)
        e[k] = h
        out[k] = (f(x0 + e) - f(x0 - e)) / (2 * h)
    return out
