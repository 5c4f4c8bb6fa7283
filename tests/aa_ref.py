"""Float64 torch restatement of the two rasterizer options of N16 (include/gags_raster.h has the rules): the antialiased
opacity compensation and absgrad.  TEST INFRASTRUCTURE ONLY.  `project` and `composite` are oracle/dense_ref.py's, restated
with the compensation as a fourth output of the projection and with the per-(pixel, Gaussian) offsets dx, dy kept as [P,N]
tensors that retain their gradient: d loss / d dx[p, n] IS pixel p's term of v_means2d[n].x over all channels, so absgrad is
the sum over pixels of its absolute value.  Everything follows the dtype of its inputs, so the same code run in float32 on
the CPU is the yardstick the GPU tests measure the kernels against.  The integer decisions (radii, depth order) come from
the fp32 oracle, as in tests/test_general_camera_gpu.py::dense_full."""
import numpy as np
import torch

TILE = 16


def quat_to_rotmat(q):
    q = q / q.norm(dim=-1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    R = torch.stack([
        1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=-1)
    return R.reshape(-1, 3, 3)


def cov2d(means, quats, scales, viewmat, K, width, height):
    """(s00, s01, s11) BEFORE eps2d, camera-space point (x, y, z) and (fx, fy, cx, cy)."""
    Rcw, t = viewmat[:3, :3], viewmat[:3, 3]
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    R = quat_to_rotmat(quats)
    M = R * scales[:, None, :]
    cov = M @ M.transpose(1, 2)
    p = means @ Rcw.T + t
    cov_c = Rcw @ cov @ Rcw.T
    x, y, z = p.unbind(-1)
    tanx, tany = 0.5 * width / fx, 0.5 * height / fy
    lxp, lxn = (width - cx) / fx + 0.3 * tanx, cx / fx + 0.3 * tanx
    lyp, lyn = (height - cy) / fy + 0.3 * tany, cy / fy + 0.3 * tany
    rz = 1.0 / z
    tx = z * torch.minimum(lxp, torch.maximum(-lxn, x * rz))
    ty = z * torch.minimum(lyp, torch.maximum(-lyn, y * rz))
    zero = torch.zeros_like(z)
    J = torch.stack([fx * rz, zero, -fx * tx * rz * rz, zero, fy * rz, -fy * ty * rz * rz], -1).reshape(-1, 2, 3)
    c2 = J @ cov_c @ J.transpose(1, 2)
    return (c2[:, 0, 0], c2[:, 0, 1], c2[:, 1, 1]), (x, y, z), (fx, fy, cx, cy)


def compensation(s00, s01, s11, eps2d):
    """comp = sqrt(max(0, det_o / det_b)) of the covariance before the blur; no constant in the divisor."""
    det_o = s00 * s11 - s01 * s01
    det_b = (s00 + eps2d) * (s11 + eps2d) - s01 * s01
    r = det_o / det_b
    pos = r > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, r, torch.ones_like(r))), torch.zeros_like(r))


def compensation_partials(s00, s01, s11, eps2d):
    """The backward's closed form: (r, d r / d s00, d r / d s11, d r / d s01) with r = det_o / det_b and (a, b, c) the conic."""
    S00, S11 = s00 + eps2d, s11 + eps2d
    det_b = S00 * S11 - s01 * s01
    a, b, c = S11 / det_b, -s01 / det_b, S00 / det_b
    r = (s00 * s11 - s01 * s01) / det_b
    return r, (1 - r) * a - eps2d / det_b, (1 - r) * c - eps2d / det_b, 2 * (1 - r) * b


def project(means, quats, scales, viewmat, K, width, height, eps2d=0.3, radii=None):
    """dense_ref.project with the compensation: (means2d, z, conics, comp).  No culling except that comp is 0 where
    radii == 0 (when radii are given): the caller masks the rest with the oracle's radii."""
    (s00, s01, s11), (x, y, z), (fx, fy, cx, cy) = cov2d(means, quats, scales, viewmat, K, width, height)
    a, b, c = s00 + eps2d, s01, s11 + eps2d
    det = a * c - b * b
    conics = torch.stack([c / det, -b / det, a / det], -1)
    rz = 1.0 / z
    means2d = torch.stack([fx * x * rz + cx, fy * y * rz + cy], -1)
    comp = compensation(s00, s01, s11, eps2d)
    if radii is not None:
        vis = torch.as_tensor(np.asarray(radii) > 0, device=comp.device)
        comp = torch.where(vis, comp, torch.zeros_like(comp))
    return means2d, z, conics, comp


def composite(means2d, conics, opacities, colors, backgrounds, width, height, radii, order, include=None):
    """dense_ref.composite with dx, dy kept.  Returns (out [H,W,D], alphas [H,W], aux): aux["include"] = the [P,N] blend
    decisions (columns in depth order), aux["dx"], aux["dy"] = the [P,N] offsets with retain_grad(), aux["order"], aux["n_blend"].
    include given: the blend decisions of another run (a float32 evaluation takes the float64 run's)."""
    dev, dt = means2d.device, means2d.dtype
    order_t = torch.as_tensor(np.asarray(order), dtype=torch.long, device=dev)
    m2, cn, op, col = means2d[order_t], conics[order_t], opacities[order_t], colors[order_t]
    ii, jj = torch.meshgrid(torch.arange(height, device=dev), torch.arange(width, device=dev), indexing="ij")
    ii, jj = ii.reshape(-1), jj.reshape(-1)
    px, py = jj.to(dt) + 0.5, ii.to(dt) + 0.5
    dx = m2[None, :, 0] - px[:, None]
    dy = m2[None, :, 1] - py[:, None]
    if dx.requires_grad:
        dx.retain_grad()
        dy.retain_grad()
    sigma = 0.5 * (cn[None, :, 0] * dx * dx + cn[None, :, 2] * dy * dy) + cn[None, :, 1] * dx * dy
    alpha = torch.clamp(op[None] * torch.exp(-sigma), max=0.999)
    n = alpha.shape[1]
    if include is None:
        rad = torch.as_tensor(np.asarray(radii)[np.asarray(order)], dtype=torch.float32, device=dev)
        tile_w, tile_h = (width + TILE - 1) // TILE, (height + TILE - 1) // TILE
        m2f = m2.detach().to(torch.float32)
        xmin = torch.clamp(torch.floor(m2f[:, 0] / TILE - rad / TILE), 0, tile_w)
        xmax = torch.clamp(torch.ceil(m2f[:, 0] / TILE + rad / TILE), 0, tile_w)
        ymin = torch.clamp(torch.floor(m2f[:, 1] / TILE - rad / TILE), 0, tile_h)
        ymax = torch.clamp(torch.ceil(m2f[:, 1] / TILE + rad / TILE), 0, tile_h)
        tyi, txi = (ii // TILE).to(torch.float32), (jj // TILE).to(torch.float32)
        member = ((txi[:, None] >= xmin[None]) & (txi[:, None] < xmax[None]) &
                  (tyi[:, None] >= ymin[None]) & (tyi[:, None] < ymax[None]) & (rad[None] > 0))
        valid = member & (sigma >= 0) & (alpha >= 1.0 / 255.0)
        a_eff = torch.where(valid, alpha, torch.zeros_like(alpha))
        next_T = torch.cumprod(1.0 - a_eff, dim=1)
        stop = valid & (next_T.detach() <= 1e-4)
        idx = torch.arange(n, device=dev)[None].expand_as(stop)
        first_stop = torch.where(stop, idx, torch.full_like(idx, n)).min(dim=1).values
        include = valid & (idx < first_stop[:, None])
    a_inc = torch.where(include, alpha, torch.zeros_like(alpha))
    T_incl = torch.cumprod(1.0 - a_inc, dim=1)
    T_before = torch.cat([torch.ones_like(T_incl[:, :1]), T_incl[:, :-1]], dim=1)
    w = a_inc * T_before
    T_final = T_incl[:, -1] if n > 0 else torch.ones(px.shape[0], dtype=dt, device=dev)
    out = w @ col
    if backgrounds is not None:
        out = out + T_final[:, None] * backgrounds[None]
    alphas = 1.0 - T_final
    aux = dict(include=include, dx=dx, dy=dy, order=order_t, n_blend=int(include.sum().item()))
    return out.reshape(height, width, col.shape[1]), alphas.reshape(height, width), aux


def absgrad_of(aux, n):
    """absgrad [N,2] after backward(): SUM over pixels of (|d loss / d dx|, |d loss / d dy|), back in Gaussian order."""
    dx, dy = aux["dx"], aux["dy"]
    a = torch.stack([dx.grad.abs().sum(0), dy.grad.abs().sum(0)], -1)
    out = torch.zeros(n, 2, dtype=a.dtype, device=a.device)
    out[aux["order"]] = a
    return out


def full(s, w, h, colors, bg, v_out, v_alpha, radii, depths, *, antialiased, dtype=torch.float64, dev="cpu", include=None,
         eps2d=0.3, raw=False):
    """One scene through project + composite + backward in `dtype`: dict(out, alphas, comp, include, n_blend, g = every
    gradient incl. "means2d" and "absgrad"), numpy.  radii / depths: the fp32 oracle's.  raw: the leaves are the STORED
    parameters s["raw"] (rotation un-normalised, log scales, opacity logits), activated here in `dtype` as the model's getters
    do, and g carries "_xyz", "_rotation", "_scaling", "_opacity" instead of the activated names."""
    def tm(a, rg=False):
        return torch.tensor(np.asarray(a), dtype=dtype, device=dev, requires_grad=rg)

    n = s["means"].shape[0]
    C = tm(colors, True)
    if raw:
        M, Rr, Sl, Ol = (tm(s["raw"][k], True) for k in ("xyz", "rotation", "scaling_log", "opacity_logit"))
        Q, S, O = torch.nn.functional.normalize(Rr), torch.exp(Sl), torch.sigmoid(Ol).reshape(-1)
    else:
        M, Q, S, O = tm(s["means"], True), tm(s["quats"], True), tm(s["scales"], True), tm(s["opacities"], True)
    m2, z, con, comp = project(M, Q, S, tm(s["viewmat"]), tm(s["K"]), w, h, eps2d=eps2d, radii=radii)
    m2.retain_grad()
    op = O * comp if antialiased else O
    order = np.lexsort((np.arange(n), np.asarray(depths)))
    out, alphas, aux = composite(m2, con, op, C, None if bg is None else tm(bg), w, h, radii, order, include=include)
    ((out * tm(v_out)).sum() + (alphas * tm(v_alpha)).sum()).backward()
    g = dict(means2d=m2.grad, colors=C.grad, absgrad=absgrad_of(aux, n))
    if raw:
        g.update(_xyz=M.grad, _rotation=Rr.grad, _scaling=Sl.grad, _opacity=Ol.grad)
    else:
        g.update(opacities=O.grad, means=M.grad, quats=Q.grad, scales=S.grad)
    return dict(out=out.detach().cpu().numpy(), alphas=alphas.detach().cpu().numpy(), comp=comp.detach().cpu().numpy(),
                include=aux["include"], n_blend=aux["n_blend"], g={k: v.detach().cpu().numpy() for k, v in g.items()})
