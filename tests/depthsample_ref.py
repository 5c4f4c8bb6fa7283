"""numpy float32 restatement of depth_SAM.py's point-to-pixel min-depth mapping (include/gags_next.h N6) in the kernel's
stated operation order: ((M[r,0] x + M[r,1] y) + M[r,2] z) + M[r,3], then (xc fx) / zc + cx, round half to even, the
inside test in float, |d - zc| <= vis_thresh d; the highest visible point index wins a pixel.  numpy's float32
arithmetic is IEEE with one rounding per operation (no FMA), its division correctly rounded.  Does not import gags_amd.

Also the float64 projection the GPU tests compare against, and the margin band in which the two may disagree."""
import numpy as np

F = np.float32


def decide(xyz, M, K, depth, vis_thresh=0.25, cut_bound=0):
    """One camera: (visible [N] bool, v [N] int32, u [N] int32, d [N] float32) -- v, u, d only meaningful where visible."""
    x, y, z = (np.ascontiguousarray(xyz[:, k], dtype=F) for k in range(3))
    M, K = np.asarray(M, F), np.asarray(K, F)
    h, w = depth.shape
    with np.errstate(all="ignore"):
        r = [((M[i, 0] * x + M[i, 1] * y) + M[i, 2] * z) + M[i, 3] for i in range(3)]
        u = (r[0] * K[0, 0]) / r[2] + K[0, 2]
        v = (r[1] * K[1, 1]) / r[2] + K[1, 2]
        ur, vr = np.rint(u), np.rint(v)
        cut = F(cut_bound)
        inside = (ur >= cut) & (ur < F(w) - cut) & (vr >= cut) & (vr < F(h) - cut)
        ui = np.where(inside, ur, 0).astype(np.int32)
        vi = np.where(inside, vr, 0).astype(np.int32)
        d = np.where(inside, depth[vi, ui], F(0)).astype(F)
        vis = inside & (np.abs(d - r[2]) <= F(vis_thresh) * d)
    return vis, vi, ui, d


def depth_sample(xyz, viewmats, Ks, depths, vis_thresh=0.25, cut_bound=0, cams=None):
    """All cameras: dict of mapping [N, C, 2] int32 (v, u), visible [N, C] bool, min_depth [N] float32 (inf where no camera
    sees the point) and samples [C, H, W] float32.  `cams`: only these camera indices get a sample map (min_depth always
    runs over all of them)."""
    n, c = xyz.shape[0], depths.shape[0]
    h, w = depths.shape[1:]
    mapping = np.zeros((n, c, 2), np.int32)
    visible = np.zeros((n, c), bool)
    md = np.full(n, np.inf, F)
    for k in range(c):
        vis, vi, ui, d = decide(xyz, viewmats[k], Ks[k], depths[k], vis_thresh, cut_bound)
        mapping[vis, k, 0], mapping[vis, k, 1], visible[:, k] = vi[vis], ui[vis], vis
        md = np.where(vis, np.minimum(md, d), md)
    cams = range(c) if cams is None else cams
    samples = np.zeros((len(cams), h, w), F)
    idx = np.arange(n, dtype=np.int64)
    for j, k in enumerate(cams):
        vis = visible[:, k]
        win = np.full(h * w, -1, np.int64)
        np.maximum.at(win, mapping[vis, k, 0].astype(np.int64) * w + mapping[vis, k, 1], idx[vis])
        samples[j] = np.where(win >= 0, md[np.maximum(win, 0)], F(0)).reshape(h, w)
    return {"mapping": mapping, "visible": visible, "min_depth": md, "samples": samples}


def project64(xyz, M, K):
    """(u, v, zc) in float64 from the float32 inputs."""
    x = np.asarray(xyz, np.float64)
    M, K = np.asarray(M, np.float64), np.asarray(K, np.float64)
    r = x @ M[:3, :3].T + M[:3, 3]
    with np.errstate(all="ignore"):
        return r[:, 0] * K[0, 0] / r[:, 2] + K[0, 2], r[:, 1] * K[1, 1] / r[:, 2] + K[1, 2], r[:, 2]


def decide64(xyz, M, K, depth, vis_thresh=0.25):
    """The same decision from a float64 projection; also the band where float32 and float64 may disagree:
    u or v within 1e-3 px of a half-integer, or | |d - zc| - vis_thresh d | <= 1e-5 d.  Returns (visible, v, u, band)."""
    u, v, zc = project64(xyz, M, K)
    h, w = depth.shape
    with np.errstate(all="ignore"):
        ur, vr = np.rint(u), np.rint(v)
        inside = (ur >= 0) & (ur < w) & (vr >= 0) & (vr < h)
        ui = np.where(inside, ur, 0).astype(np.int64)
        vi = np.where(inside, vr, 0).astype(np.int64)
        d = np.where(inside, depth[vi, ui], 0).astype(np.float64)
        vis = inside & (np.abs(d - zc) <= F(vis_thresh) * d)
        half = lambda t: np.abs(t - np.floor(t) - 0.5) < 1e-3  # noqa: E731
        band = half(u) | half(v) | (inside & (np.abs(np.abs(d - zc) - F(vis_thresh) * d) <= 1e-5 * np.abs(d)))
    return vis, vi, ui, band
