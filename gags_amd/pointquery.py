"""3-D open-vocabulary query on the Gaussians (include/gags_next.h N5): compute_relvancy.py:273-394 `pcd_relvancy`
(--pcd_mode), which asks "which Gaussians are the <phrase>?" with no camera.

Per Gaussian the 16-d `semantic_*` feature goes through CNN_decoder to 512-d (`decoder(f.T[..., None])`, chunks of
`chunk` Gaussians), then the LERF relevancy against every positive phrase (RelevancyHead, one read for all phrases), a
min-max normalisation and threshold per phrase (csrc/pointquery.hip, min / max on the device), and
utils/pcd_utils.py:204-219 `smooth_pcd_mask`: a radius-neighbour vote over the masked Gaussians, which the reference
runs as a Python loop with one KD-tree ball query per point, as one grid + radix sort + capped scan on the GPU.

    smooth_point_mask(mask, xyz, radius, threshold)   smooth_pcd_mask, for [N] or [K, N] masks
    point_relevancy(feature, decoder, head)           get_relevancy(decode(feature), j)[:, 0] for every phrase j
    query_points(feature, xyz, decoder, head)         pcd_relvancy for all phrases: relevancy, normalized, masks
    recolor_dc(features_dc, mask, bg_color)           the f_dc pcd_relvancy writes with save_pcd=True
    query_ply(path, decoder, head, prompts, ...)       the same from / to point_cloud.ply

The distance rule is scipy's for three coordinates: ((dx*dx + dy*dy) + dz*dz) <= r*r in float64 from the float32
coordinates.  The Open3D windows and mask_color="rel" (a matplotlib colormap) are out of scope."""
import os

import numpy as np
import torch

from . import _lib
from .io_formats import read_ply_table
from ._lib import check, ptr

C0 = 0.28209479177387814  # compute_relvancy.py:34
MASK_RED = (1.0, 0.1, 0.05)  # mask_color="default" (:377)


@torch.no_grad()
def smooth_point_mask(mask, xyz, radius=0.1, threshold=10, return_counts=False):
    """utils/pcd_utils.py:204-219 smooth_pcd_mask (same defaults) for mask [N] or [K, N] (bool or 0 / 1) over xyz [N, 3]
    fp32: out_i = c_i > threshold, or mask_i when 10 <= c_i <= threshold, with c_i the masked points within `radius` of
    point i (itself included).  Returns the bool mask of mask's shape; with return_counts also the int32 counts
    min(c_i, max(threshold + 1, 10))."""
    _lib.on_gpu("pointquery", mask, xyz)
    m = mask.reshape(1, -1) if mask.dim() == 1 else mask
    if m.dim() != 2 or xyz.dim() != 2 or xyz.shape[1] != 3 or xyz.shape[0] != m.shape[1]:
        raise ValueError(f"smooth_point_mask: mask {tuple(mask.shape)} and xyz {tuple(xyz.shape)} do not match ([K,] N and [N, 3])")
    k, n = m.shape
    m8 = (m != 0).to(torch.uint8).contiguous()
    p = xyz.float().contiguous()
    out = torch.empty(k, n, dtype=torch.uint8, device=p.device)
    counts = torch.empty(k, n, dtype=torch.int32, device=p.device) if return_counts else None
    lib = _lib.load()
    nb = lib.gags_point_mask_smooth_scratch_bytes(k, n)
    scratch = _lib.scratch(nb, p.device)
    check(lib.gags_point_mask_smooth(k, n, ptr(p), ptr(m8), float(radius), int(threshold), ptr(out), ptr(counts),
                                     ptr(scratch), nb, _lib.stream()), "gags_point_mask_smooth")
    out = out.bool().reshape(mask.shape)
    return (out, counts.reshape(mask.shape)) if return_counts else out


def _point_probs(semantic_feature, decoder, head, chunk, fused=False):
    """[n_pos, N, 2] relevancy pairs of the decoded features, `chunk` Gaussians per decoder call; fused=True: all N in one
    CNN_decoder.query call (nothing per layer is held, so nothing is chunked)."""
    _lib.on_gpu("pointquery", semantic_feature)
    if semantic_feature.dim() != 2:
        raise ValueError(f"semantic_feature must be [N, C], got {tuple(semantic_feature.shape)}")
    if chunk <= 0:
        raise ValueError("chunk must be positive")
    f = semantic_feature.float()  # (the fp16 tables of precision="f16" training: exact upcast)
    n = f.shape[0]
    if fused:  # [C, N, 1] over the table's own pixel-major memory: read in place
        return decoder.query(f.t()[..., None], head, pairs=True)
    probs = torch.empty(head.pos_embeds.shape[0], n, 2, device=f.device)
    with torch.no_grad():
        for s in range(0, n, chunk):
            x = f[s:s + chunk]
            # [C, m, 1] over pixel-major memory: the decoder reads it without a copy, and its [512, m, 1] output is a
            # view of [m, 512] rows -- the reference's .squeeze(-1).permute(1, 0) (compute_relvancy.py:333-356)
            feat = decoder(x.t()[..., None]).squeeze(-1).t()
            part = head._all(feat)
            if x.shape[0] == n:
                return part
            probs[:, s:s + x.shape[0]] = part
            del feat, part
    return probs


def point_relevancy(semantic_feature, decoder, head, chunk=1_000_000, fused=False):
    """compute_relvancy.py:333-361: for every positive phrase j of `head`, get_relevancy(decoder(f)[N, 512], j)[:, 0]
    -> [n_pos, N].  semantic_feature [N, 16] on the GPU (fp32 or fp16); decoded under no_grad, `chunk` Gaussians at a
    time (the decoder holds every layer's activations of a call).  fused=True: one CNN_decoder.query call over all N
    (N15: decoder and relevancy in one kernel in the 16-bit tiers, no chunking; equal up to the head's fp32 summation
    order); the default is the path every earlier result came from."""
    return _point_probs(semantic_feature, decoder, head, chunk, fused)[..., 0].contiguous()


@torch.no_grad()
def query_points(semantic_feature, xyz, decoder, head, rel_thresh=0.4, radius=0.05, threshold=20, chunk=1_000_000,
                 fused=False):
    """pcd_relvancy (compute_relvancy.py:273-394, its constants as defaults) for all positive phrases of `head` in one call.
    Returns a dict of [n_pos, N] device tensors: relevancy (fp32), normalized (clip((r - min) / (max - min + 1e-9) * 2 - 1,
    0, 1)), mask_raw (normalized > rel_thresh) and mask (after smooth_pcd_mask(mask_raw, xyz, radius, threshold)).  fused: as
    point_relevancy's."""
    _lib.on_gpu("pointquery", semantic_feature, xyz)
    if xyz.shape != (semantic_feature.shape[0], 3):
        raise ValueError(f"xyz must be [N, 3] with N = {semantic_feature.shape[0]}, got {tuple(xyz.shape)}")
    probs = _point_probs(semantic_feature, decoder, head, chunk, fused)
    k, n = probs.shape[0], probs.shape[1]
    normalized = torch.empty(k, n, device=probs.device)
    mask_raw = torch.empty(k, n, dtype=torch.uint8, device=probs.device)
    lib = _lib.load()
    nb = lib.gags_point_relevancy_mask_scratch_bytes(k, n)
    scratch = _lib.scratch(nb, probs.device)
    check(lib.gags_point_relevancy_mask(k, n, ptr(probs), float(rel_thresh), ptr(normalized), ptr(mask_raw), ptr(scratch), nb,
                                        _lib.stream()), "gags_point_relevancy_mask")
    mask = smooth_point_mask(mask_raw, xyz, radius, threshold)
    return {"relevancy": probs[..., 0].contiguous(), "normalized": normalized, "mask_raw": mask_raw.bool(), "mask": mask}


@torch.no_grad()
def recolor_dc(features_dc, mask, bg_color="mix", mask_color="default"):
    """compute_relvancy.py:319-324,372-394 with save_pcd=True: the f_dc the reference writes, [N, 3] fp32 ([K, N, 3] for
    a [K, N] mask).  rgb = f_dc C0 + 0.5 min-max normalised per channel over all points (float64, as the reference's
    numpy); masked points red, the others bg_color "RGB" (rgb), "gray" (0.5) or "mix" (0.5 rgb + 0.3); then back to
    f_dc = (c (max - min) + min - 0.5) / C0.  features_dc: [N, 3] or [N, 1, 3]."""
    if mask_color != "default":
        raise NotImplementedError("mask_color='rel' colours by a matplotlib colormap, which gags_amd does not carry; "
                                  "only mask_color='default' (red) is supported")
    if bg_color not in ("RGB", "gray", "mix"):
        raise ValueError(f"bg_color must be 'RGB', 'gray' or 'mix', got {bg_color!r}")
    _lib.on_gpu("pointquery", features_dc, mask)
    fdc = features_dc.reshape(-1, 3).double()
    m = mask.bool()
    if m.shape[-1] != fdc.shape[0]:
        raise ValueError(f"mask {tuple(mask.shape)} does not match features_dc {tuple(features_dc.shape)}")
    rgb = fdc * C0 + 0.5
    lo, hi = rgb.min(0).values, rgb.max(0).values
    rgb = (rgb - lo) / (hi - lo)
    if bg_color == "RGB":
        bg = 1.0 * rgb
    elif bg_color == "gray":
        bg = torch.full_like(rgb, 0.5)
    else:
        bg = 0.5 * rgb + 0.3 * torch.ones_like(rgb)
    red = torch.tensor(MASK_RED, dtype=torch.float64, device=rgb.device)
    seg = torch.where(m[..., None], red, bg)
    seg = seg * (hi - lo) + lo
    return ((seg - 0.5) / C0).float()


_PLY_TYPE_NAMES = {"<f4": "float", "<f8": "double", "|u1": "uchar", "|i1": "char", "<i2": "short", "<u2": "ushort",
                   "<i4": "int", "<u4": "uint"}


def _write_ply_table(path, data):
    """One `vertex` element of the structured array `data`, binary little-endian, in its own column order and types."""
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % data.shape[0]
    header += "".join(f"property {_PLY_TYPE_NAMES[data.dtype[nm].str]} {nm}\n" for nm in data.dtype.names) + "end_header\n"
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(np.ascontiguousarray(data).tobytes())


@torch.no_grad()
def query_ply(path, decoder, head, prompts=None, rel_thresh=0.4, radius=0.05, threshold=20, bg_color="mix",
              chunk=1_000_000, save_dir=None, device="cuda", fused=False):
    """pcd_relvancy from point_cloud.ply: reads x y z, semantic_* and f_dc_*, runs query_points, and with `save_dir` writes
    <name>_<prompt>.ply per phrase (`prompts`: one name per positive phrase of `head`) with only f_dc_0..2 changed
    (recolor_dc).  Returns query_points' dict, plus "paths" when files were written.  fused: as point_relevancy's."""
    names, table = read_ply_table(path)
    sem_cols = sorted([nm for nm in names if nm.startswith("semantic_")], key=lambda s: int(s.split("_")[-1]))
    if not sem_cols:
        raise ValueError(f"{path}: no semantic_* properties")
    col = lambda nm: np.asarray(table[nm], np.float32)  # noqa: E731
    xyz = torch.from_numpy(np.stack([col("x"), col("y"), col("z")], axis=1)).to(device)
    feat = torch.from_numpy(np.stack([col(nm) for nm in sem_cols], axis=1)).to(device)
    res = query_points(feat, xyz, decoder, head, rel_thresh, radius, threshold, chunk, fused)
    if save_dir is not None:
        k = res["mask"].shape[0]
        if prompts is None or len(prompts) != k:
            raise ValueError(f"query_ply: save_dir needs one prompt per positive phrase ({k})")
        fdc = torch.from_numpy(np.stack([np.asarray(table[f"f_dc_{i}"], np.float64) for i in range(3)], axis=1)).to(device)
        new = recolor_dc(fdc, res["mask"], bg_color).cpu().numpy()
        stem = os.path.splitext(os.path.basename(path))[0]
        os.makedirs(save_dir, exist_ok=True)
        res["paths"] = []
        for j, prompt in enumerate(prompts):
            out = table.copy()
            for i in range(3):
                out[f"f_dc_{i}"] = new[j, :, i]
            p = os.path.join(save_dir, f"{stem}_{prompt}.ply")
            _write_ply_table(p, out)
            res["paths"].append(p)
    return res
