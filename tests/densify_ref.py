"""Restatement of the reference's adaptive density control in plain torch, without the reference:
scene/gaussian_model.py:261-264 reset_opacity, :321-482 densify_and_prune / densify_and_clone / densify_and_split /
prune_points / add_densification_stats, utils/general_utils.py:78-99 build_rotation, :29-62 get_expon_lr_func, train.py:209.

It runs on whatever device and in whatever float type its inputs have (float32: thresholds compare as torch compares a
float32 tensor with a Python scalar, i.e. rounded to float32; float64: in double).  tests/golden/make_golden_densify.py ties
it to the reference's own methods (tests/golden/densify_vectors.npz); the GPU tests use it at shapes the fixture does not hold.

densify_and_prune as a pure function of per-Gaussian data -- the rule the kernels implement:
  g = accum / denom, NaN -> 0;  m = max exp(scaling);  o = sigmoid(opacity)
  clone = |g| >= max_grad and m <= percent_dense extent;  split = g >= max_grad and m > percent_dense extent
  prune(row) = o < min_opacity, or -- when max_screen_size is truthy -- 0 > max_screen_size (max_radii2D was zeroed by the
  clone step) or world size > 0.1 extent, the world size being m for originals and clones and m / 1.6 for children
  output = kept originals (not split, not pruned), surviving clones, surviving first children, surviving second children
"""
import numpy as np
import torch

NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "semantic_feature")
KEEP, CLONE, CHILD_A, CHILD_B = 0, 1, 2, 3


def build_rotation(r):
    norm = torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])
    q = r / norm[:, None]
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    rows = [1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
            2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
            2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]
    return torch.stack(rows, dim=1).reshape(-1, 3, 3)


def decide(accum, denom, scaling, opacity, percent_dense, max_grad, min_opacity, extent, max_screen_size):
    """(keep, clone_ok, split, child_ok): boolean [N] each."""
    g = (accum / denom).reshape(-1)
    g = torch.where(g.isnan(), torch.zeros_like(g), g)
    e = torch.exp(scaling)
    m = e.max(dim=1).values
    clone = (g.abs() >= max_grad) & (m <= percent_dense * extent)
    split = (g >= max_grad) & (m > percent_dense * extent)
    faint = torch.sigmoid(opacity).reshape(-1) < min_opacity
    prune, prune_ch = faint, faint
    if max_screen_size:
        big_vs = torch.zeros_like(m) > max_screen_size
        prune = faint | big_vs | (m > 0.1 * extent)
        prune_ch = faint | big_vs | ((e / (0.8 * 2)).max(dim=1).values > 0.1 * extent)
    return ~split & ~prune, clone & ~prune, split, split & ~prune_ch


def plan(keep, clone_ok, split, child_ok):
    """(src, kind, zrow, n_split) of every output row, in the contract's order."""
    idx = lambda m: m.nonzero().reshape(-1)  # noqa: E731
    n_split = int(split.sum())
    rank = torch.cumsum(split.long(), 0) - 1
    k, c, h = idx(keep), idx(clone_ok), idx(child_ok)
    src = torch.cat([k, c, h, h])
    kind = torch.cat([torch.full_like(k, KEEP), torch.full_like(c, CLONE), torch.full_like(h, CHILD_A),
                      torch.full_like(h, CHILD_B)])
    zrow = torch.cat([torch.full_like(k, -1), torch.full_like(c, -1), rank[h], rank[h] + n_split])
    return src, kind, zrow, n_split


def densify_and_prune(tensors, accum, denom, percent_dense, max_grad, min_opacity, extent, max_screen_size, samples,
                      moments=None):
    """tensors: name -> [N, ...]; moments: name -> (exp_avg, exp_avg_sq); samples: [2 n_split, 3] standard normal (the
    reference's torch.normal(0, std) is randn * std).  Returns a dict: the gathered tensors under their names, "moments",
    "src", "kind", "zrow", "n_split"."""
    keep, clone_ok, split, child_ok = decide(accum, denom, tensors["scaling"], tensors["opacity"], percent_dense, max_grad,
                                             min_opacity, extent, max_screen_size)
    src, kind, zrow, n_split = plan(keep, clone_ok, split, child_ok)
    out = {name: t[src] for name, t in tensors.items() if t is not None}
    child = kind >= CHILD_A
    if bool(child.any()):
        s, z = src[child], samples.to(tensors["xyz"].dtype)[zrow[child]]
        e = torch.exp(tensors["scaling"][s])
        t = e * z
        R = build_rotation(tensors["rotation"][s])
        out["xyz"][child] = torch.bmm(R, t[..., None]).squeeze(-1) + tensors["xyz"][s]
        out["scaling"][child] = torch.log(e / (0.8 * 2))
    res = dict(out, src=src, kind=kind, zrow=zrow, n_split=n_split, moments={})
    for name, (m1, m2) in (moments or {}).items():
        sel = (kind == KEEP).reshape((-1,) + (1,) * (m1.dim() - 1))
        res["moments"][name] = (torch.where(sel, m1[src], torch.zeros_like(m1[src])),
                                torch.where(sel, m2[src], torch.zeros_like(m2[src])))
    return res


def add_stats(accum, denom, max_radii, grad, radii, update_filter, visibility_filter, width, height):
    """One view's statistics; returns the new (accum [N,1], denom [N,1], max_radii [N])."""
    g = grad.clone()
    g[:, 0] *= width * 0.5
    g[:, 1] *= height * 0.5
    norm = torch.norm(g[:, :2], dim=-1, keepdim=True)
    u = update_filter.reshape(-1, 1)
    accum = torch.where(u, accum + norm.to(accum.dtype), accum)
    denom = torch.where(u, denom + 1, denom)
    max_radii = torch.where(visibility_filter, torch.max(max_radii, radii.to(max_radii.dtype)), max_radii)
    return accum, denom, max_radii


def reset_opacity(opacity):
    x = torch.min(torch.sigmoid(opacity), torch.ones_like(opacity) * 0.01)
    return torch.log(x / (1 - x))


def expon_lr(step, lr_init, lr_final, lr_delay_steps=0, lr_delay_mult=1.0, max_steps=1000000):
    if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
        return 0.0
    delay = 1.0
    if lr_delay_steps > 0:
        delay = lr_delay_mult + (1 - lr_delay_mult) * np.sin(0.5 * np.pi * np.clip(step / lr_delay_steps, 0, 1))
    t = np.clip(step / max_steps, 0, 1)
    return float(delay * np.exp(np.log(lr_init) * (1 - t) + np.log(lr_final) * t))
