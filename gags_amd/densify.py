"""Adaptive density control on the GPU (include/gags_next.h "N8"; csrc/densify.hip).

The reference's `densify_and_prune` (scene/gaussian_model.py:321-482) is a chain of boolean-mask indexing: every
`x[mask]` is a `nonzero` plus a host wait, and a densify rewrites every parameter and both Adam moments three times
(`cat` the clones, `cat` the children, two prunes).  All of its decisions depend only on the SOURCE Gaussian, so here it is

    decide (4 flags / Gaussian) -> 4 prefix sums -> ONE 16-byte readback -> plan (src, kind, z row per OUTPUT row)
    -> ONE gather of every tensor and moment -> children (positions and scales of the split children)

`GaussianModel` (gags_amd/scene.py) exposes this under the reference's method names; this module holds the mechanics.
GPU tensors only -- there is no CPU path.
"""
import ctypes
import math

import numpy as np
import torch
from torch import nn

from . import _lib

# optimizer group name -> attribute of the model (scene/gaussian_model.py:193-199, 358-364)
GROUPS = (("xyz", "_xyz"), ("f_dc", "_features_dc"), ("f_rest", "_features_rest"), ("opacity", "_opacity"),
          ("scaling", "_scaling"), ("rotation", "_rotation"), ("semantic_feature", "_semantic_feature"))
STATS = ("xyz_gradient_accum", "denom", "max_radii2D")


def _need_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("gags_amd.densify: no CPU path (tensors must live on the GPU)")


def _f32c(t, what):
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise RuntimeError(f"gags_amd.densify: {what} must be a contiguous float32 tensor")
    return t


def _mask(m, n, dev):
    """A boolean / byte mask as the bytes the kernels read (None stays None: `radii > 0`)."""
    if m is None:
        return None
    _need_gpu(m)
    if m.numel() != n:
        raise ValueError("mask length differs from the number of Gaussians")
    m = m.reshape(-1).contiguous()
    return m.view(torch.uint8) if m.dtype == torch.bool else (m != 0).view(torch.uint8)


def ensure_stats(model):
    """The three statistics tensors, created as zeros when the model has none of the right length."""
    n, dev = model._xyz.shape[0], model._xyz.device
    for name, shape in (("xyz_gradient_accum", (n, 1)), ("denom", (n, 1)), ("max_radii2D", (n,))):
        t = getattr(model, name, None)
        if not torch.is_tensor(t) or tuple(t.shape) != shape or t.device != dev or t.dtype != torch.float32:
            setattr(model, name, torch.zeros(shape, device=dev))


def stats(model, grad, radii, update_filter, visibility_filter, width, height):
    """One launch of gags_densify_stats.  grad None: only max_radii2D; radii None: only accum / denom."""
    _need_gpu(model._xyz, grad, radii)
    ensure_stats(model)
    n, dev = model._xyz.shape[0], model._xyz.device
    if grad is not None:
        grad = grad.reshape(-1, grad.shape[-1])
        if grad.shape[0] != n or grad.shape[1] < 2:
            raise ValueError("viewspace gradient must be [N, 2] (or [1, N, 2])")
        grad = _f32c(grad[:, :2].contiguous(), "the viewspace gradient")
    if radii is not None:
        radii = radii.reshape(-1)
        if radii.shape[0] != n:
            raise ValueError("radii must have one entry per Gaussian")
        radii = radii.to(torch.int32).contiguous()
    uf, vf = _mask(update_filter, n, dev), _mask(visibility_filter, n, dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().gags_densify_stats(
            n, _lib.ptr(grad), _lib.ptr(radii), _lib.ptr(uf), _lib.ptr(vf), float(width * 0.5), float(height * 0.5),
            _lib.ptr(model.xyz_gradient_accum), _lib.ptr(model.denom),
            _lib.ptr(model.max_radii2D if radii is not None else None), _lib.stream(dev)), "gags_densify_stats")


def viewspace_gradient(vp, absgrad=False):
    """The tensor the statistics are taken from: `vp.grad`, or with absgrad `vp.absgrad` -- what a backward of
    render(..., absgrad=True) attaches (the sum over pixels of the absolute per-pixel gradients, AbsGS)."""
    if absgrad:
        g = getattr(vp, "absgrad", None)
        if g is None:
            raise RuntimeError("densify: viewspace_points has no .absgrad (render with absgrad=True, geometry gradients wanted, "
                               "and call backward first)")
        return g
    if vp.grad is None:
        raise RuntimeError("accumulate: viewspace_points has no gradient (call backward first)")
    return vp.grad


def accumulate(model, render_pkg, absgrad=False):
    """The per-step statistics of train.py:209-211 in one launch: accum / denom from the viewspace gradient and max_radii2D
    from the radii, both over `radii > 0` (the reference passes visibility_filter for both filters).  The reference also
    scales viewspace_point_tensor.grad in place; nothing reads it afterwards and it is not written back.
    absgrad: the statistic is taken from viewspace_points.absgrad instead of .grad (render(..., absgrad=True))."""
    vp = render_pkg["viewspace_points"]
    img = render_pkg["render"]
    stats(model, viewspace_gradient(vp, absgrad), render_pkg["radii"], None, None, img.shape[2], img.shape[1])


class Plan:
    """src / kind / zrow of every output row, and the four totals (the call's only readback)."""

    def __init__(self, src, kind, zrow, totals):
        self.src, self.kind, self.zrow = src, kind, zrow
        self.n_keep, self.n_clone, self.n_split, self.n_child = totals
        self.n_out = self.n_keep + self.n_clone + 2 * self.n_child
        self.first_child = self.n_keep + self.n_clone


def plan_from_flags(flags, classes=(0, 1, 2, 3)):
    """flags [4, N] int32 (keep, clone survives, split-selected, children survive) -> Plan.  classes: the rows of `flags` that
    can hold a one; the others must be zeros and are not scanned (their prefix sums and totals are zeros)."""
    lib = _lib.load()
    n, dev = flags.shape[1], flags.device
    with torch.cuda.device(dev):
        st = _lib.stream(dev)
        cum = torch.empty_like(flags) if len(classes) == 4 else torch.zeros_like(flags)
        totals = torch.zeros(4, dtype=torch.int32, device=dev)
        nbytes = int(lib.gags_scan_scratch_bytes(n))
        scratch = _lib.scratch(nbytes, dev)
        for k in (classes if n else ()):
            _lib.check(lib.gags_cumsum_i32(n, _lib.ptr(flags[k]), _lib.ptr(cum[k]), _lib.ptr(totals[k:]), _lib.ptr(scratch),
                                           nbytes, st), "gags_cumsum_i32")
        tot = [int(v) for v in totals.cpu().tolist()]  # the one readback: 16 bytes
        n_out = tot[0] + tot[1] + 2 * tot[3]
        if n_out >= 2 ** 31:
            raise RuntimeError("densify: more than 2^31 - 1 output rows")
        src = torch.empty(n_out, dtype=torch.int32, device=dev)
        kind = torch.empty(n_out, dtype=torch.uint8, device=dev)
        zrow = torch.empty(n_out, dtype=torch.int32, device=dev)
        _lib.check(lib.gags_densify_plan(n, _lib.ptr(flags), _lib.ptr(cum), _lib.ptr(totals), n_out, _lib.ptr(src),
                                         _lib.ptr(kind), _lib.ptr(zrow), st), "gags_densify_plan")
    return Plan(src, kind, zrow, tot)


def gather(n_out, src, kind, items):
    """items: (in_tensor [N, ...], moment?) -> the gathered tensors [n_out, ...], one launch per 24 tensors.  A zero-width
    tensor is not handed to the kernel."""
    lib = _lib.load()
    dev = src.device
    outs, descs = [], []
    for t, moment in items:
        _need_gpu(t)
        _f32c(t, "a gathered tensor")
        out = torch.empty((n_out,) + tuple(t.shape[1:]), dtype=torch.float32, device=dev)
        outs.append(out)
        row = int(math.prod(t.shape[1:]))
        if row > 0 and n_out > 0:
            descs.append(_lib.GatherDesc(t.data_ptr(), out.data_ptr(), row,
                                         _lib.GAGS_GATHER_MOMENT if moment else _lib.GAGS_GATHER_COPY))
    with torch.cuda.device(dev):
        for k in range(0, len(descs), _lib.GAGS_GATHER_MAX_DESC):
            part = descs[k:k + _lib.GAGS_GATHER_MAX_DESC]
            table = (_lib.GatherDesc * len(part))(*part)
            _lib.check(lib.gags_densify_gather(n_out, _lib.ptr(src), _lib.ptr(kind), len(part),
                                               ctypes.cast(table, ctypes.c_void_p), _lib.stream(dev)), "gags_densify_gather")
    return outs


def _group_of(model, name):
    if model.optimizer is None:
        return None
    for group in model.optimizer.param_groups:
        if group.get("name") == name:
            return group
    return None


def apply_plan(model, plan, with_stats):
    """Gather every parameter (and the Adam moments of those that sit in a named group and have state) through `plan`,
    replace the parameters and re-key the optimizer state as the reference does.  with_stats: the three statistics follow the
    kept rows (prune_points); otherwise they become zeros of the new length (densification_postfix).  Returns the OLD
    (xyz, scaling, rotation), which the children kernel reads."""
    ensure_stats(model)
    items, slots = [], []
    for name, attr in GROUPS:
        p = getattr(model, attr, None)
        if p is None:
            continue
        group = _group_of(model, name)
        state = model.optimizer.state.get(group["params"][0], None) if group is not None else None
        if group is not None and group["params"][0] is not p:
            raise RuntimeError(f"densify: optimizer group '{name}' does not hold the model's {attr}")
        items.append((p.detach(), False))
        has = bool(state) and "exp_avg" in state
        if has:
            items += [(state["exp_avg"], True), (state["exp_avg_sq"], True)]
        slots.append((name, attr, p, group, state if has else None))
    if with_stats:
        items += [(getattr(model, s), False) for s in STATS]
    outs = iter(gather(plan.n_out, plan.src, plan.kind, items))
    old = (model._xyz.detach(), model._scaling.detach(), model._rotation.detach())
    for name, attr, p, group, state in slots:
        new = next(outs)
        if group is not None:
            stored = model.optimizer.state.pop(p, None)
            if state is not None:
                stored["exp_avg"], stored["exp_avg_sq"] = next(outs), next(outs)
            q = nn.Parameter(new.requires_grad_(True))
            group["params"][0] = q
            if stored is not None:
                model.optimizer.state[q] = stored
        else:
            q = nn.Parameter(new, requires_grad=p.requires_grad) if isinstance(p, nn.Parameter) else new.requires_grad_(
                p.requires_grad)
        setattr(model, attr, q)
    dev = old[0].device
    if with_stats:
        for s in STATS:
            setattr(model, s, next(outs))
    else:
        model.xyz_gradient_accum = torch.zeros((plan.n_out, 1), device=dev)
        model.denom = torch.zeros((plan.n_out, 1), device=dev)
        model.max_radii2D = torch.zeros((plan.n_out,), device=dev)
    model.invalidate_activations()
    return old


def densify_and_prune(model, max_grad, min_opacity, extent, max_screen_size, generator=None, samples=None):
    _need_gpu(model._xyz)
    lib = _lib.load()
    ensure_stats(model)
    n, dev = model._xyz.shape[0], model._xyz.device
    scaling, opacity = _f32c(model._scaling.detach(), "_scaling"), _f32c(model._opacity.detach(), "_opacity")
    flags = torch.empty((4, n), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.gags_densify_decide(
            n, _lib.ptr(model.xyz_gradient_accum), _lib.ptr(model.denom), _lib.ptr(scaling), _lib.ptr(opacity),
            float(max_grad), float(model.percent_dense * extent), float(min_opacity), float(0.1 * extent),
            float(max_screen_size) if max_screen_size else 0.0, 1 if max_screen_size else 0, _lib.ptr(flags), _lib.stream(dev)),
            "gags_densify_decide")
    plan = plan_from_flags(flags)
    n_z = 2 * plan.n_split
    if samples is not None:
        _need_gpu(samples)
        if tuple(samples.shape) != (n_z, 3):
            raise ValueError(f"samples must be [{n_z}, 3] (2 x the number of split-selected Gaussians)")
        z = _f32c(samples.float().contiguous(), "samples")
    elif n_z:
        z = torch.randn((n_z, 3), device=dev, generator=generator)
    else:
        z = None
    xyz, scal, rot = apply_plan(model, plan, with_stats=False)
    if plan.n_child:
        with torch.cuda.device(dev):
            _lib.check(lib.gags_densify_children(
                plan.n_out, plan.first_child, n, _lib.ptr(plan.src), _lib.ptr(plan.zrow), _lib.ptr(xyz), _lib.ptr(scal),
                _lib.ptr(rot), _lib.ptr(z), n_z, _lib.ptr(model._xyz), _lib.ptr(model._scaling), _lib.stream(dev)),
                "gags_densify_children")
    return plan


def prune_points(model, mask):
    """Drop the Gaussians where `mask` is set: the same plan with only the keep class; the statistics follow."""
    _need_gpu(model._xyz, mask)
    n, dev = model._xyz.shape[0], model._xyz.device
    flags = torch.zeros((4, n), dtype=torch.int32, device=dev)
    flags[0] = _mask(mask, n, dev) == 0
    plan = plan_from_flags(flags, classes=(0,))
    apply_plan(model, plan, with_stats=True)
    return plan


def reset_opacity(model):
    lib = _lib.load()
    _need_gpu(model._opacity)
    old = model._opacity
    dev = old.device
    group = _group_of(model, "opacity")
    if group is not None and group["params"][0] is not old:
        raise RuntimeError("densify: optimizer group 'opacity' does not hold the model's _opacity")
    new = _f32c(old.detach().clone(), "_opacity")
    state = model.optimizer.state.get(old, None) if group is not None else None
    m1 = state.get("exp_avg") if state else None
    m2 = state.get("exp_avg_sq") if state else None
    with torch.cuda.device(dev):
        _lib.check(lib.gags_reset_opacity(new.numel(), _lib.ptr(new), _lib.ptr(m1), _lib.ptr(m2), _lib.stream(dev)),
                   "gags_reset_opacity")
    if group is not None:
        stored = model.optimizer.state.pop(old, None)
        q = nn.Parameter(new.requires_grad_(True))
        group["params"][0] = q
        if stored is not None:
            model.optimizer.state[q] = stored
    else:
        q = nn.Parameter(new, requires_grad=old.requires_grad)
    model._opacity = q
    model.invalidate_activations()


def expon_lr(step, lr_init, lr_final, lr_delay_steps=0, lr_delay_mult=1.0, max_steps=1000000):
    """utils/general_utils.py:29-62 get_expon_lr_func, evaluated: log-linear from lr_init to lr_final over max_steps, eased in
    by a sine over lr_delay_steps.  numpy's exp / log / sin, as there, so that the values are the reference's to the bit."""
    if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
        return 0.0
    delay = 1.0
    if lr_delay_steps > 0:
        delay = lr_delay_mult + (1 - lr_delay_mult) * np.sin(0.5 * np.pi * np.clip(step / lr_delay_steps, 0, 1))
    t = np.clip(step / max_steps, 0, 1)
    return float(delay * np.exp(np.log(lr_init) * (1 - t) + np.log(lr_final) * t))
