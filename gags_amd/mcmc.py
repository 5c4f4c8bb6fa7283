"""MCMC density control on the GPU (include/gags_next.h "N18"; csrc/mcmc.hip; DESIGN.md section 7 "N18").

The density strategy with a hard cap on N ("3D Gaussian Splatting as Markov Chain Monte Carlo"): dead Gaussians are moved onto
live ones (`relocate`), N grows by 5 % per refinement up to `cap_max` (`sample_add`), positions get opacity-gated noise every
step (`inject_noise`), and two regularisers keep Gaussians dying (`regularisation`).  `MCMCStrategy` holds the schedule.

    weights (sigmoid, float64) -> torch cumsum -> sample (binary search, integer counts) -> relocation values (float64, in place)
    -> relocate: row copies in place, ONE readback (the number of dead rows)
    -> sample_add: one gather through densify.apply_plan (kept rows, then one copy per draw)

`GaussianModel.relocate_gs` / `add_new_gs` (gags_amd/scene.py) are the method forms.  GPU tensors only -- there is no CPU path;
the schedule and the growth target are pure functions.
"""
import ctypes
import math

import torch

from . import _lib
from . import densify

MIN_OPACITY = 0.005


def _need_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("gags_amd.mcmc: no CPU path (tensors must live on the GPU)")


def _typed(t, dtype, what):
    if t.dtype != dtype or not t.is_contiguous():
        raise RuntimeError(f"gags_amd.mcmc: {what} must be a contiguous {str(dtype).replace('torch.', '')} tensor")
    return t


def _f32c(t, what):
    return _typed(t, torch.float32, what)


def _wrote(model, *params):
    """After a raw-pointer write: move the version counters and drop the model's cached activations."""
    for p in params:
        torch.autograd.graph.increment_version(p)
    if model is not None:
        model.invalidate_activations()


# ---- pure functions: the schedule (R7) and the growth target (R4) ---------------------------------------------------------
def n_target(n, cap_max):
    """min(cap_max, int(1.05 n)): the row count one growth step aims at (a model at or above it adds nothing)."""
    return min(int(cap_max), int(1.05 * n))


def refines(step, refine_start_iter, refine_stop_iter, refine_every):
    return refine_start_iter < step < refine_stop_iter and step % refine_every == 0


# ---- R2 -------------------------------------------------------------------------------------------------------------------
def sample(weights, n, uniforms=None, generator=None):
    """n draws from the rows of `weights` [N] (float64, non-negative) -> (draws [n] int32, counts [N] int32, cdf [N] float64).
    uniforms: the [n] float64 draws from [0, 1); otherwise torch.rand(generator=generator) on the device."""
    _need_gpu(weights, uniforms)
    w = _typed(weights.reshape(-1), torch.float64, "weights")
    rows, dev = w.shape[0], w.device
    n = int(n)
    if n < 0 or (n > 0 and rows == 0):
        raise ValueError("sample: n must be >= 0, and there must be a row to draw from")
    cdf = torch.cumsum(w, 0)
    if uniforms is None:
        u = torch.rand(n, dtype=torch.float64, device=dev, generator=generator)
    else:
        if uniforms.numel() != n:
            raise ValueError(f"uniforms must hold {n} values")
        u = _typed(uniforms.reshape(-1), torch.float64, "uniforms")
    draws = torch.empty(n, dtype=torch.int32, device=dev)
    counts = torch.zeros(rows, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().gags_mcmc_sample(rows, _lib.ptr(cdf), n, _lib.ptr(u), _lib.ptr(draws), _lib.ptr(counts),
                                                _lib.stream(dev)), "gags_mcmc_sample")
    return draws, counts, cdf


# ---- R1 -------------------------------------------------------------------------------------------------------------------
def _relocation_in_place(opacity, scaling, k, bias, min_opacity):
    n, dev = opacity.numel(), opacity.device
    if scaling.shape[0] != n or k.numel() != n:
        raise ValueError("opacity, scaling and the ratios must have one row per Gaussian")
    with torch.cuda.device(dev):
        _lib.check(_lib.load().gags_mcmc_relocation(n, _lib.ptr(k), bias, float(min_opacity), _lib.ptr(opacity),
                                                    _lib.ptr(scaling), _lib.stream(dev)), "gags_mcmc_relocation")


def relocation_values(opacity_logit, scaling_log, ratios, min_opacity=MIN_OPACITY):
    """Out of place: the stored (logit, log-scales) of a source drawn `ratios - 1` times.  ratios [N] integers, clamped to
    [1, 51]; a row with a ratio below 1 is returned as it is."""
    _need_gpu(opacity_logit, scaling_log, ratios)
    op = _f32c(opacity_logit.detach(), "opacity_logit").clone()
    sc = _f32c(scaling_log.detach(), "scaling_log").clone()
    _relocation_in_place(op, sc, ratios.reshape(-1).to(torch.int32).contiguous(), 0, min_opacity)
    return op, sc


def _weights(model, excluded=None):
    w = torch.sigmoid(model._opacity.detach().reshape(-1).double())
    return w if excluded is None else w.masked_fill_(excluded, 0.0)


def _slots(model):
    """(parameter, exp_avg, exp_avg_sq) of every stored tensor the model has; the moments are None without optimizer state."""
    out = []
    for name, attr in densify.GROUPS:
        p = getattr(model, attr, None)
        if p is None:
            continue
        group = densify._group_of(model, name)
        if group is not None and group["params"][0] is not p:
            raise RuntimeError(f"mcmc: optimizer group '{name}' does not hold the model's {attr}")
        state = model.optimizer.state.get(p, None) if group is not None else None
        has = bool(state) and "exp_avg" in state
        out.append((p, state["exp_avg"] if has else None, state["exp_avg_sq"] if has else None))
    return out


# ---- R3 -------------------------------------------------------------------------------------------------------------------
def relocate(model, dead_mask=None, min_opacity=MIN_OPACITY, uniforms=None, generator=None):
    """Move every dead Gaussian onto a live one drawn by opacity; in place, N unchanged.  Returns the number relocated.
    dead_mask: [N] bool / bytes (default: sigmoid(opacity) <= min_opacity).  The call's one readback is the dead count."""
    _need_gpu(model._xyz, dead_mask, uniforms)
    lib = _lib.load()
    n, dev = model._xyz.shape[0], model._xyz.device
    if n == 0:
        return 0
    if dead_mask is None:
        dead_mask = torch.sigmoid(model._opacity.detach()).reshape(-1) <= min_opacity
    dead = densify._mask(dead_mask, n, dev)
    rows = torch.empty(n, dtype=torch.int64, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        nbytes = int(lib.gags_compact_mask_scratch_bytes(n))
        scratch = _lib.scratch(nbytes, dev)
        _lib.check(lib.gags_compact_mask(n, _lib.ptr(dead), n, _lib.ptr(rows), _lib.ptr(count), _lib.ptr(scratch), nbytes,
                                         _lib.stream(dev)), "gags_compact_mask")
    n_dead = int(count.item())  # the one readback
    if n_dead == 0 or n_dead == n:
        return 0
    draws, counts, _ = sample(_weights(model, dead.bool()), n_dead, uniforms, generator)
    slots = _slots(model)
    for p, _, _ in slots:
        _f32c(p, "a stored parameter")
    _relocation_in_place(model._opacity.detach(), model._scaling.detach(), counts, 1, min_opacity)
    descs = []
    for p, m1, m2 in slots:
        row = int(math.prod(p.shape[1:]))
        if row == 0:
            continue
        descs.append(_lib.GatherDesc(p.data_ptr(), p.data_ptr(), row, _lib.GAGS_GATHER_COPY))
        for m in (m1, m2):
            if m is not None:
                _f32c(m, "an Adam moment")
                descs.append(_lib.GatherDesc(m.data_ptr(), m.data_ptr(), row, _lib.GAGS_GATHER_MOMENT))
    with torch.cuda.device(dev):
        for a in range(0, len(descs), _lib.GAGS_GATHER_MAX_DESC):
            part = descs[a:a + _lib.GAGS_GATHER_MAX_DESC]
            table = (_lib.GatherDesc * len(part))(*part)
            _lib.check(lib.gags_mcmc_copy_rows(n_dead, _lib.ptr(rows), _lib.ptr(draws), n, len(part),
                                               ctypes.cast(table, ctypes.c_void_p), _lib.stream(dev)), "gags_mcmc_copy_rows")
    _wrote(model, *[p for p, _, _ in slots])
    return n_dead


# ---- R4 -------------------------------------------------------------------------------------------------------------------
def sample_add(model, cap_max, min_opacity=MIN_OPACITY, uniforms=None, generator=None):
    """Grow to n_target(N, cap_max) rows: draw the sources by opacity, apply the relocation values to them, append one copy of
    its source per draw (zero moments; the existing moments stay), statistics to zeros.  Returns the number added; 0 changes
    nothing at all."""
    _need_gpu(model._xyz, uniforms)
    n, dev = model._xyz.shape[0], model._xyz.device
    n_add = max(0, n_target(n, cap_max) - n)
    if n_add <= 0 or n == 0:
        return 0
    if n + n_add >= 2 ** 31:
        raise RuntimeError("mcmc: more than 2^31 - 1 rows")
    draws, counts, _ = sample(_weights(model), n_add, uniforms, generator)
    _f32c(model._opacity, "_opacity"), _f32c(model._scaling, "_scaling")
    _relocation_in_place(model._opacity.detach(), model._scaling.detach(), counts, 1, min_opacity)
    _wrote(model, model._opacity, model._scaling)
    src = torch.cat([torch.arange(n, dtype=torch.int32, device=dev), draws])
    kind = torch.cat([torch.full((n,), _lib.GAGS_KIND_KEEP, dtype=torch.uint8, device=dev),
                      torch.full((n_add,), _lib.GAGS_KIND_CLONE, dtype=torch.uint8, device=dev)])
    densify.apply_plan(model, densify.Plan(src, kind, None, (n, n_add, 0, 0)), with_stats=False)
    return n_add


# ---- R5 -------------------------------------------------------------------------------------------------------------------
def inject_noise(model, scaler, noise=None, generator=None):
    """xyz += Sigma (z gate scaler) in one launch, in place.  noise: z [N, 3] float32; otherwise torch.randn(generator=)."""
    _need_gpu(model._xyz, noise)
    n, dev = model._xyz.shape[0], model._xyz.device
    if noise is None:
        z = torch.randn((n, 3), device=dev, generator=generator)
    else:
        if tuple(noise.shape) != (n, 3):
            raise ValueError(f"noise must be [{n}, 3]")
        z = _f32c(noise, "noise")
    xyz = _f32c(model._xyz, "_xyz")
    with torch.cuda.device(dev):
        _lib.check(_lib.load().gags_mcmc_noise(
            n, _lib.ptr(_f32c(model._opacity.detach(), "_opacity")), _lib.ptr(_f32c(model._scaling.detach(), "_scaling")),
            _lib.ptr(_f32c(model._rotation.detach(), "_rotation")), _lib.ptr(z), float(scaler), _lib.ptr(xyz),
            _lib.stream(dev)), "gags_mcmc_noise")
    _wrote(model, model._xyz)


# ---- R6 -------------------------------------------------------------------------------------------------------------------
class _Regularisation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, opacity, scaling, opacity_reg, scale_reg):
        lib = _lib.load()
        op, sc = _f32c(opacity.detach(), "_opacity"), _f32c(scaling.detach(), "_scaling")
        n, dev = op.numel(), op.device
        if tuple(sc.shape) != (n, 3):
            raise ValueError("scaling must be [N, 3] with one row per opacity")
        out = torch.empty(1, device=dev)
        with torch.cuda.device(dev):
            partials = torch.empty(int(lib.gags_mcmc_reg_partials(n)), device=dev)
            _lib.check(lib.gags_mcmc_reg_fwd(n, _lib.ptr(op), _lib.ptr(sc), opacity_reg, scale_reg, _lib.ptr(partials),
                                             partials.numel() * 4, _lib.ptr(out), _lib.stream(dev)), "gags_mcmc_reg_fwd")
        ctx.save_for_backward(opacity, scaling)
        ctx.regs = (opacity_reg, scale_reg)
        return out.reshape(())

    @staticmethod
    def backward(ctx, v):
        opacity, scaling = ctx.saved_tensors
        op, sc = opacity.detach(), scaling.detach()
        dev = op.device
        vd = v.detach().reshape(1).float().contiguous()  # (read on the device: no readback inside the backward pass)
        v_op, v_sc = torch.empty_like(op), torch.empty_like(sc)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().gags_mcmc_reg_bwd(op.numel(), _lib.ptr(op), _lib.ptr(sc), *ctx.regs, _lib.ptr(vd),
                                                     _lib.ptr(v_op), _lib.ptr(v_sc), _lib.stream(dev)), "gags_mcmc_reg_bwd")
        return v_op, v_sc, None, None


def regularisation(model, opacity_reg=0.01, scale_reg=0.01):
    """opacity_reg mean(sigmoid(_opacity)) + scale_reg mean(exp(_scaling)) as one scalar with a closed-form backward."""
    _need_gpu(model._opacity, model._scaling)
    return _Regularisation.apply(model._opacity, model._scaling, float(opacity_reg), float(scale_reg))


# ---- R7 -------------------------------------------------------------------------------------------------------------------
class MCMCStrategy:
    def __init__(self, cap_max=1_000_000, noise_lr=5e5, refine_start_iter=500, refine_stop_iter=25_000, refine_every=100,
                 min_opacity=MIN_OPACITY):
        self.cap_max, self.noise_lr, self.min_opacity = int(cap_max), float(noise_lr), float(min_opacity)
        self.refine_start_iter, self.refine_stop_iter, self.refine_every = refine_start_iter, refine_stop_iter, refine_every

    def refines(self, step):
        return refines(step, self.refine_start_iter, self.refine_stop_iter, self.refine_every)

    def step_post_backward(self, model, step, lr, generator=None):
        """After backward (and the optimizer step) of iteration `step`: a refinement when the schedule says so -- relocate, then
        grow -- and the position noise, scaled by lr (the xyz group's) * noise_lr, always.  Returns (n_relocated, n_added)."""
        n_relocated = n_added = 0
        if self.refines(step):
            n_relocated = relocate(model, None, self.min_opacity, generator=generator)
            n_added = sample_add(model, self.cap_max, self.min_opacity, generator=generator)
        inject_noise(model, lr * self.noise_lr, generator=generator)
        return n_relocated, n_added
