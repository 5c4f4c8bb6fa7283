"""Optimizer of the distillation flow.

The reference optimises exactly one tensor, `_semantic_feature [N, D]`, with
`torch.optim.Adam(l, lr=0.0, eps=1e-15)` and a per-group lr (`/root/reference/scene/gaussian_model.py:192-208`),
stepped once per iteration (`/root/reference/train.py:221-223`).  `FeatureAdam` keeps that constructor, the
`step()/zero_grad()/state_dict()` interface and the state layout (`step`, `exp_avg`, `exp_avg_sq`) but runs the
update as ONE pass of a hand-written HIP kernel (`gags_adam_step`): 28 B of HBM traffic per element instead of
the several passes of the stock implementation.  GPU tensors only -- there is no CPU path.

`SelectiveAdam` is the opt-in row-selective variant: rows of the `[N, ...]` parameters that a visibility
mask leaves out, or whose gradient row is all zero, are not touched -- parameter and both moments keep their bits, the
moments do not decay -- and all parameters of a step go into one launch of `gags_adam_step_rows` per 8 tensors.
"""
import ctypes

import torch

from . import _lib


class FeatureAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False):
        if weight_decay != 0 or amsgrad:
            raise NotImplementedError("the reference uses plain Adam (no weight decay, no amsgrad)")
        if not 0.0 <= lr or not 0.0 <= eps or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("invalid Adam hyper-parameter")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=0, amsgrad=False))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not p.is_cuda:
                    raise RuntimeError("gags_amd.optim.FeatureAdam: no CPU path (parameters must live on the GPU)")
                if p.dtype != torch.float32 or p.grad.dtype != torch.float32 or p.grad.is_sparse:
                    raise RuntimeError("FeatureAdam: dense float32 parameters and gradients only")
                if not p.is_contiguous():
                    raise RuntimeError("FeatureAdam: parameter must be contiguous")
                g = p.grad.contiguous()
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["step"] += 1
                with torch.cuda.device(p.device):
                    stream = _lib.stream(p.device)
                    _lib.check(lib.gags_adam_step(p.numel(), _lib.ptr(p), _lib.ptr(g), _lib.ptr(st["exp_avg"]),
                                                  _lib.ptr(st["exp_avg_sq"]), float(group["lr"]), float(b1), float(b2),
                                                  float(group["eps"]), int(st["step"].item()), stream),
                               "gags_adam_step")
                # the kernel wrote `p` through its raw pointer: move the version counter as torch's own optimizers do, for
                # everything keyed on it (decoders._pack_weights' cache of packed weights, autograd's saved-tensor checks)
                torch.autograd.graph.increment_version(p)
        return loss


class SelectiveAdam(FeatureAdam):
    """FeatureAdam's constructor, state layout and checkpoints; `step(visibility)` updates only the selected rows.

    skip_zero_rows: a row whose gradient row holds no non-zero bit pattern (-0.0 is zero, NaN is not) is skipped, per
    parameter.  bias_correction=False: step_size = lr and sqrt(exp_avg_sq) is not rescaled.  Both are
    attributes of the optimizer, not of its groups, so that a state_dict loads into a FeatureAdam and back."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, skip_zero_rows=False,
                 bias_correction=True):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad)
        self.skip_zero_rows = bool(skip_zero_rows)
        self.bias_correction = bool(bias_correction)

    @torch.no_grad()
    def step(self, visibility=None, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        work = []  # (parameter, contiguous gradient, state, group)
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not p.is_cuda:
                    raise RuntimeError("gags_amd.optim.SelectiveAdam: no CPU path (parameters must live on the GPU)")
                if p.dtype != torch.float32 or p.grad.dtype != torch.float32 or p.grad.is_sparse:
                    raise RuntimeError("SelectiveAdam: dense float32 parameters and gradients only")
                if not p.is_contiguous():
                    raise RuntimeError("SelectiveAdam: parameter must be contiguous")
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                work.append((p, p.grad.contiguous(), st, group))
        if not work:
            return loss
        dev = work[0][0].device
        firsts = {p.shape[0] if p.dim() else 1 for p, _, _, _ in work}
        mask = None
        if visibility is not None:
            if not torch.is_tensor(visibility) or not visibility.is_cuda or visibility.device != dev:
                raise RuntimeError("gags_amd.optim.SelectiveAdam: no CPU path (visibility must live on the parameters' GPU)")
            if visibility.dtype not in (torch.bool, torch.uint8) or visibility.dim() != 1:
                raise RuntimeError("SelectiveAdam: visibility is a [N] bool or uint8 tensor")
            if firsts != {visibility.numel()}:
                raise RuntimeError(f"SelectiveAdam: visibility has {visibility.numel()} rows, the parameters' first dimensions "
                                   f"are {sorted(firsts)}")
            mask = visibility.contiguous()
            mask = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
        # one row count per launch: N when the parameters agree on it, else every parameter is ONE row (a dense step)
        n_rows = firsts.pop() if len(firsts) == 1 else 1
        if any(p.device != dev for p, _, _, _ in work):
            raise RuntimeError("SelectiveAdam: parameters on one device only")
        flags = (_lib.GAGS_ADAM_SKIP_ZERO_ROWS if self.skip_zero_rows else 0) | \
                (0 if self.bias_correction else _lib.GAGS_ADAM_NO_BIAS_CORRECTION)
        by_step = {}  # the kernel takes one global step per launch: parameters of one count travel together
        for p, g, st, group in work:
            st["step"] += 1
            if n_rows == 0 or p.numel() == 0:
                continue
            b1, b2 = group["betas"]
            desc = _lib.AdamTensor(p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                                   p.numel() // n_rows, float(group["lr"]), float(b1), float(b2), float(group["eps"]))
            by_step.setdefault(int(st["step"].item()), []).append(desc)
        lib = _lib.load()
        with torch.cuda.device(dev):
            stream = _lib.stream(dev)
            for count, descs in by_step.items():
                d = descs[0]
                if len(work) == 1 and mask is None and flags == 0 and (d.param | d.grad | d.exp_avg | d.exp_avg_sq) % 16 == 0:
                    # one tensor and nothing to select: the dense kernel writes the same bits and is the faster of the two on
                    # narrow rows (docs/LAB_NOTES.md "Selective Adam (N19)")
                    _lib.check(lib.gags_adam_step(n_rows * d.width, d.param, d.grad, d.exp_avg, d.exp_avg_sq, d.lr, d.beta1,
                                                  d.beta2, d.eps, count, stream), "gags_adam_step")
                    continue
                for k in range(0, len(descs), _lib.GAGS_ADAM_MAX_TENSORS):
                    part = descs[k:k + _lib.GAGS_ADAM_MAX_TENSORS]
                    table = (_lib.AdamTensor * len(part))(*part)
                    _lib.check(lib.gags_adam_step_rows(n_rows, len(part), ctypes.cast(table, ctypes.c_void_p), _lib.ptr(mask),
                                                       flags, count, stream), "gags_adam_step_rows")
        for p, _, _, _ in work:  # as FeatureAdam.step: the kernel wrote through raw pointers
            torch.autograd.graph.increment_version(p)
        return loss
