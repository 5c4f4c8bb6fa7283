#!/usr/bin/env python
"""Generate tests/golden/photometric_vectors.npz by IMPORTING the reference's own Python (a checkout of it: the
environment variable GAGS_REFERENCE, default /root/reference): inputs and results of the RGB stage's photometric loss.  Only data is stored.

    python tests/golden/make_golden_photometric.py

For every case `<kind>_<shape>` (kinds and shapes below):
  _x, _y        the image and the ground truth, float32
  _ssim         utils/loss_utils.py:168-198 ssim(x, y)
  _l1           utils/loss_utils.py:20 l1_loss(x, y)
  _psnr         utils/image_utils.py:17-19 psnr(x, y)   ([shape[0], 1]: the first dimension is the reference's batch)
  _loss         (1 - 0.2) * l1 + 0.2 * (1 - ssim)       (train.py's photometric loss at arguments/__init__.py:88's lambda_dssim)
  _grad         d loss / d x by autograd
  _ssimb        ssim(x, y, size_average=False)          (the batch case only: the reference's form needs four dimensions)
each twice: suffix 64 = the reference run on float64 copies of the float32 inputs, suffix 32 = run on the float32 inputs.
  window        the eleven taps of utils/loss_utils.py:158-160 gaussian(11, 1.5), float32
  floor_value   the largest |float32 - float64| over ssim, l1 and loss of the cases that are not `flat`
  floor_grad    the largest max|grad32 - grad64| / max|grad64| over the same cases
"""
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("GAGS_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "photometric_vectors.npz")

SHAPES = [(3, 5, 7), (3, 16, 16), (3, 33, 17), (3, 47, 63), (1, 64, 48), (2, 3, 20, 24)]
KINDS = ("near", "rand", "flat")
LAMBDA = 0.2


def case_name(kind, shape):
    return kind + "_" + "x".join(str(s) for s in shape)


def make_inputs(kind, shape, g):
    if kind == "near":  # a render close to its target; a few pixels EXACTLY on it (sign(0) = 0 in the L1 gradient)
        y = torch.rand(shape, generator=g)
        x = (y + 0.05 * torch.randn(shape, generator=g)).clamp(0.0, 1.0)
        flat_x, flat_y = x.reshape(-1), y.reshape(-1)
        idx = torch.randperm(flat_x.numel(), generator=g)[:max(3, flat_x.numel() // 50)]
        flat_x[idx] = flat_y[idx]
    elif kind == "rand":
        x, y = torch.rand(shape, generator=g), torch.rand(shape, generator=g)
    else:  # low contrast: E[x^2] - mu^2 cancels
        x = 0.5 + 1e-3 * torch.rand(shape, generator=g)
        y = x + 1e-3 * torch.randn(shape, generator=g)
    return x.float().contiguous(), y.float().contiguous()


def main():
    for name in ("cv2", "matplotlib", "matplotlib.pyplot"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
    sys.path.insert(0, REF)
    from utils import loss_utils as LU
    from utils import image_utils as IU

    def run(x, y, dtype):
        x = x.to(dtype).requires_grad_(True)
        y = y.to(dtype)
        s, l1 = LU.ssim(x, y), LU.l1_loss(x, y)
        loss = (1.0 - LAMBDA) * l1 + LAMBDA * (1.0 - s)
        (grad,) = torch.autograd.grad(loss, x)
        res = {"ssim": s, "l1": l1, "psnr": IU.psnr(x, y), "loss": loss, "grad": grad}
        if x.dim() == 4:
            res["ssimb"] = LU.ssim(x, y, size_average=False)
        return {k: v.detach().numpy() for k, v in res.items()}

    out = {"window": LU.gaussian(11, 1.5).float().numpy()}
    g = torch.Generator().manual_seed(20260)
    floor_value = floor_grad = 0.0
    for kind in KINDS:
        for shape in SHAPES:
            x, y = make_inputs(kind, shape, g)
            name = case_name(kind, shape)
            out[name + "_x"], out[name + "_y"] = x.numpy(), y.numpy()
            r64, r32 = run(x, y, torch.float64), run(x, y, torch.float32)
            for k, v in r64.items():
                out[f"{name}_{k}64"] = v
            for k, v in r32.items():
                out[f"{name}_{k}32"] = v
            dv = max(abs(float(r32[k]) - float(r64[k])) for k in ("ssim", "l1", "loss"))
            dg = float(np.abs(r32["grad"].astype(np.float64) - r64["grad"]).max() / np.abs(r64["grad"]).max())
            print(f"{name:18s} |ssim32 - ssim64| {abs(float(r32['ssim']) - float(r64['ssim'])):.2e}  value {dv:.2e}  grad {dg:.2e}")
            if kind != "flat":
                floor_value, floor_grad = max(floor_value, dv), max(floor_grad, dg)
    out["floor_value"], out["floor_grad"] = np.array(floor_value), np.array(floor_grad)
    print(f"floor_value {floor_value:.3e}  floor_grad {floor_grad:.3e}")
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
