"""Float64 restatement of the RGB stage's photometric loss in plain torch, without the reference:
utils/loss_utils.py:20 l1_loss, :158-198 gaussian / create_window / ssim / _ssim, utils/image_utils.py:17-19 psnr and
(1 - lambda) l1 + lambda (1 - ssim).  tests/test_photometric_cpu.py ties it to the reference's own float64 results
(tests/golden/photometric_vectors.npz) to 1e-12; the GPU tests use it as the yardstick at shapes the fixture does not hold.
Runs on the CPU (or on whatever device its inputs live on); inputs of any float type are taken to float64 first."""
import math

import torch
import torch.nn.functional as F

C1, C2 = 0.01 ** 2, 0.03 ** 2


def window_1d():
    """The eleven taps as the reference forms them: exp(-(x - 5)^2 / (2 * 1.5^2)) in Python doubles, rounded into a float32
    tensor, divided by its float32 sum."""
    g = torch.tensor([math.exp(-(x - 5) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)], dtype=torch.float32)
    return g / g.sum()


def window_2d(channel, like):
    """[channel, 1, 11, 11]: the float32 outer product of the taps, THEN converted (the reference's `window.type_as`)."""
    w = window_1d()[:, None]
    return (w @ w.t()).float()[None, None].expand(channel, 1, 11, 11).contiguous().to(like)


def ssim_map(x, y):
    x, y = x.double(), y.double()
    squeeze = x.dim() == 3
    if squeeze:
        x, y = x[None], y[None]
    c = x.shape[1]
    win = window_2d(c, x)
    mu1, mu2 = F.conv2d(x, win, padding=5, groups=c), F.conv2d(y, win, padding=5, groups=c)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1 = F.conv2d(x * x, win, padding=5, groups=c) - mu1_sq
    s2 = F.conv2d(y * y, win, padding=5, groups=c) - mu2_sq
    s12 = F.conv2d(x * y, win, padding=5, groups=c) - mu1_mu2
    m = ((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))
    return m[0] if squeeze else m


def ssim(x, y, size_average=True):
    m = ssim_map(x, y)
    return m.mean() if size_average else m.reshape(m.shape[0], -1).mean(1)


def l1_loss(x, y):
    return (x.double() - y.double()).abs().mean()


def psnr(x, y):
    mse = ((x.double() - y.double()) ** 2).reshape(x.shape[0], -1).mean(1, keepdim=True)
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


def photometric_loss(x, y, lambda_dssim=0.2):
    return (1.0 - lambda_dssim) * l1_loss(x, y) + lambda_dssim * (1.0 - ssim(x, y))


def value_and_grad(fn, x, *args):
    """(fn(x, *args) float64, d sum(fn) / d x float64) by autograd on a float64 copy of x."""
    xd = x.detach().double().requires_grad_(True)
    v = fn(xd, *args)
    (g,) = torch.autograd.grad(v.sum(), xd)
    return v.detach(), g
