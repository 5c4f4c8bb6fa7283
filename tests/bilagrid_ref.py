"""N24: the float64 reference of the bilateral grid (include/gags_next.h "N24", DESIGN.md 7 "N24"), the inputs of its tests
and the error yardstick.

Two statements of the same rule:
  * the tent form in plain torch (slice_tent, grads_tent): the sum over ALL nodes with tent(t) = max(0, 1 - |t|) weights, and the
    backward written out as the rule states it (the guide's slope in the cell [floor z, floor z + 1], none through a clamped
    or boundary coordinate) -- nothing is left to autograd's choice of a subgradient;
  * the torch.nn.functional.grid_sample composition (slice_grid_sample), differentiated by autograd, in any dtype on any
    device: in float64 on the CPU it pins the tent form (tests/test_bilagrid_cpu.py), in float32 on the GPU it is the
    yardstick the kernels' error is measured with (tests/test_bilagrid_gpu.py).
Images here are [H, W, 3]; grids [12, L, Gh, Gw].
"""
import numpy as np
import torch

GRAY = (0.299, 0.587, 0.114)
FRAC_LO, FRAC_HI = 0.05, 0.95
EDGE_PIXELS = {"negative": (-0.2, -0.1, -0.3), "above": (1.3, 1.2, 1.5), "black": (0.0, 0.0, 0.0)}


def tent(t):
    return torch.clamp(1.0 - t.abs(), min=0.0)


def _coords(h, w, L, gh, gw, rgb):
    """x [W], y [H], gray [H,W], z [H,W] of the rule, in rgb's dtype."""
    dt = rgb.dtype
    x = ((torch.arange(w, dtype=dt) + 0.5) / w) * (gw - 1)
    y = ((torch.arange(h, dtype=dt) + 0.5) / h) * (gh - 1)
    gray = (GRAY[0] * rgb[..., 0] + GRAY[1] * rgb[..., 1]) + GRAY[2] * rgb[..., 2]
    z = gray.clamp(0.0, 1.0) * (L - 1)
    return x, y, gray, z


def _weights(grid, rgb):
    _, L, gh, gw = grid.shape
    h, w, _ = rgb.shape
    x, y, gray, z = _coords(h, w, L, gh, gw, rgb)
    wx = tent(x[:, None] - torch.arange(gw, dtype=rgb.dtype))           # [W, Gw]
    wy = tent(y[:, None] - torch.arange(gh, dtype=rgb.dtype))           # [H, Gh]
    wz = tent(z[..., None] - torch.arange(L, dtype=rgb.dtype))          # [H, W, L]
    return wx, wy, wz, gray, z


def _apply(A, rgb):
    """out[r] = A[4r] R + A[4r+1] G + A[4r+2] B + A[4r+3]; A [12,H,W], rgb [H,W,3] -> [H,W,3]."""
    A = A.reshape(3, 4, *A.shape[1:])
    p = rgb.permute(2, 0, 1)
    return ((A[:, :3] * p[None]).sum(1) + A[:, 3]).permute(1, 2, 0)


def slice_tent(grid, rgb):
    """The rule's forward: grid [12,L,Gh,Gw], rgb [H,W,3] (same dtype, CPU) -> [H,W,3]."""
    wx, wy, wz, _, _ = _weights(grid, rgb)
    A = torch.einsum("clmn,ijl,im,jn->cij", grid, wz, wy, wx)
    return _apply(A, rgb)


def grads_tent(grid, rgb, v_out):
    """(v_grid, v_rgb) of the rule's backward, written out; also returns the guide term alone (v_rgb's second summand)."""
    _, L, gh, gw = grid.shape
    wx, wy, wz, gray, z = _weights(grid, rgb)
    p1 = torch.cat([rgb, torch.ones_like(rgb[..., :1])], -1)                         # [H,W,4]
    v_A = (v_out[..., :, None] * p1[..., None, :]).reshape(*rgb.shape[:2], 12).permute(2, 0, 1)   # [12,H,W], channel 4r + c
    v_grid = torch.einsum("cij,ijl,im,jn->clmn", v_A, wz, wy, wx)
    A = torch.einsum("clmn,ijl,im,jn->cij", grid, wz, wy, wx).reshape(3, 4, *rgb.shape[:2])
    direct = torch.einsum("rcij,ijr->ijc", A[:, :3], v_out)
    z0 = z.floor().clamp(max=L - 2).long()
    lv = torch.arange(L)
    dwz = (lv == (z0[..., None] + 1)).to(rgb.dtype) - (lv == z0[..., None]).to(rgb.dtype)   # slope in the cell [z0, z0 + 1]
    dA = torch.einsum("clmn,ijl,im,jn->cij", grid, dwz, wy, wx)
    zu = gray * (L - 1)
    m = ((zu > 0) & (zu < L - 1)).to(rgb.dtype)
    guide = (m * (L - 1) * (dA * v_A).sum(0))[..., None] * torch.tensor(GRAY, dtype=rgb.dtype)
    return v_grid, direct + guide, guide


def reached(grid_shape, rgb):
    """[L,Gh,Gw] bool: nodes with a non-zero weight from some pixel.  Everywhere else the reference's v_grid is exactly 0."""
    dummy = torch.zeros(grid_shape, dtype=rgb.dtype)
    wx, wy, wz, _, _ = _weights(dummy, rgb)
    return torch.einsum("ijl,im,jn->lmn", wz, wy, wx) > 0


def slice_grid_sample(grid, rgb):
    """The same slice as a composition of torch operators, in grid's dtype on grid's device, differentiable by autograd."""
    _, L, gh, gw = grid.shape
    h, w, _ = rgb.shape
    dt, dev = rgb.dtype, rgb.device
    xs = (torch.arange(w, dtype=dt, device=dev) + 0.5) / w
    ys = (torch.arange(h, dtype=dt, device=dev) + 0.5) / h
    gray = (GRAY[0] * rgb[..., 0] + GRAY[1] * rgb[..., 1]) + GRAY[2] * rgb[..., 2]
    coords = torch.stack([(2 * xs - 1)[None, :].expand(h, w), (2 * ys - 1)[:, None].expand(h, w), 2 * gray - 1], -1)
    A = torch.nn.functional.grid_sample(grid[None], coords[None, None], mode="bilinear", align_corners=True,
                                        padding_mode="border")[0, :, 0]      # [12,H,W]
    return _apply(A, rgb)


def value_and_grads(fn, grid, rgb, v_out):
    """(out, v_grid, v_rgb) of a differentiable slice `fn` by autograd."""
    g = grid.detach().clone().requires_grad_(True)
    p = rgb.detach().clone().requires_grad_(True)
    out = fn(g, p)
    out.backward(v_out)
    return out.detach(), g.grad, p.grad


# ---- inputs --------------------------------------------------------------------------------------------------------------------

def gray64(rgb):
    r = rgb.double()
    return (GRAY[0] * r[..., 0] + GRAY[1] * r[..., 1]) + GRAY[2] * r[..., 2]


def edge_kind(rgb):
    """[H,W] int: 0 an interior pixel, 1 gray < 0, 2 gray > 1, 3 exact black."""
    g = gray64(rgb)
    black = (rgb == 0).all(-1)
    return torch.where(black, 3, torch.where(g < 0, 1, torch.where(g > 1, 2, 0)))


def check_inputs(rgb, L):
    """The property the tests' images are built to have, checked in float64 on the float32 values: every pixel is one of the
    deliberate edge pixels or has 0 < gray < 1 with frac(gray (L - 1)) in [FRAC_LO, FRAC_HI].  Returns edge_kind(rgb)."""
    kind = edge_kind(rgb)
    z = gray64(rgb) * (L - 1)
    frac = z - z.floor()
    ok = (kind > 0) | ((z > 0) & (z < L - 1) & (frac >= FRAC_LO) & (frac <= FRAC_HI))
    assert bool(ok.all()), f"{int((~ok).sum())} pixels are neither edge pixels nor inside [{FRAC_LO}, {FRAC_HI}]"
    return kind


def make_image(h, w, L, seed, edges=True, force=None):
    """rgb [H,W,3] float32 with check_inputs' property.  Interior pixels: colours in (0.02, 0.98) rescaled so that the
    fraction of gray (L - 1) lies in [0.1, 0.9].  edges: with at least 6 pixels, pixels 1, P // 2 and P - 1 become the three
    EDGE_PIXELS.  force: the name of an edge pixel that pixel 0 becomes (for images too small for `edges`)."""
    rng = np.random.default_rng(seed)
    rgb = torch.from_numpy(rng.uniform(0.05, 0.95, (h, w, 3))).double()
    z = gray64(rgb) * (L - 1)
    cell = z.floor()
    frac = (z - cell).clamp(0.1, 0.9)
    rgb = (rgb * ((cell + frac) / z)[..., None]).float()
    flat = rgb.reshape(-1, 3)
    n = flat.shape[0]
    if edges and n >= 6:
        for pos, name in zip((1, n // 2, n - 1), EDGE_PIXELS):
            flat[pos] = torch.tensor(EDGE_PIXELS[name])
    if force is not None:
        flat[0] = torch.tensor(EDGE_PIXELS[force])
    check_inputs(rgb, L)
    return rgb


def make_grid(L, gh, gw, seed, spread=0.3):
    """[12,L,Gh,Gw] float32: the identity transform plus noise."""
    g = torch.Generator().manual_seed(seed)
    eye = torch.eye(4)[:3].reshape(12, 1, 1, 1)
    return (eye + spread * torch.randn(12, L, gh, gw, generator=g)).float()


def smooth_grid(L, gh, gw, gain=0.25):
    """A known smooth grid: a colour transform that drifts across the image and with luminance (the target of the short loop)."""
    zz, yy, xx = torch.meshgrid(torch.linspace(0, 1, L), torch.linspace(0, 1, gh), torch.linspace(0, 1, gw), indexing="ij")
    g = torch.eye(4)[:3].reshape(12, 1, 1, 1).repeat(1, L, gh, gw)
    g[0] += gain * xx
    g[5] -= gain * yy
    g[10] += gain * zz
    g[3] += 0.1 * gain * (xx - yy)
    g[1] += 0.5 * gain * zz * xx
    return g.float()


def make_cotangent(h, w, seed):
    g = torch.Generator().manual_seed(seed + 1000)
    return torch.randn(h, w, 3, generator=g)


# ---- TV ------------------------------------------------------------------------------------------------------------------------

def tv_ref(grids):
    """(2 / B) sum_d sum (forward difference along d)^2 / n_d, n_d the differences of one image; grids [B,12,L,Gh,Gw]."""
    b = grids.shape[0]
    total = 0.0
    for d in (2, 3, 4):
        diff = grids.narrow(d, 1, grids.shape[d] - 1) - grids.narrow(d, 0, grids.shape[d] - 1)
        total = total + (diff ** 2).sum() / (diff.numel() // b)
    return 2.0 * total / b


# ---- the short loop ------------------------------------------------------------------------------------------------------------

def sgd_loop_ref(grids, idx, rgb, target, lr, steps):
    """`steps` plain-SGD steps on mean((slice(grids[idx], rgb) - target)^2) in grids' dtype on the CPU, with the rule's own
    backward; returns the grids afterwards."""
    grids = grids.clone()
    for _ in range(steps):
        out = slice_tent(grids[idx], rgb)
        v_out = 2.0 * (out - target) / out.numel()
        v_grid, _, _ = grads_tent(grids[idx], rgb, v_out)
        grids[idx] -= lr * v_grid
    return grids


# ---- the yardstick -------------------------------------------------------------------------------------------------------------

def bound(yardstick_err, ref):
    """What a kernel's max abs error against the float64 reference `ref` may be: 4 x the error of the float32 torch composition
    of the same inputs (two fp32 evaluations of the same sums in different orders differ by small factors: the N15 precedent),
    with a floor of 8 float32 ulps of the reference's largest magnitude for cases where that error happens to be zero."""
    floor = 8.0 * float(np.spacing(np.float32(float(ref.abs().max()))))
    return max(4.0 * float(yardstick_err), floor)
