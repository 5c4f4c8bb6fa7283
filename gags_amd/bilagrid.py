"""Bilateral grid colour correction (include/gags_next.h "N24", csrc/bilagrid.hip).

Every training image owns a small 3-D grid of 3 x 4 colour transforms, indexed by pixel position and by the pixel's own
luminance; the rendered image is corrected by the transform sliced out of its grid, so that exposure and white-balance
differences between the photographs of a capture are explained by the grids and not by floaters or view-dependent colour.
A total-variation term keeps the grids smooth.

    slice(grid, rgb)                grid [12, L, Gh, Gw], rgb [3,H,W] or [H,W,3] -> the corrected image, same logical shape
    total_variation_loss(grids)     grids [B, 12, L, Gh, Gw] -> scalar
    BilateralGrid(num, grid_X=16, grid_Y=16, grid_W=8)   .grids [num, 12, grid_W, grid_Y, grid_X], identity at the start

The rule (DESIGN.md 7 "N24"): channel 4 r + c of a grid is entry (r, c) of a 3 x 4 matrix, columns 0..2 multiply (R, G, B),
column 3 is the bias; the matrix of a pixel is the grid interpolated trilinearly at (column, row, luminance) --
torch.nn.functional.grid_sample(mode="bilinear", align_corners=True, padding_mode="border").  GPU tensors only: there is no
CPU path.
"""
import torch

from . import _lib
from ._lib import check, ptr

MAX_L, MAX_G = 16, 64  # what the kernels take: 2 <= L <= 16, 2 <= Gh, Gw <= 64


def _check_grid(grid, rank, what):
    if not torch.is_tensor(grid) or grid.dim() != rank or grid.shape[rank - 4] != 12:
        shape = tuple(grid.shape) if torch.is_tensor(grid) else type(grid).__name__
        raise ValueError(f"{what}: expected {'[B, 12, L, Gh, Gw]' if rank == 5 else '[12, L, Gh, Gw]'}, got {shape}")
    if grid.dtype != torch.float32:
        raise ValueError(f"{what}: expected float32, got {grid.dtype}")
    L, gh, gw = grid.shape[-3:]
    if not (2 <= L <= MAX_L and 2 <= gh <= MAX_G and 2 <= gw <= MAX_G):
        raise ValueError(f"{what}: grid sizes must be 2 <= L <= {MAX_L} and 2 <= Gh, Gw <= {MAX_G}, got L={L} Gh={gh} Gw={gw}")
    return L, gh, gw


def _image_view(rgb, what):
    """(channel-first?, h, w, element strides of plane / row / column) of a [3,H,W] or [H,W,3] float32 image read where it
    lies.  A [3,H,3] tensor is taken as [3,H,W]."""
    if not torch.is_tensor(rgb) or rgb.dim() != 3 or 3 not in (rgb.shape[0], rgb.shape[2]):
        shape = tuple(rgb.shape) if torch.is_tensor(rgb) else type(rgb).__name__
        raise ValueError(f"{what}: expected [3,H,W] or [H,W,3], got {shape}")
    if rgb.dtype != torch.float32:
        raise ValueError(f"{what}: expected float32, got {rgb.dtype}")
    if rgb.numel() == 0:
        raise ValueError(f"{what}: empty image {tuple(rgb.shape)}")
    if rgb.shape[0] == 3:
        return True, rgb.shape[1], rgb.shape[2], (rgb.stride(0), rgb.stride(1), rgb.stride(2))
    return False, rgb.shape[0], rgb.shape[1], (rgb.stride(2), rgb.stride(0), rgb.stride(1))


class _Slice(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grid, rgb):
        L, gh, gw = _check_grid(grid, 4, "bilagrid.slice: grid")
        chw, h, w, strides = _image_view(rgb, "bilagrid.slice: rgb")
        _lib.on_gpu("bilagrid", grid, rgb)
        if grid.device != rgb.device:
            raise ValueError(f"bilagrid.slice: grid on {grid.device}, rgb on {rgb.device}")
        grid = grid.contiguous()
        out = torch.empty(h, w, 3, device=rgb.device)
        check(_lib.load().gags_bilagrid_slice_fwd(L, gh, gw, h, w, ptr(grid), ptr(rgb), *strides, ptr(out), _lib.stream()),
              "gags_bilagrid_slice_fwd")
        ctx.save_for_backward(grid, rgb)
        ctx.geom = (L, gh, gw, h, w, strides, chw)
        return out.permute(2, 0, 1) if chw else out

    @staticmethod
    def backward(ctx, v_out):
        grid, rgb = ctx.saved_tensors
        L, gh, gw, h, w, strides, chw = ctx.geom
        need_grid, need_rgb = ctx.needs_input_grad
        if not (need_grid or need_rgb):
            return None, None
        v = v_out.permute(1, 2, 0) if chw else v_out  # [H,W,3] logically, read through whatever strides it has
        if v.dtype != torch.float32:
            v = v.float()
        lib = _lib.load()
        dev = rgb.device
        v_rgb = torch.empty(h, w, 3, device=dev) if need_rgb else None
        v_grid = torch.empty_like(grid) if need_grid else None
        nbytes = lib.gags_bilagrid_scratch_bytes(L, gh, gw) if need_grid else 0
        scratch = _lib.scratch(nbytes, dev) if need_grid else None
        check(lib.gags_bilagrid_slice_bwd(L, gh, gw, h, w, ptr(grid), ptr(rgb), *strides, ptr(v), v.stride(2), v.stride(0),
                                          v.stride(1), ptr(v_rgb), ptr(v_grid), ptr(scratch), nbytes, _lib.stream()),
              "gags_bilagrid_slice_bwd")
        if need_rgb and chw:
            v_rgb = v_rgb.permute(2, 0, 1)
        return v_grid, v_rgb


def slice(grid, rgb):  # noqa: A001  (gsplat's name for the operation)
    """The image `rgb` ([3,H,W] or [H,W,3], float32, any strides: the [3,H,W] view render() returns is read where it lies)
    corrected by `grid` [12, L, Gh, Gw]: the result has rgb's logical shape over fresh [H,W,3] memory.  Differentiable in
    both; the grid's gradient is bit-reproducible (no atomics), each gradient is computed only if needed."""
    return _Slice.apply(grid, rgb)


class _TotalVariation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grids):
        L, gh, gw = _check_grid(grids, 5, "bilagrid.total_variation_loss: grids")
        if grids.shape[0] < 1:
            raise ValueError("bilagrid.total_variation_loss: no grids")
        _lib.on_gpu("bilagrid", grids)
        g = grids.contiguous()
        lib = _lib.load()
        b = g.shape[0]
        partials = torch.empty(lib.gags_bilagrid_tv_partials(b, L, gh, gw), 3, dtype=torch.float64, device=g.device)
        out = torch.empty(1, device=g.device)
        check(lib.gags_bilagrid_tv_fwd(b, L, gh, gw, ptr(g), ptr(partials), ptr(out), _lib.stream()), "gags_bilagrid_tv_fwd")
        ctx.save_for_backward(g)
        return out[0]

    @staticmethod
    def backward(ctx, v):
        (g,) = ctx.saved_tensors
        b, _, L, gh, gw = g.shape
        vd = v.detach().reshape(1).float().contiguous()  # (read on the device: no readback inside the backward pass)
        v_g = torch.empty_like(g)
        check(_lib.load().gags_bilagrid_tv_bwd(b, L, gh, gw, ptr(g), ptr(vd), ptr(v_g), _lib.stream()), "gags_bilagrid_tv_bwd")
        return v_g


def total_variation_loss(grids):
    """(2 / B) sum over the axes d in (L, Gh, Gw) of mean_d (g[.. d + 1 ..] - g[.. d ..])^2 of grids [B, 12, L, Gh, Gw], mean_d
    over the differences of ONE image along d: one pass, double partial sums added in a fixed order."""
    return _TotalVariation.apply(grids)


class BilateralGrid(torch.nn.Module):
    """`num` grids, one per training image: .grids [num, 12, grid_W, grid_Y, grid_X] (grid_W levels of luminance), every node the
    identity transform at the start, so a fresh grid returns the image.  forward(rgb, idx) slices grid `idx`; tv_loss() is
    total_variation_loss of all of them."""

    def __init__(self, num, grid_X=16, grid_Y=16, grid_W=8):
        super().__init__()
        num = int(num)
        if num < 1:
            raise ValueError(f"BilateralGrid: num must be >= 1, got {num}")
        if not (2 <= grid_W <= MAX_L and 2 <= grid_Y <= MAX_G and 2 <= grid_X <= MAX_G):
            raise ValueError(f"BilateralGrid: 2 <= grid_W <= {MAX_L} and 2 <= grid_Y, grid_X <= {MAX_G} wanted, got "
                             f"grid_W={grid_W} grid_Y={grid_Y} grid_X={grid_X}")
        eye = torch.eye(4)[:3].reshape(12, 1, 1, 1)
        self.grids = torch.nn.Parameter(eye.repeat(num, 1, grid_W, grid_Y, grid_X).reshape(num, 12, grid_W, grid_Y, grid_X))

    def forward(self, rgb, idx):
        idx = int(idx)
        if not 0 <= idx < self.grids.shape[0]:
            raise IndexError(f"BilateralGrid: idx {idx} out of range for {self.grids.shape[0]} grids")
        return slice(self.grids[idx], rgb)

    def tv_loss(self):
        return total_variation_loss(self.grids)
