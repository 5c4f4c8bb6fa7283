"""Mean squared distance of every point to its three nearest neighbours (include/gags_next.h N9, csrc/knn.hip): what
`simple_knn._C.distCUDA2` computes for `GaussianModel.create_from_pcd` (scene/gaussian_model.py:167), whose square root
becomes the initial scale of each Gaussian.

    from gags_amd import distCUDA2          # instead of: from simple_knn._C import distCUDA2

The result is defined to the bit: for point i over all j != i, d2 = (dx*dx + dy*dy) + dz*dz in float32 without FMA, the three
smallest values b0 <= b1 <= b2, dist2[i] = ((b0 + b1) + b2) / 3 -- equal to a float32 brute force (tests/knn_ref.py).
There is no CPU path."""

import torch

from . import _lib
from ._lib import check, ptr

BOX = 256  # sorted points per box of the traversal (csrc/knn.hip KNN_BOX): the sizes at which the kernel changes path


@torch.no_grad()
def dist2(points):
    """points [N, 3] on the GPU, N >= 4 -> [N] float32.  Float32 contiguous input is used as it is, anything else is
    converted first (a float64 cloud is ROUNDED to float32, as the reference's `.float().cuda()` does)."""
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"gags_amd.knn.dist2: points must be [N, 3], got {tuple(points.shape)}")
    n = points.shape[0]
    if n < 4:
        raise ValueError(f"gags_amd.knn.dist2: {n} points, but three neighbours need at least 4")
    if not points.is_cuda:
        raise RuntimeError("gags_amd.knn.dist2: no CPU path (the points must live on the GPU)")
    p = points.detach().float().contiguous()
    out = torch.empty(n, dtype=torch.float32, device=p.device)
    lib = _lib.load()
    nb = lib.gags_knn3_dist2_scratch_bytes(n)
    scratch = _lib.scratch(nb, p.device)
    with torch.cuda.device(p.device):
        check(lib.gags_knn3_dist2(n, ptr(p), ptr(out), ptr(scratch), nb, _lib.stream()), "gags_knn3_dist2")
    return out


distCUDA2 = dist2
