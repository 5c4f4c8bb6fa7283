"""Shared input builders for the parity tests (seeded, CPU-generated so that the oracle and
the GPU see bit-identical inputs)."""
import contextlib

import numpy as np
import torch

from gags_amd import synthetic as syn


def scene_arrays(n, d, width, height, seed=0, view=None, scale_mult=1.0, sh=False):
    """Activated parameters as numpy arrays + camera matrices (what crosses the rasterization boundary)."""
    cam = syn.make_camera(width, height, view=view, device="cpu")
    p = syn.make_gaussians(n, d, width, height, seed=seed, scale0=syn.SCALE0 * scale_mult)
    vm, K = syn.camera_matrices(cam)
    out = dict(
        means=p["xyz"].numpy(),
        quats=torch.nn.functional.normalize(p["rotation"]).numpy(),
        scales=p["scaling_log"].exp().numpy(),
        opacities=torch.sigmoid(p["opacity_logit"]).reshape(-1).numpy(),
        colors=None if d == 0 else p["semantic_feature"].numpy(),
        sh=torch.cat([p["features_dc"], p["features_rest"]], dim=1).numpy(),
        viewmat=vm.numpy().copy(), K=K, cam=cam, raw=p)
    return out


def _ypr_rotation(yaw, pitch, roll):
    """Camera-to-world rotation Ry(yaw) Rx(pitch) Rz(roll), float64."""
    cy_, sy_, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Ry = np.array([[cy_, 0.0, sy_], [0.0, 1.0, 0.0], [-sy_, 0.0, cy_]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, cp, -sp], [0.0, sp, cp]])
    Rz = np.array([[cr, -sr, 0.0], [sr, cr, 0.0], [0.0, 0.0, 1.0]])
    return Ry @ Rx @ Rz


def general_scene(n, d, width, height, seed, *, fx, fy, cx, cy, ypr, centre, spread, scale_mult, z_range=(2, 12)):
    """scene_arrays for a COLMAP-like camera: camera-to-world rotation R from (yaw, pitch, roll), camera centre C anywhere,
    viewmat = [R^T | -R^T C], fx != fy and an arbitrary principal point.  The Gaussians are drawn in the camera frame --
    pixel position uniform over `spread` x the image about its centre, unprojected through this K at a depth uniform in
    `z_range` -- and moved to world coordinates; every other parameter is make_gaussians' for the seed.  spread > 1.3 puts
    Gaussians beyond the tangent clamp of the projection (pixel outside [-0.15 W, 1.15 W], likewise in y)."""
    R = _ypr_rotation(*ypr)
    C = np.asarray(centre, np.float64)
    vm = np.eye(4)
    vm[:3, :3] = R.T
    vm[:3, 3] = -R.T @ C
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32)
    p = syn.make_gaussians(n, d, width, height, seed=seed, scale0=syn.SCALE0 * scale_mult)
    g = torch.Generator(device="cpu")
    g.manual_seed(seed + 7919)
    u = torch.rand(n, 3, generator=g, dtype=torch.float64).numpy()
    px = 0.5 * width + (u[:, 0] - 0.5) * spread * width
    py = 0.5 * height + (u[:, 1] - 0.5) * spread * height
    z = z_range[0] + (z_range[1] - z_range[0]) * u[:, 2]
    pc = np.stack([(px - cx) / fx * z, (py - cy) / fy * z, z], axis=1)
    p["xyz"] = torch.from_numpy((pc @ R.T + C).astype(np.float32))
    return dict(
        means=p["xyz"].numpy(),
        quats=torch.nn.functional.normalize(p["rotation"]).numpy(),
        scales=p["scaling_log"].exp().numpy(),
        opacities=torch.sigmoid(p["opacity_logit"]).reshape(-1).numpy(),
        colors=None if d == 0 else p["semantic_feature"].numpy(),
        sh=torch.cat([p["features_dc"], p["features_rest"]], dim=1).numpy(),
        viewmat=vm.astype(np.float32), K=K, cam=None, raw=p, R=R, C=C)


# General cameras shared by the CPU and the GPU tests, in units of the image (fx, fy, cx, cy are multiplied by W, W, W, H):
# yaw / pitch / roll up to 2.5 rad, |C| up to ~10, fx/fy from 0.75 to 1.4, principal point off-centre and, in "pp_outside",
# left of the image.
GENERAL_CAMERAS = {
    "pitch_roll": dict(fx=0.94, fy=0.70, cx=0.47, cy=0.54, ypr=(0.7, -0.4, 0.3), centre=(3.0, -1.5, 7.0), spread=1.5),
    "behind": dict(fx=0.70, fy=0.92, cx=0.56, cy=0.42, ypr=(2.5, 1.1, -2.0), centre=(-6.0, 4.0, -5.0), spread=1.6),
    "pp_outside": dict(fx=1.10, fy=0.78, cx=-0.15, cy=0.51, ypr=(-1.2, 0.5, 2.5), centre=(0.5, -9.0, 3.0), spread=1.9),
    "upside_down": dict(fx=0.80, fy=0.95, cx=0.52, cy=0.62, ypr=(0.2, -2.2, 0.9), centre=(5.0, 5.0, -6.0), spread=1.7),
}


def general_camera(name, width, height):
    """Keyword arguments of general_scene for one of GENERAL_CAMERAS at an image size."""
    c = GENERAL_CAMERAS[name]
    return dict(fx=c["fx"] * width, fy=c["fy"] * width, cx=c["cx"] * width, cy=c["cy"] * height, ypr=c["ypr"],
                centre=c["centre"], spread=c["spread"])


def clamp_census(s, width, height, radii):
    """(visible Gaussians with an active tangent clamp in x, in y, visible, culled) for a scene and the radii it produced:
    float64 restatement of the limits of SURVEY A3 (x/z outside [-(cx/fx + 0.3 tan), (W - cx)/fx + 0.3 tan])."""
    vm, K = s["viewmat"].astype(np.float64), s["K"].astype(np.float64)
    p = s["means"].astype(np.float64) @ vm[:3, :3].T + vm[:3, 3]
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    xr, yr = p[:, 0] / p[:, 2], p[:, 1] / p[:, 2]
    out_x = (xr > (width - cx) / fx + 0.15 * width / fx) | (xr < -(cx / fx + 0.15 * width / fx))
    out_y = (yr > (height - cy) / fy + 0.15 * height / fy) | (yr < -(cy / fy + 0.15 * height / fy))
    vis = np.asarray(radii) > 0
    return int((vis & out_x).sum()), int((vis & out_y).sum()), int(vis.sum()), int((~vis).sum())


def rel_l2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def to_dev(a, dev="cuda"):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@contextlib.contextmanager
def spy_entries(*names):
    """Counting spies on entries of the loaded library (the pattern of tests/test_route_gpu.py): yields the list that
    receives (name, args) of every call, in order.  For A/B tests that must show that B ran."""
    from gags_amd import _lib
    lib, calls = _lib.load(), []
    real = {name: getattr(lib, name) for name in names}

    def spy(name):
        def f(*args):
            calls.append((name, args))
            return real[name](*args)
        return f
    for name in names:
        setattr(lib, name, spy(name))
    try:
        yield calls
    finally:
        for name in names:
            setattr(lib, name, real[name])


# The default forward of an fp32 table contracts its 128-channel slices on the 16-bit matrix cores with both operands split
# into three bf16 terms (exact operands, products to 2^-23, fp32 accumulation by the matrix core): as close to the exact sum
# as the sequential fp32 fmaf chain of the oracle -- both sit ~2e-7 (rel-L2) from the float64 sum at C3
# (tests/test_fullsize_gpu.py::test_default_forward_is_as_close_to_float64_as_the_exact_kernel) -- but not bit-identical to
# it.  Two fp32 evaluations of one sum that are each ~2e-7 from the truth differ by up to ~3e-7; measured 2.8e-7 at C3.
# GAGS_FWD_EXACT selects the kernel that IS the oracle's chain, bit for bit.
FWD_SPLIT_TOL = 5e-7


def check_forward(out, o_out, out_exact=None):
    """Default-forward render against the oracle: bit-identical below 128 channels (those widths run the exact fp32 kernels),
    within FWD_SPLIT_TOL from there on; `out_exact` (rendered with GAGS_FWD_EXACT) must be bit-identical at any width."""
    out, o_out = np.asarray(out), np.asarray(o_out)
    if o_out.shape[-1] < 128:
        np.testing.assert_array_equal(out, o_out)
    else:
        e = rel_l2(out, o_out)
        assert e <= FWD_SPLIT_TOL, e
        tail = o_out.shape[-1] - o_out.shape[-1] % 128  # channels behind the last 128-slice run the exact kernels
        if tail < o_out.shape[-1]:
            np.testing.assert_array_equal(out[..., tail:], o_out[..., tail:])
    if out_exact is not None:
        np.testing.assert_array_equal(np.asarray(out_exact), o_out)
