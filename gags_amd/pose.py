"""Trainable camera poses (N17): a small SE(3)-like correction in front of a camera's world-to-camera matrix.

rasterization() differentiates with respect to `viewmats`, and render() hands a camera's
`world_view_transform` straight through, so a pose becomes trainable by making that matrix a function of a parameter:

    poses = PoseDelta(len(cameras)).cuda()
    opt = torch.optim.Adam(poses.parameters(), lr=1e-3)
    pkg = render(poses.camera(cam, i), gaussians, pipe, bg)     # loss.backward() reaches poses.delta

This is 4 x 4 torch arithmetic: plumbing, no kernel.

Trainable intrinsics (N23): rasterization() also differentiates with respect to `Ks` and `radial_coeffs`, and render() hands a
camera's `K` / `radial_coeffs` through when they require grad, so IntrinsicsDelta makes them functions of parameters the same
way -- one set per physical sensor, shared by its cameras -- and composes with PoseDelta:

    intr = IntrinsicsDelta(n_sensors).cuda()
    pkg = render(intr.camera(poses.camera(cam, i), sensor_of[i]), gaussians, pipe, bg)"""
import copy
import math

import torch
from torch import nn

_SERIES_BELOW = 1e-4   # theta^2 under which sin(t)/t and (1 - cos t)/t^2 are summed as series (next term: t^6 / 5040 < 2e-16)


def so3_exp(omega):
    """Rodrigues' formula: exp(omega^) [3,3] for a rotation vector omega [3].  R = I + a K + b K^2 with a = sin(t)/t,
    b = (1 - cos t)/t^2, t = |omega|; both are functions of t^2 and are summed as series near 0, so that value and gradient at
    omega = 0 are finite and exact (R = I, dR/d omega_k = the k-th generator)."""
    t2 = (omega * omega).sum()
    small = t2 < _SERIES_BELOW
    a_ser = 1.0 - t2 / 6.0 + t2 * t2 / 120.0
    b_ser = 0.5 - t2 / 24.0 + t2 * t2 / 720.0
    t2s = torch.where(small, torch.ones_like(t2), t2)   # (keeps sqrt and the divisions away from 0 in the branch not taken)
    t = torch.sqrt(t2s)
    a = torch.where(small, a_ser, torch.sin(t) / t)
    b = torch.where(small, b_ser, (1.0 - torch.cos(t)) / t2s)
    x, y, z = omega.unbind(-1)
    zero = torch.zeros_like(x)
    K = torch.stack([zero, -z, y, z, zero, -x, -y, x, zero]).reshape(3, 3)
    return torch.eye(3, dtype=omega.dtype, device=omega.device) + a * K + b * _mm(K, K)


def _mm(a, b):
    """A small matrix product as multiply + sum: products with the 0s and 1s of an identity stay exact on every backend."""
    return (a[:, :, None] * b[None, :, :]).sum(1)


class PoseDelta(nn.Module):
    """One correction per camera: delta [n_cameras, 6] = (translation tau, rotation vector omega), zeros at start.
    forward(viewmat, idx) = [[exp(omega^), tau], [0, 1]] @ viewmat: the correction acts in the camera frame, on the left of
    the world-to-camera matrix; at delta = 0 the result is `viewmat` bit for bit."""

    def __init__(self, n_cameras):
        super().__init__()
        self.delta = nn.Parameter(torch.zeros(int(n_cameras), 6))

    def transform(self, idx):
        """The 4 x 4 correction of camera idx."""
        d = self.delta[idx]
        top = torch.cat([so3_exp(d[3:]), d[:3, None]], dim=1)
        bottom = torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=d.dtype, device=d.device)
        return torch.cat([top, bottom], dim=0)

    def forward(self, viewmat, idx):
        """viewmat: world-to-camera [4,4] (row-major, as rasterization() takes it).  Returns the adjusted [4,4]."""
        return _mm(self.transform(idx).to(viewmat.dtype), viewmat)

    def camera(self, cam, idx):
        """A shallow copy of `cam` whose world_view_transform is the adjusted matrix (in the camera class's transposed
        convention: world_view_transform = W2C^T); camera_center and -- where the camera carries a projection_matrix -- the
        full_proj_transform are recomputed from it.  Everything else is shared with `cam`."""
        out = copy.copy(cam)
        w2c = self.forward(cam.world_view_transform.transpose(0, 1), idx)
        out.world_view_transform = w2c.transpose(0, 1)
        if hasattr(cam, "camera_center"):
            out.camera_center = torch.inverse(w2c.double())[:3, 3].to(w2c.dtype)
        if hasattr(cam, "full_proj_transform") and hasattr(cam, "projection_matrix"):
            out.full_proj_transform = _mm(out.world_view_transform, cam.projection_matrix.to(w2c.dtype))
        return out


class IntrinsicsDelta(nn.Module):
    """One correction per group of cameras that share a physical sensor (N23): log_focal [n_groups, 2] (fx, fy are scaled by
    its exponential: a focal length stays positive and a step is relative), principal [n_groups, 2] (added to cx, cy, pixels)
    and coeffs [n_groups, 4] (added to the fisheye's k1 .. k4), all zeros at start.  At zero the camera's own values come
    back bit for bit."""

    def __init__(self, n_groups):
        super().__init__()
        n_groups = int(n_groups)
        if n_groups < 1:
            raise ValueError("IntrinsicsDelta needs at least one group")
        self.log_focal = nn.Parameter(torch.zeros(n_groups, 2))
        self.principal = nn.Parameter(torch.zeros(n_groups, 2))
        self.coeffs = nn.Parameter(torch.zeros(n_groups, 4))

    def _base_K(self, cam):
        K = getattr(cam, "K", None)
        if K is not None:
            K = torch.as_tensor(K).detach()
            if K.numel() != 9:
                raise ValueError("a camera's K must be [3,3]")
            return K.to(device=self.log_focal.device, dtype=torch.float32).reshape(3, 3)
        if getattr(cam, "camera_model", "pinhole") != "pinhole":
            raise ValueError(f"a {cam.camera_model!r} camera needs an explicit K [3,3] attribute")
        w, h = int(cam.image_width), int(cam.image_height)   # (render()'s FoV -> K of a pinhole camera)
        return torch.tensor([[w / (2 * math.tan(cam.FoVx * 0.5)), 0, w / 2.0], [0, h / (2 * math.tan(cam.FoVy * 0.5)), h / 2.0],
                             [0, 0, 1]], dtype=torch.float32, device=self.log_focal.device)

    def camera(self, cam, group=0):
        """A shallow copy of `cam` whose K is [[fx exp(l0), 0, cx + p0], [0, fy exp(l1), cy + p1], [0, 0, 1]] and -- for a
        fisheye camera only -- whose radial_coeffs are the camera's (zeros when it has none) plus coeffs[group]; float32
        tensors on the parameters' device that require grad, which render() hands through as they are.  Everything else,
        the pose included, is shared with `cam`: it composes with PoseDelta.camera in either order."""
        group = int(group)
        if not 0 <= group < self.log_focal.shape[0]:
            raise ValueError(f"group {group} out of range: this IntrinsicsDelta has {self.log_focal.shape[0]}")
        base = self._base_K(cam)
        s, p = torch.exp(self.log_focal[group]), self.principal[group]
        zero, one = base.new_zeros(()), base.new_ones(())
        out = copy.copy(cam)
        out.K = torch.stack([base[0, 0] * s[0], zero, base[0, 2] + p[0],
                             zero, base[1, 1] * s[1], base[1, 2] + p[1], zero, zero, one]).reshape(3, 3)
        if getattr(cam, "camera_model", "pinhole") == "fisheye":
            c = getattr(cam, "radial_coeffs", None)
            if c is None:
                c = base.new_zeros(4)
            else:
                c = torch.as_tensor(c).detach()
                if c.numel() != 4:
                    raise ValueError("a camera's radial_coeffs must be [4]")
                c = c.to(device=base.device, dtype=torch.float32).reshape(4)
            out.radial_coeffs = c + self.coeffs[group]
        return out
