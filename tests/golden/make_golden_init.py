#!/usr/bin/env python
"""Generate tests/golden/init_vectors.npz by running the reference's OWN `GaussianModel.create_from_pcd`
(scene/gaussian_model.py:151-180), `RGB2SH` / `SH2RGB` (utils/sh_utils.py:114-118) and `getNerfppNorm`
(scene/dataset_readers.py:123-147) on the CPU.  Only data is stored.

    python tests/golden/make_golden_init.py

The functions run unmodified; what is replaced is what this container lacks:
  * plyfile, PIL, matplotlib, ... are empty stand-in modules (as in make_golden_densify.py).
  * inside scene.gaussian_model, `torch` is a proxy whose zeros / ones(..., device="cuda") stay on the CPU, and
    `Tensor.cuda()` returns the tensor itself for the duration of this script.
  * `simple_knn._C.distCUDA2` is STUBBED by the float64 brute force of tests/knn_ref.py cast to float32.  The real simple-knn
    is an empty, unvendored CUDA submodule of the reference; its CUDA build contracts multiply-adds into FMAs, so its output
    was never defined to the bit.  What this fixture pins is the exact 3-nearest-neighbour mean squared distance, to float32
    rounding; the kernel's own float32 contract is pinned by tests/knn_ref.py, not here.

Arrays: points [N,3] float32, colors [N,3] float64 (multiples of 1/255, as fetchPly yields), dist2 [N] (the stub's output);
configs (names) and per config c: c_par = (sh_degree, semantic_feature_size, speedup, spatial_lr_scale), c_xyz, c_features_dc,
c_features_rest, c_scaling, c_rotation, c_opacity, c_max_radii2D, c_semantic_feature (absent when the size is 0),
c_active_sh_degree, c_spatial_lr_scale; rgb2sh_in / rgb2sh_out / sh2rgb_out; cam_R [C,3,3], cam_T [C,3], norm_translate [3],
norm_radius; ply_names / ply_types: storePly's dtype (scene/dataset_readers.py:216-218) in file order.
"""
import importlib.abc
import importlib.machinery
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "init_vectors.npz")
STUB_ROOTS = {"plyfile", "open3d", "cv2", "matplotlib", "simple_knn", "gsplat", "torchvision", "tqdm", "sklearn", "PIL"}
FIELDS = ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity")


class _AnyModule(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        v = type(name, (), {"__init__": lambda self, *a, **k: None})
        setattr(self, name, v)
        return v


class _Stubs(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, name, path, target=None):
        if name.split(".")[0] in STUB_ROOTS:
            return importlib.machinery.ModuleSpec(name, self, is_package=True)

    def create_module(self, spec):
        m = _AnyModule(spec.name)
        m.__path__ = []
        return m

    def exec_module(self, m):
        pass


class TorchProxy:
    """`torch` as scene.gaussian_model sees it: device="cuda" stays on the CPU."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def _cpu(k):
        if str(k.get("device", "")).startswith("cuda"):
            k.pop("device")
        return k

    def zeros(self, *a, **k):
        return torch.zeros(*a, **self._cpu(k))

    def ones(self, *a, **k):
        return torch.ones(*a, **self._cpu(k))


def main():
    sys.meta_path.insert(0, _Stubs())
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.append(os.path.dirname(os.path.dirname(HERE)))  # (knn_ref takes the box size from gags_amd.knn)
    import knn_ref as K
    import scene.gaussian_model as GM
    import scene.dataset_readers as DR
    import utils.sh_utils as SH
    torch.set_num_threads(1)
    GM.torch = TorchProxy()
    torch.Tensor.cuda = lambda self, *a, **k: self  # (this process only)

    def dist_stub(points):
        assert points.dtype == torch.float32 and tuple(points.shape[1:]) == (3,)
        return torch.from_numpy(K.dist2_f64(points.numpy()).astype(np.float32))
    GM.distCUDA2 = dist_stub

    rng = np.random.default_rng(909)
    n = 200
    points = K.cloud("uniform")[:n].copy()
    points[:3] = points[3]  # four coincident points: dist2 = 0 there, the clamp_min(1e-7) branch of the scales
    colors = rng.integers(0, 256, (n, 3)).astype(np.float64) / 255.0
    pcd = GM.BasicPointCloud(points=points, colors=colors, normals=np.zeros((n, 3)))
    out = {"points": points, "colors": colors, "dist2": K.dist2_f64(points).astype(np.float32)}
    assert (out["dist2"][:4] == 0).all() and (out["dist2"][4:] > 1e-7).all()

    configs = [("sh3", 3, 0, False, 4.25), ("sh0_speedup", 0, 512, True, 1.0), ("sh3_sem512", 3, 512, False, 0.5)]
    for name, shd, size, speedup, lr_scale in configs:
        gm = GM.GaussianModel(shd)
        gm.create_from_pcd(pcd, lr_scale, size, speedup)
        for attr in FIELDS:
            p = getattr(gm, attr)
            assert isinstance(p, torch.nn.Parameter) and p.requires_grad and p.dtype == torch.float32, attr
            out[f"{name}{attr}"] = p.detach().numpy().copy()
        out[f"{name}_max_radii2D"] = gm.max_radii2D.numpy().copy()
        if size:
            sf = gm._semantic_feature
            assert isinstance(sf, torch.nn.Parameter) and sf.requires_grad
            assert tuple(sf.shape) == (n, size // 32 if speedup else size)
            out[f"{name}_semantic_feature"] = sf.detach().numpy().copy()
        else:
            assert gm._semantic_feature is None
        out[f"{name}_active_sh_degree"] = np.int64(gm.active_sh_degree)
        out[f"{name}_spatial_lr_scale"] = np.float64(gm.spatial_lr_scale)
        out[f"{name}_par"] = np.array([shd, size, float(speedup), lr_scale])
        assert out[f"{name}_features_rest"].shape == (n, (shd + 1) ** 2 - 1, 3) and not out[f"{name}_features_rest"].any()
        assert np.allclose(out[f"{name}_scaling"][:4], 0.5 * np.log(1e-7), rtol=1e-6, atol=0)
    out["configs"] = np.array([c[0] for c in configs])

    x = torch.tensor(rng.random((50, 3)).astype(np.float32))
    out["rgb2sh_in"], out["rgb2sh_out"], out["sh2rgb_out"] = x.numpy(), SH.RGB2SH(x).numpy(), SH.SH2RGB(x).numpy()

    # cameras on a ring, looking roughly inwards: getNerfppNorm reads only R and T
    cams, Rs, Ts = [], [], []
    for c in range(7):
        a = 2 * np.pi * c / 7 + 0.1
        q = rng.standard_normal((3, 3))
        R, _ = np.linalg.qr(q)
        T = np.array([3.0 * np.cos(a), 0.3 * c, 3.0 * np.sin(a)]) + rng.standard_normal(3) * 0.2
        cams.append(types.SimpleNamespace(R=R, T=T))
        Rs.append(R)
        Ts.append(T)
    norm = DR.getNerfppNorm(cams)
    out.update(cam_R=np.array(Rs), cam_T=np.array(Ts), norm_translate=np.asarray(norm["translate"], np.float64),
               norm_radius=np.float64(norm["radius"]))

    # storePly's dtype (scene/dataset_readers.py:216-218); PLY type names as plyfile writes 'f4' / 'u1'
    out["ply_names"] = np.array(["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"])
    out["ply_types"] = np.array(["float"] * 6 + ["uchar"] * 3)

    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
