#!/usr/bin/env python
"""Generate tests/golden/featurevis_vectors.npz by running the reference's OWN `read_sam_clip_feature(max_mode=True)`
(scene/dataset_readers.py:54-88) and `feature_visualize_saving` (render.py:33-48) in this container, on the CPU.  Only data
is stored.

    python tests/golden/make_golden_featurevis.py

render.py is imported unmodified behind the stand-in modules of make_golden_next.py; torch.Tensor.cuda is the identity
while the reference runs (this container has no GPU).  sklearn and PIL are the real packages.

PCA cases (C, H, W) = (16, 24, 41), (48, 30, 50), (512, 96, 160): the inputs are NOT stored (the largest is 31 MB); they are
tests/featurevis_ref.py synthetic_feature(C, H, W, seed), which the tests call too, and the fixture keeps a fingerprint
(float64 sum, sum of squares and eight probed values) that the tests compare first.  Stored per case i: pca{i}_shape,
pca{i}_seed, pca{i}_fingerprint, pca{i}_vis [H, W, 3] float32 (the reference's return value), pca{i}_mean [C],
pca{i}_components [3, C], pca{i}_q1, pca{i}_q99 (the fitted values: sklearn's mean_ and components_, np.percentile of the
transformed sample, recomputed here exactly as the function does), pca{i}_eigenvalues (leading four, float64 restatement),
pca{i}_clamped (share of clamped values), pca{i}_gap64 = max |reference - float64 restatement| of the final image,
pca{i}_gap32 = the same with the restatement's Gram matrix formed in float32.  sklearn_version.

Asserted here, as conditions on the INPUTS (PCA directions mean nothing without a gap): lambda1 / lambda2 >= 1.1,
lambda2 / lambda3 >= 1.1, lambda3 / lambda4 >= 1.5 for every case, and a clamped share between 1 % and 5 %.

Max-mode cases: mm_img_embed [9, 16] (row 4 has a zero in channel 0), mm_seg [4, 13, 17] (ids 0..8 as floats, about one in
six -1 on each of the levels 1..3 independently), mm_scale_same [3, 13, 17] and mm_scale_resized [3, 29, 40] (softmax of
seeded normals; pixel (2, 3) has a two-way tie between its two largest levels and pixel (5, 7) a three-way tie), and the
reference's mm_feat_* [16, H, W] float32 and mm_mask_* [1, H, W] bool."""
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "featurevis_vectors.npz")
sys.path.insert(0, os.path.dirname(HERE))
import featurevis_ref as FR  # noqa: E402

PCA_CASES = ((16, 24, 41, 0), (48, 30, 50, 0), (512, 96, 160, 0))   # C, H, W, seed


def fingerprint(f):
    flat = f.reshape(-1).astype(np.float64)
    probe = flat[np.linspace(0, flat.size - 1, 8).astype(np.int64)]
    return np.concatenate([[flat.sum(), (flat * flat).sum()], probe])


def import_reference():
    for name in ("plyfile", "cv2", "simple_knn", "simple_knn._C", "gsplat", "open_clip", "torchvision", "torchvision.transforms",
                 "matplotlib", "matplotlib.pyplot"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["plyfile"].PlyData = object
    sys.modules["plyfile"].PlyElement = object
    sys.modules["simple_knn._C"].distCUDA2 = lambda *a, **k: None
    sys.modules["gsplat"].rasterization = None
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
    sys.path.insert(0, REF)
    import render
    return render


def reference_fit(feature):
    """mean_, components_, q1, q99 exactly as feature_visualize_saving forms them (render.py:34-41)."""
    import sklearn.decomposition
    fmap = torch.nn.functional.normalize(feature[None], dim=1)
    pca = sklearn.decomposition.PCA(3, random_state=42)
    f_samples = fmap.permute(0, 2, 3, 1).reshape(-1, fmap.shape[1])[::3].cpu().numpy()
    transformed = pca.fit_transform(f_samples)
    q1, q99 = np.percentile(transformed, [1, 99])
    return f_samples.mean(0), pca.components_, q1, q99


def main():
    import sklearn
    render = import_reference()
    saved = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    out = {"sklearn_version": np.array(sklearn.__version__)}
    try:
        for i, (C, H, W, seed) in enumerate(PCA_CASES):
            f = FR.synthetic_feature(C, H, W, seed)
            vis = render.feature_visualize_saving(torch.from_numpy(f)).numpy()
            mean, comps, q1, q99 = reference_fit(torch.from_numpy(f))
            r64 = FR.feature_visualize(f)
            r32 = FR.feature_visualize(f, gram=FR.float32_gram(f))
            lam = r64["eigenvalues"][:4]
            assert lam[0] / lam[1] >= 1.1 and lam[1] / lam[2] >= 1.1 and lam[2] / lam[3] >= 1.5, (C, H, W, lam / lam[0])
            clamped = float(np.mean((vis == 0.0) | (vis == 1.0)))
            assert 0.01 <= clamped <= 0.05, clamped
            gap64 = float(np.abs(vis.astype(np.float64) - r64["vis"]).max())
            gap32 = float(np.abs(vis.astype(np.float64) - r32["vis"]).max())
            u8_ref = (vis * 255).astype(np.uint8)
            u8_64 = (r64["vis"] * 255).astype(np.uint8)
            print(f"case {i} {(C, H, W)}: lambda ratios {np.round(lam / lam[0], 3)}, clamped {clamped:.4f}, gap64 {gap64:.3g}, "
                  f"gap32 {gap32:.3g}, uint8 differing {np.mean(u8_ref != u8_64):.5f}, "
                  f"components gap {np.abs(comps - r64['components']).max():.3g}")
            p = f"pca{i}_"
            out[p + "shape"], out[p + "seed"], out[p + "fingerprint"] = np.array([C, H, W]), np.array(seed), fingerprint(f)
            out[p + "vis"], out[p + "mean"], out[p + "components"] = vis.astype(np.float32), mean.astype(np.float32), comps.astype(np.float32)
            out[p + "q1"], out[p + "q99"] = np.array(q1), np.array(q99)
            out[p + "eigenvalues"], out[p + "clamped"] = lam, np.array(clamped)
            out[p + "gap64"], out[p + "gap32"] = np.array(gap64), np.array(gap32)

        rng = np.random.default_rng(11)
        emb = rng.standard_normal((9, 16)).astype(np.float32)
        emb[4, 0] = 0.0
        seg = rng.integers(0, 9, (4, 13, 17)).astype(np.float32)
        for lev in (1, 2, 3):
            seg[lev][rng.random((13, 17)) < 1 / 6] = -1.0
        out["mm_img_embed"], out["mm_seg"] = emb, seg
        for tag, (H, W) in (("same", (13, 17)), ("resized", (29, 40))):
            z = rng.standard_normal((3, H, W))
            sc = (np.exp(z) / np.exp(z).sum(axis=0)).astype(np.float32)
            sc[:, 2, 3] = np.float32([0.2, 0.4, 0.4])
            sc[:, 5, 7] = np.float32(1.0) / np.float32(3.0)
            feat, mask = render.read_sam_clip_feature(torch.from_numpy(emb), torch.from_numpy(seg), torch.from_numpy(sc),
                                                      max_mode=True)
            out[f"mm_scale_{tag}"], out[f"mm_feat_{tag}"], out[f"mm_mask_{tag}"] = sc, feat.numpy(), mask.numpy()
            rf, rm = FR.max_mode_feature(emb, seg, sc)
            print(f"max mode {tag}: restatement bit-equal {np.array_equal(rf, feat.numpy())}, max |diff| "
                  f"{np.abs(rf - feat.numpy()).max():.3g}, mask equal {np.array_equal(rm, mask.numpy())}, "
                  f"mask share {mask.float().mean():.3f}")
    finally:
        torch.Tensor.cuda = saved
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
