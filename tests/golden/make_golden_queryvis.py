#!/usr/bin/env python
"""Generate tests/golden/queryvis_vectors.npz by running the reference's OWN `activate_stream`
(/root/reference/compute_relvancy.py:70-144), `colormap_saving` and `smooth_GPU` (eval/utils.py:66-110) and
`apply_colormap` (eval/colormaps.py:45-113) in this container.  Only data is stored.

    python tests/golden/make_golden_queryvis.py

The reference functions run unmodified.  What is replaced is what this container lacks or what writes files (the module stubs
of make_golden_activate.py, plus open3d; matplotlib is the REAL one: the turbo table comes from it):
  * cv2.filter2D -> make_golden_activate.filter2d_box, the exact float64 box sum rounded to float32; every call is recorded
    (the second call per phrase is avg2, the box mean of `output`).
  * mediapy.write_image -> a recorder keyed by path: the float RGB images the reference would have written.
  * Path.mkdir -> a no-op; compute_relvancy.show_result (a matplotlib figure: lerf_composited_whitebg) -> a no-op.
  * colormap_saving / smooth_GPU are wrapped (the real function runs, its return value is recorded): `output` and the mask.
  * clip_model: an object with `positives` and a `get_max_across` that returns the stored relevancy maps; activate_stream writes
    the heat map back into that tensor, which is how it is read here.

compute_loss (:396-447) needs a trained scene on disk; its three expressions (:440-446) are restated below, once in torch
float32 (what the reference computes) and once in float64, on random maps."""
import os
import sys
import types
from pathlib import Path

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "queryvis_vectors.npz")
sys.path.insert(0, HERE)
from make_golden_activate import filter2d_box  # noqa: E402

THRESH = 0.4


def bumps(g, k, h, w, n0=2):
    """Noisy maps with a few Gaussian bumps, as make_golden_activate.py draws them."""
    yy, xx = torch.meshgrid(torch.arange(h).float(), torch.arange(w).float(), indexing="ij")
    maps = []
    for j in range(k):
        m = 0.35 + 0.05 * torch.randn(h, w, generator=g)
        for _ in range(n0 + j):
            cy, cx = torch.rand(2, generator=g) * torch.tensor([h, w])
            sg = 6 + 10 * torch.rand(1, generator=g)
            m = m + 0.5 * torch.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * sg ** 2))
        maps.append(m.clamp(0, 1))
    return torch.stack(maps)


def edge_set(heat, output, b, q, thresh):
    """B of the end-to-end test: pixels where a LUT argument times 255 lies within 2e-3 of an integer >= 1, or heat within 1e-5
    of 0.5, or output within 1e-5 of the threshold.  The integer 0 is no bin edge: every argument is clipped to [0, 1] and the
    whole of [0, 1 / 255) has index 0, so the many pixels clipped to exactly 0 cannot change bins and stay OUT of B (counting
    them would put three quarters of the fixture into the excluded set).  Returns (B, its three parts)."""
    def near_int(t):
        s = t.astype(np.float64) * 255.0
        return (np.abs(s - np.rint(s)) < 2e-3) & (np.rint(s) >= 1)
    lut_edge = near_int(output) | near_int(q) | near_int(b)
    heat_edge = np.abs(heat.astype(np.float64) - 0.5) < 1e-5
    out_edge = np.abs(output.astype(np.float64) - thresh) < 1e-5
    return lut_edge | heat_edge | out_edge, lut_edge, heat_edge, out_edge


def main():
    class _Sub:
        def __class_getitem__(cls, item):
            return cls
    stubs = ("plyfile", "cv2", "simple_knn", "simple_knn._C", "gsplat", "open_clip", "torchvision", "torchvision.transforms",
             "mediapy", "jaxtyping", "tqdm", "open3d", "segment_anything")
    for name in stubs:
        sys.modules[name] = types.ModuleType(name)
    sys.modules["plyfile"].PlyData = sys.modules["plyfile"].PlyElement = object
    sys.modules["simple_knn._C"].distCUDA2 = lambda *a, **k: None
    sys.modules["gsplat"].rasterization = None
    sys.modules["segment_anything"].SamAutomaticMaskGenerator = sys.modules["segment_anything"].sam_model_registry = None
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    sys.modules["jaxtyping"].Bool = sys.modules["jaxtyping"].Float = _Sub
    sys.modules["tqdm"].tqdm = lambda x, *a, **k: x
    rec = {"filter": [], "images": {}, "output": [], "mask": []}

    def filter2d(src, ddepth, kernel):
        out = filter2d_box(src, ddepth, kernel)
        rec["filter"].append(np.array(out).copy())
        return out
    sys.modules["cv2"].filter2D = filter2d
    sys.modules["mediapy"].write_image = lambda path, image, fmt="png": rec["images"].__setitem__(str(path), np.array(image).copy())
    sys.path.insert(0, REF)
    import matplotlib
    import compute_relvancy as C
    from eval import colormaps

    real_saving, real_smooth = C.colormap_saving, C.smooth_GPU

    def saving(image, opts, path):
        out = real_saving(image, opts, path)
        if image.shape[-1] == 1:
            rec["output"].append(out[..., 0].clone())
        return out

    def smooth(mask, *a, **k):
        out = real_smooth(mask, *a, **k)
        rec["mask"].append(np.array(out).copy())
        return out
    C.colormap_saving, C.smooth_GPU = saving, smooth
    C.show_result = lambda image, save_path: None
    Path.mkdir = lambda self, *a, **k: None  # (the reference creates its output folders)
    options = colormaps.ColormapOptions(colormap="turbo", normalize=True, colormap_min=-1.0, colormap_max=1.0)  # (:219-224)

    lut = np.asarray(matplotlib.colormaps["turbo"].colors, np.float64).astype(np.float32)
    out = {"qv_lut": lut, "qv_thresh": np.array(THRESH, np.float32)}
    g = torch.Generator().manual_seed(777)
    valid1 = bumps(g, 3, 70, 94)
    act = os.path.join(HERE, "activate_vectors.npz")
    if os.path.exists(act):
        assert np.array_equal(np.load(act)["act_valid_map"], valid1.numpy()), "case 1 is the activate fixture's maps"
    g2 = torch.Generator().manual_seed(778)
    valid2 = bumps(g2, 1, 34, 300, n0=3)

    def rgb8(h, w):
        """An 8-bit picture as compute_relvancy.py:261-263 loads it: (uint8 / 255.0).astype(float32)."""
        u8 = torch.randint(0, 256, (h, w, 3), generator=g2, dtype=torch.uint8).numpy()
        return torch.from_numpy((u8 / 255.0).astype(np.float32))
    image1, image2 = rgb8(70, 94), rgb8(34, 300)
    shares = []
    for case, (valid, image, names) in enumerate(((valid1, image1, ("alpha", "beta", "gamma")), (valid2, image2, ("delta",))), 1):
        for v in rec.values():
            v.clear()
        heat = valid.clone()
        clip = types.SimpleNamespace(positives=names, get_max_across=lambda sem, heat=heat: heat[None])
        C.activate_stream(None, image, clip, Path("/nonexistent"), idx=7, thresh=THRESH, colormap_options=options)
        k = len(names)
        assert len(rec["filter"]) == 2 * k and len(rec["output"]) == k and len(rec["mask"]) == k and len(rec["images"]) == 3 * k
        pre = f"qv{case}_"
        out[pre + "image"] = image.numpy()
        if case != 1:   # (case 1's maps are activate_vectors.npz act_valid_map)
            out[pre + "valid_map"] = valid.numpy()
        out[pre + "heat"] = heat.numpy()                                       # valid_map[k] after :108
        out[pre + "output"] = torch.stack(rec["output"]).numpy()
        out[pre + "mask"] = np.stack(rec["mask"]).astype(np.uint8)
        out[pre + "avg2"] = np.stack([a.reshape(valid.shape[1:]) for a in rec["filter"][1::2]])
        out[pre + "pmax"] = torch.stack([torch.clip(heat[j] - 0.5, 0, 1).max() for j in range(k)]).numpy()   # p_i.max() of :119
        for folder in ("heatmap", "lerf_composited", "mask_composited"):
            out[pre + folder] = np.stack([rec["images"][f"/nonexistent/{folder}/{n}_00007.png"] for n in names]).astype(np.float32)
        # the share of pixels in the end-to-end test's excluded set B
        ht, ou, a2 = out[pre + "heat"], out[pre + "output"], out[pre + "avg2"]
        p = np.clip(ht - np.float32(0.5), 0, 1)
        q = np.clip(p / (out[pre + "pmax"][:, None, None] + np.float32(1e-6)), 0, 1)
        b = np.clip(np.float32(0.5) * ou + np.float32(0.5) * a2, 0, 1)
        B, le, he, oe = edge_set(ht, ou, b, q, THRESH)
        shares.append(B.mean())
        print(f"case {case}: {valid.shape}  |B| = {B.sum()} of {B.size} pixels ({100 * B.mean():.3f} %): LUT edges {le.sum()}, "
              f"heat edges {he.sum()}, threshold edges {oe.sum()}; mask ones {out[pre + 'mask'].mean():.3f}, "
              f"heat >= 0.5 {(ht >= 0.5).mean():.3f}")
        assert B.mean() <= 0.02, "the fixture must keep the excluded set within 2 % of the pixels"
    out["qv_edge_share"] = np.array(shares, np.float64)

    # ---- loss maps: compute_relvancy.py:440-446 restated in float32 (the reference's arithmetic) and in float64
    gl = torch.Generator().manual_seed(779)
    for case, (c, h, w) in enumerate(((512, 9, 13), (16, 40, 70)), 1):
        # gt as read_sam_clip_feature assembles it: one of a few unit embeddings per pixel, blocky segments; the prediction is
        # gt + noise, rounded to float16 values (stored as float16 to keep the file small; exact in float32)
        emb = torch.nn.functional.normalize(torch.randn(5, c, generator=gl), dim=1)
        seg = torch.randint(0, 5, ((h + 3) // 4, (w + 4) // 5), generator=gl).repeat_interleave(4, 0).repeat_interleave(5, 1)[:h, :w]
        gt = emb[seg].permute(2, 0, 1).contiguous()
        feat = (gt + 0.3 / c ** 0.5 * torch.randn(c, h, w, generator=gl)).half().float()
        mask = torch.rand(1, h, w, generator=gl) > 0.3
        assert bool(mask.any()) and not bool(mask.all())
        res = {}
        for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
            gtm, fm = gt.to(dt) * mask, feat.to(dt) * mask
            res[tag] = (torch.sqrt(torch.sum((gtm - fm) ** 2, dim=0)), torch.mean(torch.abs(fm), dim=0),
                        torch.mean(torch.abs(gtm), dim=0))
        pre = f"lm{case}_"
        out[pre + "feature_f16"], out[pre + "gt"], out[pre + "mask"] = feat.half().numpy(), gt.numpy(), mask.numpy()
        assert torch.equal(feat.half().float(), feat)
        for j, name in enumerate(("l2", "mean_abs_pred", "mean_abs_gt")):
            out[pre + name + "_f32"], out[pre + name + "_f64"] = res["f32"][j].numpy(), res["f64"][j].numpy()
            out[pre + name + "_err_ref"] = np.float64(np.abs(res["f32"][j].double().numpy() - res["f64"][j].numpy()).max())
            print(f"loss maps case {case} {name}: err_ref {float(out[pre + name + '_err_ref']):.3e}, max {float(res['f64'][j].max()):.4f}")
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(out), "arrays")
    assert os.path.getsize(OUT) < 1_000_000


if __name__ == "__main__":
    main()
