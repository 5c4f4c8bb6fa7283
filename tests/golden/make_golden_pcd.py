#!/usr/bin/env python
"""Generate tests/golden/pcd_query_vectors.npz by running the reference's OWN `pcd_relvancy` (compute_relvancy.py:273-394,
--pcd_mode) and `smooth_pcd_mask` (utils/pcd_utils.py:204-219, scipy's KDTree) in this container.  Only data is stored.

    python tests/golden/make_golden_pcd.py

The reference functions run unmodified; what is replaced is what this container lacks or what opens windows / files:
  * plyfile.PlyData.read -> an object serving the cloud's columns; its `write` records the f_dc it would write.
  * open3d, cv2, matplotlib, open_clip, ... are empty stand-in modules; tqdm is a pass-through; `vis_pcd` and the colormap
    record their inputs (the second colormap call of a phrase receives the normalised relevancy, :378).
  * .cuda() on modules and tensors is the identity (no GPU here); torch.load returns {'module_state_dict': ...} of
    make_golden_next.decoder_weights(0), loaded into the reference's CNN_decoder(16, 512).
  * OpenCLIPNetwork: a stand-in whose get_relevancy IS the reference's method, over seeded unit embeddings; the positive
    phrases are decoded directions of two clusters.
scipy's KDTree is real.  Asserted here: the KD-tree's neighbour counts equal a float64 brute force of
((dx*dx + dy*dy) + dz*dz) <= r*r on every cloud and radius (a lattice with many pairs at exactly r included), the smoothed
masks equal that rule, every branch of the rule occurs, and the end-to-end relevancy is bimodal with no normalised value
within 5e-3 of rel_thresh.

Arrays:  cloud names `lattice`, `blobs`, `dups`:  <cloud>_xyz [N,3] f32, <cloud>_mask [K,N] bool;
         for every parameter set p (PARAMS[p] = (radius, threshold)): <cloud>_p<p>_out [K,N] bool (the reference's
         smooth_pcd_mask), <cloud>_p<p>_count [K,N] int32 (uncapped masked-neighbour counts, brute force).
         e2e_*: the pcd_relvancy run: xyz, sem [N,16], f_dc [N,3], pos [2,512], neg [4,512], rel_thresh, relevancy [2,N],
         normalized [2,N], mask_raw [2,N], mask [2,N], fdc_<bg> [2,N,3] (what save_pcd writes) for bg in RGB / gray / mix.
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
OUT = os.path.join(HERE, "pcd_query_vectors.npz")
PARAMS = [(0.05, 20), (0.1, 10), (0.0625, 4)]  # pcd_relvancy's, smooth_pcd_mask's defaults, a binary radius with threshold < 10
STUB_ROOTS = {"plyfile", "open3d", "cv2", "matplotlib", "open_clip", "segment_anything", "simple_knn", "gsplat",
              "torchvision", "mediapy", "jaxtyping", "tqdm"}


class _AnyModule(types.ModuleType):
    """A stand-in module: every attribute is an inert class (constructible, subscriptable)."""
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        v = type(name, (), {"__init__": lambda self, *a, **k: None, "__class_getitem__": classmethod(lambda c, i: c)})
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


def brute_counts(xyz, masks, r):
    """[K, N] masked-neighbour counts under ((dx*dx + dy*dy) + dz*dz) <= r*r, float64 (numpy does not fuse)."""
    x = xyz.astype(np.float64)
    d = x[:, None, :] - x[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    within = d2 <= r * r
    return np.stack([within[:, m].sum(1) for m in masks]).astype(np.int32), within.sum(1)


def rule(mask, c, threshold):
    return (c > threshold) | (mask & (c >= 10))


def coherent_mask(xyz, centre, rad, rng, flip):
    m = np.linalg.norm(xyz - centre, axis=1) < rad
    return m ^ (rng.random(len(m)) < flip)


def clouds(rng):
    out = {}
    # lattice, binary spacing 2^-5 from a binary origin: at r = 2^-4 the axis pairs at two steps sit at exactly r
    h = 2.0 ** -5
    g = np.stack(np.meshgrid(*[np.arange(10)] * 3, indexing="ij"), -1).reshape(-1, 3)
    xyz = (0.5 + g * h).astype(np.float32)
    c = xyz.mean(0)
    out["lattice"] = (xyz, np.stack([coherent_mask(xyz, c, 0.12, rng, 0.1), rng.random(len(xyz)) < 0.5]))
    # blobs of ~150 points (sigma 0.04) plus uniform noise: counts around 10-30 at r = 0.05
    cen = rng.uniform(0, 0.8, (5, 3))
    pts = [c + 0.04 * rng.standard_normal((150, 3)) for c in cen] + [rng.uniform(-0.1, 0.9, (150, 3))]
    xyz = np.concatenate(pts).astype(np.float32)
    out["blobs"] = (xyz, np.stack([coherent_mask(xyz, cen[0], 0.08, rng, 0.05), coherent_mask(xyz, cen[1], 0.12, rng, 0.15),
                                   rng.random(len(xyz)) < 0.3]))
    # duplicated points: blobs with some points repeated 2-5 times
    base = np.concatenate([c + 0.03 * rng.standard_normal((100, 3)) for c in cen[:3]]).astype(np.float32)
    rep = rng.integers(1, 6, len(base)) * (rng.random(len(base)) < 0.3) + 1
    xyz = np.repeat(base, rep, axis=0)
    xyz = xyz[rng.permutation(len(xyz))]
    out["dups"] = (xyz, np.stack([coherent_mask(xyz, cen[0], 0.06, rng, 0.1), rng.random(len(xyz)) < 0.4]))
    return out


def main():
    sys.meta_path.insert(0, _Stubs())
    sys.path.insert(0, REF)
    sys.path.insert(0, HERE)
    from make_golden_next import decoder_weights
    from scipy.spatial import KDTree

    saved = torch.nn.Module.cuda, torch.Tensor.cuda, torch.load
    torch.nn.Module.cuda = lambda self, *a, **k: self
    torch.Tensor.cuda = lambda self, *a, **k: self
    import builtins
    real_print = builtins.print
    builtins.print = lambda *a, **k: None  # the constructors print their layer lists
    try:
        import compute_relvancy as CR
        from utils import pcd_utils as PU
        from utils.preprocess_utils import OpenCLIPNetwork
        from models.networks import CNN_decoder
        dec = CNN_decoder(16, 512)
    finally:
        builtins.print = real_print
    sys.modules["tqdm"].tqdm = lambda x, *a, **k: x
    PU.tqdm = lambda x, *a, **k: x
    PU.print = CR.print = sys.modules["models.networks"].print = lambda *a, **k: None

    rng = np.random.default_rng(2024)
    out = {}
    branches = {"set": 0, "cleared": 0, "kept_true": 0, "kept_false": 0}

    # ---------------- smooth_pcd_mask on its own ----------------
    for name, (xyz, masks) in clouds(rng).items():
        out[f"{name}_xyz"], out[f"{name}_mask"] = xyz, masks
        tree = KDTree(xyz)
        for p, (r, thr) in enumerate(PARAMS):
            c, c_all = brute_counts(xyz, masks, r)
            nb = tree.query_ball_point(xyz, r=r)
            assert np.array_equal(np.array([len(v) for v in nb]), c_all), f"{name} r={r}: KD-tree != brute force"
            res = []
            for k, m in enumerate(masks):
                assert np.array_equal(np.array([m[v].sum() for v in nb]), c[k])
                s = PU.smooth_pcd_mask(m, xyz, radius=r, threshold=thr)
                assert np.array_equal(s, rule(m, c[k], thr)), f"{name} p{p} k{k}: smooth_pcd_mask != the rule"
                mid = (c[k] >= 10) & (c[k] <= thr)
                branches["set"] += int(((c[k] > thr) & ~m).sum())
                branches["cleared"] += int(((c[k] < 10) & m).sum())
                branches["kept_true"] += int((mid & m).sum())
                branches["kept_false"] += int((mid & ~m).sum())
                res.append(s)
            out[f"{name}_p{p}_out"], out[f"{name}_p{p}_count"] = np.stack(res), c
        if name == "lattice":  # pairs at exactly r = 2^-4 exist and count
            d = xyz.astype(np.float64)[:, None] - xyz.astype(np.float64)[None]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            assert (d2 == 0.0625 * 0.0625).sum() > 1000
    assert all(v > 0 for v in branches.values()), branches

    # ---------------- pcd_relvancy end to end ----------------
    wd, _ = decoder_weights(0)
    state = {f"decoder.{2 * i}.{n}": (W[:, :, None, None] if n == "weight" else b)
             for i, (W, b) in enumerate(wd) for n in ("weight", "bias")}
    dec.load_state_dict(state)
    g = torch.Generator().manual_seed(11)
    n_cl = 6
    fcen = torch.randn(n_cl, 16, generator=g)
    cen = rng.uniform(0, 1.2, (n_cl, 3))
    lab = np.repeat(np.arange(n_cl), 150)
    xyz = cen[lab] + 0.045 * rng.standard_normal((len(lab), 3))
    # target points scattered outside their cluster, other clusters' points inside the targets' (the vote removes and adds)
    for t in (0, 1):
        stray = rng.choice(np.nonzero(lab == t)[0], 6, replace=False)
        xyz[stray] = rng.uniform(-0.3, 1.5, (6, 3))
        intr = rng.choice(np.nonzero(lab >= 2)[0], 8, replace=False)
        xyz[intr] = cen[t] + 0.02 * rng.standard_normal((8, 3))
    noise = rng.uniform(-0.3, 1.5, (60, 3))
    xyz = np.concatenate([xyz, noise]).astype(np.float32)
    lab = np.concatenate([lab, rng.integers(2, n_cl, 60)])
    sem = (fcen[lab] + 0.02 * torch.randn(len(lab), 16, generator=g)).numpy().astype(np.float32)
    f_dc = (0.8 * rng.standard_normal((len(lab), 3))).astype(np.float32)
    with torch.no_grad():
        dirs = dec(fcen.T[..., None]).squeeze(-1).T.contiguous()  # the decoded cluster directions (unit)
    # positives: clusters 0 and 1.  The decoded directions of this seeded decoder lie within ~30 degrees of each other, as
    # CLIP's generic negatives ("object", "stuff", ...) lie close to any object's embedding: the other clusters'
    # directions serve as the negatives, which spreads the relevancy over most of [0, 1]
    pos, neg = dirs[:2].contiguous(), dirs[2:].contiguous()
    prompts = "chair,table"
    rel_thresh = 0.4

    rec = {}

    class FakeClip:
        def __init__(self, config):
            self.negatives = ("object", "things", "stuff", "texture")
            self.neg_embeds = neg

        def set_positives(self, text_list):
            self.positives = text_list
            self.pos_embeds = pos

        def get_relevancy(self, embed, positive_id):
            r = OpenCLIPNetwork.get_relevancy(self, embed, positive_id)
            rec.setdefault("relevancy", []).append(r[:, 0].clone())
            return r

    class Elem:
        def __init__(self):
            self.cols = {"x": xyz[:, 0].copy(), "y": xyz[:, 1].copy(), "z": xyz[:, 2].copy()}
            self.cols.update({f"f_dc_{i}": f_dc[:, i].copy() for i in range(3)})
            self.cols.update({f"semantic_{i}": sem[:, i].copy() for i in range(16)})

        def __getitem__(self, k):
            return self.cols[k]

        def __setitem__(self, k, v):
            self.cols[k] = np.asarray(v).astype(np.float32)  # plyfile stores into the float32 property

    class FakePly:
        def __init__(self):
            self.elements = [Elem()]

        def write(self, path):
            rec.setdefault("write", []).append(np.stack([self.elements[0][f"f_dc_{i}"] for i in range(3)], 1))

    cmap_calls = []
    CR.PlyData = types.SimpleNamespace(read=lambda path: FakePly())
    CR.OpenCLIPNetwork = FakeClip
    CR.vis_pcd = lambda *a, **k: None
    CR.plt = types.SimpleNamespace(get_cmap=lambda name: (lambda x: cmap_calls.append(np.array(x)) or np.zeros((len(x), 4))))
    CR.pltcolors = types.SimpleNamespace(Normalize=lambda **k: (lambda x: x))
    smooth_rec = []
    real_smooth = CR.smooth_pcd_mask

    def smooth(mask, xyz_, radius, threshold):
        s = real_smooth(mask, xyz_, radius=radius, threshold=threshold)
        smooth_rec.append((mask.copy(), s.copy(), radius, threshold))
        return s
    CR.smooth_pcd_mask = smooth
    torch.load = lambda *a, **k: {"module_state_dict": state}
    dataset = types.SimpleNamespace(model_path="/nonexistent", speedup=True)
    try:
        for bg in ("RGB", "gray", "mix"):
            rec.clear(), cmap_calls.clear(), smooth_rec.clear()
            CR.pcd_relvancy(dataset, 30000, prompts, 512, rel_thresh=rel_thresh, mask_color="default", bg_color=bg, save_pcd=True)
            out[f"e2e_fdc_{bg}"] = np.stack(rec["write"])
    finally:
        torch.nn.Module.cuda, torch.Tensor.cuda, torch.load = saved
    assert all(rr == 0.05 and tt == 20 for _, _, rr, tt in smooth_rec)
    relv = torch.stack(rec["relevancy"]).numpy()
    normalized = np.stack(cmap_calls[1::2])
    mask_raw = np.stack([m for m, _, _, _ in smooth_rec])
    mask = np.stack([s for _, s, _, _ in smooth_rec])
    for k in range(2):
        assert relv[k].max() - relv[k].min() >= 0.4, relv[k].max() - relv[k].min()
        assert np.abs(normalized[k] - rel_thresh).min() > 5e-3, np.abs(normalized[k] - rel_thresh).min()
        c, _ = brute_counts(xyz, mask_raw[k:k + 1], 0.05)
        assert np.array_equal(mask[k], rule(mask_raw[k], c[0], 20))
        assert (mask[k] & ~mask_raw[k]).any() and (mask_raw[k] & ~mask[k]).any(), "the vote must both add and remove points"
        assert np.array_equal(mask_raw[k][:len(lab)] & (lab == k), lab == k) or mask_raw[k][lab == k].mean() > 0.9
    out.update(e2e_xyz=xyz, e2e_sem=sem, e2e_f_dc=f_dc, e2e_pos=pos.numpy(), e2e_neg=neg.numpy(),
               e2e_rel_thresh=np.float32(rel_thresh), e2e_relevancy=relv, e2e_normalized=normalized, e2e_mask_raw=mask_raw,
               e2e_mask=mask)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(out), "arrays; branches", branches,
          "e2e raw / smoothed:", mask_raw.sum(1), mask.sum(1))


if __name__ == "__main__":
    main()
