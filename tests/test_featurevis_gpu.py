"""N11 on the GPU: the max mode of read_sam_clip_feature and the PCA colouring of gags_amd.featurevis against the reference's
own outputs (tests/golden/featurevis_vectors.npz) and the numpy restatement (tests/featurevis_ref.py).

Measured on an MI355X (max |error| against float64; kernel / torch's own float32 normalize + matmul on the same card):
see MOMENTS_MEASURED below -- the bound of every case is 4 x torch's error of that case."""
import functools
import os

import numpy as np
import pytest
import torch

import featurevis_ref as FR

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
Z = np.load(os.path.join(HERE, "golden", "featurevis_vectors.npz"))
U = 2.0 ** -24
LAYOUTS = ("channel_major", "pixel_major")

# gram: max |kernel - float64| / max |torch float32 - float64| per (C, H, W), channel-major, as printed by
# test_moments_against_float64 on an MI355X
MOMENTS_MEASURED = """
(16, 24, 41)    kernel 9.8e-06 / torch 7.8e-06        (16, 1, 12)     kernel 4.5e-08 / torch 4.5e-08
(48, 30, 50)    kernel 5.7e-06 / torch 2.0e-05        (80, 10, 1229)  kernel 1.8e-05 / torch 6.7e-05
(512, 96, 160)  kernel 7.4e-06 / torch 1.1e-04
pixel-major: kernel 1.4e-05, 7.6e-06, 7.4e-06, 3.8e-08, 1.7e-05; torch the same except (80, 10, 1229): 3.5e-04.
The sum: at most 1.6e-06 (bound 3 * 2 * 2^-24 * S = 1.8e-03 at S = 5120).
Before the float accumulation chains were cut to 256 rows the kernel's error at (80, 10, 1229) was 3.3e-04, 5 x torch's.
The whole function against the reference's image: 1.8e-07 .. 7.2e-07 (bounds 7.6e-07 .. 2.0e-06), no uint8 value differs.
"""


def moment_shapes():
    from gags_amd import featurevis as fv
    chunk = fv.row_chunk()
    assert chunk == 4096          # (80, 10, 1229) below is 3 * chunk + 2 pixels: S = chunk + 1
    return [(16, 24, 41), (48, 30, 50), (512, 96, 160), (16, 1, 12), (80, 10, 1229)]


@functools.lru_cache(maxsize=None)
def feature(C, H, W, seed=0):
    f = FR.synthetic_feature(C, H, W, seed)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def ref_moments(C, H, W):
    return FR.moments(feature(C, H, W))


@functools.lru_cache(maxsize=None)
def ref_vis(C, H, W):
    return FR.feature_visualize(feature(C, H, W))


def on_gpu(f, layout):
    t = torch.from_numpy(np.array(f)).cuda()
    if layout == "pixel_major":
        t = t.permute(1, 2, 0).contiguous().permute(2, 0, 1)
        assert not t.is_contiguous()
    return t


def dev(name):
    return torch.from_numpy(Z[name]).cuda()


# ------------------------------------------------------------------------------------------------------------- max mode
@pytest.mark.parametrize("tag", ["same", "resized"])
def test_max_mode_equals_the_reference_bit_for_bit(tag):
    from gags_amd.losses import read_sam_clip_feature
    feat, mask = read_sam_clip_feature(dev("mm_img_embed"), dev("mm_seg"), dev(f"mm_scale_{tag}"), max_mode=True)  # (raises on the parent)
    assert feat.dtype == torch.float32 and mask.dtype == torch.bool and tuple(mask.shape) == (1,) + tuple(feat.shape[1:])
    np.testing.assert_array_equal(feat.cpu().numpy(), Z[f"mm_feat_{tag}"])
    np.testing.assert_array_equal(mask.cpu().numpy(), Z[f"mm_mask_{tag}"])
    rf, rm = FR.max_mode_feature(Z["mm_img_embed"], Z["mm_seg"], Z[f"mm_scale_{tag}"])
    np.testing.assert_array_equal(feat.cpu().numpy(), rf)
    np.testing.assert_array_equal(mask.cpu().numpy(), rm)


def test_max_mode_equals_default_mode_on_a_one_hot_scale_map():
    """Every id valid and a one-hot scale map: both modes pick the same level's feature.  At the seg map's own resolution (a
    single tap of weight 1), where the result does not depend on the order of the blend: max mode blends in the reference's
    order for this call, the default mode in the order it always had."""
    from gags_amd.losses import read_sam_clip_feature
    g = torch.Generator().manual_seed(3)
    emb = torch.randn(11, 32, generator=g).cuda()
    seg = torch.randint(0, 11, (4, 19, 70), generator=g).float().cuda()
    k = torch.randint(0, 3, (19, 70), generator=g)
    sc = torch.nn.functional.one_hot(k, 3).permute(2, 0, 1).float().cuda()
    fmax, mmax = read_sam_clip_feature(emb, seg, sc, max_mode=True)
    fdef, mdef = read_sam_clip_feature(emb, seg, sc)
    assert torch.equal(fmax, fdef)
    assert torch.equal(mmax, fmax[0:1] != 0) and bool(mdef.all())


# -------------------------------------------------------------------------------------------------------------- moments
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", range(5))
def test_moments_against_float64(case, layout):
    from gags_amd import featurevis as fv
    C, H, W = moment_shapes()[case]
    f = feature(C, H, W)
    rs, rg, S = ref_moments(C, H, W)
    x = on_gpu(f, layout)
    s, g = fv.feature_moments(x)
    assert s.dtype == torch.float64 and g.dtype == torch.float64
    # torch's own float32 on the same card: normalize, sample, matmul
    xs = torch.nn.functional.normalize(x.reshape(C, -1).t(), dim=1)[::3]
    tg = (xs.t() @ xs).double().cpu().numpy()
    err_t = np.abs(tg - rg).max()
    err_k = np.abs(g.cpu().numpy() - rg).max()
    err_s = np.abs(s.cpu().numpy() - rs).max()
    print(f"moments {(C, H, W)} {layout}: gram kernel {err_k:.3g} torch {err_t:.3g}; sum kernel {err_s:.3g}")
    assert err_k <= 4 * err_t
    # the sum is accumulated in float64: what is left is the rounding of x^ itself (sum of squares, sqrt, divide: 3 ulp of
    # a value of magnitude <= 1) over S samples
    assert err_s <= 3 * 2 * U * S
    assert np.array_equal(g.cpu().numpy(), g.cpu().numpy().T)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_moments_are_deterministic_and_see_only_the_sample(layout):
    from gags_amd import featurevis as fv
    C, H, W = 80, 10, 1229
    f = feature(C, H, W).copy()
    f[:, 0, 3] = 0.0                                   # an all-zero sampled pixel (p = 3)
    x = on_gpu(f, layout)
    s1, g1 = fv.feature_moments(x)
    s2, g2 = fv.feature_moments(x)
    assert torch.equal(s1, s2) and torch.equal(g1, g2)
    assert bool(torch.isfinite(g1).all()) and bool(torch.isfinite(s1).all())
    # the zero pixel contributes nothing: the moments are those of the map without it (any other value there changes them)
    X = FR.normalized_rows(f)[::3]
    keep = np.arange(X.shape[0]) != 1
    rg = X[keep].T @ X[keep]
    xs = torch.nn.functional.normalize(x.reshape(C, -1).t(), dim=1)[::3]
    err_t = np.abs((xs.t() @ xs).double().cpu().numpy() - rg).max()      # torch's own float32 error on this map, as above
    assert np.abs(g1.cpu().numpy() - rg).max() <= 4 * err_t
    assert not X[1].any()                              # (the restatement's row of that pixel is zero, not NaN)
    # pixels outside the sample may hold anything
    fl = f.reshape(C, -1).copy()
    fl[:, np.arange(H * W) % 3 != 0] = 1e30
    s3, g3 = fv.feature_moments(on_gpu(fl.reshape(C, H, W), layout))
    assert torch.equal(s1, s3) and torch.equal(g1, g3)


def test_too_few_samples_raise():
    from gags_amd import featurevis as fv
    with pytest.raises(ValueError):
        fv.feature_moments(torch.zeros(16, 3, 3, device="cuda"))
    with pytest.raises(ValueError):
        fv.feature_visualize(torch.zeros(24, 8, 8, device="cuda"))


# --------------------------------------------------------------------------------------------------------------- select
def select_inputs(n):
    rng = np.random.default_rng(n)
    a = rng.standard_normal(n).astype(np.float32)
    a[rng.integers(0, n, max(n // 4, 1))] = np.float32(-0.75)        # a repeated negative value
    a[rng.integers(0, n, max(n // 8, 1))] = np.float32(0.0)
    a[rng.integers(0, n, max(n // 8, 1))] = np.float32(-0.0)
    return a


@pytest.mark.parametrize("n", [1, 2, 100, 65537, 3 * 5120])
def test_select_is_exact(n):
    from gags_amd import featurevis as fv
    for a in (select_inputs(n), np.full(n, np.float32(-3.25))):
        s = np.sort(a)
        prev, nxt, _ = fv.percentile_ranks(n, (1, 99))
        ranks = sorted({0, n - 1, n // 2, n // 3, *prev.tolist(), *nxt.tolist()})[:8]
        got = fv.order_statistics(torch.from_numpy(a).cuda(), ranks).cpu().numpy()
        assert got.dtype == np.float32
        assert (got == s[ranks]).all(), (ranks, got, s[ranks])
        q = fv.percentiles(torch.from_numpy(a).cuda(), (1, 99))
        want = np.percentile(a, [1, 99])
        assert (np.abs(q - want) <= np.spacing(np.abs(want).astype(np.float32))).all(), (q, want)


def test_select_pools_the_sampled_rows():
    from gags_amd import featurevis as fv
    t = np.random.default_rng(5).standard_normal((1000, 3)).astype(np.float32)
    pool = np.sort(t[::3].reshape(-1))
    ranks = [0, 10, 500, pool.size - 1]
    got = fv.order_statistics(torch.from_numpy(t).cuda(), ranks, group=3, stride=9, n=pool.size).cpu().numpy()
    assert (got == pool[ranks]).all()


# ------------------------------------------------------------------------------------------------------- whole function
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("i", range(3))
def test_feature_visualize_equals_the_reference(i, layout):
    from gags_amd import featurevis as fv
    C, H, W = (int(v) for v in Z[f"pca{i}_shape"])
    f = feature(C, H, W, int(Z[f"pca{i}_seed"]))
    tol = 4 * max(float(Z[f"pca{i}_gap64"]), float(Z[f"pca{i}_gap32"]))
    x = on_gpu(f, layout)
    vis, u8 = fv.feature_visualize(x, return_uint8=True)
    assert tuple(vis.shape) == (H, W, 3) and vis.dtype == torch.float32 and u8.dtype == torch.uint8
    ref = Z[f"pca{i}_vis"]
    err = np.abs(vis.cpu().numpy().astype(np.float64) - ref).max()
    ref8 = (ref * 255).astype(np.uint8)
    d8 = np.abs(u8.cpu().numpy().astype(np.int32) - ref8.astype(np.int32))
    comps = fv.feature_pca_basis(x)[1]
    print(f"feature_visualize {(C, H, W)} {layout}: max |vis - reference| {err:.3g} (bound {tol:.3g}); uint8 differing "
          f"{(d8 != 0).mean():.5f}, by at most {d8.max()}; components {np.abs(comps.cpu().numpy() - Z[f'pca{i}_components']).max():.3g}")
    assert err <= tol
    assert d8.max() <= 1 and (d8 != 0).mean() <= 1e-3
    assert torch.equal(u8, (vis * 255).to(torch.uint8))
    assert torch.equal(fv.feature_visualize_saving(x), vis.cpu())


def test_sign_rule_and_a_given_basis():
    from gags_amd import featurevis as fv
    C, H, W = 48, 30, 50
    f = feature(C, H, W)
    x = on_gpu(f, "channel_major")
    mean, comps, q1, q99 = fv.feature_pca_basis(x)
    mean_n, comps_n, _, _ = fv.feature_pca_basis(-x)
    big = comps.abs().argmax(dim=1)
    assert bool((comps[torch.arange(3), big] > 0).all()) and bool((comps_n[torch.arange(3), big] > 0).all())
    # (the Gram matrix of -x has the same bits and the sum the opposite sign: the same covariance, the same eigenvectors)
    assert torch.equal(comps, comps_n) and torch.equal(mean, -mean_n)
    # a second map coloured in the first one's basis: the basis is used as given and left as it was
    f2 = feature(C, H, W, 1)
    basis = (mean.clone(), comps.clone(), q1, q99)
    vis2 = fv.feature_visualize(on_gpu(f2, "pixel_major"), basis=(mean, comps, q1, q99))
    assert torch.equal(mean, basis[0]) and torch.equal(comps, basis[1])
    m64, c64 = mean.double().cpu().numpy(), comps.double().cpu().numpy()
    want = np.clip(((FR.normalized_rows(f2) - m64) @ c64.T - np.float32(q1)) / np.float32(q99 - q1), 0, 1).reshape(H, W, 3)
    tol = 4 * max(float(Z["pca1_gap64"]), float(Z["pca1_gap32"]))
    assert np.abs(vis2.cpu().numpy() - want).max() <= tol


def test_layouts_agree():
    from gags_amd import featurevis as fv
    for i in range(3):
        C, H, W = (int(v) for v in Z[f"pca{i}_shape"])
        f = feature(C, H, W)
        a = fv.feature_visualize(on_gpu(f, "channel_major"))
        b = fv.feature_visualize(on_gpu(f, "pixel_major"))
        tol = 4 * max(float(Z[f"pca{i}_gap64"]), float(Z[f"pca{i}_gap32"]))
        assert float((a - b).abs().max()) <= tol


# ----------------------------------------------------------------------------------------------------------- end to end
class _Pipe:
    pass


def test_render_feature_view_and_its_files(tmp_path):
    from PIL import Image
    from gags_amd import featurevis as fv
    from gags_amd.decoders import CNN_decoder, CNN_scale_decoder
    from gags_amd.gaussian_renderer import render
    from gags_amd.losses import read_sam_clip_feature
    from gags_amd.synthetic import make_camera, make_model
    width, height, D, C = 64, 48, 16, 512
    torch.manual_seed(0)
    gaussians = make_model(3000, D, width, height, seed=0)
    dec, sdec = CNN_decoder(D, C).cuda(), CNN_scale_decoder(D, 3).cuda()
    view = make_camera(width, height)
    g = torch.Generator().manual_seed(7)
    view.img_embed = torch.randn(12, C, generator=g)
    seg = torch.randint(0, 12, (4, 24, 32), generator=g).float()
    seg[1:][torch.rand(3, 24, 32, generator=g) < 0.1] = -1.0
    view.seg_map = seg
    bg = torch.zeros(3, device="cuda")
    images = fv.render_feature_view(view, gaussians, _Pipe(), bg, dec, sdec, speedup=True)
    assert sorted(images) == sorted(["scale_map", "scale_class", "feature_vis", "gt_feature_vis", "gt_feature_vis_s",
                                     "gt_feature_vis_m", "gt_feature_vis_l"])
    assert tuple(images["scale_map"].shape) == (3, height, width) and images["scale_map"].dtype == torch.float32
    assert tuple(images["scale_class"].shape) == (height, width) and images["scale_class"].dtype == torch.float32
    for key in ("feature_vis", "gt_feature_vis", "gt_feature_vis_s", "gt_feature_vis_m", "gt_feature_vis_l"):
        assert tuple(images[key].shape) == (height, width, 3) and images[key].dtype == torch.uint8
    # the same images from the pieces, as render.py:148-175 composes them
    with torch.no_grad():
        fmap = render(view, gaussians, _Pipe(), bg, feature_mode=True)["render"]
        scale_map = sdec(fmap.detach())
        emb, segd = view.img_embed.cuda(), view.seg_map.cuda()
        gt, mask = read_sam_clip_feature(emb, segd, scale_map, max_mode=True)
        gts = fv.process_feature_map(view, scale_map)
        one = fv.process_scale_map(scale_map)
        decoded = dec(fmap)

    def u8(m):
        return (fv.feature_visualize_saving(m).numpy() * 255).astype(np.uint8)
    assert torch.equal(images["scale_map"], scale_map)
    assert torch.equal(images["scale_class"], fv.scale_visualize_saving(scale_map))
    assert set(images["scale_class"].unique().tolist()) <= {0.0, 0.5, 1.0}
    np.testing.assert_array_equal(images["feature_vis"].cpu().numpy(), u8(decoded))
    np.testing.assert_array_equal(images["gt_feature_vis"].cpu().numpy(), u8(gt * mask))
    for key, m, sm in zip(("gt_feature_vis_s", "gt_feature_vis_m", "gt_feature_vis_l"), gts, one):
        np.testing.assert_array_equal(images[key].cpu().numpy(), u8(m))
        lvl, lmask = read_sam_clip_feature(emb, segd, sm, max_mode=True)
        assert torch.equal(m, lvl * lmask)
    # the files: the reference's folders and names, and what PIL reads back
    paths = fv.save_feature_view(str(tmp_path), "test", 30000, 7, images)
    root = tmp_path / "test" / "ours_30000"
    names = {"scale_map": "scale_map/00007.png", "scale_class": "scale_map/00007_class.png",
             "feature_vis": "feature_map/00007_feature_vis.png", "gt_feature_vis": "gt_feature_map/00007_feature_vis.png",
             "gt_feature_vis_s": "gt_feature_map/00007_feature_vis_s.png", "gt_feature_vis_m": "gt_feature_map/00007_feature_vis_m.png",
             "gt_feature_vis_l": "gt_feature_map/00007_feature_vis_l.png"}
    for key, rel in names.items():
        assert paths[key] == str(root / rel) and os.path.isfile(paths[key])
        got = np.asarray(Image.open(paths[key]))
        if images[key].dtype == torch.uint8:
            want = images[key].cpu().numpy()
        else:
            t = images[key] if images[key].dim() == 3 else images[key][None].expand(3, -1, -1)
            want = (t * 255 + 0.5).clamp(0, 255).permute(1, 2, 0).to(torch.uint8).cpu().numpy()
        np.testing.assert_array_equal(got, want)
