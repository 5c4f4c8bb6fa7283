"""N12 on the GPU against the images the reference's own activate_stream produced (tests/golden/make_golden_queryvis.py ->
queryvis_vectors.npz) and against the float64 restatement of compute_loss' three maps."""
import os

import numpy as np
import pytest
import torch

import queryvis_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
Z = np.load(os.path.join(HERE, "golden", "queryvis_vectors.npz"))
ZA = np.load(os.path.join(HERE, "golden", "activate_vectors.npz"))
KEYS = ("heatmap", "lerf_composited", "mask_composited")
F = np.float32


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def golden_act(case, frames=1):
    """The golden intermediates of a case as activate_maps would return them (stats: min, max of the heat map, max of avg --
    the last is not read), repeated for `frames` frames that share the phrases."""
    pre = f"qv{case}_"
    heat = Z[pre + "heat"]
    flat = heat.reshape(heat.shape[0], -1)
    stats = np.stack([flat.min(1), flat.max(1), np.zeros(heat.shape[0], F)], 1).astype(F)
    rep = lambda a: np.concatenate([a] * frames)  # noqa: E731
    return {"heatmap": cu(rep(heat)), "output": cu(rep(Z[pre + "output"])), "mask": cu(rep(Z[pre + "mask"])), "stats": cu(rep(stats))}


def valid_map(case):
    return ZA["act_valid_map"] if case == 1 else Z[f"qv{case}_valid_map"]


@pytest.mark.parametrize("case", [1, 2])
def test_colour_kernel_reproduces_the_reference_images_bit_for_bit(case):
    from gags_amd.queryvis import colour_maps
    pre = f"qv{case}_"
    got = colour_maps(golden_act(case), cu(Z[pre + "image"]), lut=cu(Z["qv_lut"]), avg2=cu(Z[pre + "avg2"]), return_uint8=True)
    for k in KEYS:
        np.testing.assert_array_equal(got[k].cpu().numpy(), Z[pre + k], err_msg=k)
        np.testing.assert_array_equal(got[k + "_u8"].cpu().numpy(), R.to_uint8(Z[pre + k]), err_msg=k)
    # the shipped table is the default
    again = colour_maps(golden_act(case), cu(Z[pre + "image"]), avg2=cu(Z[pre + "avg2"]))
    for k in KEYS:
        assert torch.equal(again[k], got[k]), k


def test_colour_kernel_two_frames_share_the_phrases():
    """M = 2 frames x 3 phrases: maps 0..2 use image 0 (the golden's), maps 3..5 a second, different image, whose results are
    the float32 restatement's (bit-equal to the golden on the first image: tests/test_queryvis_cpu.py)."""
    from gags_amd.queryvis import colour_maps
    pre = "qv1_"
    image2 = np.ascontiguousarray(F(1) - Z[pre + "image"][::-1, ::-1])
    assert not np.array_equal(image2, Z[pre + "image"])
    images = np.stack([Z[pre + "image"], image2])
    heat = Z[pre + "heat"]
    got = colour_maps(golden_act(1, frames=2), cu(images), lut=cu(Z["qv_lut"]), avg2=cu(np.concatenate([Z[pre + "avg2"]] * 2)),
                      return_uint8=True)
    want2 = R.query_images(heat, Z[pre + "output"], Z[pre + "mask"], Z[pre + "avg2"], heat.reshape(3, -1).max(1), image2[None],
                           Z["qv_lut"])
    for k, w2 in zip(KEYS, want2):
        g = got[k].cpu().numpy()
        np.testing.assert_array_equal(g[:3], Z[pre + k], err_msg=k)
        np.testing.assert_array_equal(g[3:], w2, err_msg=k)
        np.testing.assert_array_equal(got[k + "_u8"].cpu().numpy(), R.to_uint8(g), err_msg=k)
    assert not np.array_equal(got["lerf_composited"][:3].cpu().numpy(), got["lerf_composited"][3:].cpu().numpy())


@pytest.mark.parametrize("case", [1, 2])
def test_box_mean_of_output(case):
    """avg2 against the golden's exact float64 box sums: <= 1e-6 absolute, the bound tests/test_next_gpu.py holds the same
    computation to."""
    from gags_amd.queryvis import colour_maps
    pre = f"qv{case}_"
    got = colour_maps(golden_act(case), cu(Z[pre + "image"]))
    err = np.abs(got["avg2"].cpu().numpy().astype(np.float64) - Z[pre + "avg2"]).max()
    print(f"case {case}: max |avg2 - golden| = {err:.3e}")
    assert err <= 1e-6


@pytest.mark.parametrize("case", [1, 2])
def test_query_images_end_to_end(case):
    """query_images from the relevancy maps.  Its box means are within 1e-6 of the golden's exact ones, not bit-equal, so LUT
    bins and the two thresholds may flip at their edges: B (queryvis_ref.edge_sets, from the golden's values; <= 2 % of the
    pixels, asserted by the generator and tests/test_queryvis_cpu.py) holds the pixels where that can happen.  Off B every image
    and the mask are bit-equal to the golden; inside B every LUT index is within 1 of the golden's and a branch flips only where
    its own threshold put the pixel in B.  (B leaves out the integer 0: arguments are clipped to [0, 1] and [0, 1 / 255) is one
    bin, so a pixel clipped to 0 cannot change bins -- a smaller B than the literal "within 2e-3 of an integer", a stricter test.)"""
    from gags_amd.queryvis import colour_maps, query_images
    from gags_amd.relevancy import activate_maps
    pre = f"qv{case}_"
    th = float(Z["qv_thresh"])
    valid, image = cu(valid_map(case)), cu(Z[pre + "image"])
    got = query_images(valid, image, thresh=th, return_uint8=True)
    act = activate_maps(valid, thresh=th)
    parts = colour_maps(act, image)
    g_heat, g_out, g_avg2 = Z[pre + "heat"], Z[pre + "output"], Z[pre + "avg2"]
    g_max = g_heat.reshape(g_heat.shape[0], -1).max(1)
    e = R.edge_sets(g_heat, g_out, g_avg2, g_max, th)
    B = e["B"]
    print(f"case {case}: |B| = {B.sum()} of {B.size} ({100 * B.mean():.3f} %)")
    assert B.mean() <= 0.02
    heat, outp, avg2 = (t.cpu().numpy() for t in (act["heatmap"], act["output"], parts["avg2"]))
    stats = act["stats"].cpu().numpy()
    # the two paths to the images agree, and the images are the contract applied to this run's own intermediates
    mine = R.query_images(heat, outp, act["mask"].cpu().numpy(), avg2, stats[:, 1], Z[pre + "image"][None], Z["qv_lut"])
    for k, m in zip(KEYS, mine):
        assert torch.equal(got[k], parts[k]), k
        np.testing.assert_array_equal(got[k].cpu().numpy(), m, err_msg=k)
        np.testing.assert_array_equal(got[k + "_u8"].cpu().numpy(), R.to_uint8(m), err_msg=k)
    # off B: bit-equal to the golden
    flips = 0
    for k in KEYS:
        diff = np.any(got[k].cpu().numpy() != Z[pre + k], axis=-1)
        flips += int(diff.sum())
        assert not np.any(diff & ~B), (k, int((diff & ~B).sum()))
    print(f"case {case}: pixels that differ from the golden in some image (all inside B): {flips}")
    mask = got["mask"].cpu().numpy()
    assert not np.any((mask != Z[pre + "mask"]) & ~B)
    # inside B: LUT indices within 1, branches flipped only at their own edge
    _, _, q = R.lerf_q(heat, stats[:, 1])
    _, _, g_q = R.lerf_q(g_heat, g_max)
    for name, mine_t, gold_t in (("output", outp, g_out), ("q", q, g_q), ("b", R.mask_b(outp, avg2), R.mask_b(g_out, g_avg2))):
        d = np.abs(R.lut_index(mine_t) - R.lut_index(gold_t))
        assert d.max() <= 1, name
        assert not np.any((d != 0) & ~e["lut_" + name]), name
    assert not np.any(((heat < 0.5) != (g_heat < 0.5)) & ~e["heat"])
    pred_flip = act["mask_pred"].cpu().numpy().astype(bool) != (g_out > F(th))
    assert not np.any(pred_flip & ~e["thresh"])
    if not pred_flip.any():
        np.testing.assert_array_equal(mask, Z[pre + "mask"])


LOSS_NAMES = ("l2", "mean_abs_pred", "mean_abs_gt")


def loss_layouts(feat, gt, mask):
    """feature_loss_maps on every combination of memory layouts of the two [C, H, W] maps."""
    from gags_amd.queryvis import feature_loss_maps
    pm = lambda t: t.permute(1, 2, 0).contiguous().permute(2, 0, 1)  # noqa: E731  ([C, H, W] view of [H, W, C] memory)
    res = [feature_loss_maps(feat, gt, mask), feature_loss_maps(pm(feat), pm(gt), mask), feature_loss_maps(pm(feat), gt, mask),
           feature_loss_maps(feat, pm(gt), mask),
           feature_loss_maps(feat.permute(1, 2, 0).contiguous(), gt.permute(1, 2, 0).contiguous(), mask[0], pixel_major=True)]
    assert not pm(feat).is_contiguous()
    return res


@pytest.mark.parametrize("case", [1, 2])
def test_loss_maps_are_no_worse_than_the_reference(case):
    """max |ours - float64| <= max(err_ref, 1 ulp at the map's maximum), err_ref = the reference's own float32 deviation from
    the float64 restatement on the same inputs; every layout combination gives the same bits."""
    pre = f"lm{case}_"
    feat, gt, mask = cu(Z[pre + "feature_f16"].astype(F)), cu(Z[pre + "gt"]), cu(Z[pre + "mask"])
    res = loss_layouts(feat, gt, mask)
    for j, name in enumerate(LOSS_NAMES):
        want = Z[pre + name + "_f64"]
        err = np.abs(res[0][j].cpu().numpy().astype(np.float64) - want).max()
        err_ref = float(Z[pre + name + "_err_ref"])
        ulp = float(np.spacing(F(want.max())))
        print(f"case {case} {name}: err {err:.3e}  err_ref {err_ref:.3e}  ulp(max) {ulp:.3e}")
        assert err <= max(err_ref, ulp), name
        for other in res[1:]:
            assert torch.equal(other[j], res[0][j]), name


def test_loss_maps_ragged_channels_one_channel_and_zero_mask():
    from gags_amd.queryvis import feature_loss_maps
    g = torch.Generator().manual_seed(3)
    # C = 80: a whole step of 64 channels and a ragged one; 5 x 7 pixels: a ragged workgroup.  Against the float32 restatement,
    # which differs only in the ORDER of a float64 sum (relative 1e-16 x C): at most the final float32 rounding flips, 1 ulp
    feat, gt = torch.randn(80, 5, 7, generator=g), torch.randn(80, 5, 7, generator=g)
    mask = torch.rand(1, 5, 7, generator=g) > 0.4
    res = loss_layouts(feat.cuda(), gt.cuda(), mask.cuda())
    want = R.feature_loss_maps(feat.numpy(), gt.numpy(), mask.numpy())
    for j, name in enumerate(LOSS_NAMES):
        got = res[0][j].cpu().numpy()
        assert np.all(np.abs(got.astype(np.float64) - want[j]) <= np.spacing(want[j])), name
        for other in res[1:]:
            assert torch.equal(other[j], res[0][j]), name
    # C = 1: the sums have one term -- l2 = |fl(a - b)| exactly, the means are |b| and |a|
    f1, g1 = torch.randn(1, 9, 70, generator=g).cuda(), torch.randn(1, 9, 70, generator=g).cuda()
    ones = torch.ones(9, 70, device="cuda")
    l2, mp, mg = feature_loss_maps(f1, g1, ones)
    d = g1[0].cpu().numpy() - f1[0].cpu().numpy()
    np.testing.assert_array_equal(l2.cpu().numpy(), np.sqrt(d * d))
    assert torch.equal(mp, f1[0].abs()) and torch.equal(mg, g1[0].abs())
    # an all-zero mask (any dtype) gives zeros
    for zero in (torch.zeros(9, 70, device="cuda"), torch.zeros(1, 9, 70, dtype=torch.bool, device="cuda")):
        for t in feature_loss_maps(f1, g1, zero) + feature_loss_maps(feat.cuda()[:, :, :5], gt.cuda()[:, :, :5], zero[..., :5, :5]):
            assert t.abs().max().item() == 0


@pytest.fixture(scope="module")
def view_inputs():
    from gags_amd.decoders import CNN_decoder
    from gags_amd.relevancy import RelevancyHead
    torch.manual_seed(11)
    dec = CNN_decoder(16, 512).cuda()
    g = torch.Generator().manual_seed(12)
    unit = lambda n: torch.nn.functional.normalize(torch.randn(n, 512, generator=g), dim=-1).cuda()  # noqa: E731
    head = RelevancyHead(unit(3), unit(4))
    h, w = 36, 44
    # a smooth map (relevancy regions that survive the majority filter), as the [16, h, w] view of [h, w, 16] memory render() returns
    x = torch.nn.functional.interpolate(3 * torch.randn(1, 16, 5, 6, generator=g), size=(h, w), mode="bilinear")[0]
    x = x.permute(1, 2, 0).contiguous().cuda().permute(2, 0, 1)
    image = torch.rand(h, w, 3, generator=g).cuda()
    return dec, head, x, image


def test_query_view_is_the_composition_and_never_waits_for_the_device(view_inputs):
    """query_view == query_images(get_max_across(decoder(x))) bit for bit; captured into a graph (a capture fails on any
    host synchronisation between the stages) and replayed, it gives the same bits again."""
    from gags_amd.queryvis import query_images, query_view
    dec, head, x, image = view_inputs
    keys = KEYS + ("mask",) + tuple(k + "_u8" for k in KEYS)
    with torch.no_grad():
        valid = head.get_max_across(dec(x).permute(1, 2, 0).unsqueeze(0)).squeeze(0)
        want = query_images(valid, image, return_uint8=True)
    got = query_view(x, dec, head, image, return_uint8=True)
    assert got["heatmap"].shape == (3, 36, 44, 3)
    for k in keys:
        assert torch.equal(got[k], want[k]), k
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = query_view(x, dec, head, image, return_uint8=True)
    graph.replay()
    torch.cuda.synchronize()
    for k in keys:
        assert torch.equal(cap[k], want[k]), k


def test_save_query_images_writes_the_reference_file_names(view_inputs, tmp_path):
    from PIL import Image
    from gags_amd.queryvis import query_view, save_query_images, to_uint8
    dec, head, x, image = view_inputs
    names = ("red apple", "mug", "a table")
    images = query_view(x, dec, head, image, return_uint8=True)
    paths = save_query_images(tmp_path / "relvancy_heat_map", names, 7, images)
    assert len(paths) == 9
    for k in KEYS:
        for j, n in enumerate(names):
            path = tmp_path / "relvancy_heat_map" / k / f"{n}_00007.png"
            assert str(path) == paths[k, n] and path.exists()
            np.testing.assert_array_equal(np.asarray(Image.open(path)), images[k + "_u8"][j].cpu().numpy())
    # float images alone: the same files by the declared 8-bit rule
    floats = {k: images[k] for k in KEYS}
    paths2 = save_query_images(tmp_path / "again", names, 12, floats)
    for k in KEYS:
        assert torch.equal(to_uint8(images[k]), images[k + "_u8"]), k
        np.testing.assert_array_equal(np.asarray(Image.open(paths2[k, names[1]])), images[k + "_u8"][1].cpu().numpy())
