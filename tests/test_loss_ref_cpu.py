"""tests/loss_ref.py (the float64 restatement of the distillation losses) pinned to the reference's own outputs in
tests/golden/next_vectors.npz, and its explicit resize taps pinned to torch's F.interpolate on float32 data.  This ties the
restatement to the reference; tests/test_losses_float64_gpu.py then ties the HIP kernels to the restatement at real sizes."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_ref as R

Z = np.load(os.path.join(os.path.dirname(__file__), "golden", "next_vectors.npz"))


def t(name, rg=False):
    return torch.from_numpy(Z[name]).double().requires_grad_(rg)


def close(got, ref, rel=1e-6):
    """max |got - ref| <= rel * max |ref|: the fixture is the reference's fp32 result, the restatement float64."""
    got = got.detach().double().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err, scale = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    assert err <= rel * scale, (err, scale)


def test_get_trained_seg_equals_the_fixture():
    np.testing.assert_array_equal(R.get_trained_seg(t("loss_seg4"), t("loss_scale_map")).numpy(), Z["loss_seg_trained"])
    np.testing.assert_array_equal(R.get_trained_seg(t("loss_segq"), t("loss_scale_map")).numpy(), Z["loss_seg_trained_q"])


def test_region_variance_loss_and_gradient_equal_the_fixture():
    feat = t("loss_feat", True)
    loss = R.scale_region_regulation_loss(feat, t("loss_seg_trained"))
    loss.backward()
    close(loss, Z["loss_regionvar"])
    close(feat.grad, Z["loss_regionvar_vfeat"])


def test_entropy_loss_and_gradient_equal_the_fixture():
    s = t("loss_scale_map", True)
    loss = R.scale_regulation_loss(s)
    loss.backward()
    close(loss, Z["loss_entropy"])
    close(s.grad, Z["loss_entropy_vscale"])


def test_ground_truth_l1_and_balance_loss_equal_the_fixture():
    emb, segq = t("loss_img_embed"), t("loss_segq")
    sc, pred = t("loss_scale_map", True), t("loss_pred", True)
    gt, mask = R.read_sam_clip_feature(emb, segq, sc)
    close(gt, Z["loss_gt"])
    np.testing.assert_array_equal(mask.numpy(), Z["loss_mask"])
    m = mask.double()
    l1m = R.l1_loss_map(pred * m, gt * m)
    close(l1m, Z["loss_l1_map"])
    close(R.l1_loss(pred * m, gt * m), Z["loss_l1_plain"])
    seg_tr = R.get_trained_seg(segq, sc.detach())
    loss = R.Scale_balance_loss(l1m, seg_tr)
    loss.backward()
    close(loss, Z["loss_balance"])
    close(pred.grad, Z["loss_balance_vpred"])
    close(sc.grad, Z["loss_balance_vscale"])


def test_resized_ground_truth_equals_the_fixture():
    gt, mask = R.read_sam_clip_feature(t("loss_img_embed"), t("loss_seg_lo"), t("loss_scale_map"))
    close(gt, Z["loss_gt_resized"])
    np.testing.assert_array_equal(mask.numpy(), Z["loss_mask_resized"])


def test_banded_ground_truth_equals_the_whole_image():
    emb, seg, sc = t("loss_img_embed"), t("loss_seg_lo"), t("loss_scale_map")
    whole, mw = R.read_sam_clip_feature(emb, seg, sc)
    for r0, r1 in ((0, 5), (5, 6), (6, 14)):
        band, mb = R.read_sam_clip_feature(emb, seg, sc, rows=range(r0, r1))
        assert torch.equal(band, whole[:, r0:r1]) and torch.equal(mb, mw[:, r0:r1])


def test_minus_one_reads_the_last_embedding_row():
    """id -1 is Python's last row: it still enters the blend, only the mask drops the pixel."""
    emb = torch.arange(12, dtype=torch.float64).reshape(3, 4)
    seg = torch.full((4, 1, 2), -1.0)
    seg[1:, 0, 1] = 0.0
    sc = torch.tensor([0.5, 0.25, 0.25]).reshape(3, 1, 1).expand(3, 1, 2).contiguous()
    gt, mask = R.read_sam_clip_feature(emb, seg, sc)
    assert torch.equal(gt[:, 0, 0], emb[2]) and torch.equal(gt[:, 0, 1], emb[0])
    assert mask.tolist() == [[[False, True]]]


SHAPES = [((7, 9), (67, 93)),      # up, non-integer ratios
          ((540, 960), (1080, 1920)),  # up x2
          ((1440, 1080), (730, 541)),  # down
          ((37, 53), (37, 53)),    # identity
          ((13, 17), (1, 17)),     # a single target row: bilinear scale 0
          ((13, 17), (13, 1)),     # a single target column
          ((1, 1), (5, 3)),        # a single source pixel
          ((50, 31), (97, 7)),     # up one way, down the other
          ((3, 4), (6, 8))]        # exactly x2 (the nearest resize's shift case)


@pytest.mark.parametrize("src,dst", SHAPES)
def test_explicit_taps_equal_F_interpolate(src, dst):
    """bilinear_taps / nearest_index against F.interpolate on float32 input (CPU): the nearest indices identical (the mask
    is an exact result), the blends within 1e-6 of float32 torch (a float32 blend of at most four terms of |x| <= 1)."""
    g = torch.Generator().manual_seed(src[0] * 131 + dst[1])
    x = torch.rand(2, *src, generator=g) * 2 - 1
    got = R.bilinear_resize(x, *dst)
    ref = F.interpolate(x[None], size=dst, mode="bilinear", align_corners=True)[0]
    assert float((got - ref.double()).abs().max()) <= 1e-6
    # nearest: a ramp that encodes the source coordinates recovers them exactly
    ramp = (torch.arange(src[0])[:, None] * src[1] + torch.arange(src[1])[None, :]).float()[None]
    near = F.interpolate(ramp[None], size=dst, mode="nearest")[0, 0].long()
    ny, nx = R.nearest_index(src[0], dst[0]), R.nearest_index(src[1], dst[1])
    assert torch.equal(near, ny[:, None] * src[1] + nx[None, :])
    assert torch.equal(R.nearest_resize(ramp, *dst)[0].long(), near)


def test_normalize_equals_F_normalize():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(512, 3, 5, generator=g, dtype=torch.float64)
    x[:, 0, 0] = 0.0
    assert torch.allclose(R.normalize(x), F.normalize(x, dim=0), rtol=1e-15, atol=0)


def test_balance_loss_without_segments_raises_like_the_reference():
    with pytest.raises(ValueError):
        R.Scale_balance_loss(torch.zeros(2, 3), torch.full((2, 3), -1.0))
