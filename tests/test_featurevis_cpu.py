"""N11 without a GPU: tests/featurevis_ref.py (the numpy restatement the GPU tests compare against) is tied to the reference's
own outputs in tests/golden/featurevis_vectors.npz; the host half of gags_amd.featurevis (the float64 PCA from moments, numpy's
percentile interpolation) is tied to the restatement and to numpy; the new C entries refuse bad arguments without launching."""
import ctypes
import os

import numpy as np
import pytest
import torch

import featurevis_ref as FR

HERE = os.path.dirname(os.path.abspath(__file__))
Z = np.load(os.path.join(HERE, "golden", "featurevis_vectors.npz"))
PCA_CASES = (0, 1, 2)


def fingerprint(f):
    flat = f.reshape(-1).astype(np.float64)
    probe = flat[np.linspace(0, flat.size - 1, 8).astype(np.int64)]
    return np.concatenate([[flat.sum(), (flat * flat).sum()], probe])


def case_feature(i):
    C, H, W = (int(v) for v in Z[f"pca{i}_shape"])
    return FR.synthetic_feature(C, H, W, int(Z[f"pca{i}_seed"]))


@pytest.mark.parametrize("tag", ["same", "resized"])
def test_max_mode_restatement_equals_the_reference_bit_for_bit(tag):
    feat, mask = FR.max_mode_feature(Z["mm_img_embed"], Z["mm_seg"], Z[f"mm_scale_{tag}"])
    assert feat.dtype == np.float32
    np.testing.assert_array_equal(feat, Z[f"mm_feat_{tag}"])
    np.testing.assert_array_equal(mask, Z[f"mm_mask_{tag}"])


def test_max_mode_fixture_exercises_its_edge_cases():
    emb, seg = Z["mm_img_embed"], Z["mm_seg"]
    assert emb.shape == (9, 16) and seg.shape == (4, 13, 17) and (emb[:, 0] == 0).sum() == 1
    for lev in (1, 2, 3):
        assert 0 < (seg[lev] == -1).sum() < seg[lev].size / 2
    assert len({tuple((seg[lev] == -1).ravel()) for lev in (1, 2, 3)}) == 3     # independently per level
    for tag in ("same", "resized"):
        sc = Z[f"mm_scale_{tag}"]
        assert sc[1, 2, 3] == sc[2, 2, 3] > sc[0, 2, 3]                          # a two-way tie for the maximum
        assert sc[0, 5, 7] == sc[1, 5, 7] == sc[2, 5, 7]                         # a three-way tie
    # the channel-0 quirk: a valid pixel whose selected embedding has a zero in channel 0 is masked out
    feat, mask = Z["mm_feat_same"], Z["mm_mask_same"]
    assert ((feat != 0).any(axis=0) & ~mask[0]).any()


@pytest.mark.parametrize("i", PCA_CASES)
def test_pca_restatement_equals_the_reference(i):
    f = case_feature(i)
    np.testing.assert_array_equal(fingerprint(f), Z[f"pca{i}_fingerprint"])      # the regenerated input is the recorded one
    r = FR.feature_visualize(f)
    gap64 = float(Z[f"pca{i}_gap64"])
    assert gap64 <= 1e-6 and float(Z[f"pca{i}_gap32"]) <= 1e-6
    assert np.abs(r["vis"] - Z[f"pca{i}_vis"]).max() <= gap64
    assert np.abs(r["components"] - Z[f"pca{i}_components"]).max() <= 5e-7
    assert np.abs(r["mean"] - Z[f"pca{i}_mean"]).max() <= 5e-7
    assert abs(r["q1"] - Z[f"pca{i}_q1"]) <= 5e-7 and abs(r["q99"] - Z[f"pca{i}_q99"]) <= 5e-7
    lam = r["eigenvalues"]
    assert lam[0] / lam[1] >= 1.1 and lam[1] / lam[2] >= 1.1 and lam[2] / lam[3] >= 1.5
    assert 0.01 <= float(Z[f"pca{i}_clamped"]) <= 0.05
    # the bytes render.py writes: the restatement's equal the reference's everywhere on these inputs
    np.testing.assert_array_equal((r["vis"] * 255).astype(np.uint8), (Z[f"pca{i}_vis"] * 255).astype(np.uint8))


def test_host_pca_equals_the_restatement():
    from gags_amd import featurevis as fv
    f = case_feature(1)
    s, g, S = FR.moments(f)
    mean, comps = fv.pca_from_moments(torch.from_numpy(s), torch.from_numpy(g), S)
    rmean, rcomps, _ = FR.pca_from_moments(s, g, S)
    assert np.abs(mean.numpy() - rmean).max() <= 1e-15
    assert np.abs(comps.numpy() - rcomps).max() <= 1e-12
    big = np.abs(comps.numpy()).argmax(axis=1)
    assert (comps.numpy()[np.arange(3), big] > 0).all()
    # the sign rule: the moments of the negated map give the same components
    mean_n, comps_n = fv.pca_from_moments(torch.from_numpy(-s), torch.from_numpy(g), S)
    assert np.abs(comps_n.numpy() - comps.numpy()).max() <= 1e-12 and np.abs(mean_n.numpy() + mean.numpy()).max() == 0


@pytest.mark.parametrize("n", [1, 2, 3, 100, 65537, 3 * 5120])
def test_percentile_interpolation_is_numpys(n):
    from gags_amd import featurevis as fv
    a = np.random.default_rng(n).standard_normal(n).astype(np.float32)
    prev, nxt, gamma = fv.percentile_ranks(n, (1, 99))
    assert ((0 <= prev) & (prev <= nxt) & (nxt < n)).all()
    s = np.sort(a)
    np.testing.assert_array_equal(fv.lerp_percentiles(s[prev], s[nxt], gamma), np.percentile(a, [1, 99]))


def test_new_entries_refuse_bad_arguments_without_launching():
    from gags_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    P = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.gags_sam_clip_feature_max(16, 4, 4, 4, 4, 9, None, P, P, P, P, None) == -1
    assert lib.gags_sam_clip_feature_max(12, 4, 4, 4, 4, 9, P, P, P, P, P, None) == -1        # c % 16
    assert lib.gags_sam_clip_feature_max(16, 0, 4, 4, 4, 9, P, P, P, P, P, None) == -1
    assert lib.gags_featvis_row_chunk() >= 32 and lib.gags_featvis_row_chunk() % 32 == 0
    assert lib.gags_featvis_moments_scratch_bytes(16, 12) > 0
    assert lib.gags_featvis_moments_scratch_bytes(24, 12) == 0
    assert lib.gags_featvis_moments(16, 12, None, 0, P, P, P, 1 << 20, None) == -1           # null map
    assert lib.gags_featvis_moments(24, 12, P, 0, P, P, P, 1 << 20, None) == -1              # c % 16
    assert lib.gags_featvis_moments(1040, 12, P, 0, P, P, P, 1 << 20, None) == -1            # c > 1024
    assert lib.gags_featvis_moments(16, 9, P, 0, P, P, P, 1 << 20, None) == -1               # S = 3 < 4
    assert lib.gags_featvis_moments(16, 12, P, 2, P, P, P, 1 << 20, None) == -1              # layout
    assert lib.gags_featvis_moments(16, 12, P, 0, P, P, P, 0, None) == -3                    # scratch too small
    assert lib.gags_featvis_project(16, 0, P, 0, P, P, P, None) == -1
    assert lib.gags_featvis_project(16, 12, P, 0, None, P, P, None) == -1
    ranks = (ctypes.c_int64 * 2)(0, 5)
    assert lib.gags_featvis_select_scratch_bytes(0) == 0 and lib.gags_featvis_select_scratch_bytes(9) == 0
    assert lib.gags_featvis_select_scratch_bytes(2) >= 3 * 65536 * 4
    assert lib.gags_featvis_select(5, P, 1, 1, 2, ranks, P, P, 1 << 22, None) == -1          # rank 5 of 5 values
    assert lib.gags_featvis_select(0, P, 1, 1, 2, ranks, P, P, 1 << 22, None) == -1
    assert lib.gags_featvis_select(9, P, 3, 2, 2, ranks, P, P, 1 << 22, None) == -1          # stride < group
    assert lib.gags_featvis_select(9, P, 1, 1, 9, ranks, P, P, 1 << 22, None) == -1          # more than 8 ranks
    assert lib.gags_featvis_select(9, P, 1, 1, 2, ranks, P, P, 0, None) == -3
    assert lib.gags_featvis_colour(0, P, 0.0, 1.0, P, None, None) == -1
    assert lib.gags_featvis_colour(9, None, 0.0, 1.0, P, None, None) == -1


def test_other_modes_still_raise_and_cpu_tensors_are_refused():
    from gags_amd import featurevis as fv
    from gags_amd.losses import read_sam_clip_feature
    e, seg, sc = torch.zeros(9, 16), torch.zeros(4, 5, 5), torch.zeros(3, 5, 5)
    with pytest.raises(NotImplementedError):
        read_sam_clip_feature(e, seg, sc, median_mode=True)
    with pytest.raises(NotImplementedError):
        read_sam_clip_feature(e, seg, sc, max_mode=True, show_scale_map=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        read_sam_clip_feature(e, seg, sc, max_mode=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fv.feature_visualize(torch.zeros(16, 4, 4))
