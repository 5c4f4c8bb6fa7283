"""N10 on the GPU: the bit-packed SAM mask post-processing (gags_amd/sam_masks.py, csrc/sam_masks.hip) against numpy
(packing, integer matmul), against the restatement tests/sam_masks_ref.py and against the reference's own mask_nms /
masks_update (tests/golden/sam_masks_vectors.npz).  Everything is bit-exact: there is no tolerance in this file."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sam_masks_ref as R  # noqa: E402
from sam_masks_ref import LEVELS, THRESHOLDS, Z, case_masks, case_scores, scene_levels  # noqa: E402

SIZES = [(1, 1), (5, 13), (37, 70), (64, 64)]   # one bit; one word + one bit; a 30-bit tail; an exact multiple


def SM():
    from gags_amd import sam_masks
    return sam_masks


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def chunk_size():
    """(H, W) just larger than one word chunk of one block of the pair kernel: the cross-block accumulation runs."""
    words = SM().pair_chunk_words()
    return 64, words + 3     # 64 (words + 3) pixels = words + 3 words: a second block with three words


def random_masks(seed, M, H, W):
    return R.rect_masks(np.random.default_rng(seed), M, H, W)


@pytest.mark.parametrize("hw", SIZES)
def test_pack_masks(hw):
    H, W = hw
    rng = np.random.default_rng(H * 100 + W)
    m = rng.random((7, H, W)) < 0.5
    m[0] = True
    m[1] = False
    want_bits, want_area = R.pack_bits(m)
    as_u8 = np.where(m, rng.integers(1, 256, m.shape), 0).astype(np.uint8)   # set = any nonzero byte
    assert (as_u8 > 1).any() or H * W == 1
    for src in (dev(m), dev(as_u8)):
        bits, area = SM().pack_masks(src)
        assert bits.dtype == torch.int64 and area.dtype == torch.int32
        assert bits.shape == (7, (H * W + 63) // 64)
        assert np.array_equal(bits.cpu().numpy().view(np.uint64), want_bits)
        assert np.array_equal(area.cpu().numpy(), want_area)
    assert int(area[0]) == H * W and int(area[1]) == 0
    # a non-contiguous view is packed as its values, not as its storage
    bits2, _ = SM().pack_masks(dev(m).flip(0))
    assert np.array_equal(bits2.cpu().numpy().view(np.uint64), want_bits[::-1])


@pytest.mark.parametrize("M", [1, 2, 33, 70])
def test_pair_intersections(M):
    for H, W in SIZES + [chunk_size()]:
        rng = np.random.default_rng(M * 1000 + H + W)
        m = rng.random((M, H, W)) < rng.uniform(0.2, 0.8, (M, 1, 1))
        bits, area = SM().pack_masks(dev(m))
        inter = SM().pair_intersections(bits)
        assert inter.dtype == torch.int32 and inter.shape == (M, M)
        got = inter.cpu().numpy()
        flat = m.reshape(M, -1).astype(np.int64)
        assert np.array_equal(got, flat @ flat.T), (M, H, W)
        assert np.array_equal(got, got.T)
        assert np.array_equal(np.diagonal(got), area.cpu().numpy())


def test_pair_intersections_is_repeatable():
    """Integer atomics: the same matrix on every run, and nothing is left over from the previous call's buffer."""
    H, W = chunk_size()
    m = random_masks(5, 40, H, W)
    bits, _ = SM().pack_masks(dev(m))
    a = SM().pair_intersections(bits)
    b = SM().pair_intersections(bits)
    assert torch.equal(a, b)


def gpu_nms(masks, scores, **kw):
    """The GPU's idx, colmax, keeps and selection as the restatement's dict."""
    sm = SM()
    thr = {"iou_thr": 0.7, "score_thr": 0.1, "inner_thr": 0.2, **kw}
    idx, keep, keeps, zero = sm._nms_device(dev(masks), scores.cuda(), **thr)
    bits, area = sm.pack_masks(dev(masks))
    colmax = sm.column_maxima(sm.pair_intersections(bits), area, idx)
    assert not bool(zero)
    return {"idx": idx.cpu(), "colmax": colmax.cpu(), "keeps": keeps.cpu(), "selected": sm.mask_nms(dev(masks), scores.cuda(), **kw).cpu()}


def assert_same_nms(got, want, what):
    assert torch.equal(got["idx"], want["idx"]), what
    assert got["colmax"].dtype == torch.float32
    assert got["colmax"].numpy().tobytes() == want["colmax"].numpy().tobytes(), what
    assert torch.equal(got["keeps"], want["keeps"]), what
    assert got["selected"].dtype == torch.int64 and torch.equal(got["selected"], want["selected"]), what


@pytest.mark.parametrize("case", [str(c) for c in Z["cases"]])
def test_nms_on_the_fixture(case):
    """Column maxima, the four keep vectors and the selection: the reference's own numbers, under both threshold sets."""
    masks, scores = case_masks(case), case_scores(case)
    for t, kw in THRESHOLDS.items():
        got = gpu_nms(masks, scores, **kw)
        assert np.array_equal(got["selected"].numpy(), Z[f"{case}_{t}_selected"]), t
        assert got["colmax"].numpy().tobytes() == Z[f"{case}_{t}_colmax"].tobytes(), t
        assert np.array_equal(got["keeps"].numpy(), Z[f"{case}_{t}_keeps"]), t


@pytest.mark.parametrize("seed,M,hw", [(1, 1, (5, 13)), (2, 2, (1, 1)), (3, 33, (37, 70)), (4, 70, (64, 64)), (5, 45, None)])
def test_nms_on_fresh_cases(seed, M, hw):
    H, W = hw or chunk_size()
    rng = np.random.default_rng(seed)
    masks = R.rect_masks(rng, M, H, W) if H * W > 1 else np.ones((M, 1, 1), bool)
    scores = torch.from_numpy(rng.uniform(0.6, 1.0, M))
    for kw in THRESHOLDS.values():
        assert_same_nms(gpu_nms(masks, scores, **kw), R.nms(masks, scores, **kw), (seed, kw))
    # scores in another dtype are compared in that dtype; ties go to the lower index
    s32 = scores.float()
    s32[M // 2:] = s32[0]
    assert_same_nms(gpu_nms(masks, s32), R.nms(masks, s32), (seed, "fp32 ties"))


def test_top3_fallback():
    masks = random_masks(11, 9, 37, 70)
    scores = torch.from_numpy(np.random.default_rng(11).uniform(0.2, 0.6, 9))
    kw = THRESHOLDS["call"]                       # score_thr = 0.7: nobody passes
    want = R.nms(masks, scores, **kw)
    assert want["keeps"][1].tolist() == [True] * 3 + [False] * 6
    assert_same_nms(gpu_nms(masks, scores, **kw), want, "fallback")


@pytest.mark.parametrize("scene", ["a", "b", "c"])
def test_masks_update_on_the_fixture(scene):
    levels = scene_levels(scene)
    for t, kw in THRESHOLDS.items():
        kept = SM().masks_update(*levels, **kw)
        assert isinstance(kept, tuple) and len(kept) == 4
        for lname, lvl, src in zip(LEVELS, kept, levels):
            ids = [m["id"] for m in lvl]
            assert ids == Z[f"{scene}_{lname}_{t}_kept"].tolist(), (lname, t)
            assert all(m is src[m["id"]] for m in lvl)      # the very dicts, in their original order
    kept = SM().masks_update(levels[0], [], levels[2])
    assert kept[1] == [] and len(kept) == 3


def test_seg_map_and_assemble():
    H, W = 37, 70
    masks = random_masks(21, 12, H, W)
    bits, _ = SM().pack_masks(dev(masks))
    for kept, offset in (([0, 3, 4, 9, 11], 0), ([5], 7), (list(range(12)), 100), ([], 3)):
        got = SM().seg_map(bits, torch.tensor(kept, dtype=torch.int64).cuda(), H, W, offset=offset)
        assert got.dtype == torch.int32 and got.shape == (H, W)
        assert np.array_equal(got.cpu().numpy(), R.paint(masks[kept], H, W, offset)), (kept, offset)
    # a mask painted over completely leaves no id
    over = np.stack([masks[0], masks[0] | masks[1]])
    b2, _ = SM().pack_masks(dev(over))
    seg = SM().seg_map(b2, torch.arange(2).cuda(), H, W).cpu().numpy()
    assert 0 not in seg and np.array_equal(seg, R.paint(over, H, W))
    # four levels: one empty, one with a single mask; tensors and lists of dicts alike
    lv = [masks[:5], masks[5:5], masks[5:6], masks[6:]]
    want_maps, want_len = R.concat_levels(lv, H, W)
    maps, lengths = SM().assemble_seg_maps([dev(x) for x in lv])
    assert maps.dtype == torch.int32 and maps.shape == (4, H, W) and lengths.tolist() == want_len.tolist() == [5, 0, 1, 6]
    assert np.array_equal(maps.cpu().numpy(), want_maps)
    assert (maps[1] == -1).all() and int(maps.max()) + 1 == 12
    as_dicts = [[{"segmentation": m} for m in x] for x in lv]
    maps2, lengths2 = SM().assemble_seg_maps(as_dicts)
    assert torch.equal(maps2, maps) and torch.equal(lengths2, lengths)
    empty, zero = SM().assemble_seg_maps([[], [], [], []], hw=(H, W))
    assert (empty == -1).all() and empty.shape == (4, H, W) and zero.tolist() == [0, 0, 0, 0]
    # the tail word and the word-exact size
    for h, w in ((1, 1), (5, 13), (64, 64)):
        m = random_masks(h * w, 6, h, w) if h * w > 1 else np.ones((6, 1, 1), bool)
        b, _ = SM().pack_masks(dev(m))
        got = SM().seg_map(b, torch.tensor([1, 2, 4]).cuda(), h, w, offset=2)
        assert np.array_equal(got.cpu().numpy(), R.paint(m[[1, 2, 4]], h, w, 2)), (h, w)


def test_no_masks():
    sm = SM()
    e = torch.zeros(0, 5, 13, dtype=torch.bool, device="cuda")
    sel = sm.mask_nms(e, torch.zeros(0, dtype=torch.float64, device="cuda"))
    assert sel.shape == (0,) and sel.dtype == torch.int64
    assert sm.nms_keep_indices(e, torch.zeros(0, dtype=torch.float64, device="cuda")).shape == (0,)
    bits, area = sm.pack_masks(e)
    assert bits.shape == (0, 2) and area.shape == (0,)
    assert sm.pair_intersections(bits).shape == (0, 0)


def test_zero_area_mask_raises_and_the_process_stays_healthy():
    masks = random_masks(31, 6, 37, 70)
    masks[2] = False
    scores = torch.from_numpy(np.linspace(0.9, 0.5, 6))
    with pytest.raises(ValueError, match="without a set pixel"):
        SM().mask_nms(dev(masks), scores.cuda())
    # the kernels themselves tolerate it: the counts are still exact
    bits, area = SM().pack_masks(dev(masks))
    flat = masks.reshape(6, -1).astype(np.int64)
    assert np.array_equal(SM().pair_intersections(bits).cpu().numpy(), flat @ flat.T) and int(area[2]) == 0
    colmax = SM().column_maxima(SM().pair_intersections(bits), area, torch.arange(6).cuda())
    assert not torch.isnan(colmax).any()         # a NaN never wins a maximum
    masks[2, 0, 0] = True
    assert_same_nms(gpu_nms(masks, scores), R.nms(masks, scores), "after the refusal")


def test_end_to_end_raw_masks_to_s_npy(tmp_path):
    """raw SAM levels -> masks_update -> assemble_seg_maps -> <image>_s.npy -> load_language_features."""
    from gags_amd import io_formats as IO
    levels = scene_levels("b")
    kw = THRESHOLDS["call"]
    kept = SM().masks_update(*levels, **kw)
    maps, lengths = SM().assemble_seg_maps(kept)
    want_kept = R.masks_update(*levels, **kw)
    want_maps, want_len = R.concat_levels([[m["segmentation"] for m in lvl] for lvl in want_kept], 64, 64)
    assert lengths.tolist() == want_len.tolist()
    feature = torch.zeros(int(lengths.sum()), 512)
    prefix = str(tmp_path / "frame_00001")
    IO.save_language_features(prefix, feature, maps)
    emb, seg = IO.load_language_features(prefix)
    assert emb.shape == (int(want_len.sum()), 512)
    assert seg.dtype == torch.float32 and np.array_equal(seg.numpy(), want_maps.astype(np.float32))
