"""N10 (include/gags_next.h) without a GPU: the SAM mask post-processing entries are declared, exported and typed; every
argument check returns its code before anything is launched; the fixture tests/golden/sam_masks_vectors.npz (the
reference's own mask_nms / masks_update, make_golden_sam_masks.py) equals the restatement tests/sam_masks_ref.py exactly;
the restatement's painting, level concatenation and top-3 fallback on hand-made cases; the _f.npy / _s.npy round trip."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import sam_masks_ref as R  # noqa: E402

from sam_masks_ref import LEVELS, THRESHOLDS, Z, case_masks, case_scores, scene_levels  # noqa: E402

N10 = {"gags_masks_max_count", "gags_masks_pair_chunk_words", "gags_masks_pack", "gags_masks_pairs", "gags_masks_colmax",
       "gags_masks_paint", "gags_masks_nms_scratch_bytes", "gags_masks_nms_colmax"}
EINVAL, ESCRATCH = -1, -3


@pytest.fixture(scope="module")
def lib():
    from gags_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_n10_entries_are_declared_exported_and_typed(lib):
    from gags_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(os.path.dirname(ROOT), "include", "gags_next.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(gags_masks_\w+)\s*\(", src)) == N10
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in N10:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
    for name in ("gags_masks_pack", "gags_masks_pairs", "gags_masks_paint", "gags_masks_nms_colmax", "gags_masks_nms_scratch_bytes"):
        args = _lib.SIGNATURES[name][1]
        assert args[0] is ctypes.c_int and args[1] is ctypes.c_int64, name  # M as int, the pixel count as 64 bits
    assert lib.gags_masks_max_count() >= 1024
    assert lib.gags_masks_max_count() ** 2 * 4 <= 256 << 20                 # the cap is what bounds inter
    chunk = lib.gags_masks_pair_chunk_words()
    assert chunk >= 64 and chunk % 64 == 0
    assert lib.gags_abi_version() == 2


def test_argument_checks_return_before_any_launch(lib):
    P = ctypes.c_void_p(256)  # never dereferenced: every call below returns before a launch
    cap = lib.gags_masks_max_count()
    hw = 37 * 70
    nb = lib.gags_masks_nms_scratch_bytes(40, hw)
    assert nb >= 40 * ((hw + 63) // 64) * 8 + 40 * 40 * 4
    ok = {"gags_masks_pack": [40, hw, P, P, P, None],
          "gags_masks_pairs": [40, hw, P, P, None],
          "gags_masks_paint": [40, hw, P, 7, P, 0, P, None],
          "gags_masks_nms_colmax": [40, hw, P, P, P, P, P, nb, None]}
    pointers = {"gags_masks_pack": (2, 3, 4), "gags_masks_pairs": (2, 3), "gags_masks_paint": (2, 4, 6),
                "gags_masks_nms_colmax": (2, 3, 4, 5, 6)}

    def call(name, **kw):
        a = list(ok[name])
        for i, v in kw.items():
            a[int(i[1:])] = v
        return getattr(lib, name)(*a)
    for name in ok:
        assert call(name, a0=-1) == EINVAL, name                 # negative M
        assert call(name, a0=cap + 1) == EINVAL, name            # M over the cap
        assert call(name, a1=0) == EINVAL, name                  # H W = 0
        assert call(name, a1=-5) == EINVAL, name
        assert call(name, a1=1 << 24) == EINVAL, name            # H W = 2^24
        for i in pointers[name]:
            assert call(name, **{f"a{i}": None}) == EINVAL, (name, i)
    assert call("gags_masks_nms_colmax", a7=nb - 1) == ESCRATCH  # short scratch
    assert call("gags_masks_nms_colmax", a7=0) == ESCRATCH
    assert call("gags_masks_paint", a3=-1) == EINVAL             # negative K
    assert call("gags_masks_paint", a3=41) == EINVAL             # more kept masks than masks
    assert call("gags_masks_paint", a5=-1) == EINVAL             # negative offset
    assert call("gags_masks_paint", a3=40, a5=(1 << 31) - 40) == EINVAL  # offset + K past int32
    fc = lib.gags_masks_colmax
    assert fc(-1, P, P, P, P, None) == EINVAL and fc(cap + 1, P, P, P, P, None) == EINVAL
    for i in range(1, 5):
        a = [40, P, P, P, P, None]
        a[i] = None
        assert fc(*a) == EINVAL, i
    # M == 0: nothing to do, nothing launched, every pointer may be NULL
    assert lib.gags_masks_pack(0, hw, None, None, None, None) == 0
    assert lib.gags_masks_pairs(0, hw, None, None, None) == 0
    assert fc(0, None, None, None, None, None) == 0
    assert lib.gags_masks_nms_colmax(0, hw, None, None, None, None, None, 0, None) == 0
    for bad in ((-1, hw), (cap + 1, hw), (40, 0), (40, 1 << 24), (0, hw)):
        assert lib.gags_masks_nms_scratch_bytes(*bad) == 0, bad
    assert lib.gags_masks_nms_scratch_bytes(cap, (1 << 24) - 1) > cap * cap * 4


def test_cpu_tensors_are_rejected():
    from gags_amd import sam_masks as SM
    m = torch.zeros(2, 4, 4, dtype=torch.bool)
    for fn, args in ((SM.pack_masks, (m,)), (SM.mask_nms, (m, torch.ones(2))),
                     (SM.pair_intersections, (torch.zeros(2, 1, dtype=torch.int64),)),
                     (SM.seg_map, (torch.zeros(2, 1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), 4, 4))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(*args)


def test_fixture_layout():
    cases = [str(c) for c in Z["cases"]]
    assert len(cases) == 12 and len({c.split("_")[0] for c in cases}) >= 3
    counts = sorted(int(Z[f"{c}_shape"][0]) for c in cases)
    assert counts[0] == 1 and counts[-1] == 40
    assert {tuple(int(v) for v in Z[f"{c}_shape"][1:]) for c in cases} == {(37, 70), (64, 64)}
    for c in cases:
        s = case_scores(c)
        assert s.dtype == torch.float64 and len(set(s.tolist())) == len(s)
        m = case_masks(c)
        assert m.reshape(len(m), -1).any(axis=1).all()
    assert np.array_equal(Z["thresholds_def"], [0.7, 0.1, 0.2]) and np.array_equal(Z["thresholds_call"], [0.8, 0.7, 0.5])
    for name in ("iou", "score", "inner_u", "inner_l", "quirk"):
        assert len(Z[f"decided_by_{name}"]) >= 1, name


@pytest.mark.parametrize("case", [str(c) for c in Z["cases"]])
def test_restatement_equals_the_reference(case):
    """Selected indices, the three column maxima and all four keep vectors, under both threshold sets, bit for bit."""
    masks, scores = case_masks(case), case_scores(case)
    for t, kw in THRESHOLDS.items():
        mine = R.nms(masks, scores, **kw)
        assert np.array_equal(mine["selected"].numpy(), Z[f"{case}_{t}_selected"]), t
        assert mine["colmax"].numpy().tobytes() == Z[f"{case}_{t}_colmax"].tobytes(), t
        assert np.array_equal(mine["keeps"].numpy(), Z[f"{case}_{t}_keeps"]), t


def test_what_decides_the_recorded_cases():
    """The cases the generator recorded really are decided as it says: a mask lost to one keep vector alone, and a fourth
    keep vector that the first superdiagonal (the reference's tril(diagonal=1)) changes."""
    for k, name in enumerate(("iou", "score", "inner_u", "inner_l")):
        for tag in Z[f"decided_by_{name}"]:
            keeps = Z[f"{tag}_keeps"]
            assert (~keeps[k] & np.delete(keeps, k, axis=0).all(axis=0)).any(), tag
    for tag in Z["decided_by_quirk"]:
        case, t = str(tag).rsplit("_", 1)
        plain = R.nms(case_masks(case), case_scores(case), quirk=False, **THRESHOLDS[t])
        assert not np.array_equal(plain["keeps"][3].numpy(), Z[f"{tag}_keeps"][3]), tag
        assert np.array_equal(plain["keeps"][:3].numpy(), Z[f"{tag}_keeps"][:3]), tag


@pytest.mark.parametrize("scene", ["a", "b", "c"])
def test_restatement_masks_update_equals_the_reference(scene):
    levels = scene_levels(scene)
    for t, kw in THRESHOLDS.items():
        kept = R.masks_update(*levels, **kw)
        assert isinstance(kept, tuple) and len(kept) == 4
        for lname, lvl in zip(LEVELS, kept):
            assert [m["id"] for m in lvl] == Z[f"{scene}_{lname}_{t}_kept"].tolist(), (lname, t)


def test_restatement_pack_bits():
    m = np.zeros((2, 5, 13), np.uint8)
    m[0, 0, 0] = 1
    m[0, 4, 12] = 7          # pixel 64: bit 0 of word 1
    m[1, 4, 11] = 255        # pixel 63: the top bit of word 0
    bits, area = R.pack_bits(m)
    assert bits.shape == (2, 2) and bits.dtype == np.uint64
    assert bits.tolist() == [[1, 1], [1 << 63, 0]] and area.tolist() == [2, 1]


def test_restatement_painting_and_concatenation():
    H, W = 3, 4
    a = np.zeros((H, W), bool)
    a[0:2, 0:2] = True
    b = np.zeros((H, W), bool)
    b[1:3, 1:3] = True
    c = np.zeros((H, W), bool)
    c[0:2, 0:2] = True       # covers a completely
    seg = R.paint([a, b], H, W)
    assert seg.dtype == np.int32
    assert seg.tolist() == [[0, 0, -1, -1], [0, 1, 1, -1], [-1, 1, 1, -1]]            # later mask wins, -1 is kept
    assert 0 not in R.paint([a, b, c], H, W) and 2 in R.paint([a, b, c], H, W)        # a fully overpainted mask leaves no id
    assert R.paint([], H, W).tolist() == [[-1] * W] * H
    assert R.paint([a], H, W, offset=5).tolist() == [[5, 5, -1, -1], [5, 5, -1, -1], [-1] * 4]
    maps, lengths = R.concat_levels([[a, b], [], [b], [a, b, c]], H, W)
    assert maps.shape == (4, H, W) and lengths.tolist() == [2, 0, 1, 3]
    assert maps[0].tolist() == seg.tolist()
    assert (maps[1] == -1).all()                                                       # an empty level
    assert maps[2].tolist() == [[-1] * 4, [-1, 2, 2, -1], [-1, 2, 2, -1]]              # offset 2 + 0
    assert maps[3].tolist() == [[5, 5, -1, -1], [5, 5, 4, -1], [-1, 4, 4, -1]]         # offset 3: b = 4, c = 5, a gone
    assert int(maps.max()) + 1 == int(lengths.sum())


def test_top3_fallback_by_hand():
    """Five disjoint masks (every IoU and inner rate is 0), scores all below score_thr: the reference would raise; the three
    best scores pass instead.  Then nested masks, ranked both ways round, with the inner rates worked out by hand (the
    upper test can never be empty -- column 0 has nothing above it -- so its fallback is unreachable)."""
    masks = np.zeros((5, 4, 10), bool)
    for k in range(5):
        masks[k, :, 2 * k:2 * k + 2] = True
    scores = torch.tensor([0.3, 0.5, 0.1, 0.4, 0.2], dtype=torch.float64)
    got = R.nms(masks, scores, iou_thr=0.8, score_thr=0.7, inner_thr=0.5)
    assert got["idx"].tolist() == [1, 3, 0, 4, 2]
    assert got["keeps"][1].tolist() == [True, True, True, False, False]
    assert got["selected"].tolist() == [1, 3, 0]
    assert R.filter_list(got["selected"], list("abcde")) == ["a", "b", "d"]
    # one passing score: no fallback
    got = R.nms(masks, torch.tensor([0.3, 0.9, 0.1, 0.4, 0.2], dtype=torch.float64), iou_thr=0.8, score_thr=0.7, inner_thr=0.5)
    assert got["selected"].tolist() == [1]
    # fewer than three masks, none passing: all of them
    assert R.nms(masks[:2], scores[:2], score_thr=0.7)["selected"].tolist() == [1, 0]
    # a big mask (100 px) ranked first and a small one (10 px) inside it: r_big = 0.1 < 0.5, r_small = 1 >= 0.85, so the
    # upper entry [0, 1] = 1 - 0.1 = 0.9 > 1 - inner_thr: column 1 fails the upper test, and through the superdiagonal
    # the lower test as well; ranked the other way round the lower entry [1, 0] fails column 0 of the lower test
    big = np.zeros((1, 10, 12), bool)
    big[0, :, :10] = True
    small = np.zeros((1, 10, 12), bool)
    small[0, 0, :10] = True
    pair = np.concatenate([big, small])
    got = R.nms(pair, torch.tensor([0.9, 0.8], dtype=torch.float64))
    assert got["colmax"].tolist() == [[0.0, 0.10000000149011612], [0.0, 0.8999999761581421], [0.0, 0.8999999761581421]]
    assert got["keeps"].tolist() == [[True, True], [True, True], [True, False], [True, False]]
    assert got["selected"].tolist() == [0]
    got = R.nms(pair, torch.tensor([0.8, 0.9], dtype=torch.float64))    # small first
    assert got["colmax"][2].tolist() == [0.8999999761581421, 0.0] and got["colmax"][1].tolist() == [0.0, 0.0]
    assert got["selected"].tolist() == [0]                               # the big mask survives again (rank 1)
    assert R.nms(pair, torch.tensor([0.8, 0.9], dtype=torch.float64), quirk=False)["selected"].tolist() == [0]
    # two small masks ranked before the big one that holds them: both lower entries [2, 0] and [2, 1] fail their columns,
    # the big mask's own column passes, so the lower test is not empty and no fallback is entered
    small2 = np.zeros((1, 10, 12), bool)
    small2[0, 5, :10] = True
    trio = np.concatenate([small, small2, big])
    got = R.nms(trio, torch.tensor([0.9, 0.8, 0.7], dtype=torch.float64))
    assert got["colmax"][2].tolist() == [0.8999999761581421, 0.8999999761581421, 0.0]
    assert got["keeps"][3].tolist() == [False, False, True]
    assert got["selected"].tolist() == [2]


def test_zero_area_is_refused_by_the_restatement():
    masks = np.zeros((2, 4, 4), bool)
    masks[0, 0, 0] = True
    with pytest.raises(ValueError):
        R.nms(masks, torch.tensor([0.5, 0.4], dtype=torch.float64))


def test_language_features_round_trip(tmp_path):
    from gags_amd import io_formats as IO
    rng = np.random.default_rng(0)
    feature = rng.standard_normal((7, 512)).astype(np.float16)     # the reference's CLIP embeddings arrive as half
    seg = rng.integers(-1, 7, (4, 9, 11)).astype(np.int32)
    prefix = str(tmp_path / "sub" / "frame_00001")
    pf, ps = IO.save_language_features(prefix, torch.from_numpy(feature), torch.from_numpy(seg))
    assert (pf, ps) == (prefix + "_f.npy", prefix + "_s.npy")
    assert np.load(pf).dtype == np.float32 and np.load(ps).dtype == np.float32
    assert np.load(pf).shape == (7, 512) and np.load(ps).shape == (4, 9, 11)
    emb, smap = IO.load_language_features(prefix)
    assert emb.dtype == torch.float32 and smap.dtype == torch.float32
    assert np.array_equal(emb.numpy(), feature.astype(np.float32)) and np.array_equal(smap.numpy(), seg.astype(np.float32))
    with pytest.raises(ValueError):
        IO.save_language_features(prefix, feature[:3], seg)          # a segment id without a feature row
    with pytest.raises(ValueError):
        IO.save_language_features(prefix, feature, seg[0])
