"""N14 without a GPU: the integer restatement tests/tilecut_ref.py against the reference's own get_seg_img / pad_img
(tests/golden/tilecut_vectors.npz), its resize against float64 bilinear within a DERIVED bound and at its fixed points, against
cv2 itself where tests/golden/tilecut_cv2_vectors.npz exists, and the argument validation of the C entries and of cut_tiles
(nothing is launched here)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tilecut_ref as R  # noqa: E402

SIDES = (1, 2, 3, 7, 37, 100, 223, 224, 225, 300, 447, 448, 449, 640, 1080)


def squares(l):
    """Random bytes and 0 / 255 checkerboard noise (every tap pair sees the largest step there is)."""
    g = np.random.default_rng(1000 + l)
    return g.integers(0, 256, (l, l, 3), dtype=np.uint8), (g.integers(0, 2, (l, l, 3)) * 255).astype(np.uint8)


# ---- crop, mask and pad: the reference's own squares ------------------------------------------------------------------------------
def test_fixture_holds_the_promised_cases():
    names = [c[0] for c in R.fixture_squares()]
    assert names == list(R.A_CASES) + ["b224"]
    image, masks, boxes = R.image_a()
    assert np.array_equal(R.Z["a_image"], image) and np.array_equal(R.Z["a_boxes"], boxes)   # the GPU tests rebuild the same inputs
    assert np.array_equal(np.unpackbits(R.Z["a_masks"])[:masks.size].reshape(masks.shape), masks)
    assert image.shape == (37, 70, 3) and (37 * 70) % 64 == 30 and 70 % 64 != 0


def test_crop_and_pad_equal_the_reference_bit_for_bit():
    for name, image, mask, box, want in R.fixture_squares():
        got = R.square_ref(image, mask, box)
        assert got.dtype == want.dtype == np.uint8 and got.shape == want.shape, name
        assert np.array_equal(got, want), name


def test_pad_offsets_follow_pad_img():
    """`if h > w` centres horizontally, `else` (ties included) vertically; an odd difference floors."""
    image, masks, boxes = R.image_a()
    tall, wide = R.square_ref(image, masks[0], boxes[0]), R.square_ref(image, masks[1], boxes[1])
    assert tall.shape == wide.shape == (9, 9, 3)
    assert np.array_equal(tall[:, 2:6], image[5:14, 11:15]) and not tall[:, :2].any() and not tall[:, 6:].any()
    assert np.array_equal(wide[2:6], image[20:24, 30:39]) and not wide[:2].any() and not wide[6:].any()
    bgr = R.square_ref(image, masks[0], boxes[0], bgr=True)
    assert np.array_equal(bgr, tall[..., ::-1])
    over = R.square_ref(image, masks[4], boxes[4])          # clipped as the slice clips it: 10 x 12 of a 25 x 40 box
    assert over.shape == (12, 12, 3) and np.array_equal(over[:, 1:11], image[25:37, 60:70])
    outside = R.square_ref(image, masks[7], boxes[7])       # set pixels outside the box do not appear
    assert np.array_equal(outside.any(axis=2)[2:15], masks[7, 10:23, 20:37])


@pytest.mark.parametrize("box", [(-1, 0, 5, 5), (0, -1, 5, 5), (70, 0, 1, 1), (0, 37, 1, 1), (3, 3, 0, 4), (3, 3, 4, 0), (3, 3, -2, 4)])
def test_boxes_the_reference_cannot_cut_raise(box):
    with pytest.raises(ValueError):
        R.clip_box(box, 37, 70)


# ---- the resize ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l", SIDES)
def test_resize_is_within_one_level_of_float64_bilinear(l):
    """The bound is derived, not tuned: coefficient rounding moves the value by at most 255 / 4096 < 0.0625 per axis (0.125
    together), the two >> 16 truncations by at most 0.25 each (0.5 together, in quarter levels before the final >> 2), the >> 4 by
    under 0.01, and the final rounding by 0.5: under 1.26 from the real value, hence under 2 -- i.e. at most 1 -- from its
    rounding.  Measured: 0.81 and 1."""
    for sq in squares(l):
        got, real = R.resize_ref(sq).astype(np.float64), R.bilinear_f64(sq)
        to_real, to_rounded = np.abs(got - real).max(), np.abs(got - np.rint(real)).max()
        print(f"l = {l}: {to_real:.4f} from float64 bilinear, {to_rounded:.0f} from its rounding")
        assert to_real < 1.26
        assert to_rounded <= 1


def test_identity_at_224_and_area_mean_at_448():
    for sq in squares(224):
        assert np.array_equal(R.resize_ref(sq), sq)
    for sq in squares(448):
        assert np.array_equal(R.resize_ref(sq), R.area2_ref(sq))
    s0, s1, a0, a1 = R.tap_table(448)
    assert np.array_equal(s0, 2 * np.arange(224)) and np.array_equal(s1, s0 + 1) and (a0 == 1024).all() and (a1 == 1024).all()
    s0, s1, a0, a1 = R.tap_table(224)
    assert np.array_equal(s0, np.arange(224)) and (a0 == 2048).all() and (a1 == 0).all()


def test_tap_tables_are_convex_and_inside_for_every_side():
    for l in range(1, 2049):
        s0, s1, a0, a1 = R.tap_table(l)
        assert np.array_equal(a0 + a1, np.full(224, 2048)), l
        assert a0.min() >= 0 and a1.min() >= 0, l
        assert s0.min() >= 0 and s1.max() <= l - 1 and (s1 - s0 >= 0).all() and (s1 - s0 <= 1).all(), l
    s0, s1, a0, a1 = R.tap_table(1)
    assert not s0.any() and not s1.any() and (a0 == 2048).all()    # l = 1: every tap clamps


def test_constant_squares_stay_constant():
    for l in (1, 5, 223, 449, 1080):
        for v in (0, 1, 128, 255):
            assert (R.resize_ref(np.full((l, l, 3), v, np.uint8)) == v).all(), (l, v)


@pytest.mark.skipif(not os.path.exists(R.CV2_FIXTURE), reason="tests/golden/tilecut_cv2_vectors.npz is written by "
                    "make_golden_tilecut.py --cv2 on a machine with cv2; until then the resize is restated, unpinned")
def test_resize_equals_cv2():
    z = np.load(R.CV2_FIXTURE)
    for l in z["sides"]:
        assert np.array_equal(R.resize_ref(z[f"square_{l}"]), z[f"tile_{l}"]), int(l)
    for key in z.files:
        if key.startswith(("a_tile", "b_tile")):
            assert np.array_equal(R.resize_ref(R.Z[key.replace("tile", "square")]), z[key]), key


def test_boxes_ref_and_sam_xywh():
    m = np.zeros((3, 5, 13), bool)
    m[0, 1:4, 2:9] = True
    m[2, 4, 12] = True
    b = R.boxes_ref(m)
    assert b.tolist() == [[2, 1, 8, 3], [0, 0, -1, -1], [12, 4, 12, 4]]
    assert R.sam_xywh(b).tolist() == [[2, 1, 6, 2], [0, 0, -1, -1], [12, 4, 0, 0]]
    from gags_amd import tilecut
    assert np.array_equal(tilecut.sam_xywh(b), R.sam_xywh(b))
    assert torch.equal(tilecut.sam_xywh(torch.from_numpy(b)), torch.from_numpy(R.sam_xywh(b)))


# ---- argument validation: codes, no launch ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from gags_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_c_entries_validate_before_any_launch(lib):
    buf = ctypes.create_string_buffer(64)
    P = ctypes.cast(buf, ctypes.c_void_p)   # a HOST pointer: a launch would fault, a validation error returns first
    cap = lib.gags_masks_max_count()
    assert lib.gags_tilecut_side() == 224

    def cut(n_tiles=4, H=37, W=70, image=P, bgr=0, n_masks=4, bits=P, index=P, boxes=P, u8=P, f32=P):
        return lib.gags_tilecut(n_tiles, H, W, image, bgr, n_masks, bits, index, boxes, u8, f32, None)
    assert cut(n_tiles=-1) == -1
    assert cut(H=4096, W=4096) == -1                    # H W = 2^24
    assert cut(H=0) == -1 and cut(W=0) == -1 and cut(H=-3, W=-5) == -1
    assert cut(u8=None, f32=None) == -1                 # both outputs null
    assert cut(n_tiles=cap + 1) == -1 and cut(n_masks=cap + 1) == -1
    assert cut(n_masks=-1) == -1 and cut(n_masks=0) == -1
    assert cut(bgr=2) == -1 and cut(bgr=-1) == -1
    for name in ("image", "bits", "index", "boxes"):
        assert cut(**{name: None}) == -1, name
    assert cut(n_tiles=0) == 0                           # nothing to cut: ok, nothing launched
    assert cut(n_tiles=0, u8=None, f32=None) == -1

    def box(n_masks=4, H=37, W=70, bits=P, boxes=P):
        return lib.gags_tilecut_boxes(n_masks, H, W, bits, boxes, None)
    assert box(n_masks=-1) == -1 and box(n_masks=cap + 1) == -1
    assert box(H=4096, W=4096) == -1 and box(H=0) == -1 and box(W=-1) == -1
    assert box(bits=None) == -1 and box(boxes=None) == -1
    assert box(n_masks=0) == 0


def test_cut_tiles_rejects_what_it_cannot_serve():
    from gags_amd import tilecut
    image = torch.zeros(37, 70, 3, dtype=torch.uint8)
    bits = torch.zeros(1, 41, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        tilecut.cut_tiles(image, bits, [[0, 0, 5, 5]])
    with pytest.raises(RuntimeError, match="no CPU path"):
        tilecut.mask_boxes(bits, 37, 70)
    with pytest.raises(RuntimeError, match="no CPU path"):
        tilecut.level_tiles(image, [[], [], [], []])
    # what is wrong whatever the device is a ValueError, and comes first
    with pytest.raises(ValueError, match="uint8"):
        tilecut.cut_tiles(image.float(), bits, [[0, 0, 5, 5]])
    with pytest.raises(ValueError, match="uint8"):
        tilecut.cut_tiles(image.permute(2, 0, 1), bits, [[0, 0, 5, 5]])
    for bad in ([70, 0, 5, 5], [0, 37, 5, 5], [-1, 0, 5, 5], [3, 3, 0, 4], [3, 3, 4, -1]):
        with pytest.raises(ValueError, match="does not cut"):
            tilecut.cut_tiles(image, bits, [bad])
    with pytest.raises(ValueError, match="does not cut"):
        tilecut._host_boxes(torch.tensor([[0, 0, 5, 5], [3, 3, 0, 4]]), 37, 70)
    with pytest.raises(ValueError, match=r"\[K, 4\]"):
        tilecut._host_boxes([[0, 0, 5]], 37, 70)
    assert tilecut._host_boxes([[60, 25, 25, 40]], 37, 70).tolist() == [[60, 25, 25, 40]]   # an overhang is clipped, not refused
    assert tilecut._host_boxes(np.array([[1.9, 2.9, 5.9, 5.9]]), 37, 70).tolist() == [[1, 2, 5, 5]]   # np.int32(bbox) truncates
