"""N14 on the GPU: the tile cut (gags_amd/tilecut.py, csrc/tilecut.hip) against the integer restatement tests/tilecut_ref.py and,
on the fixture's cases, against resize_ref of the reference's own padded squares (tests/golden/tilecut_vectors.npz).
Everything is bit-exact: there is no tolerance in this file."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tilecut_ref as R  # noqa: E402

SIZES = [(1, 1), (5, 13), (37, 70), (64, 64)]   # one bit; one word + one bit; a 30-bit tail; an exact multiple


def TC():
    from gags_amd import tilecut
    return tilecut


def SM():
    from gags_amd import sam_masks
    return sam_masks


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()   # (a copy: row-major and writable, whatever came in)


def pack(masks):
    return SM().pack_masks(dev(masks))[0]


def as_f32(u8):
    """[K, 224, 224, 3] uint8 -> [K, 3, 224, 224] fp32 exactly as preprocess.py:487 makes it: ON THE HOST, where torch's
    `/ 255.0` is an IEEE division (on a GPU tensor torch multiplies by the rounded reciprocal, which differs in the last bit
    for some bytes), then uploaded."""
    return (u8.cpu().float().permute(0, 3, 1, 2) / 255.0).contiguous().cuda()


_REF = {}


def want_a(bgr):
    """The restatement's tiles of image A, computed once per channel order and shared."""
    if bgr not in _REF:
        image, masks, boxes = R.image_a()
        _REF[bgr] = R.tiles_ref(image, masks, boxes, bgr=bgr)
        _REF[bgr].setflags(write=False)
    return _REF[bgr]


@pytest.mark.parametrize("bgr", [False, True])
def test_image_a_tiles_equal_the_restatement(bgr):
    image, masks, boxes = R.image_a()
    u8, f32 = TC().cut_tiles(dev(image), pack(masks), boxes, bgr=bgr, dtype=None)
    assert u8.shape == (len(R.A_CASES), 224, 224, 3) and u8.dtype == torch.uint8
    assert f32.shape == (len(R.A_CASES), 3, 224, 224) and f32.dtype == torch.float32
    got, want = u8.cpu().numpy(), want_a(bgr)
    for k, name in enumerate(R.A_CASES):
        assert np.array_equal(got[k], want[k]), (name, int((got[k] != want[k]).sum()))
    assert torch.equal(f32, as_f32(u8))
    # the single dtypes return the same tensors
    assert torch.equal(TC().cut_tiles(dev(image), pack(masks), boxes, bgr=bgr), f32)
    assert torch.equal(TC().cut_tiles(dev(image), pack(masks), boxes, bgr=bgr, dtype=torch.uint8), u8)
    if not bgr:   # l = 1: the tile is its one pixel; channel reversal is the only difference between the two orders
        assert (got[2] == image[1, 63]).all()
        assert np.array_equal(want_a(True), want_a(False)[..., ::-1])


def test_fixture_cases_equal_the_resize_of_the_references_squares():
    cases = R.fixture_squares()
    image, masks, boxes = R.image_a()
    got = TC().cut_tiles(dev(image), pack(masks), boxes, dtype=torch.uint8).cpu().numpy()
    for k, (name, _, _, _, square) in enumerate(cases[:-1]):
        assert np.array_equal(got[k], R.resize_ref(square)), name
    name, bimage, bmask, bbox, square = cases[-1]          # l = 224: the tile IS the reference's square
    tile = TC().cut_tiles(dev(bimage), pack(bmask[None]), bbox[None], dtype=torch.uint8).cpu().numpy()[0]
    assert np.array_equal(tile, square) and np.array_equal(tile, R.resize_ref(square))


@pytest.mark.parametrize("transpose", [False, True])
def test_image_b_sides_around_the_upscale_identity_and_area_switch(transpose):
    image, mask, boxes = R.image_b(transpose)
    assert image.shape[:2] == ((9, 450) if transpose else (450, 9))
    index = np.zeros(len(boxes), np.int64)                  # seven tiles of one mask
    u8, f32 = TC().cut_tiles(dev(image), pack(mask), boxes, index=index, dtype=None)
    got = u8.cpu().numpy()
    for k, l in enumerate(R.B_SIDES):
        square = R.square_ref(image, mask[0], boxes[k])
        assert square.shape[0] == l
        assert np.array_equal(got[k], R.resize_ref(square)), l
        if l == 224:
            assert np.array_equal(got[k], square)
        if l == 448:
            assert np.array_equal(got[k], R.area2_ref(square))
    assert torch.equal(f32, as_f32(u8))


def test_every_output_element_is_written():
    """The C entry on buffers pre-filled with 0xAB, each output alone and both together."""
    from gags_amd import _lib
    from gags_amd._lib import ptr
    image, masks, boxes = R.image_a()
    K = len(boxes)
    dimage, bits, dboxes = dev(image), pack(masks), dev(boxes.astype(np.int32))
    index = torch.arange(K, dtype=torch.int32, device="cuda")
    want = want_a(False)
    lib = _lib.load()
    for with_u8, with_f32 in ((True, True), (True, False), (False, True)):
        u8 = torch.full((K, 224, 224, 3), 0xAB, dtype=torch.uint8, device="cuda")
        f32 = torch.full((K * 3 * 224 * 224 * 4,), 0xAB, dtype=torch.uint8, device="cuda").view(torch.float32).view(K, 3, 224, 224)
        assert torch.isnan(f32).all() or (f32 < 0).all()   # 0xABABABAB is no value a tile holds
        rc = lib.gags_tilecut(K, 37, 70, ptr(dimage), 0, K, ptr(bits), ptr(index), ptr(dboxes), ptr(u8) if with_u8 else None,
                              ptr(f32) if with_f32 else None, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        if with_u8:
            assert np.array_equal(u8.cpu().numpy(), want)
        else:
            assert (u8 == 0xAB).all()
        if with_f32:
            assert torch.equal(f32, as_f32(dev(want)))
        else:
            assert (f32.view(torch.uint8) == 0xAB).all()


def test_a_box_the_python_layer_refuses_is_a_zero_tile_in_the_kernel():
    """The C entry never reads outside image or bits: a box outside the image, an empty one and a mask index outside [0, M)
    give all-zero tiles next to a valid one."""
    from gags_amd import _lib
    from gags_amd._lib import ptr
    image, masks, boxes = R.image_a()
    bad = np.array([boxes[0], (70, 0, 4, 4), (-1, 3, 4, 4), (3, 37, 4, 4), (3, 3, 0, 4), (3, 3, 4, -2), boxes[0], boxes[0]], np.int32)
    index = torch.tensor([0, 0, 0, 0, 0, 0, len(masks), -1], dtype=torch.int32, device="cuda")
    u8 = torch.full((len(bad), 224, 224, 3), 0xAB, dtype=torch.uint8, device="cuda")
    dimage, bits, dbad = dev(image), pack(masks), dev(bad)   # (named: a temporary's memory could be handed out again)
    rc = _lib.load().gags_tilecut(len(bad), 37, 70, ptr(dimage), 0, len(masks), ptr(bits), ptr(index), ptr(dbad),
                                  ptr(u8), None, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    got = u8.cpu().numpy()
    assert np.array_equal(got[0], want_a(False)[0]) and not got[1:].any()


def test_index_order_repeats_and_a_noncontiguous_image():
    image, masks, boxes = R.image_a()
    index = np.array([6, 0, 6, 3, 1], np.int64)             # out of order, a repeat, K != M
    want = want_a(False)[index]
    bits = pack(masks)
    for idx in (index, torch.from_numpy(index), torch.from_numpy(index).cuda(), torch.from_numpy(index).int().cuda()):
        got = TC().cut_tiles(dev(image), bits, boxes[index], index=idx, dtype=torch.uint8)
        assert np.array_equal(got.cpu().numpy(), want)
    # a non-contiguous view is cut as its values, not as its storage
    wide = dev(np.concatenate([image, image[:, ::-1]], axis=1))
    view = wide[:, :70]
    assert not view.is_contiguous()
    assert np.array_equal(TC().cut_tiles(view, bits, boxes, dtype=torch.uint8).cpu().numpy(), want_a(False))
    flipped = dev(image[..., ::-1].copy()).flip(-1)
    assert np.array_equal(TC().cut_tiles(flipped, bits, boxes, dtype=torch.uint8).cpu().numpy(), want_a(False))
    # boxes in column-major memory (what numpy's fancy column indexing returns) are read as their values
    fboxes = np.asfortranarray(boxes)
    assert not fboxes.flags.c_contiguous
    assert np.array_equal(TC().cut_tiles(dev(image), bits, fboxes, dtype=torch.uint8).cpu().numpy(), want_a(False))
    assert np.array_equal(TC().cut_tiles(dev(image), bits, torch.from_numpy(fboxes).cuda(), dtype=torch.uint8).cpu().numpy(),
                          want_a(False))
    # no tiles at all
    none = TC().cut_tiles(dev(image), bits, np.zeros((0, 4), np.int32), index=np.zeros(0, np.int64))
    assert none.shape == (0, 3, 224, 224)


def test_validation():
    image, masks, boxes = R.image_a()
    dimage, bits = dev(image), pack(masks)
    for bad in ((70, 0, 4, 4), (0, 37, 4, 4), (-1, 0, 4, 4), (3, 3, 0, 4)):
        b = boxes.copy()
        b[4] = bad
        with pytest.raises(ValueError, match="box 4"):
            TC().cut_tiles(dimage, bits, b)
    with pytest.raises(RuntimeError, match="no CPU path"):
        TC().cut_tiles(torch.from_numpy(image), bits, boxes)
    with pytest.raises(RuntimeError, match="no CPU path"):
        TC().cut_tiles(dimage, bits.cpu(), boxes)
    with pytest.raises(ValueError, match="uint8"):
        TC().cut_tiles(dimage.float(), bits, boxes)
    with pytest.raises(ValueError, match="bits"):
        TC().cut_tiles(dimage, bits[:, :-1], boxes)
    with pytest.raises(ValueError, match="no index"):
        TC().cut_tiles(dimage, bits, boxes[:3])
    with pytest.raises(ValueError, match="outside"):
        TC().cut_tiles(dimage, bits, boxes[:2], index=[0, len(masks)])


@pytest.mark.parametrize("hw", SIZES)
def test_mask_boxes(hw):
    H, W = hw
    g = np.random.default_rng(H * 100 + W)
    m = np.zeros((12, H, W), bool)
    m[1] = True
    m[2, 0, 0] = True
    m[3, H - 1, W - 1] = True
    m[4:8] = g.random((4, H, W)) < g.uniform(0.02, 0.6, (4, 1, 1))
    m[8:] = R_rects(g, 4, H, W)
    want = R.boxes_ref(m)
    got = TC().mask_boxes(pack(m), H, W)
    assert got.dtype == torch.int32 and got.shape == (12, 4)
    assert np.array_equal(got.cpu().numpy(), want)
    assert want[0].tolist() == [0, 0, -1, -1] and want[1].tolist() == [0, 0, W - 1, H - 1]
    assert want[2].tolist() == [0, 0, 0, 0] and want[3].tolist() == [W - 1, H - 1, W - 1, H - 1]
    assert np.array_equal(TC().sam_xywh(got).cpu().numpy(), R.sam_xywh(want))
    # bits beyond the last pixel are ignored
    dirty = pack(m).clone()
    if (H * W) % 64:
        dirty[:, -1] |= -1 << ((H * W) % 64)
        assert np.array_equal(TC().mask_boxes(dirty, H, W).cpu().numpy(), want)
    assert TC().mask_boxes(dirty[:0], H, W).shape == (0, 4)


def R_rects(g, n, H, W):
    out = np.zeros((n, H, W), bool)
    for k in range(n):
        y0, x0 = int(g.integers(0, H)), int(g.integers(0, W))
        out[k, y0:int(g.integers(y0, H)) + 1, x0:int(g.integers(x0, W)) + 1] = True
    return out


def test_mask_boxes_on_more_words_than_one_pass_of_the_wave():
    """A mask of more than 64 words (every lane takes a second word) whose rows straddle words: 150 x 70."""
    g = np.random.default_rng(7)
    m = np.concatenate([R_rects(g, 6, 150, 70), g.random((3, 150, 70)) < 0.001])
    assert (150 * 70 + 63) // 64 > 128
    assert np.array_equal(TC().mask_boxes(pack(m), 150, 70).cpu().numpy(), R.boxes_ref(m))


# ---- levels ---------------------------------------------------------------------------------------------------------------------
def four_levels():
    """Image A's masks as four kept levels, one of them empty: SAM dicts, a (masks, boxes) pair and a pair without boxes."""
    image, masks, boxes = R.image_a()
    dicts = [{"segmentation": masks[k], "bbox": [float(v) for v in boxes[k]]} for k in (0, 1, 2)]
    pair = (torch.from_numpy(masks[[5, 6, 7, 8]]), boxes[[5, 6, 7, 8]])
    auto = (dev(masks[[3, 6]]), None)
    split = [[0, 1, 2], [], [5, 6, 7, 8], [3, 6]]
    return image, masks, boxes, [dicts, [], pair, auto], split


def encoder():
    w = torch.randn(3 * 224 * 224, 8, generator=torch.Generator().manual_seed(14)).cuda()
    return lambda tiles: tiles.reshape(tiles.shape[0], -1) @ w


def auto_boxes(masks):
    return R.sam_xywh(R.boxes_ref(masks))


def test_level_tiles_equal_cut_tiles():
    image, masks, boxes, levels, split = four_levels()
    tiles = TC().level_tiles(dev(image), levels)
    assert [tuple(t.shape) for t in tiles] == [(3, 3, 224, 224), (0, 3, 224, 224), (4, 3, 224, 224), (2, 3, 224, 224)]
    bits = pack(masks)
    for j in (0, 2):
        assert torch.equal(tiles[j], TC().cut_tiles(dev(image), bits, boxes[split[j]], index=split[j]))
    ab = auto_boxes(masks[split[3]])                        # SAM's convention: one less than the extent
    assert ab[0].tolist() == [58, 30, 11, 6]
    assert torch.equal(tiles[3], TC().cut_tiles(dev(image), bits, ab, index=split[3]))
    assert np.array_equal((tiles[3] * 255).round().byte().permute(0, 2, 3, 1).cpu().numpy(),
                          R.tiles_ref(image, masks, ab, index=split[3]))
    with pytest.raises(ValueError, match="four"):
        TC().level_tiles(dev(image), levels[:3])


def test_embed_levels_and_language_features(tmp_path):
    from gags_amd import io_formats
    image, masks, boxes, levels, split = four_levels()
    encode = encoder()
    feature, seg_maps, lengths = TC().embed_levels(dev(image), levels, encode)
    assert feature.dtype == torch.float16 and feature.shape == (9, 8) and not feature.is_cuda
    assert lengths.tolist() == [3, 0, 4, 2]
    # the same normalise-and-half in torch on the RESTATEMENT's tiles, level by level, through the same encode
    rows = []
    for j, ks in enumerate(split):
        if not ks:
            continue
        b = auto_boxes(masks[ks]) if j == 3 else boxes[ks]
        e = encode(as_f32(dev(R.tiles_ref(image, masks, b, index=ks))))
        rows.append((e / e.norm(dim=-1, keepdim=True)).cpu().half())
    assert torch.equal(feature, torch.cat(rows))
    want_maps, want_lengths = SM().assemble_seg_maps([dev(masks[ks]) if ks else [] for ks in split], hw=(37, 70))
    assert torch.equal(seg_maps, want_maps) and torch.equal(lengths, want_lengths)
    assert int(seg_maps.max()) == 8 and (seg_maps[1] == -1).all()
    # saved and read back
    prefix = str(tmp_path / "out" / "frame_00001")
    f2, s2, l2 = TC().language_features(dev(image), levels, encode, prefix=prefix)
    assert torch.equal(f2, feature) and torch.equal(s2, seg_maps) and torch.equal(l2, lengths)
    emb, seg = io_formats.load_language_features(prefix)
    assert torch.equal(emb, feature.float()) and torch.equal(seg, seg_maps.cpu().float())
    assert not os.path.exists(str(tmp_path / "none_f.npy"))
    TC().language_features(dev(image), levels, encode)      # no prefix: nothing is written
    assert sorted(os.listdir(tmp_path / "out")) == ["frame_00001_f.npy", "frame_00001_s.npy"]


def test_all_levels_empty():
    image = dev(R.image_a()[0])
    tiles = TC().level_tiles(image, [[], [], [], []])
    assert all(tuple(t.shape) == (0, 3, 224, 224) for t in tiles)
    feature, seg_maps, lengths = TC().embed_levels(image, [[], [], [], []], encoder())
    assert feature.shape[0] == 0 and (seg_maps == -1).all() and seg_maps.shape == (4, 37, 70) and lengths.tolist() == [0] * 4
