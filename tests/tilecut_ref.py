"""Integer numpy restatement of the tile cut (include/gags_next.h N14; preprocess.py's get_seg_img, pad_img and the
cv2.resize(..., (224, 224)) of mask2segmap), written from the rule and not from the reference's text.  Crop, mask and pad are
pinned bit for bit to the reference's own functions by tests/golden/tilecut_vectors.npz (make_golden_tilecut.py).  The resize
is OpenCV's 8-bit INTER_LINEAR restated from memory: it is pinned to cv2 only where tests/golden/tilecut_cv2_vectors.npz exists
(make_golden_tilecut.py --cv2 on a machine with cv2); without it, tests/test_tilecut_cpu.py holds it to float64 bilinear within
a derived bound and to its fixed points."""
import os

import numpy as np

SIDE = 224
_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(_GOLDEN, "tilecut_vectors.npz")
CV2_FIXTURE = os.path.join(_GOLDEN, "tilecut_cv2_vectors.npz")
Z = np.load(FIXTURE) if os.path.exists(FIXTURE) else None   # (absent only while the generator writes it for the first time)


# ---- the rule ------------------------------------------------------------------------------------------------------------------
def clip_box(box, H, W):
    """(x, y, w', h') of a SAM bbox clipped as a numpy slice clips it; ValueError where the reference's slice would wrap
    around, leave the image or come back empty."""
    x, y, w, h = (int(v) for v in box)
    wc, hc = min(x + w, W) - x, min(y + h, H) - y
    if not (0 <= x < W and 0 <= y < H and wc >= 1 and hc >= 1):
        raise ValueError(f"box {(x, y, w, h)} does not cut a {H} x {W} image")
    return x, y, wc, hc


def square_ref(image, mask, box, bgr=False):
    """The padded square [l, l, 3] uint8 of one mask: crop, zero outside the mask, centre on the shorter axis."""
    image, mask = np.asarray(image), np.asarray(mask) != 0
    H, W = mask.shape
    x, y, wc, hc = clip_box(box, H, W)
    src = image[..., ::-1] if bgr else image
    crop = np.where(mask[y:y + hc, x:x + wc, None], src[y:y + hc, x:x + wc], 0).astype(np.uint8)
    l = max(wc, hc)
    ox = (l - wc) // 2 if hc > wc else 0
    oy = (l - hc) // 2 if hc <= wc else 0
    sq = np.zeros((l, l, 3), np.uint8)
    sq[oy:oy + hc, ox:ox + wc] = crop
    return sq


def tap_table(l, side=SIDE):
    """(s0, s1, a0, a1) int64 [side] each: the two source taps and their 11-bit coefficients for an axis of l pixels."""
    scale = np.float64(l) / np.float64(side)
    d = np.arange(side, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f)
    f = (f - s).astype(np.float32)
    s = s.astype(np.int64)
    low, high = s < 0, s >= l - 1
    s = np.where(low, 0, np.where(high, l - 1, s))
    f = np.where(low | high, np.float32(0), f).astype(np.float32)
    a0 = np.rint((np.float32(1) - f).astype(np.float32) * np.float32(2048)).astype(np.int64)
    a1 = np.rint(f * np.float32(2048)).astype(np.int64)
    return s, np.minimum(s + 1, l - 1), a0, a1


def resize_ref(sq, side=SIDE):
    """[l, l, C] uint8 -> [side, side, C] uint8: horizontal pass in integers, vertical pass with the two truncations."""
    sq = np.asarray(sq)
    assert sq.dtype == np.uint8 and sq.ndim == 3 and sq.shape[0] == sq.shape[1]
    s0, s1, a0, a1 = tap_table(sq.shape[0], side)
    S = sq.astype(np.int64)
    h = S[:, s0] * a0[None, :, None] + S[:, s1] * a1[None, :, None]          # [l, side, C]
    h0, h1 = h[s0] >> 4, h[s1] >> 4                                           # [side, side, C]
    out = (((a0[:, None, None] * h0) >> 16) + ((a1[:, None, None] * h1) >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def area2_ref(sq):
    """[2 n, 2 n, C] uint8 -> [n, n, C]: the rounded 2 x 2 mean (what OpenCV's area path gives at exactly 2 x)."""
    S = np.asarray(sq).astype(np.int64)
    return ((S[0::2, 0::2] + S[0::2, 1::2] + S[1::2, 0::2] + S[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def bilinear_f64(sq, side=SIDE):
    """Float64 bilinear at the same sample positions with clamped taps, unrounded: what the integer arithmetic approximates."""
    sq = np.asarray(sq)
    l = sq.shape[0]
    pos = np.clip((np.arange(side, dtype=np.float64) + 0.5) * (l / side) - 0.5, 0, l - 1)
    s = np.minimum(np.floor(pos).astype(np.int64), l - 1)
    f = pos - s
    s1 = np.minimum(s + 1, l - 1)
    S = sq.astype(np.float64)
    h = S[:, s] * (1 - f)[None, :, None] + S[:, s1] * f[None, :, None]
    return h[s] * (1 - f)[:, None, None] + h[s1] * f[:, None, None]


def tiles_ref(image, masks, boxes, index=None, bgr=False):
    """tiles_u8 [K, 224, 224, 3]: the whole contract on the host, one mask at a time (this is also the host composition
    tools/tilecut_bench.py times)."""
    index = range(len(boxes)) if index is None else index
    out = [resize_ref(square_ref(image, masks[int(m)], boxes[k], bgr)) for k, m in enumerate(index)]
    return np.stack(out) if out else np.zeros((0, SIDE, SIDE, 3), np.uint8)


def boxes_ref(masks):
    """[M, 4] int32 (x0, y0, x1, y1), inclusive tight bounds; (0, 0, -1, -1) for an empty mask."""
    out = np.zeros((len(masks), 4), np.int32)
    for k, m in enumerate(np.asarray(masks) != 0):
        ys, xs = np.nonzero(m)
        out[k] = (xs.min(), ys.min(), xs.max(), ys.max()) if len(ys) else (0, 0, -1, -1)
    return out


def sam_xywh(boxes):
    boxes = np.asarray(boxes)
    return np.stack([boxes[:, 0], boxes[:, 1], boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]], axis=1).astype(np.int32)


# ---- the cases the CPU and the GPU tests share --------------------------------------------------------------------------------
A_CASES = ("tall", "wide", "one", "last", "overhang", "whole", "holes", "outside", "roomy")


def image_a():
    """Image A, 37 x 70 (2590 pixels: 40 words and a 30-bit tail; no row starts on a word), nine masks and their boxes:
      tall      h = 9, w = 4: ox = (9 - 4) // 2, the odd difference floors       wide      h = 4, w = 9
      one       a 1 x 1 box: l = 1, every tap clamps                              last      ends on the last row and column
      overhang  the box overhangs the right and bottom edges (the slice clips)   whole     the whole image, full mask
      holes     a mask with holes                                                 outside   set pixels outside the box
      roomy     the box is larger than its mask: zeros inside"""
    g = np.random.default_rng(14)
    H, W = 37, 70
    image = g.integers(1, 256, (H, W, 3), dtype=np.uint8)   # no zero byte: a wrongly masked pixel always shows
    masks = np.zeros((len(A_CASES), H, W), bool)
    boxes = np.zeros((len(A_CASES), 4), np.int32)

    def rect(k, x, y, w, h):
        masks[k, y:y + h, x:x + w] = True
    rect(0, 11, 5, 4, 9); boxes[0] = (11, 5, 4, 9)
    rect(1, 30, 20, 9, 4); boxes[1] = (30, 20, 9, 4)
    rect(2, 63, 1, 1, 1); boxes[2] = (63, 1, 1, 1)
    rect(3, 58, 30, 12, 7); boxes[3] = (58, 30, 12, 7)
    rect(4, 60, 25, 10, 12); boxes[4] = (60, 25, 25, 40)
    masks[5] = True; boxes[5] = (0, 0, W, H)
    masks[6, 3:30, 8:50] = g.random((27, 42)) < 0.6; boxes[6] = (8, 3, 42, 27)
    masks[7] = g.random((H, W)) < 0.5; boxes[7] = (20, 10, 17, 13)
    rect(8, 25, 12, 6, 5); boxes[8] = (20, 8, 21, 16)
    return image, masks, boxes


B_SIDES = (223, 224, 225, 447, 448, 449, 450)


def image_b(transpose=False):
    """Image B, 450 x 9 (or its 9 x 450 transpose): one mask with holes and full-width boxes of every length in B_SIDES, i.e.
    the upscale boundary, the identity, the 2 x area switch and its neighbours on both sides."""
    g = np.random.default_rng(15)
    image = g.integers(1, 256, (450, 9, 3), dtype=np.uint8)
    mask = g.random((450, 9)) < 0.8
    boxes = np.array([(0, 450 - l if k % 2 else 0, 9, l) for k, l in enumerate(B_SIDES)], np.int32)
    if transpose:
        image, mask, boxes = np.ascontiguousarray(image.transpose(1, 0, 2)), np.ascontiguousarray(mask.T), boxes[:, [1, 0, 3, 2]]
    return image, mask[None], boxes


def fixture_squares():
    """[(case name, image, mask, box, the reference's padded square)] of tests/golden/tilecut_vectors.npz."""
    H, W = (int(v) for v in Z["a_shape"])
    n = len(Z["a_boxes"])
    masks = np.unpackbits(Z["a_masks"])[:n * H * W].reshape(n, H, W).astype(bool)
    out = [(str(name), Z["a_image"], masks[k], Z["a_boxes"][k], Z[f"a_square_{k}"]) for k, name in enumerate(Z["a_cases"])]
    bh, bw = (int(v) for v in Z["b_shape"])
    bmask = np.unpackbits(Z["b_mask"])[:bh * bw].reshape(bh, bw).astype(bool)
    out.append(("b224", Z["b_image"], bmask, Z["b_box"], Z["b_square"]))
    return out
